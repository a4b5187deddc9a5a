"""CPU: the ill-conditioned inputs of tests/illcond_cases.py are fair.  LAPACK in the working precision factors every case of both families and both precisions at the
sizes the device tests use, and its factor, its row solve, its vector solves and its posterior weights sit far inside the componentwise bounds F, R, V and A that
tests/test_gpu_backward_error.py asserts for the HIP kernels (printed as `RATIO_REF <case> <value>`; run with -s to see them).  So a device ratio above 1 is a
finding about the kernel: a conventional implementation leaves more than 10× headroom on exactly these matrices."""
import numpy as np
import pytest
import scipy.linalg as sla

from tests import illcond_cases as ic

SIZES = {"gp": (64, 192, 320, 1088, 1100), "spec": (64, 192, 320, 1088)}
ALL = [(prec, c, n) for prec in ("f64", "f32") for c in ic.cases(prec) for n in SIZES[c[0]]]


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 1.2e-19


def test_sample_rows():
    assert np.array_equal(ic.sample_rows(576), np.arange(576))
    for n in (1088, 1100, 1801):
        r = ic.sample_rows(n)
        assert set(range((n - 1) // 64 * 64, n)) <= set(r) and set(range(0, n, 64)) <= set(r)
        assert r.min() >= 0 and r.max() == n - 1 and len(r) <= 64 + (n + 63) // 64 + 32
        assert np.array_equal(r, ic.sample_rows(n))


def test_measures_see_a_wrong_factor():
    """each measure is far below 1 for LAPACK and above 1 once the result is perturbed by 1e-10 relative (fp64, n = 192, σ² = 1e-8)"""
    n, u = 192, ic.U["f64"]
    A, L = ic.matrix("gp", n, 1e-8, "f64"), ic.lapack_factor("gp", n, 1e-8, "f64")
    bad = L * (1 + 1e-10)
    assert ic.measure_F(A, L, u)[1] < 0.1 < 1 < ic.measure_F(A, bad, u)[1]
    assert ic.measure_F(A, L, u, inverse=((16, None),))[0] <= ic.measure_F(A, L, u)[1] and ic.measure_F(A, bad, u, inverse=((16, None),))[0] > 1
    X0 = ic.rhs((64, n), 1, "f64")
    Xh = sla.solve_triangular(L, X0.T, lower=True).T
    assert ic.measure_R(X0, Xh, L, u) < 0.1 < 1 < ic.measure_R(X0, Xh * (1 + 1e-10), L, u)
    b = ic.rhs((n, 2), 2, "f64")
    x = sla.solve_triangular(L, b, lower=True)
    assert ic.measure_V(L, x, b, u, True) < 0.1 < 1 < ic.measure_V(L, x * (1 + 1e-10), b, u, True)
    d = float(np.log(np.diagonal(L)).sum())
    assert ic.measure_D(L, d, u) < 0.1 < 1 < ic.measure_D(L, d * (1 + 1e-10), u)
    assert ic.measure_D(L, 2 * d, u, logdet=True) < 0.1
    q = (x * x).sum(0)
    assert ic.measure_Q(L, q, b, u) < 0.1 < 1 < ic.measure_Q(L, q * (1 + 1e-6), b, u)
    Lq = ic.cholesky_ld(A)
    assert np.max(np.abs(Lq.astype(np.float64) - L) / (np.abs(L) + 1e-300)) < 1e-4
    assert np.max(np.abs(ic.solve_lower_ld(np.tril(L).astype(ic.LD), b.astype(ic.LD)).astype(np.float64) - x)) < 1e-6 * np.max(np.abs(x))


@pytest.mark.parametrize("prec,case,n", ALL, ids=[f"{p}-{ic.case_id(c)}-n{n}" for p, c, n in ALL])
def test_lapack_is_far_inside_every_bound(prec, case, n):
    fam, level = case
    u = ic.U[prec]
    A = ic.matrix(fam, n, level, prec)
    L = ic.lapack_factor(fam, n, level, prec)  # asserts info == 0
    tag = f"{prec},{ic.case_id(case)},n={n}"
    out = {"F": ic.measure_F(A, L, u)[1]}
    X0 = ic.rhs((16, n), n, prec)
    Xh = sla.solve_triangular(L, X0.T, lower=True).T
    assert Xh.dtype == A.dtype
    out["R"] = ic.measure_R(X0, Xh, L, u)
    b = ic.rhs((n, 2), n + 1, prec)
    out["V_forward"] = ic.measure_V(L, sla.solve_triangular(L, b, lower=True), b, u, True)
    out["V_backward"] = ic.measure_V(L, sla.solve_triangular(L, b, lower=True, trans="T"), b, u, False)
    alpha = sla.cho_solve((L, True), b)
    assert alpha.dtype == A.dtype
    out["A"] = ic.measure_A(A, L, alpha, b, u)[1]
    for k, v in out.items():
        print(f"RATIO_REF lapack_{k}[{tag}] {v:.4g}", flush=True)
    assert all(v <= 1.0 for v in out.values()), out
    assert out["F"] <= 0.1 and max(out["R"], out["V_forward"], out["V_backward"], out["A"]) <= 0.1, out  # the headroom the device bounds rely on


def test_emulated_explicit_inverse_designs_show_the_excess_and_meet_their_own_bounds():
    """The two explicit-inverse designs of the engine in fp64 NumPy (illcond_cases.emulate_leaf_cholesky: 16 × 16 inverted diagonal blocks; emulate_tile_solve: 64 × 64
    tile inverses formed column by column) on the graded family.  They exceed substitution's bounds where the device does — F at 68 (n = 64), 1.4 (192), 1.5 (320) at
    σ² = 1e-10, the backward sweep at 12 (np = 128, three right-hand sides), against the device's 68 / 1.8 / 1.4 and 12 … 29 in profiles/r23/backward_error_ratios.txt —
    and sit far inside the bounds with the inverse terms that the GPU tests assert.  An inverse formed row by row (small LEFT residual) does not bring the backward
    sweep under substitution's bound either: a product with an explicit inverse is stable only up to cond(T), whichever residual is small."""
    u = ic.U["f64"]
    seen = {}
    for n in (64, 192, 320):
        A = ic.matrix("gp", n, 1e-10, "f64")
        own, subst = ic.measure_F(A, ic.emulate_leaf_cholesky(A), u, inverse=((16, None),))
        print(f"RATIO_EMU leaf_F[n={n}] {own:.4g} subst {subst:.4g}", flush=True)
        seen[n] = subst
        assert own <= 0.2, (n, own)
    assert 30 < seen[64] < 150 and 1 < seen[192] < 4 and 1 < seen[320] < 4, seen
    assert ic.measure_F(ic.matrix("gp", 1088, 1e-10, "f64"), ic.emulate_leaf_cholesky(ic.matrix("gp", 1088, 1e-10, "f64")), u)[1] < 1
    L = np.array(ic.lapack_factor("gp", 128, 1e-10, "f64"))
    b = ic.rhs((3, 128), 128, "f64").T
    fwd = ic.measure_V_tiles(L, ic.emulate_tile_solve(L, b, True), b, u, True)
    bwd = ic.measure_V_tiles(L, ic.emulate_tile_solve(L, b, False), b, u, False)
    rows = ic.measure_V_tiles(L, ic.emulate_tile_solve(L, b, False, by_rows=True), b, u, False)
    print(f"RATIO_EMU tile_V[np=128] forward subst {fwd[1]:.4g} backward {bwd[0]:.4g} subst {bwd[1]:.4g} backward by rows subst {rows[1]:.4g}", flush=True)
    assert fwd[1] <= 0.1 and bwd[0] <= 0.1 and 4 < bwd[1] < 40 and rows[1] > 1, (fwd, bwd, rows)
    L = np.array(ic.lapack_factor("gp", 1024, 1e-10, "f64"))
    b = ic.rhs((3, 1024), 1024, "f64").T
    assert ic.measure_V_tiles(L, ic.emulate_tile_solve(L, b, False), b, u, False)[1] < 1

