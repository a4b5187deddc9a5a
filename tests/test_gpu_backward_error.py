"""GPU: componentwise BACKWARD errors of the Cholesky factorisation and of every solve on ill-conditioned matrices (tests/illcond_cases.py: a graded GP family,
cond up to 2e12 with the factor's diagonal ratio just under the 1e5 guard of the explicit-inverse paths, and a random-spectrum family, cond up to 1e10), against
bounds that can be derived (Higham, Accuracy and Stability of Numerical Algorithms: Theorems 8.5, 10.3, 10.4).  Every other factorisation test of the suite runs
at cond <= 5.1 or compares forward against an fp64 oracle, which says nothing once cond·u reaches the tolerance; a backward error does not depend on cond at all.

Every check prints `RATIO <case> <max error / bound>` and asserts ratio <= 1; the same measure of SciPy's LAPACK result on the same input is printed as
`RATIO_REF` (tests/test_illcond_cpu.py pins that LAPACK sits below 0.1 on every case).  All residual products are formed in np.longdouble from the values the device
returned.  A ratio above 1 is a finding about the kernel, not a tolerance to widen.

Device level (gpd_*): F, R, D of gpd_potrf with rows below under every leaf variant, R of gpd_trsm, V of gpd_trsv, R and the right residual of gpd_inv_lower +
gpd_trsm_inv.  API level (GP family): F of post.data.C.U against the longdouble matrix of the same inputs, A of α, D, Q, for the single-device schedules, Strassen
updates, fp32, vector and dense noise, the sequential update, the inverse-block prediction path, the batch calls and a 2 × 2 multi-device fit.

At the API level the device assembles K itself, so the bounds carry the project's kernel-matrix tolerance t (unit_helpers.assemble_bound: 1e-14·variance in fp64,
(D + 16)·u·variance in fp32) wherever K enters: + t in F, + t·‖α̂‖₁ in A (Ĉ = C + ΔK with |ΔK| <= t gives |ΔK α̂| <= t‖α̂‖₁).

Where the design multiplies by an explicit inverse, substitution's bound does not hold and the bound of that path is asserted instead; the ratio to the
substitution bound is still printed, as `RATIO_SUBST`.  Two paths need it on these inputs (measured: profiles/r23/backward_error_ratios.txt; both reproduced to
three digits by a host emulation of the same arithmetic — illcond_cases.emulate_leaf_cholesky / emulate_tile_solve, pinned in tests/test_illcond_cpu.py — so they are
the documented cond(L_bb)·u term and nothing else):
  * F.  Every leaf forms the blocks below a 16 × 16 diagonal block T as (updated block)·inv(T)ᵀ.  On the graded family the diagonal of a one-tile factor falls by
    1e5 inside 64 columns, cond(T) reaches 1e3, and F stands at 68 (n = 64), 1.8 (192), 1.4 (320), 0.6 (1 088) times Theorem 10.3's bound at σ² = 1e-10.  Asserted:
    |A − L̂L̂ᵀ| <= γ_{n+1} |L̂||L̂|ᵀ + 2γ_16 |L̂[i, J] Tᵀ||T⁻ᵀ||Tᵀ| on the rows below each block (illcond_cases.measure_F derives it; a 2 × 2 multi-device fit with
    "multi_trsm_inv" = 1 adds the same term with the 256-wide inverse for the rows below each distribution block).
  * V, backward.  The vector solves multiply each 64-wide step by inv(T) formed column by column: a right-residual inverse, which serves the forward solve
    (held to V as it stands) but enters the backward solve through its LEFT residual, ŴT − I = T⁻¹(TŴ − I)T (illcond_cases.measure_V_tiles).  np = 128 of
    the graded family (a 64 × 64 tile with diagonal ratio 1e5) stands at 29 times V; np = 1 024 at 0.04.
  * A, single device.  α̂ comes from those two sweeps on that factor, so its bound carries both terms (illcond_cases.measure_A): n = 130 at σ² = 1e-10 (one tile with
    the whole fall of the diagonal) stands at 2.9 times Theorem 10.4, every other case below 0.02 of it.  The batch calls (substitution, 1 / L_jj) and the
    distributed solve are held to Theorem 10.4 as it stands.
The componentwise inverse terms lose the cancellation inside T⁻ᵀ and are loose where they matter (the asserted ratios there are 1e-3 and below); RATIO_SUBST is the
figure to watch for a regression.  R, D, Q and the forward V hold as the theorems state them and are asserted so.

D and Q are conditional on a factor.  gp_posterior_logdet belongs to the handle whose factor is read back, so it is held to D as it stands.  logdetcov(fx) and
sqmahal(fx, Y) run a factorisation of their own that returns no factor; two factors L̂₁, L̂₂ of the same C each satisfy F, so to first order
logdet differs by tr(C⁻¹(Δ₁ − Δ₂)) <= 2γ_{n+1} Σ|C⁻¹|∘(|L̂||L̂|ᵀ) and δᵀC⁻¹δ by 2γ_{n+1} |α|ᵀ|L̂||L̂|ᵀ|α| (α = L̂⁻ᵀz): these terms are added for those two calls, and the
ratio to the conditional bound alone is printed beside it as `RATIO_COND`, and asserted where both factorisations produce the same bits: under "deterministic" = 1,
and at n = 130, which runs no GEMM.  The cross-factor terms are forward terms of the size of cond(C)·u: everywhere else the asserted api_D / api_Q catch GROSS loss
only (their ratios are 1e-6 and below), and D on the posterior's own handle (api_D_handle) is the sharp check.

Out of scope here: VFE / DTC (K_zz with jitter is exercised at cond 1e8 in tests/test_gpu_parity.py); the logpdf gradient (a forward quantity: only its difference
between the batch and the single path is recorded); predictive variances as forward quantities; full sizes."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import illcond_cases as ic  # noqa: E402
from tests import unit_helpers as uh  # noqa: E402
from tests.conftest import rank_devices  # noqa: E402
from tests.unit_helpers import P, report  # noqa: E402

LD = ic.LD
TDT = {"f64": torch.float64, "f32": torch.float32}
PREC_CASES = [(p, c) for p in ("f64", "f32") for c in ic.cases(p)]
PREC_IDS = [f"{p}-{ic.case_id(c)}" for p, c in PREC_CASES]
F64_CASES = ic.cases("f64")
F64_IDS = [ic.case_id(c) for c in F64_CASES]
NAN = float("nan")


def report_ref(name, ratio):
    print(f"RATIO_REF {name} {ratio:.4g}", flush=True)


def check(name, ratio):
    report(name, ratio)
    assert ratio <= 1.0, (name, ratio)


def check_both(name, ratios):
    """(ratio to the bound of the path, ratio to the substitution bound): the first is asserted, the second printed as RATIO_SUBST"""
    print(f"RATIO_SUBST {name} {ratios[1]:.4g}", flush=True)
    check(name, ratios[0])


LEAF_INVERSES = ((16, None),)  # every leaf (panel64 / panel64v2 / the register-resident leaf / trsm64_mfma) multiplies the rows below a 16 × 16 block by its inverse


@pytest.fixture(scope="module")
def lib(agp):
    return agp._lib.load()


@pytest.fixture(scope="module")
def h(ctx):
    return ctx.handle


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- device level: gpd_potrf with rows below ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _potrf_ref(prec, case, n, extra):
    """F and R of LAPACK on the same input (computed once per case)"""
    L = ic.lapack_factor(case[0], n, case[1], prec)
    rf = ic.measure_F(ic.matrix(case[0], n, case[1], prec), L, ic.U[prec])[1]
    rr = None
    if extra:
        X0 = ic.rhs((extra, n), n + extra, prec)
        rr = ic.measure_R(X0, sla.solve_triangular(L, X0.T, lower=True).T, L, ic.U[prec])
    return rf, rr


def _potrf_case(lib, h, prec, case, n, extra, tag):
    from abstractgps_jl_amd._lib import check as ok

    u, dt = ic.U[prec], TDT[prec]
    A0 = ic.matrix(case[0], n, case[1], prec)
    X0 = ic.rhs((extra, n), n + extra, prec)
    m, ld = n + extra, n + 32
    buf = np.full((m + 128, ld), NAN, dtype=ic.NPDT[prec])
    buf[:n, :n] = np.where(np.tri(n, dtype=bool), A0, NAN)  # the strictly upper triangle and the padding are NaN: they must be neither read nor written
    buf[n:m, :n] = X0
    inside = ~np.isnan(buf)
    A = _dev(buf)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    logdet = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ok(uh.entry(lib, "gpd_potrf", dt)(h, P(A), ld, m, n, P(info), 0, n, P(logdet)))
    uh.sync(lib, h)
    assert info.item() == 0, (tag, info.item())
    got = A.cpu().numpy()
    assert np.array_equal(~np.isnan(got), inside), (tag, "NaN inside the factor, or the strictly upper part / the padding written")
    L = np.tril(np.nan_to_num(got[:n, :n]))
    rf, rr = _potrf_ref(prec, case, n, extra)
    report_ref(f"potrf_F[{tag}]", rf)
    check_both(f"potrf_F[{tag}]", ic.measure_F(A0, L, u, inverse=LEAF_INVERSES))
    if extra:
        report_ref(f"potrf_R[{tag}]", rr)
        check(f"potrf_R[{tag}]", ic.measure_R(X0, got[n:m, :n], L, u))
    check(f"potrf_D[{tag}]", ic.measure_D(L, logdet.item(), u))


@pytest.mark.parametrize("extra", [0, 128])
@pytest.mark.parametrize("n", [64, 192, 320, 1088])
@pytest.mark.parametrize("prec,case", PREC_CASES, ids=PREC_IDS)
def test_potrf_with_rows_below(lib, h, prec, case, n, extra):
    """the default leaves and updates: one leaf (64), three leaves (192), beyond one leaf group (320), the in-panel updates and GEMMs (1 088)"""
    _potrf_case(lib, h, prec, case, n, extra, f"{prec},{ic.case_id(case)},n={n},extra={extra}")


LEAF_VARIANTS = {"leaf_group=64": dict(leaf_group=64), "leaf_group=128": dict(leaf_group=128), "leaf_group=256": dict(leaf_group=256),
                 "leaf_group=512": dict(leaf_group=512), "leaf_v2=0": dict(leaf_v2=0), "leaf_v2=0,leaf_group=256": dict(leaf_v2=0, leaf_group=256),
                 "leaf_cols=64": dict(leaf_cols=64), "leaf_xr=128": dict(leaf_xr=128)}  # leaf_xr = 64 is what the launch picks by itself at this shape
# the in-panel updates C −= P·P[0:N]ᵀ: potrf_rec takes panel_updk_kernel for a 128 | 128 split ("upd128") and for a left half of 256 … "updk_max_k" columns, so n = 320
# (128 | 192, then 64 | 128) reaches neither; n = 512 reaches both (256 | 256, and 128 | 128 inside each half)
UPDK_VARIANTS = {"upd128=0,updk_max_k=0": dict(upd128=0, updk_max_k=0), "updk_rt=1": dict(updk_rt=1), "updk_rt=2": dict(updk_rt=2), "updk_rt=4": dict(updk_rt=4)}


VARIANT_CASES = [(p, c, v) for p, c in PREC_CASES for v in LEAF_VARIANTS if p == "f64" or v.startswith("leaf_group")]


@pytest.mark.parametrize("prec,case,variant", VARIANT_CASES, ids=[f"{p}-{ic.case_id(c)}-{v}" for p, c, v in VARIANT_CASES])
def test_potrf_leaf_variants(lib, h, prec, case, variant):
    """the leaf variants of tests/test_gpu_units.py at n = 320 with 128 rows below (fp32 has one leaf, panel64_kernel<float>: only its leaf groups are run);
    leaf_v2 = 0 is panel64_kernel<double>, whose 16 × 16 diagonal blocks are inverted"""
    with uh.params(lib, h, **LEAF_VARIANTS[variant]):
        _potrf_case(lib, h, prec, case, 320, 128, f"{prec},{ic.case_id(case)},n=320,extra=128,{variant}")


@pytest.mark.parametrize("variant", list(UPDK_VARIANTS))
@pytest.mark.parametrize("case", F64_CASES, ids=F64_IDS)
def test_potrf_in_panel_update_variants(lib, h, case, variant):
    """panel_updk_kernel<RT> with every workgroup tile forced (16 / 32 / 64 rows) and the tile GEMM in its place, at n = 512 with 128 rows below: the smallest size at
    which both of potrf_rec's in-panel branches run (fp64 only: the fp32 updates are GEMMs)"""
    with uh.params(lib, h, **UPDK_VARIANTS[variant]):
        _potrf_case(lib, h, "f64", case, 512, 128, f"f64,{ic.case_id(case)},n=512,extra=128,{variant}")


# ---- device level: gpd_trsm ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(64, 64), (192, 256), (384, 1088)])
@pytest.mark.parametrize("prec,case", PREC_CASES, ids=PREC_IDS)
def test_trsm(lib, h, prec, case, m, n):
    """X ← X L⁻ᵀ against LAPACK's factor of the case (trsm64_mfma_kernel, whose 16 × 16 diagonal blocks are inverted, and the GEMMs between the leaves)"""
    from abstractgps_jl_amd._lib import check as ok

    u, dt = ic.U[prec], TDT[prec]
    L = ic.lapack_factor(case[0], n, case[1], prec)
    ld = n + 32
    Lp = np.zeros((n + 128, ld), dtype=L.dtype)
    Lp[:n, :n] = L
    X0 = ic.rhs((m + 128, ld), m + n, prec)
    X = _dev(X0)
    Ld = _dev(Lp)
    torch.cuda.synchronize()
    ok(uh.entry(lib, "gpd_trsm", dt)(h, P(X), ld, m, P(Ld), ld, n))
    uh.sync(lib, h)
    got = X.cpu().numpy()
    assert np.array_equal(got[m:], X0[m:]) and np.array_equal(got[:m, n:], X0[:m, n:])
    tag = f"{prec},{ic.case_id(case)},{m}x{n}"
    report_ref(f"trsm_R[{tag}]", ic.measure_R(X0[:m, :n], sla.solve_triangular(L, X0[:m, :n].T, lower=True).T, L, u))
    check(f"trsm_R[{tag}]", ic.measure_R(X0[:m, :n], got[:m, :n], L, u))


# ---- device level: gpd_trsv ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_", [128, 1024])
@pytest.mark.parametrize("prec,case", PREC_CASES, ids=PREC_IDS)
def test_trsv(lib, h, prec, case, np_):
    """the vector solves, which multiply by I − inv(L_jj) of every 64 × 64 tile (trtri_64_kernel) with no guard: forward (V as it stands) and backward (V with the
    left-residual term of the tile inverses: module docstring), one and three right-hand sides, every diagonal block size, with and without "deterministic"; the
    strictly upper triangle is NaN"""
    from abstractgps_jl_amd._lib import check as ok

    u, dt = ic.U[prec], TDT[prec]
    L = ic.lapack_factor(case[0], np_, case[1], prec)
    ld = np_ + 32
    Lp = np.full((np_, ld), NAN, dtype=L.dtype)
    Lp[:, :np_] = np.where(np.tri(np_, dtype=bool), L, NAN)
    Ld = _dev(Lp)
    R0 = ic.rhs((3, np_), np_, prec)
    worst = {}
    for fwd in (1, 0):
        xr = sla.solve_triangular(L, R0.T, lower=True, trans=0 if fwd else 1)
        report_ref(f"trsv_V[{prec},{ic.case_id(case)},np={np_},{'forward' if fwd else 'backward'}]", ic.measure_V(L, xr, R0.T, u, bool(fwd)))
    for det in (0, 1):
        for nbv in (128, 256, 512):
            with uh.params(lib, h, trsv_nb=nbv, deterministic=det):
                for nrhs in (1, 3):
                    for fwd in (1, 0):
                        W = _dev(R0[:nrhs])
                        torch.cuda.synchronize()
                        ok(uh.entry(lib, "gpd_trsv", dt)(h, P(Ld), ld, np_, P(W), np_, nrhs, fwd))
                        uh.sync(lib, h)
                        x = W.cpu().numpy().T
                        assert np.isfinite(x).all()
                        tag = f"{prec},{ic.case_id(case)},np={np_},nrhs={nrhs},trsv_nb={nbv},deterministic={det},{'forward' if fwd else 'backward'}"
                        both = ic.measure_V_tiles(L, x, R0[:nrhs].T, u, bool(fwd))
                        worst[tag] = both[1] if fwd else both[0]
                        print(f"RATIO_SUBST trsv_V[{tag}] {both[1]:.4g}", flush=True)
                        report(f"trsv_V[{tag}]", worst[tag])
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# ---- device level: gpd_inv_lower + gpd_trsm_inv ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [True, False], ids=["levels", "recursion"])
@pytest.mark.parametrize("nb", [64, 256, 384])
@pytest.mark.parametrize("case", F64_CASES, ids=F64_IDS)
def test_inv_lower_and_trsm_inv(lib, h, case, nb, two):
    """W = −inv(L) of an nb × nb block (fp64 only) and X ← −X Wᵀ.  The inverse is held to the RIGHT residual |LŴ + I| <= γ_{nb+1} |L||Ŵ|: that is what an inverse formed
    by substitution on the columns of the identity satisfies (Higham §14.2, Method 1; the 64 × 64 tiles here, + 1 for the reciprocal of the diagonal), what the level-wise
    products keep in this emulated and measured range, and what the product needs: X̂Lᵀ − X = −X (LŴ + I)ᵀ + ΔLᵀ.  The LEFT residual |ŴL + I| / (γ_nb |Ŵ||L|) is
    printed as RATIO_INFO only: no such bound holds for a right-residual method (SciPy's solve_triangular(L, I) — LAPACK's trtrs on the identity, not trtri — sits at
    4 000 times it on the graded family), and nothing
    here multiplies by W from the left.  R for the product, as it stands."""
    from abstractgps_jl_amd._lib import check as ok

    u = ic.U["f64"]
    L = ic.lapack_factor(case[0], nb, case[1], "f64")
    ld = nb + 32
    Lp = np.zeros((nb + 128, ld))
    Lp[:nb, :nb] = np.where(np.tri(nb, dtype=bool), L, NAN)
    Ld = _dev(Lp)
    W, S1, S2 = (torch.zeros(nb + 128, ld, dtype=torch.float64, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    ok(lib.gpd_inv_lower(h, P(Ld), ld, nb, P(W), ld, P(S1), P(S2) if two else None))
    uh.sync(lib, h)
    Wh = W.cpu().numpy()[:nb, :nb]
    assert np.isfinite(Wh).all() and not np.triu(Wh, 1).any()
    tag = f"{ic.case_id(case)},nb={nb},{'levels' if two else 'recursion'}"
    Ll, Wl = np.tril(L).astype(LD), Wh.astype(LD)
    Wref = -sla.solve_triangular(L, np.eye(nb), lower=True)
    tri, eye = np.tri(nb, dtype=bool), np.eye(nb, dtype=LD)
    left = lambda Wx: ic._max_ratio(np.abs(Wx @ Ll + eye)[tri], (ic.gamma(nb, u) * (np.abs(Wx) @ np.abs(Ll)))[tri])
    right = lambda Wx: ic._max_ratio(np.abs(Ll @ Wx + eye)[tri], (ic.gamma(nb + 1, u) * (np.abs(Ll) @ np.abs(Wx)))[tri])
    report_ref(f"inv_lower_right[{tag}]", right(Wref.astype(LD)))
    print(f"RATIO_INFO inv_lower_left[{tag}] {left(Wl):.4g} (solve_triangular(L, I) {left(Wref.astype(LD)):.4g})", flush=True)
    m = 64 * 5
    X0 = ic.rhs((m + 128, ld), nb, "f64")
    X = _dev(X0)
    S = torch.zeros(m + 128, ld, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ok(lib.gpd_trsm_inv(h, P(X), ld, m, P(W), ld, nb, P(S), ld))
    uh.sync(lib, h)
    got = X.cpu().numpy()
    assert np.array_equal(got[m:], X0[m:]) and np.array_equal(got[:m, nb:], X0[:m, nb:])
    report_ref(f"trsm_inv_R[{tag}]", ic.measure_R(X0[:m, :nb], sla.solve_triangular(L, X0[:m, :nb].T, lower=True).T, L, u))
    r_right, r_prod = right(Wl), ic.measure_R(X0[:m, :nb], got[:m, :nb], L, u)
    report(f"inv_lower_right[{tag}]", r_right)
    report(f"trsm_inv_R[{tag}]", r_prod)
    assert r_right <= 1.0 and r_prod <= 1.0, (tag, r_right, r_prod)


# ---- API level ---------------------------------------------------------------------------------------------------------------------------------------------------
def _ktol(prec):
    """the project's kernel-matrix tolerance per unit of prior variance for one-dimensional inputs (what tests/test_gpu_assemble.py asserts for that dtype)"""
    return uh.assemble_bound(TDT[prec], 1) / uh.VARIANCE


def _targets(x, n):
    rng = np.random.default_rng(n + 11)
    y = np.sin(2.0 * x.astype(np.float64)) + 0.1 * rng.standard_normal(n)
    return y.astype(x.dtype)


def _noise_ld(noise, n):
    """Σy in longdouble from the (already cast) values the API is given"""
    s = np.asarray(noise)
    return LD(float(s)) * np.eye(n, dtype=LD) if s.ndim == 0 else (np.diag(s.astype(LD)) if s.ndim == 1 else s.astype(LD))


@functools.lru_cache(maxsize=None)
def _api_ref(prec, n, s2):
    """F and A of LAPACK in the working precision on the rounded longdouble matrix of the scalar-noise problem"""
    x = ic.gp_inputs(n, prec)
    Cl = ic.gp_kernel_ld(x, x) + _noise_ld(ic.NPDT[prec](s2), n)
    Cw = Cl.astype(ic.NPDT[prec])
    L = sla.cholesky(Cw, lower=True)
    y = _targets(x, n)
    tol = 2 * ic.U[prec]  # the rounding of C (entries <= 1 + σ²) to the working precision
    return ic.measure_F(Cl, L, ic.U[prec], tol)[1], ic.measure_A(Cl, L, sla.cho_solve((L, True), y), y, ic.U[prec], tol)[1]


def _three_columns(delta):
    return np.stack([delta, np.cos(3 * delta.astype(np.float64)).astype(delta.dtype), delta[::-1]], axis=1)


def _factor_of(post, n, tag):
    U = np.array(post.data.C.U)
    assert U.shape == (n, n) and not np.tril(U, -1).any(), (tag, "the strictly lower part of C.U is not zero")
    return np.ascontiguousarray(U.T)


def _check_fit(agp, post, fx, Cl, delta, prec, tag, terms=True, inverse=LEAF_INVERSES, segments=(0,), same_bits=False, tiles=64):
    """F, A and D of a posterior against the longdouble matrix Cl of its inputs; with `terms` also logdetcov(fx) and sqmahal(fx, three columns)"""
    n, u, tol = Cl.shape[0], ic.U[prec], _ktol(prec)
    L = _factor_of(post, n, tag)
    check_both(f"api_F[{tag}]", ic.measure_F(Cl, L, u, tol, inverse, segments))
    check_both(f"api_A[{tag}]", ic.measure_A(Cl, L, np.asarray(post.data.alpha), delta, u, tol, inverse if tiles else (), segments, tiles))
    ld = C.c_double()
    agp._lib.check(post.data.C.ctx.lib.gp_posterior_logdet(post.data.C.handle, C.byref(ld)))
    check(f"api_D_handle[{tag}]", ic.measure_D(L, ld.value, u, logdet=True))
    if not terms:
        return L
    L64 = L.astype(np.float64)
    Labs = np.abs(L64) @ np.abs(L64).T  # fp64 is enough below: these products enter bounds only
    Linv = sla.solve_triangular(L64, np.eye(n), lower=True)
    cross_d = 2 * ic.gamma(n + 1, u) * float((np.abs(Linv.T @ Linv) * Labs).sum())
    lg = np.log(np.diagonal(L).astype(LD))
    cond_d = float(2 * ic.gamma(n + 2, u) * np.abs(lg).sum())
    err_d = float(abs(LD(float(agp.logdetcov(fx))) - 2 * lg.sum()))
    print(f"RATIO_COND api_D[{tag}] {err_d / cond_d:.4g}", flush=True)
    assert not same_bits or err_d <= cond_d, (tag, err_d / cond_d)
    check(f"api_D[{tag}]", err_d / (cond_d + cross_d))
    Y = _three_columns(delta)
    q = np.asarray(agp.sqmahal(fx, Y))
    Ll = np.tril(L).astype(LD)
    z = ic.solve_lower_ld(Ll, Y.astype(LD))
    za = np.abs(z)
    cond_q = 2 * ic.gamma(n, u) * np.einsum("ij,ij->j", za, np.abs(Linv).astype(LD) @ (np.abs(Ll) @ za)) + ic.gamma(n, u) * (z * z).sum(0)
    al = np.abs(sla.solve_triangular(L64, z.astype(np.float64), lower=True, trans=1))
    cross_q = 2 * ic.gamma(n + 1, u) * np.einsum("ij,ij->j", al, Labs @ al)
    err_q = np.abs(q.astype(LD) - (z * z).sum(0))
    print(f"RATIO_COND api_Q[{tag}] {float(np.max(err_q / cond_q)):.4g}", flush=True)
    assert not same_bits or float(np.max(err_q / cond_q)) <= 1.0, (tag, float(np.max(err_q / cond_q)))
    check(f"api_Q[{tag}]", float(np.max(err_q / (cond_q + cross_q.astype(LD)))))
    return L


def _scalar_fit(agp, ctx, prec, n, s2, tag, terms=True, inverse=LEAF_INVERSES, same_bits=False, tiles=64):
    x = ic.gp_inputs(n, prec)
    y = _targets(x, n)
    s2w = ic.NPDT[prec](s2)
    fx = agp.GP(agp.SqExponentialKernel(), ctx=ctx)(x, s2w)
    post = agp.posterior(fx, y)  # a PosDefException on any of these inputs is a failure
    Cl = ic.gp_kernel_ld(x, x) + _noise_ld(s2w, n)
    rf, ra = _api_ref(prec, n, s2)
    report_ref(f"api_F[{prec},n={n},s2={s2:g}]", rf)
    report_ref(f"api_A[{prec},n={n},s2={s2:g}]", ra)
    _check_fit(agp, post, fx, Cl, y, prec, tag, terms, inverse, same_bits=same_bits, tiles=tiles)
    post.data.C.free()


def _context(agp, **kw):
    ctx = agp.Context(0)
    for k, v in kw.items():
        ctx.set_param(k, v)
    return ctx


@pytest.mark.parametrize("n", [130, 320])
@pytest.mark.parametrize("s2", ic.GP_LEVELS["f64"])
def test_api_single_device_defaults(agp, n, s2):
    """n = 130 is padded to 256: one 128-column leaf, the 128 | 128 in-panel update (panel_updk_kernel), one more leaf — no GEMM launch, so no atomics: logdetcov and
    sqmahal reproduce the posterior's factor bit for bit and are held to the conditional D and Q as the theorems state them"""
    ctx = _context(agp)
    try:
        _scalar_fit(agp, ctx, "f64", n, s2, f"f64,n={n},s2={s2:g},defaults", same_bits=n == 130)
    finally:
        ctx.close()


SCHEDULES = [{"nb": 512, "lookahead": 1, "lookahead_min_n": 0}, {"nb": 0}, {"nb": 512, "leaf_cols": 64}, {"deterministic": 1}, {"gemm_streamk": 0}]


@pytest.mark.parametrize("kw", SCHEDULES, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in SCHEDULES])
@pytest.mark.parametrize("s2", ic.GP_LEVELS["f64"])
def test_api_single_device_schedules(agp, s2, kw):
    """n = 1 100 (padded 1 152) under the parameter sets of test_fit_schedules (three panels with look-ahead, the unblocked path, 64-column leaves) and without
    atomics; logdetcov / sqmahal factor again under the same parameters, so they run under every set"""
    ctx = _context(agp, **kw)
    try:
        _scalar_fit(agp, ctx, "f64", 1100, s2, f"f64,n=1100,s2={s2:g}," + ",".join(f"{k}={v}" for k, v in kw.items()), same_bits=kw == SCHEDULES[3])
    finally:
        ctx.close()


@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("s2", ic.GP_LEVELS["f64"])
def test_api_strassen_updates(agp, s2, group):
    """the settings and the smallest size at which tests/test_gpu_strassen_grouped.py sees split updates (nb = 256, floors at 256, n = 1 801 padded to 1 920), per block
    and grouped.  That a split update ran is read off the GEMM flop count: seven products instead of eight per split make it smaller than that of the same fit with
    "strassen_min_rows" = 0 (classical updates only).  logdetcov / sqmahal factor again with split updates, the three columns as rows carried below them."""
    n = 1801
    flops = {}
    for split in (1, 0):
        ctx = _context(agp, nb=256, strassen_min_rows=256 if split else 0, strassen_group=group, strassen_group_min_rows=256, time_kernels=1)
        try:
            if split:
                _scalar_fit(agp, ctx, "f64", n, s2, f"f64,n={n},s2={s2:g},strassen_group={group}")
            else:  # the same three calls, so that the two flop counts cover the same work
                x = ic.gp_inputs(n, "f64")
                y = _targets(x, n)
                fx = agp.GP(agp.SqExponentialKernel(), ctx=ctx)(x, s2)
                agp.posterior(fx, y).data.C.free()
                agp.logdetcov(fx)
                agp.sqmahal(fx, _three_columns(y))
            flops[split] = ctx.timings()["gemm_flops"]
        finally:
            ctx.close()
    assert 0 < flops[1] < flops[0], flops


@pytest.mark.parametrize("n", [320, 1100])
@pytest.mark.parametrize("s2", ic.GP_LEVELS["f32"])
def test_api_single_device_fp32(agp, n, s2):
    """F against the matrix of the fp32 cast of the inputs"""
    ctx = _context(agp)
    try:
        _scalar_fit(agp, ctx, "f32", n, s2, f"f32,n={n},s2={s2:g},defaults")
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["vector", "dense"])
@pytest.mark.parametrize("s2", ic.GP_LEVELS["f64"])
def test_api_noise_forms(agp, s2, form):
    """a noise vector log-uniform in [σ², 100 σ²], and the dense Σy of tests/test_gpu_poisoned_blocks.py scaled so that its smallest eigenvalue is σ²"""
    n = 320
    x = ic.gp_inputs(n, "f64")
    y = _targets(x, n)
    if form == "vector":
        noise = s2 * 100.0 ** np.random.default_rng(3).uniform(0, 1, n)
    else:
        from tests.test_gpu_poisoned_blocks import _dense_sigma

        S = _dense_sigma(n, 3)
        noise = S * (s2 / np.linalg.eigvalsh(S)[0])
        noise = np.ascontiguousarray(0.5 * (noise + noise.T))
    ctx = _context(agp)
    try:
        fx = agp.GP(agp.SqExponentialKernel(), ctx=ctx)(x, noise)
        post = agp.posterior(fx, y)
        _check_fit(agp, post, fx, ic.gp_kernel_ld(x, x) + _noise_ld(noise, n), y, "f64", f"f64,n={n},s2={s2:g},noise={form}")
        post.data.C.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("dib_nb", [2048, 0])
@pytest.mark.parametrize("s2", ic.GP_LEVELS["f64"])
def test_api_sequential_update(agp, s2, dib_nb):
    """posterior(post(x2, σ²), y2) on (300, 77) points: the extended factor against the full matrix of [x1; x2], and its α"""
    n1, n2 = 300, 77
    n = n1 + n2
    xa = ic.gp_inputs(n, "f64")[np.random.default_rng(5).permutation(n)]
    y = _targets(xa, n)
    ctx = _context(agp, dib_nb=dib_nb)
    try:
        f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
        p1 = agp.posterior(f(xa[:n1].copy(), s2), y[:n1])
        p2 = agp.posterior(p1(xa[n1:].copy(), s2), y[n1:])
        _check_fit(agp, p2, None, ic.gp_kernel_ld(xa, xa) + _noise_ld(s2, n), y, "f64", f"f64,n={n1}+{n2},s2={s2:g},dib_nb={dib_nb}", terms=False,
                   segments=(0, n1))  # the new block's leaves start at its own first column
    finally:
        ctx.close()


@pytest.mark.parametrize("s2", ic.GP_LEVELS["f64"])
def test_api_inverse_block_prediction(agp, s2):
    """"dib_nb" = 128 on an n = 320 posterior: the forward solve V = K* L⁻ᵀ of var / cov runs through explicit inverses of 128-column diagonal blocks.  cov against the
    longdouble value from the device's own factor, cov = K** − VVᵀ.  Bound (R carried forward): V̂L̂ᵀ = K* + E with |E| <= γ_n |V̂||L̂|ᵀ + t, so |V̂ − V| <= ΔV :=
    (γ_n |V||L|ᵀ + t) |L⁻ᵀ|, and |côv − cov| <= ΔV|V|ᵀ + |V|ΔVᵀ + γ_{n+2} |V||V|ᵀ + t + u |K**| (the product, the subtraction, the assembly of K**)."""
    n, ns, u, tol = 320, 128, ic.U["f64"], _ktol("f64")
    x = ic.gp_inputs(n, "f64")
    y = _targets(x, n)
    xs = np.random.default_rng(9).uniform(0, 1 / ic.GP_ELL, ns)
    ctx = _context(agp, dib_nb=128)
    try:
        post = agp.posterior(agp.GP(agp.SqExponentialKernel(), ctx=ctx)(x, s2), y)
        L = _factor_of(post, n, "dib")
        cov = np.array(post.cov(xs))
        var = np.array(post.var(xs))
    finally:
        ctx.close()
    Ll = np.tril(L).astype(LD)
    V = ic.solve_lower_ld(Ll, ic.gp_kernel_ld(x, xs)).T  # ns × n
    Kss = ic.gp_kernel_ld(xs, xs)
    ref = Kss - V @ V.T
    V64, L64 = np.abs(V.astype(np.float64)), np.abs(L.astype(np.float64))
    Linv = np.abs(sla.solve_triangular(L.astype(np.float64), np.eye(n), lower=True))
    dV = (ic.gamma(n, u) * (V64 @ L64.T) + tol) @ Linv.T
    bound = dV @ V64.T + V64 @ dV.T + ic.gamma(n + 2, u) * (V64 @ V64.T) + tol + u * np.abs(Kss.astype(np.float64))
    tag = f"f64,n={n},ns={ns},s2={s2:g},dib_nb=128"
    check(f"api_cov[{tag}]", ic._max_ratio(np.abs(cov.astype(LD) - ref), bound.astype(LD)))
    check(f"api_var[{tag}]", ic._max_ratio(np.abs(var.astype(LD) - np.diagonal(ref)), np.diagonal(bound).astype(LD)))


BATCH_N = (1, 65, 128, 320, 1000)


@functools.lru_cache(maxsize=None)
def _batch_reference(n, s2):
    """longdouble factor, α, logpdf and the logpdf bound of one batch problem"""
    u, tol = ic.U["f64"], _ktol("f64")
    x = ic.gp_inputs(n, "f64")
    y = _targets(x, n)
    Cl = ic.gp_kernel_ld(x, x) + _noise_ld(s2, n)
    Ll = ic.cholesky_ld(Cl)
    z = ic.solve_lower_ld(Ll, y.astype(LD)[:, None])
    al = ic.solve_lower_ld(Ll[::-1, ::-1].T, z[::-1])[::-1, 0]  # Lᵀα = z by the same substitution on the reversed system
    lg = np.log(np.diagonal(Ll))
    q = (z * z).sum()
    lp = -(n * np.log(2 * LD(np.pi)) + 2 * lg.sum() + q) / 2
    L64 = np.abs(Ll.astype(np.float64))
    Labs = L64 @ L64.T
    Cinv = np.abs(sla.cho_solve((Ll.astype(np.float64), True), np.eye(n)))
    aa = np.abs(al.astype(np.float64))
    bound = ic.gamma(3 * n + 1, u) * ((Cinv * Labs).sum() + aa @ Labs @ aa) / 2 + tol * (Cinv.sum() + aa.sum() ** 2) / 2 \
        + 4 * u * (n * np.log(2 * np.pi) + 2 * float(np.abs(lg).sum()) + float(q)) / 2
    return dict(x=x, y=y, Cl=Cl, Ll=Ll, alpha=al, lp=lp, bound=float(bound))


def test_api_batch_calls(agp):
    """logpdf_batch(return_alpha=True), mean_and_var_batch and logpdf_and_grad_batch in one call each over n ∈ {1, 65, 128, 320, 1000} × the three fp64 noise levels.
    A on every α with the longdouble factor of C in the bound (the batch returns none).  Each logpdf against the longdouble value under the first-order bound
    γ_{3n+1} (Σ|C⁻¹|∘(|L||L|ᵀ) + |α|ᵀ|L||L|ᵀ|α|) / 2 (logdet and the quadratic form under the backward error of Theorems 10.3 / 10.4), plus the same two sums under the
    assembly tolerance t and 4u on the three terms of the final sum.  That bound is LOOSE — LAPACK sits at 1e-4 of it — and is there to catch gross loss only.  The
    gradient is a forward quantity and is not bounded: its relative difference from logpdf_and_grad on the same problems is printed as GRAD_RELDIFF, not asserted."""
    u, tol = ic.U["f64"], _ktol("f64")
    probs = [(n, s2) for n in BATCH_N for s2 in ic.GP_LEVELS["f64"]]
    refs = [_batch_reference(n, s2) for n, s2 in probs]
    f = agp.GP(agp.SqExponentialKernel())
    fxs = [f(r["x"], s2) for r, (n, s2) in zip(refs, probs)]
    ys = [r["y"] for r in refs]
    xs = [np.linspace(0.1, 3.0, 5) for _ in probs]
    lp_a, alphas = agp.logpdf_batch(fxs, ys, return_alpha=True)
    _, lp_p = agp.mean_and_var_batch(fxs, ys, xs, return_logpdf=True)
    lp_g, grads = agp.logpdf_and_grad_batch(fxs, ys)
    bad = {}
    for i, ((n, s2), r) in enumerate(zip(probs, refs)):
        tag = f"n={n},s2={s2:g}"
        lap = sla.cho_factor(r["Cl"].astype(np.float64), lower=True)
        a_ref = sla.cho_solve(lap, r["y"])
        lp_ref = -0.5 * (n * np.log(2 * np.pi) + 2 * np.log(np.diagonal(lap[0])).sum() + r["y"] @ a_ref)
        report_ref(f"batch_A[{tag}]", ic.measure_A(r["Cl"], r["Ll"], a_ref, r["y"], u, tol)[1])
        report_ref(f"batch_logpdf[{tag}]", float(abs(LD(lp_ref) - r["lp"])) / r["bound"])
        out = {"batch_A": ic.measure_A(r["Cl"], r["Ll"], np.asarray(alphas[i]), r["y"], u, tol)[1]}
        for name, lp in (("batch_logpdf", lp_a[i]), ("batch_predict_logpdf", lp_p[i]), ("batch_grad_logpdf", lp_g[i])):
            out[name] = float(abs(LD(float(lp)) - r["lp"])) / r["bound"]
        for k, v in out.items():
            report(f"{k}[{tag}]", v)
            if not v <= 1.0:
                bad[f"{k}[{tag}]"] = v
        _, g1 = agp.logpdf_and_grad(fxs[i], ys[i])
        for key in ("variance", "noise"):
            a, b = float(np.ravel(grads[i][key])[0]), float(np.ravel(g1[key])[0])
            print(f"GRAD_RELDIFF batch_vs_single_d{key}[{tag}] {abs(a - b) / max(abs(b), 1e-300):.4g}", flush=True)
    assert not bad, bad


@pytest.mark.parametrize("inv", [0, 1])
def test_api_multi_device(agp, inv):
    """2 × 2 virtual ranks, nb = 256, n = 1 100, σ² = 1e-8 (√(1 / σ²) = 1e4: under the guard, so "multi_trsm_inv" = 1 does use −inv(L_kk)): F on the gathered factor, A"""
    n, s2 = 1100, 1e-8
    ctx = agp.Context(devices=rank_devices(4), P=2, Q=2, nb=256)
    try:
        ctx.set_param("multi_trsm_inv", inv)
        _scalar_fit(agp, ctx, "f64", n, s2, f"f64,n={n},s2={s2:g},2x2,multi_trsm_inv={inv}", terms=False,
                    inverse=((16, 256), (256, None)) if inv else LEAF_INVERSES, tiles=0)  # α of the distributed solve: Theorem 10.4 as it stands
    finally:
        ctx.close()
