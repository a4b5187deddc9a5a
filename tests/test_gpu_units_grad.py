"""GPU: the kernels that turn a factorisation into gradients, WITHOUT a factorisation — kgrad_fast_kernel<T, 4|8|16>, kgrad_kernel<T>, kgradx_kernel, noise_grad_kernel
(gpd_grad_contract) and vgrad_fast_kernel<T, 4|8|16, XG>, vgrad_kernel<T, 16, true, XG> (gpd_vgrad), each in fp64 and fp32, on caller-supplied weights.  The API
tests reach them only behind a fit whose conditioning hides anything below 1e-8 (fp64) / 5e-3 (fp32), and never name the output that is wrong.  Three kinds of check:

  exact      all inputs coincide, so κ = 1 exactly and every derivative term is exactly 0: with integer weights that float cannot hold (products of numbers near 2¹²) the
             variance sum, the noise terms and the row sums are integers below 2⁵³ and must EQUAL the reference — an fp32 accumulator, a weight rounded to T before it
             is added, a ½ that is not ½ is a whole-number error.
  one-hot    one non-zero weight: every output is a single term, held to the per-element bound with no summation; everything the weight does not reach must be exactly 0.
             Names a wrong tile map, a lost ½ on the diagonal, a strict-lower pair counted once or twice, a wrong sign.
  dense      random mixed-sign weights against the longdouble reference, |Δ| <= the derived componentwise bound (tests/grad_units_ref.py: reference, derivation, m).
The composite form (gpd_grad_contract_sum: kgrad_sum_kernel, kgradx_sum_kernel) has the exact and the dense check on one kernel with a Periodic, an RQ and a White factor.

Memory the contract (include/gpmi355.h) says is never used holds NaN; outputs beyond their valid range hold a sentinel and must come back bit-identical.  Each bounded
check prints `RATIO <kernel instance> <output> <case> <max error / bound>`; a ratio above 1 is a finding about the kernel, not a tolerance to widen."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import grad_units_ref as R  # noqa: E402
from tests import unit_helpers as uh  # noqa: E402
from tests.unit_helpers import P, SENTINEL  # noqa: E402

VARIANCE = 1.5  # exact in fp32: the kernels take the variance in T
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
NAN = float("nan")
KIND = ["SE", "Matern12", "Matern32", "Matern52"]
TRANSFORM = ["none", "Scale", "ARD"]
D_ALL = [1, 4, 5, 8, 9, 16, 17, 32, 33]  # the instance boundaries (D <= 4 / 8 / 16, the chunked form beyond) and the 16-dimension chunk boundary


@pytest.fixture(scope="module")
def lib(agp):
    return agp._lib.load()


@pytest.fixture(scope="module")
def h(ctx):
    return ctx.handle


def tname(npdt):
    return "f32" if npdt == np.float32 else "f64"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def up128(n):
    return (n + 127) // 128 * 128


def scales(rng, d, tr):
    return [] if tr == 0 else (0.6 + 0.8 * rng.random(1 if tr == 1 else d)).tolist()


def points(rng, d, n, scale, npdt):
    """pre-scaled inputs u = s∘x, dimension-major [d][n] in T: x uniform on [0, √(6/D)]^D as unit_helpers.assemble_problem draws it (κ mid-range for every D)"""
    x = rng.random((d, n)) * np.sqrt(6.0 / d)
    s = np.ones(d) if not scale else (np.full(d, scale[0]) if len(scale) == 1 else np.asarray(scale))
    return (x * s[:, None]).astype(npdt)


def kernel_struct(agp, kind, npdt, scale):
    arr = (C.c_double * max(len(scale), 1))(*scale)
    return agp._lib.gp_kernel(kind, 1 if npdt == np.float32 else 0, VARIANCE, len(scale), arr if scale else None), arr


def hold(inst, output, case, got, out, init=None):
    """one bounded check: got against out.val (+ init) within out.bound (from init), reported and asserted"""
    want = out.val if init is None else out.val + R._wide(init)
    bound = out.bound if init is None else out.bound_from(init)
    rt = R.ratio(R._wide(got) - want, bound)
    uh.report(f"{inst} {output} {case}", rt)
    assert rt <= 1.0, (inst, output, case, rt)


# ---- gpd_grad_contract -----------------------------------------------------------------------------------------------------------------------------------------
def kgrad_instance(npdt, d, ld):
    """the kernel launch_kgrad (csrc/gpmi355.hip) picks — for the labels only"""
    if d <= 16 and (ld * np.dtype(npdt).itemsize) % 16 == 0:
        return f"kgrad_fast_kernel<{tname(npdt)},{4 if d <= 4 else 8 if d <= 8 else 16}>"
    return f"kgrad_kernel<{tname(npdt)}>"


def run_contract(agp, lib, h, npdt, kind, scale, x, ci, alpha, n, want_gx, ld_extra=0, init=None):
    """one gpd_grad_contract call.  x: [d][n], ci: [n][n] (lower used), alpha: [n] — placed in NaN-filled device buffers of the padded shapes.  Returns g, dn, gx as
    NumPy arrays (valid ranges only) after checking that everything beyond them kept its bits.  init: (g, gx) start values; default zeros."""
    from abstractgps_jl_amd._lib import check

    d, npad = x.shape[0], up128(n)
    e = 16 // np.dtype(npdt).itemsize
    ld = npad + e + ld_extra  # production pads the leading dimension too; ld_extra = 1 (f64) / 2 (f32) breaks the 16-byte rows
    Ci = np.full((n, ld), NAN, dtype=npdt)
    Ci[:, :n][np.tril_indices(n)] = ci[np.tril_indices(n)]
    a = np.full(npad, NAN, dtype=npdt)
    a[:n] = alpha
    X = np.full((d, npad), NAN, dtype=npdt)
    X[:, :n] = x
    nsc = len(scale)
    ng = 2 + max(nsc, 1)
    g0 = np.full(ng + 2, SENTINEL)
    g0[:2 + nsc] = 0.0 if init is None else init[0][:2 + nsc]
    gx0 = np.full((d, npad), SENTINEL)
    gx0[:, :n] = 0.0 if init is None else init[1]
    dn0 = np.full(npad, SENTINEL, dtype=npdt)
    Ci_d, a_d, X_d, g_d, dn_d, gx_d = dev(Ci), dev(a), dev(X), dev(g0), dev(dn0), dev(gx0)
    kern, keep = kernel_struct(agp, kind, npdt, scale)
    torch.cuda.synchronize()
    fn = getattr(lib, "gpd_grad_contract" + ("_f32" if npdt == np.float32 else ""))
    check(fn(h, C.byref(kern), P(Ci_d), ld, P(a_d), P(X_d), n, npad, d, P(g_d), P(dn_d), P(gx_d) if want_gx else None))
    uh.sync(lib, h)
    g, dn, gx = g_d.cpu().numpy(), dn_d.cpu().numpy(), gx_d.cpu().numpy()
    assert np.array_equal(g[2 + nsc:].view(np.int64), g0[2 + nsc:].view(np.int64)), "g beyond its 2 + nscale entries changed"
    assert np.array_equal(dn[n:], dn0[n:]), "dn beyond n changed"
    assert np.array_equal(gx[:, n:], gx0[:, n:]), "gx beyond n changed"
    if not want_gx:
        assert np.array_equal(gx, gx0), "gx was written although NULL was passed"
    return g[:2 + nsc], dn[:n], gx[:, :n], ld


def check_contract(agp, lib, h, npdt, kind, tr, d, n, want_gx, rng, case, ld_extra=0, nonzero=False):
    scale = scales(rng, d, tr)
    x = points(rng, d, n, scale, npdt)
    ci = rng.standard_normal((n, n)).astype(npdt)
    alpha = rng.standard_normal(n).astype(npdt)
    ref = R.contract_reference(kind, VARIANCE, len(scale), scale, x, ci, alpha, n, up128(n), want_gx)
    init = (rng.standard_normal(2 + len(scale)), rng.standard_normal((d, n))) if nonzero else None
    g, dn, gx, ld = run_contract(agp, lib, h, npdt, kind, scale, x, ci, alpha, n, want_gx, ld_extra, init)
    inst = kgrad_instance(npdt, d, ld)
    hold(inst, "g[variance]", case, g[0], ref["g0"], None if init is None else init[0][0])
    if scale:
        hold(inst, "g[scale]", case, g[2:], ref["gs"], None if init is None else init[0][2:])
    hold(f"noise_grad_kernel<{tname(npdt)}>", "g[noise]", case, g[1], ref["g1"], None if init is None else init[0][1])
    hold(f"noise_grad_kernel<{tname(npdt)}>", "dn", case, dn, ref["dn"])
    if want_gx:
        hold(f"kgradx_kernel<{tname(npdt)}>", "gx", case, gx, ref["gx"], None if init is None else init[1])
    return g, dn, gx


CONTRACT_N = [1, 127, 128, 129, 300]
# pairwise selection (as tests/vfe_cols_cases.py): every D with every kind, every kind with every transform, every n with every kind; gx with and without
CONTRACT_CASES = [(d, CONTRACT_N[(i + r) % 5], r, (i + r) % 3, (i + r) % 2 == 0) for i, d in enumerate(D_ALL) for r in range(4)]


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,n,kind,tr,want_gx", CONTRACT_CASES, ids=[f"D{d}-n{n}-{KIND[k]}-{TRANSFORM[t]}-{'gx' if x else 'nogx'}" for d, n, k, t, x in CONTRACT_CASES])
def test_grad_contract_dense(agp, lib, h, npdt, d, n, kind, tr, want_gx):
    rng = np.random.default_rng(7 + 1000 * d + 10 * n + kind)
    case = f"D{d}-n{n}-{KIND[kind]}-{TRANSFORM[tr]}"
    check_contract(agp, lib, h, npdt, kind, tr, d, n, want_gx, rng, case)
    if (d + kind) % 2 == 0:  # and once from non-zero outputs: the "+="
        check_contract(agp, lib, h, npdt, kind, tr, d, n, want_gx, rng, case + "-nonzero", nonzero=True)


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,tr", [(5, 2), (16, 1), (3, 0)])
def test_grad_contract_unaligned_leading_dimension(agp, lib, h, npdt, d, tr):
    """a leading dimension whose rows are not 16-byte aligned sends D <= 16 to kgrad_kernel — the branch production's padded ld never takes.  Same inputs, same bound."""
    for extra, want in ((0, "kgrad_fast_kernel"), (1 if npdt == np.float64 else 2, "kgrad_kernel")):
        rng = np.random.default_rng(50 + d)
        e = 16 // np.dtype(npdt).itemsize
        assert kgrad_instance(npdt, d, up128(300) + e + extra).startswith(want)
        check_contract(agp, lib, h, npdt, 3, tr, d, 300, True, rng, f"D{d}-n300-Matern52-{TRANSFORM[tr]}-ld+{extra}", ld_extra=extra)


def one_hot_positions(n):
    return [(0, 0), (77, 77), (127, 126), (128, 127), (128, 0), (n - 1, n - 1), (n - 1, 0)]


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", range(4), ids=KIND)
@pytest.mark.parametrize("n,d", [(129, 3), (300, 3), (129, 8), (129, 16), (129, 20)], ids=["129", "300", "129-D8", "129-D16", "129-D20"])
def test_grad_contract_one_hot(agp, lib, h, npdt, kind, n, d):
    """−C⁻¹ zero except one (i, j), α = 0: g[0] is the single product w κ_ij (½ w on the diagonal), every scale entry a single term, gx non-zero in columns i and j
    only and of opposite sign there; all else exactly 0.  The last probe makes the pair coincide (r = 0): Matern12 must add exactly 0 to scales and inputs, and stay finite.
    D = 3, 8, 16 name kgrad_fast_kernel<T, 4|8|16>, D = 20 kgrad_kernel and the two-chunk kgradx_kernel (the ids of the D = 3 cases are the bare n)."""
    tr = 2
    rng = np.random.default_rng(90 + n + kind + (0 if d == 3 else d))
    scale = scales(rng, d, tr)
    x = points(rng, d, n, scale, npdt)
    alpha = np.zeros(n, dtype=npdt)
    probes = [(p, False) for p in one_hot_positions(n)] + [((128, 127), True)]
    for (i, j), coincide in probes:
        xx = x.copy()
        if coincide:
            xx[:, i] = xx[:, j]
        ci = np.zeros((n, n), dtype=npdt)
        ci[i, j] = npdt(rng.choice([-1, 1]) * (0.5 + rng.random()))
        ref = R.contract_reference(kind, VARIANCE, d, scale, xx, ci, alpha, n, up128(n), True)
        g, dn, gx, ld = run_contract(agp, lib, h, npdt, kind, scale, xx, ci, alpha, n, True)
        inst, case = kgrad_instance(npdt, d, ld), f"{KIND[kind]}-n{n}-({i},{j}){'-r0' if coincide else ''}"
        assert np.isfinite(g).all() and np.isfinite(gx).all() and np.isfinite(dn).all(), (inst, case)
        hold(inst, "g[variance]", case, g[0], ref["g0"])
        hold(inst, "g[scale]", case, g[2:], ref["gs"])
        hold(f"noise_grad_kernel<{tname(npdt)}>", "g[noise]", case, g[1], ref["g1"])
        hold(f"noise_grad_kernel<{tname(npdt)}>", "dn", case, dn, ref["dn"])
        hold(f"kgradx_kernel<{tname(npdt)}>", "gx", case, gx, ref["gx"])
        touched = np.zeros(n, dtype=bool)
        if i != j:
            touched[[i, j]] = True
            assert np.array_equal(gx[:, i], -gx[:, j]), (case, "the two ends of a pair get opposite input gradients")
            assert coincide or (gx[:, i] != 0).all(), (case, "a strict-lower pair must reach the inputs")
        assert not gx[:, ~touched].any(), (case, "gx is non-zero away from rows i and j")
        if i == j or coincide:
            assert not g[2:].any() and not gx.any(), (case, "r = 0 adds exactly 0 to the scales and the inputs")
        assert (dn != 0).sum() == (1 if i == j else 0), (case, "dn sees the diagonal only")


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,n", [(3, 300), (8, 129), (16, 128), (20, 300)])
def test_grad_contract_exact_on_coincident_points(agp, lib, h, npdt, d, n):
    """every input the same point: κ = 1 and d² = 0 exactly for every kind, so g[0] = Σ_{j<=i} (α_i α_j + c_ij)(½ on the diagonal), g[1] = Σ_i ½(α_i² + c_ii) and the
    scale / input sums are exactly 0.  α_i = ±(4090 … 4099) and c_ij = 4097·(−3 … 3): the weights are integers of 25 bits — exact in fp64, not in float; the sums stay
    below 300²·2²⁵ < 2⁴²."""
    rng = np.random.default_rng(n + d)
    alpha = (rng.choice([-1, 1], n) * rng.integers(4090, 4100, n)).astype(npdt)
    ci = (4097 * rng.integers(-3, 4, (n, n))).astype(npdt)
    x = np.repeat(points(rng, d, 1, [], npdt), n, axis=1)
    a, c = alpha.astype(np.int64), np.tril(ci.astype(np.int64))
    w2 = np.tril(np.outer(a, a)) + c                                   # twice the diagonal weight, once the strict-lower one
    want_g0 = float(np.tril(w2, -1).sum()) + float(np.diag(w2).sum()) / 2
    v = (a * a + np.diag(c)) / 2.0                                     # exact in fp64 (26 bits)
    for kind in range(4):
        for tr in (0, 2):
            scale = scales(rng, d, tr)
            g, dn, gx, ld = run_contract(agp, lib, h, npdt, kind, scale, x, ci, alpha, n, True)
            tag = (kgrad_instance(npdt, d, ld), KIND[kind], TRANSFORM[tr], n)
            assert g[0] == want_g0, (tag, "g[variance]", g[0] - want_g0)
            assert g[1] == v.sum(), (f"noise_grad_kernel<{tname(npdt)}>", "g[noise]", g[1] - v.sum())
            assert np.array_equal(dn, v.astype(npdt)), (f"noise_grad_kernel<{tname(npdt)}>", "dn")
            assert not g[2:].any() and not gx.any(), (tag, "coincident points add exactly 0 to the scales and the inputs")


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,n", [(3, 300), (16, 129)])
def test_grad_contract_sum_exact_on_coincident_points(agp, lib, h, npdt, d, n):
    """the composite form (kgrad_sum_kernel once per 16 θ entries, kgradx_sum_kernel) on k = σ₁² Periodic(r) · RQ(α)∘Scale(s) + σ₂² White with every input the same
    point: each factor is exactly 1 (sinpi 0 = 0, log1p 0 = 0, White on equal inputs), so the two variance entries of g are Σ_{j<=i} w_ij exactly, every other θ entry
    (r_p: sinpi² = 0; s: r² = 0; α: q = 0) and gx exactly 0.  Weights as in the single-kind test: 25-bit integers.  D = 16 has 21 θ entries: two launches."""
    from abstractgps_jl_amd._lib import check

    L = agp._lib
    rng = np.random.default_rng(n + d + 1)
    alpha = (rng.choice([-1, 1], n) * rng.integers(4090, 4100, n)).astype(npdt)
    ci = (4097 * rng.integers(-3, 4, (n, n))).astype(npdt)
    a, c = alpha.astype(np.int64), np.tril(ci.astype(np.int64))
    w2 = np.tril(np.outer(a, a)) + c
    want = float(np.tril(w2, -1).sum()) + float(np.diag(w2).sum()) / 2
    v = (a * a + np.diag(c)) / 2.0
    dp = C.POINTER(C.c_double)
    r_p, s_, al = (C.c_double * d)(*(0.7 + rng.random(d))), (C.c_double * 1)(1.3), (C.c_double * 1)(2.5)
    f1 = (L.gp_kfactor * 2)(L.gp_kfactor(4, 0, None, d, C.cast(r_p, dp)), L.gp_kfactor(5, 1, C.cast(s_, dp), 1, C.cast(al, dp)))
    f2 = (L.gp_kfactor * 1)(L.gp_kfactor(6, 0, None, 0, None))
    terms = (L.gp_kterm * 2)(L.gp_kterm(1.5, 2, f1), L.gp_kterm(0.25, 1, f2))
    ks = L.gp_ksum(1 if npdt == np.float32 else 0, 2, terms)
    nth = 1 + d + 2 + 1  # σ₁², r (D), s, α, σ₂²
    npad, e = up128(n), 16 // np.dtype(npdt).itemsize
    ld = npad + e
    Ci = np.full((n, ld), NAN, dtype=npdt)
    Ci[:, :n][np.tril_indices(n)] = ci[np.tril_indices(n)]
    av, X = np.full(npad, NAN, dtype=npdt), np.full((d, npad), NAN, dtype=npdt)
    av[:n] = alpha
    X[:, :n] = np.repeat(points(rng, d, 1, [], npdt), n, axis=1)
    g0 = np.full(2 + nth + 2, SENTINEL)
    g0[1:2 + nth] = 0.0  # g[0] is not touched by the composite form
    gx0 = np.full((d, npad), SENTINEL)
    gx0[:, :n] = 0.0
    Ci_d, a_d, X_d, g_d, dn_d, gx_d = dev(Ci), dev(av), dev(X), dev(g0), dev(np.full(npad, SENTINEL, dtype=npdt)), dev(gx0)
    torch.cuda.synchronize()
    fn = getattr(lib, "gpd_grad_contract_sum" + ("_f32" if npdt == np.float32 else ""))
    check(fn(h, C.byref(ks), P(Ci_d), ld, P(a_d), P(X_d), n, npad, d, P(g_d), P(dn_d), P(gx_d)))
    uh.sync(lib, h)
    g, dn, gx = g_d.cpu().numpy(), dn_d.cpu().numpy(), gx_d.cpu().numpy()
    tag = f"kgrad_sum_kernel<{tname(npdt)},{4 if d <= 4 else 16}>"
    assert g[0] == SENTINEL and np.array_equal(g[2 + nth:], g0[2 + nth:]), (tag, "g[0] or g beyond its 2 + nθ entries changed")
    th = g[2:2 + nth]
    assert th[0] == want and th[nth - 1] == want, (tag, "the two variance entries", th[0] - want, th[nth - 1] - want)
    assert not th[1:nth - 1].any(), (tag, "r_p, s and α get exactly 0 from coincident points", th)
    assert g[1] == v.sum() and np.array_equal(dn[:n], v.astype(npdt)) and np.array_equal(dn[n:], np.full(npad - n, SENTINEL, dtype=npdt)), f"noise_grad_kernel<{tname(npdt)}>"
    assert not gx[:, :n].any() and np.array_equal(gx[:, n:], gx0[:, n:]), (f"kgradx_sum_kernel<{tname(npdt)}>", "gx")


def run_contract_sum(agp, lib, h, npdt, s1, r, s, a, s2, x, ci, alpha, n, init=None):
    """one gpd_grad_contract_sum call for k = σ₁² Periodic(r) · RQ(α)∘Scale(s) + σ₂² White on NaN-padded buffers; returns θ's part of g, g[1], dn, gx (valid ranges)
    after the sentinel checks.  init: (θ start values, gx start values); default zeros."""
    from abstractgps_jl_amd._lib import check

    L = agp._lib
    d, npad, e = x.shape[0], up128(n), 16 // np.dtype(npdt).itemsize
    dp = C.POINTER(C.c_double)
    r_p, s_, al = (C.c_double * d)(*r), (C.c_double * 1)(s), (C.c_double * 1)(a)
    f1 = (L.gp_kfactor * 2)(L.gp_kfactor(4, 0, None, d, C.cast(r_p, dp)), L.gp_kfactor(5, 1, C.cast(s_, dp), 1, C.cast(al, dp)))
    f2 = (L.gp_kfactor * 1)(L.gp_kfactor(6, 0, None, 0, None))
    terms = (L.gp_kterm * 2)(L.gp_kterm(s1, 2, f1), L.gp_kterm(s2, 1, f2))
    ks = L.gp_ksum(1 if npdt == np.float32 else 0, 2, terms)
    nth, ld = d + 4, npad + e
    Ci = np.full((n, ld), NAN, dtype=npdt)
    Ci[:, :n][np.tril_indices(n)] = ci[np.tril_indices(n)]
    av, X = np.full(npad, NAN, dtype=npdt), np.full((d, npad), NAN, dtype=npdt)
    av[:n], X[:, :n] = alpha, x
    g0 = np.full(2 + nth + 2, SENTINEL)
    g0[1] = 0.0
    g0[2:2 + nth] = 0.0 if init is None else init[0]
    gx0 = np.full((d, npad), SENTINEL)
    gx0[:, :n] = 0.0 if init is None else init[1]
    dn0 = np.full(npad, SENTINEL, dtype=npdt)
    Ci_d, a_d, X_d, g_d, dn_d, gx_d = dev(Ci), dev(av), dev(X), dev(g0), dev(dn0), dev(gx0)
    torch.cuda.synchronize()
    fn = getattr(lib, "gpd_grad_contract_sum" + ("_f32" if npdt == np.float32 else ""))
    check(fn(h, C.byref(ks), P(Ci_d), ld, P(a_d), P(X_d), n, npad, d, P(g_d), P(dn_d), P(gx_d)))
    uh.sync(lib, h)
    g, dn, gx = g_d.cpu().numpy(), dn_d.cpu().numpy(), gx_d.cpu().numpy()
    assert g[0] == SENTINEL and np.array_equal(g[2 + nth:], g0[2 + nth:]), "g[0] or g beyond its 2 + nθ entries changed"
    assert np.array_equal(dn[n:], dn0[n:]) and np.array_equal(gx[:, n:], gx0[:, n:]), "dn / gx beyond n changed"
    return g[2:2 + nth], g[1], dn[:n], gx[:, :n]


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,n", [(3, 300), (16, 129), (16, 300), (3, 1)])
def test_grad_contract_sum_dense(agp, lib, h, npdt, d, n):
    """the composite form on random mixed-sign weights against grad_units_ref.composite_reference: every θ entry (σ₁², each r_p, s, α, σ₂²) and gx within the derived
    bound, from zeroed and from non-zero outputs.  D = 16 has 20 θ entries — two launches of kgrad_sum_kernel, the second holding r_15, s, α, σ₂² — so an entry mapped
    to the wrong chunk or slot is a gross error in a named entry.  θ values are exact in fp32 (the device casts θ to T inside the factors); one coincident pair gives
    the White term an off-diagonal contribution."""
    rng = np.random.default_rng(300 + d + n)
    s1, s, a, s2 = 1.5, 1.25, 2.5, 0.25
    r = (0.75 + rng.integers(0, 33, d) / 64.0).tolist()
    x = points(rng, d, n, [], npdt)
    if n > 5:
        x[:, 5] = x[:, 2]
    ci, alpha = rng.standard_normal((n, n)).astype(npdt), rng.standard_normal(n).astype(npdt)
    ref = R.composite_reference(s1, r, s, a, s2, x, ci, alpha, n, up128(n))
    dr = 4 if d <= 4 else 16
    names = ["σ₁²"] + [f"r{p}" for p in range(d)] + ["s", "α", "σ₂²"]
    for init in (None, (rng.standard_normal(d + 4), rng.standard_normal((d, n)))):
        th, g1, dn, gx = run_contract_sum(agp, lib, h, npdt, s1, r, s, a, s2, x, ci, alpha, n, init)
        case = f"D{d}-n{n}" + ("" if init is None else "-nonzero")
        for q, name in enumerate(names):  # entry by entry: the failing θ is named
            one = R.Out(ref["theta"].val[q], ref["theta"].abs[q], ref["theta"].bound[q], ref["theta"].natom)
            hold(f"kgrad_sum_kernel<{tname(npdt)},{dr}>", f"g[{name}]", case, th[q], one, None if init is None else init[0][q])
        hold(f"kgradx_sum_kernel<{tname(npdt)},{dr}>", "gx", case, gx, ref["gx"], None if init is None else init[1])
        hold(f"noise_grad_kernel<{tname(npdt)}>", "g[noise]", case, g1, ref["g1"])
        hold(f"noise_grad_kernel<{tname(npdt)}>", "dn", case, dn, ref["dn"])


# ---- gpd_vgrad -------------------------------------------------------------------------------------------------------------------------------------------------
def vgrad_instance(npdt, d, ldc, xg):
    if d <= 16 and ldc % 2 == 0:
        return f"vgrad_fast_kernel<{tname(npdt)},{4 if d <= 4 else 8 if d <= 8 else 16},XG={int(xg)}>"
    return f"vgrad_kernel<{tname(npdt)},16,true,XG={int(xg)}>"


def run_vgrad(agp, lib, h, npdt, kind, scale, xr, xc, cm, explicit_w, rs, bv, nu, zfac, want_gx, want_rows, ld_extra=0, init=None):
    """one gpd_vgrad call on NaN-padded device buffers; returns g, gz, gx, rowq, rowp (valid ranges) after the sentinel checks.  init: dict of start values."""
    from abstractgps_jl_amd._lib import check

    d, nr, nc = xr.shape[0], xr.shape[1], xc.shape[1]
    nrp, ncp = up128(nr), up128(nc)
    ldc = ncp + 2 + ld_extra
    Cm = np.full((nr, ldc), NAN, dtype=npdt)
    Cm[:, :nc] = cm
    Xr, Xc = np.full((d, nrp), NAN, dtype=npdt), np.full((d, ncp), NAN, dtype=npdt)
    Xr[:, :nr], Xc[:, :nc] = xr, xc
    pad = lambda v, n, m, t: np.concatenate([np.asarray(v, dtype=t), np.full(m - n, NAN, dtype=t)])  # noqa: E731
    nsc = len(scale)
    init = init or {}
    g0 = np.full(2 + max(nsc, 1) + 2, SENTINEL)
    g0[0] = init.get("g", np.zeros(2 + nsc))[0]
    g0[2:2 + nsc] = init.get("g", np.zeros(2 + nsc))[2:]
    gz0, gx0 = np.full((d, ncp), SENTINEL), np.full((d, nrp), SENTINEL)
    gz0[:, :nc], gx0[:, :nr] = init.get("gz", 0.0), init.get("gx", 0.0)
    rq0, rp0 = np.full(nrp, SENTINEL), np.full(nrp, SENTINEL)
    rq0[:nr], rp0[:nr] = init.get("rowq", 0.0), init.get("rowp", 0.0)
    bufs = [dev(a) for a in (Cm, Xr, Xc, g0, gz0, gx0, rq0, rp0)]
    Cm_d, Xr_d, Xc_d, g_d, gz_d, gx_d, rq_d, rp_d = bufs
    if explicit_w:
        rs_d = bv_d = nu_d = None
    else:
        rs_d, bv_d, nu_d = dev(pad(rs, nr, nrp, npdt)), dev(pad(bv, nr, nrp, npdt)), dev(pad(nu, nc, ncp, np.float64))
    kern, keep = kernel_struct(agp, kind, npdt, scale)
    torch.cuda.synchronize()
    fn = getattr(lib, "gpd_vgrad" + ("_f32" if npdt == np.float32 else ""))
    opt = lambda t, on: P(t) if on and t is not None else None  # noqa: E731
    check(fn(h, P(Cm_d), ldc, explicit_w, P(Xr_d), nrp, P(Xc_d), ncp, d, C.byref(kern), opt(rs_d, True), opt(bv_d, True), opt(nu_d, True), nr, nc, P(g_d), P(gz_d), ncp,
             zfac, opt(rq_d, want_rows), opt(rp_d, want_rows), opt(gx_d, want_gx), nrp))
    uh.sync(lib, h)
    g, gz, gx, rq, rp = (t.cpu().numpy() for t in (g_d, gz_d, gx_d, rq_d, rp_d))
    assert g[1] == SENTINEL and np.array_equal(g[2 + nsc:], g0[2 + nsc:]), "g[1] or g beyond its entries changed"
    assert np.array_equal(gz[:, nc:], gz0[:, nc:]) and np.array_equal(gx[:, nr:], gx0[:, nr:]), "gz / gx beyond nc / nr changed"
    assert np.array_equal(rq[nr:], rq0[nr:]) and np.array_equal(rp[nr:], rp0[nr:]), "rowq / rowp beyond nr changed"
    if not want_gx:
        assert np.array_equal(gx, gx0), "gx was written although NULL was passed"
    if not want_rows or explicit_w:
        assert np.array_equal(rq, rq0) and np.array_equal(rp, rp0), "rowq / rowp written although not asked for"
    return g[:2 + nsc], gz[:, :nc], gx[:, :nr], rq[:nr], rp[:nr], ldc


def check_vgrad(agp, lib, h, npdt, kind, tr, d, nr, nc, explicit_w, want_gx, rng, case, ld_extra=0, nonzero=False):
    scale = scales(rng, d, tr)
    xr, xc = points(rng, d, nr, scale, npdt), points(rng, d, nc, scale, npdt)
    cm = rng.standard_normal((nr, nc)).astype(npdt)
    rs, bv, nu = (0.5 + rng.random(nr)).astype(npdt), rng.standard_normal(nr).astype(npdt), rng.standard_normal(nc)
    zfac = 2.0 if explicit_w else 1.0
    ref = R.rect_reference(kind, VARIANCE, len(scale), scale, xr, xc, cm, explicit_w, rs, bv, nu, nr, nc, zfac, want_gx)
    init = None
    if nonzero:
        init = {"g": rng.standard_normal(2 + len(scale)), "gz": rng.standard_normal((d, nc)), "gx": rng.standard_normal((d, nr)), "rowq": rng.standard_normal(nr),
                "rowp": rng.standard_normal(nr)}
    g, gz, gx, rq, rp, ldc = run_vgrad(agp, lib, h, npdt, kind, scale, xr, xc, cm, explicit_w, rs, bv, nu, zfac, want_gx, True, ld_extra, init)
    inst = vgrad_instance(npdt, d, ldc, want_gx)
    case += f"-w{explicit_w}"
    i0 = (lambda k: None) if init is None else (lambda k: init[k])  # noqa: E731
    hold(inst, "g[variance]", case, g[0], ref["g0"], None if init is None else init["g"][0])
    if scale:
        hold(inst, "g[scale]", case, g[2:], ref["gs"], None if init is None else init["g"][2:])
    hold(inst, "gz", case, gz, ref["gz"], i0("gz"))
    if want_gx:
        hold(inst, "gx", case, gx, ref["gx"], i0("gx"))
    if not explicit_w:
        hold(inst, "rowq", case, rq, ref["rowq"], i0("rowq"))
        hold(inst, "rowp", case, rp, ref["rowp"], i0("rowp"))


VGRAD_SHAPES = [(128, 128), (300, 129), (257, 1)]
VGRAD_CASES = [(d, VGRAD_SHAPES[(i + r) % 3], r, (i + 2 * r) % 3, (i + r) % 2, ((i + r) // 2) % 2 == 0) for i, d in enumerate(D_ALL) for r in range(4)]


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,shape,kind,tr,explicit_w,want_gx", VGRAD_CASES,
                         ids=[f"D{d}-{s[0]}x{s[1]}-{KIND[k]}-{TRANSFORM[t]}-w{w}-{'gx' if x else 'nogx'}" for d, s, k, t, w, x in VGRAD_CASES])
def test_vgrad_dense(agp, lib, h, npdt, d, shape, kind, tr, explicit_w, want_gx):
    rng = np.random.default_rng(11 + 1000 * d + shape[0] + kind)
    case = f"D{d}-{shape[0]}x{shape[1]}-{KIND[kind]}-{TRANSFORM[tr]}"
    check_vgrad(agp, lib, h, npdt, kind, tr, d, shape[0], shape[1], explicit_w, want_gx, rng, case)
    if (d + kind) % 2 == 1:
        check_vgrad(agp, lib, h, npdt, kind, tr, d, shape[0], shape[1], explicit_w, want_gx, rng, case + "-nonzero", nonzero=True)


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,tr,explicit_w", [(5, 2, 0), (16, 1, 1), (3, 0, 0)])
def test_vgrad_unaligned_leading_dimension(agp, lib, h, npdt, d, tr, explicit_w):
    """an odd ldc sends D <= 16 to vgrad_kernel — the branch production's even ld never takes.  Same inputs, same bound."""
    for extra, want in ((0, "vgrad_fast_kernel"), (1, "vgrad_kernel")):
        rng = np.random.default_rng(60 + d)
        assert vgrad_instance(npdt, d, up128(129) + 2 + extra, True).startswith(want)
        check_vgrad(agp, lib, h, npdt, 2, tr, d, 300, 129, explicit_w, True, rng, f"D{d}-300x129-Matern32-{TRANSFORM[tr]}-ldc+{extra}", ld_extra=extra)


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", range(4), ids=KIND)
@pytest.mark.parametrize("explicit_w,d", [(0, 3), (1, 3), (0, 8), (1, 16), (0, 20)], ids=["0", "1", "0-D8", "1-D16", "0-D20"])
def test_vgrad_one_hot(agp, lib, h, npdt, kind, explicit_w, d):
    """the weights of a 300 × 129 rectangle zero except one (i, j) (explicit_w = 0: cm one-hot and b = 0, so W_ij = −2 rs_i cm_ij there and 0 elsewhere): g[0] a single
    product, gz non-zero in column j only, gx in row i only, opposite in sign; rowq in row i only.  The last probe makes row i and column j coincide (r = 0)."""
    tr, nr, nc = 2, 300, 129  # (D = 8, 16, 20: vgrad_fast_kernel<T, 8|16> and vgrad_kernel; the ids of the D = 3 cases are the bare explicit_w)
    rng = np.random.default_rng(190 + kind + explicit_w + (0 if d == 3 else d))
    scale = scales(rng, d, tr)
    xr, xc = points(rng, d, nr, scale, npdt), points(rng, d, nc, scale, npdt)
    rs, bv, nu = (0.5 + rng.random(nr)).astype(npdt), np.zeros(nr, dtype=npdt), rng.standard_normal(nc)
    probes = [(p, False) for p in [(0, 0), (77, 77), (127, 126), (128, 127), (128, 0), (nr - 1, nc - 1), (nr - 1, 0), (0, nc - 1)]] + [((128, 127), True)]
    for (i, j), coincide in probes:
        xcc = xc.copy()
        if coincide:
            xcc[:, j] = xr[:, i]
        cm = np.zeros((nr, nc), dtype=npdt)
        cm[i, j] = npdt(rng.choice([-1, 1]) * (0.5 + rng.random()))
        ref = R.rect_reference(kind, VARIANCE, d, scale, xr, xcc, cm, explicit_w, rs, bv, nu, nr, nc, 1.0, True)
        g, gz, gx, rq, rp, ldc = run_vgrad(agp, lib, h, npdt, kind, scale, xr, xcc, cm, explicit_w, rs, bv, nu, 1.0, True, True)
        inst, case = vgrad_instance(npdt, d, ldc, True), f"{KIND[kind]}-w{explicit_w}-({i},{j}){'-r0' if coincide else ''}"
        assert all(np.isfinite(a).all() for a in (g, gz, gx, rq, rp)), (inst, case)
        hold(inst, "g[variance]", case, g[0], ref["g0"])
        hold(inst, "g[scale]", case, g[2:], ref["gs"])
        hold(inst, "gz", case, gz, ref["gz"])
        hold(inst, "gx", case, gx, ref["gx"])
        assert np.array_equal(gz[:, j], -gx[:, i]), (case, "row input and column input get opposite gradients")
        assert coincide or ((gz[:, j] != 0).all() and g[0] != 0), (case, "the weight must reach its outputs")
        assert not np.delete(gz, j, axis=1).any() and not np.delete(gx, i, axis=1).any(), (case, "gz / gx non-zero away from column j / row i")
        if coincide:
            assert not g[2:].any() and not gz.any() and not gx.any(), (case, "r = 0 adds exactly 0 to the scales and the inputs")
        if not explicit_w:
            hold(inst, "rowq", case, rq, ref["rowq"])
            assert rq[i] != 0 and not np.delete(rq, i).any(), (case, "rowq is non-zero in row i only")
            hold(inst, "rowp", case, rp, ref["rowp"])  # ν is dense: every row has its sum, whatever the weights are


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,shape", [(3, (300, 129)), (8, (128, 128)), (16, (257, 1)), (20, (300, 129))])
def test_vgrad_exact_on_coincident_points(agp, lib, h, npdt, d, shape):
    """every row and column input the same point: κ = 1 exactly, so g[0] = Σ W_ij, rowq[i] = −σ² Σ_j cm_ij, rowp[i] = σ² Σ_j ν_j, and scales / gz / gx are exactly 0.
    rs_i = 4097·(±1 … 3), cm_ij = 4099·(−3 … 3), b and ν small integers: W_ij = rs_i (−2 cm_ij + b_i ν_j) is an integer of up to 29 bits whose product term float
    cannot hold; all sums stay below 2⁵³ (σ² = 1.5 keeps the row sums exact)."""
    nr, nc = shape
    rng = np.random.default_rng(nr + nc + d)
    rs = (4097 * rng.choice([-3, -2, -1, 1, 2, 3], nr)).astype(npdt)
    bv = rng.integers(-3, 4, nr).astype(npdt)
    nu = rng.integers(-3, 4, nc).astype(np.float64)
    cm = (4099 * rng.integers(-3, 4, (nr, nc))).astype(npdt)
    pt = points(rng, d, 1, [], npdt)
    xr, xc = np.repeat(pt, nr, axis=1), np.repeat(pt, nc, axis=1)
    c64 = cm.astype(np.float64)
    W = rs.astype(np.float64)[:, None] * (-2 * c64 + bv.astype(np.float64)[:, None] * nu[None, :])
    for kind in range(4):
        for explicit_w in (0, 1):
            g, gz, gx, rq, rp, ldc = run_vgrad(agp, lib, h, npdt, kind, [], xr, xc, cm, explicit_w, rs, bv, nu, 1.0, True, True)
            tag = (vgrad_instance(npdt, d, ldc, True), KIND[kind], explicit_w, shape)
            want = c64.sum() if explicit_w else W.sum()
            assert g[0] == want, (tag, "g[variance]", g[0] - want)
            assert not gz.any() and not gx.any(), (tag, "coincident points add exactly 0 to the inputs")
            if not explicit_w:
                assert np.array_equal(rq, -VARIANCE * c64.sum(1)), (tag, "rowq")
                assert np.array_equal(rp, np.full(nr, VARIANCE * nu.sum())), (tag, "rowp")
