"""GPU: the kernels every prediction passes through, WITHOUT a fit in front — kvec_kernel / kvec_sum_kernel (gpd_kvec), kmul_kernel / kmul_sum_kernel /
kmul_reduce_kernel (gpd_kmul) and kpgrad_kernel / kpgrad_sum_kernel (gpd_kpgrad), each in fp64 and fp32, on caller-supplied weights.  The API tests reach them only
behind weights alpha = C⁻¹(y − m) whose conditioning hides anything below 1e-8 (fp64) / 1e-3 (fp32).  Four kinds of check:

  exact      every input the same point (κ = 1 in every kind), a power-of-two variance, integer weights: out must EQUAL variance·Σα — strip masks, split bookkeeping,
             reduce order, columns that never mix (column c = (c + 1) × a base vector), an fp32 accumulator where fp64 is documented; sentinels outside the outputs.
  one-hot    alpha = e_i in column c: out[c][·] = k(·, x_i) within the per-element bound, every other column exactly 0 — the A / B fragment lane maps of kmul_body.
  dense      random mixed-sign weights against the longdouble reference, |Δ| <= the derived componentwise bound (tests/predict_units_ref.py: derivation and counts).
  contract   memory the header (include/gpmi355.h) says is not read or never used holds NaN — and the bits equal a run with zeros there; two calls give the same bits;
             a column's bits do not depend on S or on the other columns; "cols_kernel_splits" is what the split rule gives for (n, ns).
Each bounded check prints `RATIO <kernel> <output> <case> <max error / bound>`; a ratio above 1 is a finding about the kernel, not a tolerance to widen."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import predict_units_ref as R  # noqa: E402
from tests import unit_helpers as uh  # noqa: E402
from tests.test_gpu_units_grad import DTYPES, IDS, KIND, NAN, TRANSFORM, dev, hold, points, scales, tname, up128  # noqa: E402
from tests.unit_helpers import P, SENTINEL  # noqa: E402

VARIANCE = 1.5
COMP = dict(s1=1.5, s=1.25, a=2.5, s2=0.25)  # σ₁²·Periodic(r)·RQ(α)∘Scale(s) + σ₂²·White, every θ exact in fp32


@pytest.fixture(scope="module")
def lib(agp):
    return agp._lib.load()


@pytest.fixture(scope="module")
def h(ctx):
    return ctx.handle


class Kern:
    """a single kind (`scale`: the list the inputs were pre-scaled with — read by gpd_kpgrad alone) or the composite kernel of COMP with periods r; keeps its arrays alive"""

    def __init__(self, agp, npdt, kind=None, variance=VARIANCE, scale=(), r=None, s1=COMP["s1"], s2=COMP["s2"]):
        L, dt = agp._lib, 1 if npdt == np.float32 else 0
        self.sum, self.kind, self.variance, self.scale, self.r, self.s1, self.s2 = r is not None, kind, variance, list(scale), r, s1, s2
        dp = C.POINTER(C.c_double)
        if self.sum:
            d = len(r)
            self._a = [(C.c_double * d)(*r), (C.c_double * 1)(COMP["s"]), (C.c_double * 1)(COMP["a"])]
            self._f1 = (L.gp_kfactor * 2)(L.gp_kfactor(4, 0, None, d, C.cast(self._a[0], dp)), L.gp_kfactor(5, 1, C.cast(self._a[1], dp), 1, C.cast(self._a[2], dp)))
            self._f2 = (L.gp_kfactor * 1)(L.gp_kfactor(6, 0, None, 0, None))
            self._t = (L.gp_kterm * 2)(L.gp_kterm(s1, 2, self._f1), L.gp_kterm(s2, 1, self._f2))
            self.c = L.gp_ksum(dt, 2, self._t)
        else:
            self._a = (C.c_double * max(len(self.scale), 1))(*self.scale)
            self.c = L.gp_kernel(kind, dt, variance, len(self.scale), self._a if self.scale else None)

    def fn(self, lib, name, npdt):
        return getattr(lib, f"gpd_{name}{'_sum' if self.sum else ''}{'_f32' if npdt == np.float32 else ''}")

    def elements(self, xs, x):
        if self.sum:
            return R.composite_elements(self.s1, self.r, COMP["s"], COMP["a"], self.s2, xs, x)
        return R.kind_elements(self.kind, self.variance, len(self.scale), self.scale, xs, x)

    def label(self, d):
        return f"sum<{1 if d <= 1 else 4 if d <= 4 else 16}>" if self.sum else KIND[self.kind]


def periods(rng, d):
    return (0.75 + rng.integers(0, 33, d) / 64.0).tolist()


def padded(a, shape, fill, npdt):
    """a in the top-left corner of an array of `shape` otherwise holding `fill`"""
    out = np.full(shape, fill, dtype=npdt)
    out[tuple(slice(0, s) for s in a.shape)] = a
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    it = np.int32 if a.dtype == np.float32 else np.int64
    return a.dtype == b.dtype and np.array_equal(a.view(it), b.view(it))


def counter(lib, h, name):
    from abstractgps_jl_amd._lib import check

    v = C.c_int64()
    check(lib.gp_ctx_get_param(h, name.encode(), C.byref(v)))
    return v.value


def run_kvec(lib, h, npdt, kern, xs, x, alpha, fill=NAN):
    """gpd_kvec on buffers whose columns beyond ns / n hold `fill`; out beyond ns keeps its sentinel.  Returns out[:ns]."""
    from abstractgps_jl_amd._lib import check

    (d, ns), n = xs.shape, x.shape[1]
    ldxs, ldx = ns + 5, n + 3
    XS, X, A = dev(padded(xs, (d, ldxs), fill, npdt)), dev(padded(x, (d, ldx), fill, npdt)), dev(padded(alpha, (n + 6,), fill, npdt))
    out0 = np.full(ns + 4, SENTINEL, dtype=npdt)
    out = dev(out0)
    torch.cuda.synchronize()
    check(kern.fn(lib, "kvec", npdt)(h, C.byref(kern.c), P(XS), ldxs, ns, P(X), ldx, n, d, P(A), P(out)))
    uh.sync(lib, h)
    o = out.cpu().numpy()
    assert np.array_equal(o[ns:], out0[ns:]), "out beyond ns changed"
    return o[:ns]


def run_kmul(lib, h, npdt, kern, xs, x, alpha, fill=NAN):
    """gpd_kmul: xs padded to a multiple of 128 points, x / alpha columns beyond n, xs columns beyond ns hold `fill`; rows >= S and columns >= ns of out keep their
    sentinel.  Returns (out[:S, :ns], cols_kernel_splits after the call, the growth of cols_kernel_calls)."""
    from abstractgps_jl_amd._lib import check

    (d, ns), n, S = xs.shape, x.shape[1], alpha.shape[0]
    ldxs, ldx, lda, ldo = up128(ns), n + 3, n + 5, ns + 7
    XS, X, A = dev(padded(xs, (d, ldxs), fill, npdt)), dev(padded(x, (d, ldx), fill, npdt)), dev(padded(alpha, (S, lda), fill, npdt))
    out0 = np.full((S + 2, ldo), SENTINEL, dtype=npdt)
    out = dev(out0)
    calls = counter(lib, h, "cols_kernel_calls")
    torch.cuda.synchronize()
    check(kern.fn(lib, "kmul", npdt)(h, C.byref(kern.c), P(XS), ldxs, ns, P(X), ldx, n, d, P(A), lda, S, P(out), ldo))
    uh.sync(lib, h)
    o = out.cpu().numpy()
    assert np.array_equal(o[S:], out0[S:]) and np.array_equal(o[:, ns:], out0[:, ns:]), "out rows >= S or columns >= ns changed"
    return o[:S, :ns], counter(lib, h, "cols_kernel_splits"), counter(lib, h, "cols_kernel_calls") - calls


def run_kpgrad(lib, h, npdt, kern, xs, x, alpha, W, j0, cnt, want_gm=True, want_gv=True, fill=NAN):
    """gpd_kpgrad for the test points [j0, j0 + cnt) of xs ([d][ns]); W: [cnt][n].  ldw > n, ldg > ns; W columns beyond n hold `fill`.  Returns gm, gv ([d][cnt]; None
    when not asked for) after checking that nothing outside columns [j0, j0 + cnt) — and no output passed as NULL — was written."""
    from abstractgps_jl_amd._lib import check

    (d, ns), n = xs.shape, x.shape[1]
    assert 0 <= j0 and j0 + cnt <= ns and W.shape == (cnt, n)
    ldxs, ldx, ldw, ldg = ns + 3, n + 3, n + 5, ns + 4
    XS, X, A = dev(padded(xs, (d, ldxs), fill, npdt)), dev(padded(x, (d, ldx), fill, npdt)), dev(padded(alpha, (n + 6,), fill, npdt))
    Wd = dev(padded(W, (cnt, ldw), fill, npdt))
    g0 = np.full((d, ldg), SENTINEL)
    gm, gv = dev(g0), dev(g0)
    torch.cuda.synchronize()
    check(kern.fn(lib, "kpgrad", npdt)(h, C.byref(kern.c), P(XS), ldxs, P(X), ldx, n, d, P(A) if want_gm else None, P(Wd) if want_gv else None, ldw if want_gv else 0,
                                       P(gm) if want_gm else None, P(gv) if want_gv else None, ldg, j0, cnt))
    uh.sync(lib, h)
    res = []
    for g, want in ((gm, want_gm), (gv, want_gv)):
        o = g.cpu().numpy()
        outside = np.ones(ldg, dtype=bool)
        outside[j0:j0 + cnt] = not want
        assert np.array_equal(o[:, outside], g0[:, outside]), "an entry outside columns [j0, j0 + cnt), or an output passed as NULL, was written"
        res.append(o[:, j0:j0 + cnt] if want else None)
    return res


def coincident(rng, d, ns, n, npdt):
    pt = points(rng, d, 1, [], npdt)
    return np.repeat(pt, ns, axis=1), np.repeat(pt, n, axis=1)


def all_kernels(agp, npdt, rng, d, variance=2.0):
    """the four kinds and — D <= 16 — the composite kernel with σ₁² + σ₂² = 2 (1.5·1·1 + 0.5: exact); on coincident inputs every one of them is exactly 2"""
    ks = [Kern(agp, npdt, kind=k, variance=variance) for k in range(4)]
    return ks + ([Kern(agp, npdt, r=periods(rng, d), s1=1.5, s2=0.5)] if d <= 16 else [])


# ---- exact ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,ns,d", [(1, 1, 1), (255, 3, 4), (256, 2, 5), (257, 65, 16), (416, 3, 20)])
def test_kvec_exact_on_coincident_points(agp, lib, h, npdt, n, ns, d):
    """out[j] = 2·Σα exactly: the terms 2·α_i are integers as wide as T holds (25 bits in fp32, 26 in fp64) and the partial sums wider still — exact in the documented
    fp64 accumulator, rounded by a float one — while the total is small enough for T to hold exactly"""
    rng = np.random.default_rng(n + ns + d)
    bitsw = 23 if npdt == np.float32 else 24
    big = (rng.choice([-1, 1], n // 2) * (2 ** bitsw + 2 * rng.integers(0, 2 ** (bitsw - 1) - 8, n // 2) + 1)).astype(np.int64)
    # every large weight has a partner of the opposite sign a few units away, at a random place: the partial sums are as wide as the weights, the total is small —
    # T holds it exactly, so whatever an accumulator narrower than fp64 lost on the way is still there at the end
    alpha = rng.permutation(np.concatenate([big, 2 * rng.integers(-3, 4, n // 2) - big, 1 + 2 * rng.integers(0, 9, n % 2)]))
    assert len(alpha) == n and np.array_equal(alpha.astype(npdt).astype(np.int64), alpha) and abs(2 * alpha.sum()) < 2 ** 24
    want = npdt(2.0 * float(alpha.sum()))  # one rounding to T
    xs, x = coincident(rng, d, ns, n, npdt)
    for kern in all_kernels(agp, npdt, rng, d):
        out = run_kvec(lib, h, npdt, kern, xs, x, alpha.astype(npdt))
        assert np.array_equal(out, np.full(ns, want)), (kern.label(d), tname(npdt), out[0] - want)


EXACT_KMUL = [(1, 1, 1, 1), (31, 63, 15, 4), (32, 64, 16, 5), (33, 65, 17, 16), (225, 1, 128, 4), (288, 65, 17, 16), (300, 200, 1, 2), (400, 3, 128, 5),
              (416, 64, 16, 1), (129, 3, 2, 20)]


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,ns,S,d", EXACT_KMUL)
def test_kmul_exact_on_coincident_points(agp, lib, h, npdt, n, ns, S, d):
    """out[c][j] = 2·(c + 1)·Σ base exactly, for every strip count, split and column block: fp64 with 25-bit bases; fp32 — whose MFMA accumulates in fp32 by design —
    with bases in [−3, 3], so that every partial sum stays below 2·128·3·416 < 2²⁴.  Rows >= S and columns >= ns keep their sentinel (run_kmul)."""
    rng = np.random.default_rng(n + ns + S + d)
    base = rng.integers(-3, 4, n) if npdt == np.float32 else rng.choice([-1, 1], n) * (2 ** 24 + rng.integers(0, 2 ** 24, n))
    alpha = (np.arange(1, S + 1)[:, None] * base[None, :]).astype(np.int64)
    want = np.repeat((2 * alpha.sum(1))[:, None], ns, axis=1)
    xs, x = coincident(rng, d, ns, n, npdt)
    nsplit = R.kmul_split(n, ns)[0]
    for kern in all_kernels(agp, npdt, rng, d):
        out, splits, calls = run_kmul(lib, h, npdt, kern, xs, x, alpha.astype(npdt))
        assert np.array_equal(out.astype(np.float64), want.astype(np.float64)), (kern.label(d), tname(npdt), np.abs(out - want).max())
        if d <= 16:
            assert (splits, calls) == (nsplit, 1), (kern.label(d), splits, nsplit, calls)
        else:
            assert calls == 0, "the kvec loop of a single kind with D > 16 does not count as a kmul launch"


@pytest.mark.parametrize("n,ns,nsplit", [(224, 1, 1), (225, 1, 2), (288, 64, 2), (300, 65, 2), (400, 200, 3)])
def test_the_split_rule_is_the_documented_one(n, ns, nsplit):
    """2 × 4 strips at n = 225 (the smallest that splits), 5 + 4 at 288, 5 + 5 at 300, 5 + 5 + 3 at 400 — what the exact and dense tests assert the ctx counter against"""
    assert R.kmul_split(n, ns)[0] == nsplit


# ---- one-hot ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("which,n,d", [(0, 33, 3), (1, 300, 3), (2, 33, 16), (3, 300, 5), ("sum", 33, 4), ("sum", 300, 16)])
def test_kmul_one_hot(agp, lib, h, npdt, which, n, d):
    """alpha = e_i in column c for i at the strip edges (0, 31, 32, n − 1) and c at the MFMA column-block edges (0, 15, 16, S − 1), every (i, c) pair over four
    launches: out[c][·] = k(·, x_i) to the per-element bound alone, every other column exactly 0"""
    S, ns = 21, 70
    rng = np.random.default_rng(600 + n + d)
    kern = Kern(agp, npdt, r=periods(rng, d)) if which == "sum" else Kern(agp, npdt, kind=which)
    xs, x = points(rng, d, ns, [], npdt), points(rng, d, n, [], npdt)
    el = kern.elements(xs, x)
    rows, cols = [0, 31, 32, n - 1], [0, 15, 16, S - 1]
    for rot in range(4):
        alpha = np.zeros((S, n), dtype=npdt)
        for q, c in enumerate(cols):
            alpha[c, rows[(q + rot) % 4]] = 1
        ref = R.kmul_reference(el, alpha, n, ns, npdt)
        out, _, _ = run_kmul(lib, h, npdt, kern, xs, x, alpha)
        hold(f"kmul<{tname(npdt)}>", "one-hot", f"{kern.label(d)}-n{n}-D{d}-rot{rot}", out, ref)
        assert not np.delete(out, cols, axis=0).any() and (out[cols] != 0).all()


# ---- dense ------------------------------------------------------------------------------------------------------------------------------------------------------
N_ALL, NS_ALL, S_ALL, D_ALL = [1, 31, 32, 33, 129, 225, 300, 400], [1, 63, 64, 65, 200], [1, 15, 16, 17, 128], [1, 4, 5, 16]
# pairwise selection: every n with every kind, every D and every transform with every kind; ns and S cycle against n at different strides
DENSE = [(n, NS_ALL[(i + r) % 5], S_ALL[(i + 2 * r) % 5], r, D_ALL[(i + r) % 4], (i + r) % 3) for i, n in enumerate(N_ALL) for r in range(4)]
DENSE += [(300, 3, 3, 2, 17, 2), (129, 65, 2, 1, 20, 1)]  # D > 16: kvec_kernel, and kmul's per-column kvec loop
DENSE_SUM = [(33, 1, 1, 1), (225, 63, 15, 2), (129, 64, 16, 4), (300, 65, 17, 5), (400, 200, 128, 16)]


def check_kvec_kmul(lib, h, npdt, kern, xs, x, rng, S):
    """kvec on column 0's weights and kmul on all S columns against the reference; each twice (same bits)"""
    (d, ns), n = xs.shape, x.shape[1]
    alpha = rng.standard_normal((S, n)).astype(npdt)
    el = kern.elements(xs, x)
    tag = f"{kern.label(d)}-n{n}-ns{ns}-S{S}-D{d}"
    out = run_kvec(lib, h, npdt, kern, xs, x, alpha[0])
    hold(f"kvec<{tname(npdt)}>", "out", tag, out, R.kvec_reference(el, alpha[0], npdt))
    assert same_bits(out, run_kvec(lib, h, npdt, kern, xs, x, alpha[0])), "kvec: two calls, two results"
    om, splits, calls = run_kmul(lib, h, npdt, kern, xs, x, alpha)
    single_hi_d = not kern.sum and d > 16
    ref = R.kmul_reference(el, alpha, n, ns, npdt)
    if single_hi_d:  # S kvec launches: kvec's bound, column by column
        per = [R.kvec_reference(el, alpha[c], npdt) for c in range(S)]
        ref = R.Out(np.stack([o.val for o in per]), np.stack([o.abs for o in per]), np.stack([o.bound for o in per]), 0)
        assert calls == 0
    else:
        assert (splits, calls) == (R.kmul_split(n, ns)[0], 1), (tag, splits, calls)
    hold(f"kmul<{tname(npdt)}>", "out", tag, om, ref)
    om2, _, _ = run_kmul(lib, h, npdt, kern, xs, x, alpha)
    assert same_bits(om, om2), "kmul: two calls, two results"
    return alpha, om


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,ns,S,kind,d,tr", DENSE, ids=[f"n{n}-ns{ns}-S{S}-{KIND[k]}-D{d}-{TRANSFORM[t]}" for n, ns, S, k, d, t in DENSE])
def test_kvec_kmul_dense(agp, lib, h, npdt, n, ns, S, kind, d, tr):
    rng = np.random.default_rng(11 + 1000 * d + 10 * n + kind + ns)
    scale = scales(rng, d, tr)
    xs, x = points(rng, d, ns, scale, npdt), points(rng, d, n, scale, npdt)
    xs[:, ns // 2] = x[:, n // 2]  # a test point on a training point (Matern12 at r = 0: κ = 1)
    check_kvec_kmul(lib, h, npdt, Kern(agp, npdt, kind=kind, scale=scale), xs, x, rng, S)


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,ns,S,d", DENSE_SUM)
def test_kvec_kmul_sum_dense(agp, lib, h, npdt, n, ns, S, d):
    """the composite kernel (kvec_sum_kernel / kmul_sum_kernel<T, 1|4|16>) with a coincident pair: White contributes σ₂² there and nowhere else"""
    rng = np.random.default_rng(21 + 1000 * d + n)
    xs, x = points(rng, d, ns, [], npdt), points(rng, d, n, [], npdt)
    xs[:, ns // 2] = x[:, n // 2]
    check_kvec_kmul(lib, h, npdt, Kern(agp, npdt, r=periods(rng, d)), xs, x, rng, S)


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,ns", [(129, 65), (300, 3), (400, 64)])
def test_kmul_column_bits_do_not_depend_on_the_other_columns(agp, lib, h, npdt, n, ns):
    """column 16 of S = 33 against the same weights alone (S = 1), as column 0 of S = 17 among other contents, and as column 127 of S = 128: the same bits"""
    d = 5
    rng = np.random.default_rng(n + ns)
    xs, x = points(rng, d, ns, [], npdt), points(rng, d, n, [], npdt)
    for kern in (Kern(agp, npdt, kind=3), Kern(agp, npdt, r=periods(rng, d))):
        a33 = rng.standard_normal((33, n)).astype(npdt)
        want = run_kmul(lib, h, npdt, kern, xs, x, a33)[0][16]
        for S, c in ((1, 0), (17, 0), (128, 127)):
            a = rng.standard_normal((S, n)).astype(npdt)
            a[c] = a33[16]
            assert same_bits(run_kmul(lib, h, npdt, kern, xs, x, a)[0][c], want), (kern.label(d), S, c)


KPG_N, KPG_D = [1, 255, 256, 257, 300], [1, 3, 16, 17, 20, 33]
KPG = [(d, KPG_N[(i + r) % 5], r, (i + r) % 3, (i + 2 * r) % 3) for i, d in enumerate(KPG_D) for r in range(4)]
MODE = ["gm", "gv", "both"]


def check_kpgrad(lib, h, npdt, kern, xs, x, rng, mode, tag):
    (d, ns), n = xs.shape, x.shape[1]
    j0, cnt = 2, ns - 3  # j0 > 0, and a last test point the launch does not cover
    alpha, W = rng.standard_normal(n).astype(npdt), rng.standard_normal((cnt, n)).astype(npdt)
    want_gm, want_gv = mode != 1, mode != 0
    el = kern.elements(xs[:, j0:j0 + cnt], x)
    rm, rv = R.kpgrad_reference(el, d, alpha if want_gm else None, W if want_gv else None, n, kern.sum)
    gm, gv = run_kpgrad(lib, h, npdt, kern, xs, x, alpha, W, j0, cnt, want_gm, want_gv)
    gm2, gv2 = run_kpgrad(lib, h, npdt, kern, xs, x, alpha, W, j0, cnt, want_gm, want_gv)
    inst = f"kpgrad_sum<{tname(npdt)}>" if kern.sum else f"kpgrad<{tname(npdt)}>"
    for name, g, g2, ref in (("gm", gm, gm2, rm), ("gv", gv, gv2, rv)):
        if g is not None:
            hold(inst, name, tag, g, ref)
            assert same_bits(g, g2), (name, "two calls, two results")
    return gm, gv


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,n,kind,tr,mode", KPG, ids=[f"D{d}-n{n}-{KIND[k]}-{TRANSFORM[t]}-{MODE[m]}" for d, n, k, t, m in KPG])
def test_kpgrad_dense(agp, lib, h, npdt, d, n, kind, tr, mode):
    rng = np.random.default_rng(31 + 1000 * d + 10 * n + kind)
    scale = scales(rng, d, tr)
    ns = 8
    xs, x = points(rng, d, ns, scale, npdt), points(rng, d, n, scale, npdt)
    xs[:, 3] = x[:, n // 2]  # a test point on a training point
    gm, gv = check_kpgrad(lib, h, npdt, Kern(agp, npdt, kind=kind, scale=scale), xs, x, rng, mode, f"{KIND[kind]}-D{d}-n{n}-{TRANSFORM[tr]}-{MODE[mode]}")
    assert all(np.isfinite(g).all() for g in (gm, gv) if g is not None)


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", [1, 3, 17])
def test_kpgrad_matern12_on_a_training_point_gets_no_contribution_from_it(agp, lib, h, npdt, d):
    """n = 1 and the test point ON the training point: κ' is taken as 0, so gm and gv are exactly 0 (not NaN from 0/0); one step away they are not"""
    rng = np.random.default_rng(d)
    x = points(rng, d, 1, [], npdt)
    xs = np.repeat(x, 4, axis=1)
    xs[:, 3] += npdt(0.25)
    kern = Kern(agp, npdt, kind=1)
    gm, gv = run_kpgrad(lib, h, npdt, kern, xs, x, np.ones(1, dtype=npdt), np.ones((4, 1), dtype=npdt), 0, 4)
    assert not gm[:, :3].any() and not gv[:, :3].any() and (gm[:, 3] < 0).all() and (gv[:, 3] > 0).all()


@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,n,mode", [(1, 257, 2), (4, 300, 0), (5, 256, 1), (16, 300, 2)])
def test_kpgrad_sum_dense(agp, lib, h, npdt, d, n, mode):
    rng = np.random.default_rng(41 + 1000 * d + n)
    xs, x = points(rng, d, 8, [], npdt), points(rng, d, n, [], npdt)
    xs[:, 3] = x[:, n // 2]
    check_kpgrad(lib, h, npdt, Kern(agp, npdt, r=periods(rng, d)), xs, x, rng, mode, f"D{d}-n{n}-{MODE[mode]}")


# ---- read, never used -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("which,d", [(2, 5), (1, 20), ("sum", 4)])
def test_nan_where_the_header_says_not_read_or_never_used(agp, lib, h, npdt, which, d):
    """x and alpha columns in [n, ld), xs columns in [ns, padded), W columns >= n: NaN there gives the bits zeros give"""
    n, ns, S = 300, 65, 17
    rng = np.random.default_rng(70 + d)
    kern = Kern(agp, npdt, r=periods(rng, d)) if which == "sum" else Kern(agp, npdt, kind=which)
    xs, x = points(rng, d, ns, [], npdt), points(rng, d, n, [], npdt)
    alpha, W = rng.standard_normal((S, n)).astype(npdt), rng.standard_normal((ns, n)).astype(npdt)
    res = {}
    for fill in (NAN, 0.0):
        gm, gv = run_kpgrad(lib, h, npdt, kern, xs, x, alpha[0], W, 0, ns, fill=fill)
        res[fill != 0.0] = [run_kvec(lib, h, npdt, kern, xs, x, alpha[0], fill), run_kmul(lib, h, npdt, kern, xs, x, alpha, fill)[0], gm, gv]
    for name, a, z in zip(("kvec", "kmul", "gm", "gv"), res[True], res[False]):
        assert same_bits(a, z) and np.isfinite(a).all(), name
