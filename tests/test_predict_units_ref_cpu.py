"""CPU: the longdouble reference of the prediction-kernel unit tests (tests/predict_units_ref.py) against a 40-digit mpmath restatement of the same sums, as
test_grad_units_ref_cpu.py does for the gradient contractions (its kd_mp / M / close are reused): every kind and transform, values drawn in fp64 and in fp32.  The
reference has to agree within 1e-3 of the bound it hands to the GPU tests.  And the bound must not be vacuous: for each operation, dropping ONE term of the sum moves
every output by more than its bound."""
import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from tests import predict_units_ref as R  # noqa: E402
from tests.test_grad_units_ref_cpu import M, close, kd_mp  # noqa: E402

VARIANCE = 1.5
N, NS, D, S = 10, 4, 3, 3
CASES = [(kind, nscale, npdt) for kind in range(4) for nscale in (0, 1, D) for npdt in (np.float64, np.float32)]
IDS = [f"kind{k}-ns{s}-{np.dtype(t).name}" for k, s, t in CASES]


def problem(npdt, seed):
    rng = np.random.default_rng(seed)
    pts = lambda n: (rng.random((D, n)) * np.sqrt(6.0 / D)).astype(npdt)  # noqa: E731
    wts = lambda *s: (rng.choice([-1, 1], s) * (0.5 + rng.random(s))).astype(npdt)  # noqa: E731  (|w| >= 0.5: a dropped term is never negligible)
    xs, x = pts(NS), pts(N)
    xs[:, 1] = x[:, 7]  # a test point on a training point: Matern12's κ' = 0 branch, White's 1
    return rng, xs, x, wts


def mp_kind(kind, nscale, scale, xs, x, j, i):
    """(σ²κ, [∂/∂xs_jp]) of pair (j, i) in mpmath"""
    t = [M(xs[p, j]) - M(x[p, i]) for p in range(D)]
    k, dk = kd_mp(kind, sum(tp * tp for tp in t))
    var = mp.mpf(VARIANCE)
    sp = lambda p: mp.mpf(1) if nscale == 0 else M(scale[0] if nscale == 1 else scale[p])  # noqa: E731
    return var * k, [2 * sp(p) * var * dk * t[p] for p in range(D)]


def mp_composite(s1, r, s, a, s2, xs, x, j, i):
    t = [M(xs[p, j]) - M(x[p, i]) for p in range(D)]
    kP = mp.e ** (-sum((mp.sinpi(tp) / M(rp)) ** 2 for tp, rp in zip(t, r)) / 2)
    r2 = sum(tp * tp for tp in t)
    q = M(s) ** 2 * r2 / (2 * M(a))
    kR = mp.e ** (-M(a) * mp.log1p(q))
    dk = -kR / (2 * (1 + q))
    val = M(s1) * kP * kR + (M(s2) if r2 == 0 else 0)
    return val, [M(s1) * (-kR * kP * mp.pi / 2 * mp.sinpi(2 * t[p]) / M(r[p]) ** 2 + kP * 2 * dk * M(s) ** 2 * t[p]) for p in range(D)]


def hold_all(el, pair, xs, x, alpha, A, W, npdt, composite):
    """the three references on one set of elements against the mpmath sums over pair(j, i); returns the Outs"""
    F = [[pair(j, i) for i in range(N)] for j in range(NS)]
    kv = R.kvec_reference(el, alpha, npdt)
    close("kvec", kv.val, [sum(F[j][i][0] * M(alpha[i]) for i in range(N)) for j in range(NS)], kv.bound)
    km = R.kmul_reference(el, A, N, NS, npdt)
    close("kmul", km.val, [[sum(F[j][i][0] * M(A[c, i]) for i in range(N)) for j in range(NS)] for c in range(S)], km.bound)
    gm, gv = R.kpgrad_reference(el, D, alpha, W, N, composite)
    close("gm", gm.val, [[sum(F[j][i][1][p] * M(alpha[i]) for i in range(N)) for j in range(NS)] for p in range(D)], gm.bound)
    close("gv", gv.val, [[-2 * sum(F[j][i][1][p] * M(W[j, i]) for i in range(N)) for j in range(NS)] for p in range(D)], gv.bound)
    assert R.kpgrad_reference(el, D, None, W, N, composite)[0] is None and R.kpgrad_reference(el, D, alpha, None, N, composite)[1] is None
    return kv, km, gm, gv


def not_vacuous(el, alpha, A, W, kv, km, gm, gv, skip_j):
    """one dropped term (training point 0) exceeds the bound of EVERY output it belongs to (skip_j: the test point whose derivative terms vanish by construction)"""
    a, Aw, Ww = R._wide(alpha), R._wide(A), R._wide(W)
    assert (np.abs(el.F[:, 0] * a[0]) > kv.bound).all(), "kvec"
    assert (np.abs(Aw[:, :1] * el.F[None, :, 0]) > km.bound).all(), "kmul"
    keep = [j for j in range(NS) if j != skip_j]
    for p in range(D):
        dF, _ = el.dF(p)
        assert (np.abs(dF[keep, 0] * a[0]) > gm.bound[p][keep]).all(), ("gm", p)
        assert (2 * np.abs(dF[keep, 0] * Ww[keep, 0]) > gv.bound[p][keep]).all(), ("gv", p)


@pytest.mark.parametrize("kind,nscale,npdt", CASES, ids=IDS)
def test_single_kind_references_against_mpmath(kind, nscale, npdt):
    rng, xs, x, wts = problem(npdt, 300 + 10 * kind + nscale)
    scale = (0.5 + rng.random(nscale)).tolist()
    alpha, A, W = wts(N), wts(S, N), wts(NS, N)
    el = R.kind_elements(kind, VARIANCE, nscale, scale, xs, x)
    outs = hold_all(el, lambda j, i: mp_kind(kind, nscale, scale, xs, x, j, i), xs, x, alpha, A, W, npdt, False)
    not_vacuous(el, alpha, A, W, *outs, skip_j=None)
    if kind == 1:  # the coincident pair (test point 1, training point 7) contributes exactly nothing to the derivative
        assert all(float(el.dF(p)[0][1, 7]) == 0.0 and float(el.dF(p)[1][1, 7]) == 0.0 for p in range(D))


@pytest.mark.parametrize("npdt", [np.float64, np.float32], ids=["float64", "float32"])
def test_composite_references_against_mpmath(npdt):
    rng, xs, x, wts = problem(npdt, 400)
    s1, r, s, a, s2 = 1.5, [0.75, 1.25, 0.875], 1.25, 2.5, 0.25
    alpha, A, W = wts(N), wts(S, N), wts(NS, N)
    el = R.composite_elements(s1, r, s, a, s2, xs, x)
    outs = hold_all(el, lambda j, i: mp_composite(s1, r, s, a, s2, xs, x, j, i), xs, x, alpha, A, W, npdt, True)
    not_vacuous(el, alpha, A, W, *outs, skip_j=None)
    assert float(el.F[1, 7]) == s1 + s2  # White on the coincident pair


def test_one_hot_weights_are_held_to_the_element_bound_alone():
    """a single non-zero weight: the bound is the per-element error (plus the roundings of that one term) — no γ_m of a sum that adds exact zeros"""
    for npdt in (np.float64, np.float32):
        _, xs, x, _ = problem(npdt, 500)
        u = R.unit(npdt)
        el = R.kind_elements(3, VARIANCE, 0, [], xs, x)
        A = np.zeros((S, N), dtype=npdt)
        A[1, 4] = 1
        km = R.kmul_reference(el, A, N, NS, npdt)
        assert not km.bound[0].any() and not km.bound[2].any() and not km.val[0].any()
        assert (km.bound[1] <= el.e[:, 4] + u * (el.F[:, 4] + el.e[:, 4])).all() and (km.bound[1] >= el.e[:, 4]).all()
        kv = R.kvec_reference(el, A[1], npdt)
        assert (kv.bound <= (el.e[:, 4] + 2 * u * (el.F[:, 4] + el.e[:, 4])) * (1 + 2 * u)).all()


def test_the_split_rule_gives_the_shapes_the_gpu_tests_name():
    assert [R.kmul_split(n, 1) for n in (224, 225, 288, 300, 400)] == [(1, 7), (2, 4), (2, 5), (2, 5), (3, 5)]
    assert R.kmul_split(400, 64 * 511 + 1) == (1, 13) and R.kmul_split(400, 64 * 256) == (2, 7)
