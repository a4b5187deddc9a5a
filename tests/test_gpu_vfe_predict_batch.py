"""GPU: agp.approx_mean_and_var_batch (gp_vfe_predict_batch) — predictive mean and variance of many small sparse GPs in one call — against the oracle's fp64
vfe_posterior(...).mean / .var (src/sparse_approximations.jl:183-217), with the bounds tests/test_gpu_random_vfe.py grants gp_vfe_predict at jitter 1e-4:
mean atol 1e-7, var atol 1e-8 (the formula in NumPy stays below 1e-13 / 4e-14 on such problems: room for the device's summation order, not for a wrong block)."""
import numpy as np
import pytest

from oracle import gp_oracle as o
from tests.test_gpu_vfe_batch import Problem

pytestmark = pytest.mark.gpu
COUNTER = "vfe_predict_batch_kernel_problems"


@pytest.fixture()
def pseg(agp, monkeypatch):
    """The measurement override: the kernels take every n of this file whatever GPMI355_VFE_PREDICT_BATCH_MAX_N routes to them.  Returns the predict SEG."""
    monkeypatch.setenv("GPMI_VFE_PREDICT_BATCH_MAX_N", str(4 * agp._lib.vfe_batch_limits()["SEG"]))
    return agp._lib.vfe_predict_batch_limits()["SEG"]


def _points(p, ns, seed):
    """ns test points of problem p: pseudo-inputs and training inputs first (the smallest variances: the cancellation shows there), then U(−2, 2)"""
    d = p.z.shape[1]
    return np.vstack([p.z[:3], p.x.X[:3], np.random.default_rng(seed).uniform(-2, 2, (ns, d))])[:ns]


def _table(agp, name, P):
    """(m, n, d, kind, transform, diagonal noise, mean, DTC, ns) per problem: every M, ns, D, kind, transform, noise, mean and approximation of the issue"""
    SEG = agp._lib.vfe_batch_limits()["SEG"]
    if name == "per_problem":
        rows = [(1, 1, 1, 0, 0, False, None, False, 1), (63, 63, 3, 1, 1, True, 0.7, True, 63), (64, 64, 16, 2, 2, False, None, False, 64),
                (65, 65, 3, 3, 0, True, None, True, 65), (128, 300, 1, 0, 1, False, -0.4, False, P - 1), (65, 200, 3, 1, 2, True, None, False, P),
                (63, SEG + 1, 16, 2, 0, False, 1.1, True, P + 1), (128, 400, 3, 3, 2, True, 0.3, False, 2 * P + 37), (40, 100, 2, 0, 0, False, None, False, 0)]
        ps = [Problem(agp, 110 + i, *r[:8]) for i, r in enumerate(rows)]
        return ps, [agp.RowVecs(_points(p, r[8], 200 + i)) for i, (p, r) in enumerate(zip(ps, rows))]
    X = np.random.default_rng(6998).uniform(-2, 2, (300, 3))  # one (x, y) object and ONE set of test points for every problem: nx = ny = nxs = 1
    data = (agp.RowVecs(X), np.cos(X.sum(1)))
    rows = [(1, 0, 0, False, None, True), (64, 1, 1, False, 0.5, False), (128, 2, 2, False, None, False), (65, 3, 1, False, None, True)]
    ps = [Problem(agp, 130 + i, m, 300, 3, kind, tr, vec, mean, dtc, data=data) for i, (m, kind, tr, vec, mean, dtc) in enumerate(rows)]
    return ps, [agp.RowVecs(_points(ps[2], P + 1, 250))]


_CASES = {}


def _case(agp, name, P):
    """the table's problems, test points and oracle predictions, computed once"""
    if name not in _CASES:
        ps, xs = _table(agp, name, P)
        refs = []
        for b, p in enumerate(ps):
            post, t = o.vfe_posterior(p.of, p.z, p.jitter, p.ofx, p.y), xs[b % len(xs)].X
            refs.append((post.mean(t), post.var(t)) if len(t) else (np.empty(0), np.empty(0)))
        _CASES[name] = (ps, xs, refs)
    return _CASES[name]


def _call(agp, ps, xs, **kw):
    return agp.approx_mean_and_var_batch([p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps], xs, **kw)


@pytest.mark.parametrize("name,what", [("per_problem", 3), ("shared", 3), ("per_problem", 1), ("shared", 2)])
def test_batch_matches_oracle(agp, pseg, name, what):
    ps, xs, refs = _case(agp, name, pseg)
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    means, vars_, obj = _call(agp, ps, xs, what=what, return_objective=True)
    assert ctx.get_param(COUNTER) - served == len(ps)
    assert np.array_equal(obj, agp.elbo_batch([p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps]))
    assert (means is None) == (what == 2) and (vars_ is None) == (what == 1)
    for side, (got, atol) in enumerate(((means, 1e-7), (vars_, 1e-8))):
        if got is None:
            continue
        err = [float(np.max(np.abs(got[b] - refs[b][side]), initial=0.0)) for b in range(len(ps))]
        print(f"{name} what={what} {'mean var'.split()[side]}: largest deviation per problem {['%.1e' % e for e in err]}")
        for b, p in enumerate(ps):
            assert got[b].shape == refs[b][side].shape
            np.testing.assert_allclose(got[b], refs[b][side], atol=atol, rtol=0, err_msg=f"{name}[{b}] m={p.m}")


def test_routing_mixes_kernel_and_single_path(agp, pseg):
    ps = [Problem(agp, 150, 40, 300, 2, 0, 1, False, None, False), Problem(agp, 151, 129, 300, 2, 1, 0, True, 0.2, True),
          Problem(agp, 152, 64, 200, 3, 2, 2, False, None, False)]
    p32 = Problem(agp, 153, 20, 150, 2, 0, 0, False, None, False)
    fx32, y32 = p32.f(agp.RowVecs(p32.x.X.astype(np.float32)), p32.sig), p32.y.astype(np.float32)
    xs = [agp.RowVecs(_points(p, 70, 260 + i)) for i, p in enumerate(ps)] + [agp.RowVecs(_points(p32, 33, 270).astype(np.float32))]
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    means, vars_ = agp.approx_mean_and_var_batch([p.approx for p in ps + [p32]], [p.fx for p in ps] + [fx32], [p.y for p in ps] + [y32], xs)
    assert ctx.get_param(COUNTER) - served == 2
    for b in (0, 2):
        post = o.vfe_posterior(ps[b].of, ps[b].z, ps[b].jitter, ps[b].ofx, ps[b].y)
        np.testing.assert_allclose(means[b], post.mean(xs[b].X), atol=1e-7, rtol=0)
        np.testing.assert_allclose(vars_[b], post.var(xs[b].X), atol=1e-8, rtol=0)
    # the routed problems ARE their single calls: the same path, the same bits
    for b, single in ((1, agp.posterior(ps[1].approx, ps[1].fx, ps[1].y)), (3, agp.posterior(p32.approx, fx32, y32))):
        m, v = single.mean_and_var(xs[b])
        assert means[b].dtype == m.dtype and np.array_equal(means[b], m) and np.array_equal(vars_[b], v)
    assert means[3].dtype == np.float32


def test_bits_do_not_depend_on_the_company(agp, pseg):
    ps = [Problem(agp, 160 + i, m, n, 2, i % 4, i % 3, i % 2 == 0, None, i % 2 == 1) for i, (m, n) in enumerate([(100, 700), (1, 5), (64, 64), (128, 130)])]
    xs = [agp.RowVecs(_points(p, ns, 280 + i)) for i, (p, ns) in enumerate(zip(ps, [70, 3, pseg + 5, 64]))]
    alone = _call(agp, ps[:1], xs[:1])
    for r, b in ((_call(agp, ps, xs), 0), (_call(agp, ps[1:] + ps[:1], xs[1:] + xs[:1]), 3), (_call(agp, ps, xs), 0)):
        assert np.array_equal(r[0][b], alone[0][0]) and np.array_equal(r[1][b], alone[1][0])
    # the same points at another offset of a longer set: they straddle a tile edge and the segment edge there
    long = np.random.default_rng(290).uniform(-2, 2, (pseg + 100, 2))
    long[pseg - 30:pseg + 40] = xs[0].X
    m, v = _call(agp, ps[:1], [agp.RowVecs(long)])
    assert np.array_equal(m[0][pseg - 30:pseg + 40], alone[0][0]) and np.array_equal(v[0][pseg - 30:pseg + 40], alone[1][0])


def test_failure_is_data(agp, pseg):
    good = [Problem(agp, 170, 30, 200, 2, 0, 1, False, None, False), Problem(agp, 171, 70, 500, 3, 3, 0, True, 0.5, True)]
    bad = Problem(agp, 172, 40, 300, 2, 0, 0, False, None, False, jitter=0.0, dup_z=True, variance=1.0)  # K_zz[:2, :2] is exactly [[1, 1], [1, 1]]
    with pytest.raises(o.PosDefException):  # a genuine failure: the oracle's Cholesky of K_zz refuses it too
        o.vfe_posterior(bad.of, bad.z, 0.0, bad.ofx, bad.y)
    ps = [good[0], bad, good[1]]
    xs = [agp.RowVecs(_points(p, 40, 300 + i)) for i, p in enumerate(ps)]
    with pytest.raises(agp.PosDefException) as e:
        _call(agp, ps, xs)
    assert e.value.info > 0 and e.value.index == 1
    means, vars_, obj = _call(agp, ps, xs, return_objective=True, on_error="nan")
    assert np.isnan(obj[1]) and np.isnan(means[1]).all() and np.isnan(vars_[1]).all()
    for b in (0, 2):
        alone = _call(agp, [ps[b]], [xs[b]])
        assert np.array_equal(means[b], alone[0][0]) and np.array_equal(vars_[b], alone[1][0])
