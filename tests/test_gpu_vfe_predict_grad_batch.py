"""GPU: agp.approx_mean_and_var_grad_batch (gp_vfe_predict_grad_batch) — predictions of many small sparse GPs and their gradients w.r.t. the test inputs in one
call — against the oracle's vfe_posterior(...).mean / .var (atol 1e-7 / 1e-8, the bounds of tests/test_gpu_vfe_predict_batch.py) and the fp64 reference
tests/predict_grad_ref.py::sparse_grads (rtol 1e-7, atol 1e-8·max(1, max|g_ref|), the bounds of tests/test_gpu_predict_grad.py).
Largest deviations measured over the two tables: mean 2.8e-14, var 6.2e-15, dmean 1.8e-13, dvar 1.7e-14."""
import numpy as np
import pytest

from oracle import gp_oracle as o
from tests.predict_grad_ref import sparse_grads
from tests.test_gpu_vfe_batch import Problem
from tests.test_gpu_vfe_predict_batch import _points

pytestmark = pytest.mark.gpu
COUNTER = "vfe_predict_grad_batch_kernel_problems"


@pytest.fixture()
def pseg(agp, monkeypatch):
    """The measurement overrides: the kernels take every n of this file whatever the two MAX_N macros route to them.  Returns the predict SEG."""
    for name in ("GPMI_VFE_PREDICT_GRAD_BATCH_MAX_N", "GPMI_VFE_PREDICT_BATCH_MAX_N"):
        monkeypatch.setenv(name, str(4 * agp._lib.vfe_batch_limits()["SEG"]))
    return agp._lib.vfe_predict_batch_limits()["SEG"]


def _table(agp, name, P):
    """(m, n, d, kind, transform, diagonal noise, mean, DTC, ns) per problem: every M, ns, D, kind, transform, noise, mean and approximation of the issue"""
    if name == "per_problem":
        rows = [(1, 1, 1, 0, 0, False, None, False, 1), (63, 63, 3, 1, 1, True, 0.7, True, 63), (64, 64, 16, 2, 2, False, None, False, 64),
                (65, 65, 3, 3, 0, True, None, True, 65), (128, 300, 1, 0, 1, False, -0.4, False, P - 1), (17, 200, 3, 1, 2, True, None, False, P + 1),
                (63, 150, 16, 2, 0, False, 1.1, True, 70), (128, 400, 3, 3, 2, True, 0.3, False, 2 * P + 37), (40, 100, 2, 0, 0, False, None, False, 0)]
        ps = [Problem(agp, 410 + i, *r[:8]) for i, r in enumerate(rows)]
        return ps, [agp.RowVecs(_points(p, r[8], 500 + i)) for i, (p, r) in enumerate(zip(ps, rows))]
    X = np.random.default_rng(6997).uniform(-2, 2, (300, 3))  # one (x, y) object and ONE set of test points for every problem: nx = ny = nxs = 1
    data = (agp.RowVecs(X), np.cos(X.sum(1)))
    rows = [(1, 0, 0, False, None, True), (64, 1, 1, False, 0.5, False), (128, 2, 2, False, None, False), (65, 3, 1, False, None, True)]
    ps = [Problem(agp, 430 + i, m, 300, 3, kind, tr, vec, mean, dtc, data=data) for i, (m, kind, tr, vec, mean, dtc) in enumerate(rows)]
    return ps, [agp.RowVecs(_points(ps[2], P + 1, 550))]


_CASES = {}


def _case(agp, name, P):
    """the table's problems, test points and references (mean, var, dmean, dvar), computed once"""
    if name not in _CASES:
        ps, xs = _table(agp, name, P)
        refs = []
        for b, p in enumerate(ps):
            post, t = o.vfe_posterior(p.of, p.z, p.jitter, p.ofx, p.y), xs[b % len(xs)].X
            refs.append((post.mean(t), post.var(t)) + sparse_grads(post, t) if len(t) else (np.empty(0),) * 2 + (np.empty(t.shape),) * 2)
        _CASES[name] = (ps, xs, refs)
    return _CASES[name]


def _call(agp, ps, xs, **kw):
    return agp.approx_mean_and_var_grad_batch([p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps], xs, **kw)


def _same(a, b):
    return all((u is None and v is None) or np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


@pytest.mark.parametrize("what", [3, 1, 2])
@pytest.mark.parametrize("name", ["per_problem", "shared"])
def test_batch_matches_oracle(agp, pseg, name, what):
    ps, xs, refs = _case(agp, name, pseg)
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    quads = _call(agp, ps, xs, what=what)
    assert ctx.get_param(COUNTER) - served == len(ps)
    worst = [0.0] * 4
    for b, (p, got, ref) in enumerate(zip(ps, quads, refs)):
        for side, (v, r) in enumerate(zip(got, ref)):
            if not what & (1 + side % 2):
                assert v is None
                continue
            assert v.shape == r.shape, (name, b, side)
            worst[side] = max(worst[side], float(np.max(np.abs(v - r), initial=0.0)))
            atol = (1e-7, 1e-8)[side] if side < 2 else 1e-8 * max(1.0, float(np.max(np.abs(r), initial=0.0)))
            np.testing.assert_allclose(v, r, atol=atol, rtol=0 if side < 2 else 1e-7, err_msg=f"{name}[{b}] m={p.m} {'mean var dmean dvar'.split()[side]}")
    print(f"{name} what={what}: largest deviation mean {worst[0]:.1e} var {worst[1]:.1e} dmean {worst[2]:.1e} dvar {worst[3]:.1e}")


@pytest.mark.parametrize("name", ["per_problem", "shared"])
def test_values_are_the_bits_of_the_prediction_call(agp, pseg, name):
    ps, xs, _ = _case(agp, name, pseg)
    quads, obj = _call(agp, ps, xs, return_objective=True)
    means, vars_, obj0 = agp.approx_mean_and_var_batch([p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps], xs, return_objective=True)
    assert np.array_equal(obj, obj0)
    for q, m, v in zip(quads, means, vars_):
        assert np.array_equal(q[0], m) and np.array_equal(q[1], v)


def test_routing_mixes_kernel_and_single_path(agp, pseg):
    ps = [Problem(agp, 450, 40, 300, 2, 0, 1, False, None, False), Problem(agp, 451, 129, 300, 2, 1, 0, True, 0.2, True),
          Problem(agp, 452, 64, 200, 3, 2, 2, False, None, False)]
    p32 = Problem(agp, 453, 20, 150, 2, 0, 0, False, None, False)
    fx32, y32 = p32.f(agp.RowVecs(p32.x.X.astype(np.float32)), p32.sig), p32.y.astype(np.float32)
    xs = [agp.RowVecs(_points(p, 70, 560 + i)) for i, p in enumerate(ps)] + [agp.RowVecs(_points(p32, 33, 570).astype(np.float32))]
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    quads = agp.approx_mean_and_var_grad_batch([p.approx for p in ps + [p32]], [p.fx for p in ps] + [fx32], [p.y for p in ps] + [y32], xs)
    assert ctx.get_param(COUNTER) - served == 2
    # the routed problems ARE their single calls: the same path, the same bits
    for b, single in ((1, agp.posterior(ps[1].approx, ps[1].fx, ps[1].y)), (3, agp.posterior(p32.approx, fx32, y32))):
        assert _same(quads[b], single.mean_and_var_grad(xs[b])) and quads[b][2].dtype == xs[b].X.dtype
    assert _same(quads[0], _call(agp, ps[:1], xs[:1])[0])


def test_bits_do_not_depend_on_the_company(agp, pseg):
    ps = [Problem(agp, 460 + i, m, n, 2, i % 4, i % 3, i % 2 == 0, None, i % 2 == 1) for i, (m, n) in enumerate([(100, 700), (1, 5), (64, 64), (128, 130)])]
    xs = [agp.RowVecs(_points(p, ns, 580 + i)) for i, (p, ns) in enumerate(zip(ps, [70, 3, pseg + 5, 64]))]
    alone = _call(agp, ps[:1], xs[:1])[0]
    for r, b in ((_call(agp, ps, xs), 0), (_call(agp, ps[1:] + ps[:1], xs[1:] + xs[:1]), 3), (_call(agp, ps, xs), 0)):
        assert _same(r[b], alone)
    # the same points at another offset of a longer set: they straddle a tile edge and the segment edge there
    long = np.random.default_rng(590).uniform(-2, 2, (pseg + 100, 2))
    long[pseg - 30:pseg + 40] = xs[0].X
    assert _same([v[pseg - 30:pseg + 40] for v in _call(agp, ps[:1], [agp.RowVecs(long)])[0]], alone)


def test_failure_is_data(agp, pseg):
    good = [Problem(agp, 470, 30, 200, 2, 0, 1, False, None, False), Problem(agp, 471, 70, 500, 3, 3, 0, True, 0.5, True)]
    bad = Problem(agp, 472, 40, 300, 2, 0, 0, False, None, False, jitter=0.0, dup_z=True, variance=1.0)  # K_zz[:2, :2] is exactly [[1, 1], [1, 1]]
    ps = [good[0], bad, good[1]]
    xs = [agp.RowVecs(_points(p, 40, 600 + i)) for i, p in enumerate(ps)]
    with pytest.raises(agp.PosDefException) as e:
        _call(agp, ps, xs)
    assert e.value.info > 0 and e.value.index == 1
    quads, obj = _call(agp, ps, xs, return_objective=True, on_error="nan")
    assert np.isnan(obj[1]) and all(np.isnan(v).all() and v.shape == r.shape for v, r in zip(quads[1], (xs[1].X[:, 0],) * 2 + (xs[1].X,) * 2))
    for b in (0, 2):
        assert _same(quads[b], _call(agp, [ps[b]], [xs[b]])[0])
