"""GPU: agp.elbo_and_grad_batch (gp_vfe_grad_batch) — value and gradient of many small sparse GPs in one call — against the oracle's dense N×N calculus
(oracle.gp_oracle.elbo_grad).  Bounds are the project's own: objective rel 1e-8 / abs 1e-7 (tests/test_gpu_vfe_batch.py); every gradient output
max|g − ref| / max(max|ref|, 1) <= max(1e-7, 1e-11 / jitter) (the rule of tests/test_gpu_vfe_grad.py), jitter 1e-4."""
import numpy as np
import pytest

from oracle import gp_oracle as o
from tests.test_gpu_vfe_batch import Problem

pytestmark = pytest.mark.gpu
COUNTER = "vfe_grad_batch_kernel_problems"
TOL = max(1e-7, 1e-11 / 1e-4)


@pytest.fixture()
def kernels_on(agp, monkeypatch):
    """The measurement overrides: the kernels take every n of this file.  Returns SEG."""
    lim = agp._lib.vfe_batch_limits()
    monkeypatch.setenv("GPMI_VFE_GRAD_BATCH_MAX_N", str(4 * lim["SEG"]))
    monkeypatch.setenv("GPMI_VFE_BATCH_MAX_N", str(4 * lim["SEG"]))
    return lim["SEG"]


def _call(agp, ps, **kw):
    return agp.elbo_and_grad_batch([p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps], wrt_x=True, **kw)


def _same(g, h):
    assert g.keys() == h.keys()
    return all((g[k] is None and h[k] is None) or np.array_equal(g[k], h[k]) for k in g)


def _batch(agp, name, SEG):
    """(m, n, d, kind, transform, diagonal noise, mean, DTC) per problem: every M, n, D, kind, transform, noise and mean form of the issue, VFE and DTC mixed."""
    if name == "per_problem":
        rows = [(1, 1, 1, 0, 0, False, None, False), (63, 63, 3, 1, 1, True, 0.7, True), (64, 65, 16, 2, 2, False, None, False),
                (65, SEG - 1, 3, 3, 0, True, None, True), (128, SEG, 1, 0, 1, False, -0.4, False), (128, SEG + 65, 3, 1, 2, True, 0.3, True),
                (1, 63, 16, 2, 1, False, 1.1, True)]
        return [Problem(agp, 110 + i, *r) for i, r in enumerate(rows)]
    n, d = SEG + 65, 3  # one (x, y) object for every problem: nx = ny = 1, and every problem its own dx
    X = np.random.default_rng(6998).uniform(-2, 2, (n, d))
    data = (agp.RowVecs(X), np.cos(X.sum(1)))
    rows = [(63, 0, 0, False, None, True), (128, 3, 2, False, None, False), (65, 1, 1, False, None, True)]
    return [Problem(agp, 130 + i, m, n, d, kind, tr, vec, mean, dtc, data=data) for i, (m, kind, tr, vec, mean, dtc) in enumerate(rows)]


@pytest.mark.parametrize("name", ["per_problem", "shared"])
def test_batch_matches_oracle(agp, kernels_on, name):
    ps = _batch(agp, name, kernels_on)
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    obj, grads = _call(agp, ps)
    assert ctx.get_param(COUNTER) - served == len(ps)
    worst = {}
    for b, (p, g) in enumerate(zip(ps, grads)):
        ref_obj = (o.dtc_log_evidence if p.dtc else o.elbo)(p.of, p.z, p.jitter, p.ofx, p.y)
        ref = o.elbo_grad(p.of, p.z, p.jitter, p.ofx, p.y, vfe=not p.dtc)
        pairs = {k: (g[k], ref[k]) for k in ("variance", "y", "mean", "z", "x")}
        pairs["noise"] = (g["noise_diag"] if np.ndim(p.sig) else g["noise"], ref["noise"])
        assert (g["scale"] is None) == (ref["scale"] is None)
        if ref["scale"] is not None:
            pairs["scale"] = (g["scale"], ref["scale"])
        errs = {}
        for k, (a, r) in pairs.items():
            a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
            assert a.size == r.size, (b, k, a.shape, r.shape)
            errs[k] = np.max(np.abs(a.reshape(r.shape) - r)) / max(np.max(np.abs(r)), 1.0)
            worst[k] = max(worst.get(k, 0.0), errs[k])
        print(f"{name}[{b}] m={p.m} n={len(p.y)}: objective rel {abs(obj[b] - ref_obj) / abs(ref_obj):.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert float(obj[b]) == pytest.approx(ref_obj, rel=1e-8, abs=1e-7), (name, b)
        assert max(errs.values()) <= TOL, (name, b, errs)
    print(f"{name}: worst " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_routing_mixes_kernel_and_single_path(agp, kernels_on):
    ps = [Problem(agp, 150, 40, 300, 2, 0, 1, False, None, False), Problem(agp, 151, 129, 300, 2, 1, 0, False, 0.2, True),
          Problem(agp, 152, 64, 200, 3, 2, 2, False, None, False)]
    p32 = Problem(agp, 153, 20, 150, 2, 0, 0, False, None, False)
    fx32, y32 = p32.f(agp.RowVecs(p32.x.X.astype(np.float32)), p32.sig), p32.y.astype(np.float32)
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    obj, grads = agp.elbo_and_grad_batch([p.approx for p in ps + [p32]], [p.fx for p in ps] + [fx32], [p.y for p in ps] + [y32], wrt_x=True)
    assert ctx.get_param(COUNTER) - served == 2
    # The routed problems ARE their single calls: the same path, and the same bits wherever that path has bits of its own.  The single path's reverse pass adds
    # its 128×128 tiles' sums of ∂/∂variance, ∂/∂scale and ∂/∂z with fp64 atomicAdd: over the observations (one addend per tile) and then, onto the same
    # accumulators, over the K_zz square.  Up to two addends commute; at M = 129 the K_zz square alone is 2×2 tiles, so four addends reach variance and scale
    # and two more each column of z, in the order the scheduler picks: two single calls differ in the last bits there, at any n.  Those three are held to the
    # gradient tolerance of this file instead.  The objective, y, mean, noise and x have at most two addends per entry (two column tiles; two blocks of 256
    # observations for Σ∂/∂σ²) and are compared bit for bit, as is everything of the fp32 problem (M = 20: one column tile, one K_zz tile).
    for b, (a, fx, y), loose in ((1, (ps[1].approx, ps[1].fx, ps[1].y), ("variance", "scale", "z")), (3, (p32.approx, fx32, y32), ())):
        sobj, sg = agp.elbo_and_grad(a, fx, y, wrt_x=True)
        sg.pop("noise_diag")  # the single call returns the vector for a scalar σ² too
        if b == 3:  # dnoise_out holds the call's dtype: the fp32 problem's sum is the single call's double, rounded once
            sg["noise"] = float(np.float32(sg["noise"]))
        assert grads[b].keys() == sg.keys(), b
        for k in loose:
            g, s = grads[b][k], sg[k]
            assert (g is None) == (s is None), (b, k)
            if s is not None:
                assert np.shape(g) == np.shape(s) and np.max(np.abs(np.asarray(g) - s)) / max(np.max(np.abs(s)), 1.0) <= TOL, (b, k)
        strict = [k for k in sg if k not in loose]
        assert obj[b] == sobj and _same({k: grads[b][k] for k in strict}, {k: sg[k] for k in strict}), b
    assert "z" in grads[1] and "z" not in grads[3] and grads[3]["y"].dtype == np.float32


def test_bits_do_not_depend_on_the_batch(agp, kernels_on):
    SEG = kernels_on
    ps = [Problem(agp, 160 + i, m, n, 2, i % 4, i % 3, i % 2 == 0, None, i % 2 == 1)
          for i, (m, n) in enumerate([(100, 2 * SEG + 37), (1, 5), (64, 64), (33, 700), (128, 130)])]
    alone = _call(agp, ps[:1])
    for r, b in ((_call(agp, ps), 0), (_call(agp, ps[1:] + ps[:1]), 4), (_call(agp, ps), 0)):
        assert r[0][b] == alone[0][0] and _same(r[1][b], alone[1][0])
    assert alone[0][0] == agp.elbo_batch([ps[0].approx], [ps[0].fx], [ps[0].y])[0]


def test_failure_is_data(agp, kernels_on):
    good = [Problem(agp, 170, 30, 200, 2, 0, 1, False, None, False), Problem(agp, 171, 70, 500, 3, 3, 0, True, 0.5, True)]
    bad = Problem(agp, 172, 40, 300, 2, 0, 0, False, None, False, jitter=0.0, dup_z=True, variance=1.0)  # K_zz[:2, :2] is exactly [[1, 1], [1, 1]]
    ps = [good[0], bad, good[1]]
    with pytest.raises(agp.PosDefException) as e:
        _call(agp, ps)
    assert e.value.info > 0 and e.value.index == 1
    obj, grads = _call(agp, ps, on_error="nan")
    assert np.isnan(obj[1]) and all(np.isnan(v).all() for v in grads[1].values() if v is not None)
    assert set(grads[1]) == set(grads[0])
    for b in (0, 2):
        alone = _call(agp, [ps[b]])
        assert obj[b] == alone[0][0] and _same(grads[b], alone[1][0])
