"""GPU: agp.elbo_batch / approx_log_evidence_batch (gp_vfe_batch) — many small sparse GPs in one call — against the oracle's fp64 restatement of
src/sparse_approximations.jl:58-75, 248-313 (elbo, dtc_log_evidence, vfe_posterior), with the bounds tests/test_gpu_random_vfe.py grants gp_vfe_fit:
objective rel 1e-8 / abs 1e-7, K(x*, z) α within 1e-7 of the oracle posterior's mean at nine points, U α = m_ε to 1e-10 relative."""
import numpy as np
import pytest

from oracle import gp_oracle as o

pytestmark = pytest.mark.gpu
COUNTER = "vfe_batch_kernel_problems"


@pytest.fixture()
def kernels_on(agp, monkeypatch):
    """The measurement override: the kernels take every n of this file whatever GPMI355_VFE_BATCH_MAX_N routes to them.  Returns SEG."""
    lim = agp._lib.vfe_batch_limits()
    monkeypatch.setenv("GPMI_VFE_BATCH_MAX_N", str(4 * lim["SEG"]))
    return lim["SEG"]


class Problem:
    """One sparse problem as tests/test_gpu_random_vfe.py builds them: X ~ U(−2, 2), z a jittered subset, jitter 1e-4, σ² ∈ [0.02, 0.3]."""

    def __init__(self, agp, seed, m, n, d, kind, tr, vec, mean, dtc, data=None, jitter=1e-4, dup_z=False, variance=None):
        rng = np.random.default_rng(7000 + seed)
        variance = float(rng.uniform(0.3, 2.5)) if variance is None else variance
        scale = None if tr == 0 else (float(rng.uniform(0.4, 1.6)) if tr == 1 else rng.uniform(0.4, 1.6, d))
        if data is None:
            X = rng.uniform(-2, 2, (n, d))
            data = (agp.RowVecs(X), np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n))
        self.x, self.y = data
        X = self.x.X
        self.z = X[rng.permutation(n)[:m]] + 0.01 * rng.standard_normal((m, d))
        if dup_z:
            self.z[1] = self.z[0]
        self.sig = rng.uniform(0.02, 0.3, n) if vec else float(rng.uniform(0.02, 0.3))
        self.jitter, self.dtc, self.m = jitter, dtc, m
        kern = variance * agp.Kernel(kind)
        if scale is not None:
            kern = kern @ (agp.ScaleTransform(scale) if np.ndim(scale) == 0 else agp.ARDTransform(scale))
        self.f = agp.GP(kern) if mean is None else agp.GP(mean, kern)
        self.of = o.GP(o.Kernel(kind, variance, scale), mean)
        self.approx = (agp.DTC if dtc else agp.VFE)(self.f(agp.RowVecs(self.z), jitter))
        self.fx = self.f(self.x, self.sig)
        self.ofx = o.FiniteGP(self.of, X, self.sig)
        self.xs = rng.uniform(-2, 2, (9, d))

    def check(self, obj, alpha, m_eps, desc):
        ref = (o.dtc_log_evidence if self.dtc else o.elbo)(self.of, self.z, self.jitter, self.ofx, self.y)
        post = o.vfe_posterior(self.of, self.z, self.jitter, self.ofx, self.y)
        mean = o.gp_mean(self.of, self.xs) + o.gp_cov(self.of, self.xs, self.z) @ alpha
        res = np.linalg.norm(post.U @ alpha - m_eps) / np.linalg.norm(m_eps)
        print(f"{desc}: objective rel {abs(obj - ref) / abs(ref):.2e}  mean abs {np.max(np.abs(mean - post.mean(self.xs))):.2e}  U α − m_ε rel {res:.2e}")
        assert float(obj) == pytest.approx(ref, rel=1e-8, abs=1e-7), desc
        np.testing.assert_allclose(mean, post.mean(self.xs), atol=1e-7, rtol=0, err_msg=desc)
        assert res <= 1e-10, desc


def _batch(agp, name, SEG):
    """(m, n, d, kind, transform, diagonal noise, mean, DTC) per problem: every M, n, D, kind, transform, noise and mean form of the issue, VFE and DTC mixed."""
    if name == "per_problem":
        rows = [(1, 1, 1, 0, 0, False, None, False), (63, 63, 3, 1, 1, True, 0.7, True), (64, 64, 16, 2, 2, False, None, False),
                (65, 65, 3, 3, 0, True, None, True), (128, SEG - 1, 1, 0, 1, False, -0.4, False), (65, SEG, 3, 1, 2, True, None, False),
                (63, SEG + 1, 16, 2, 0, False, 1.1, True), (128, 2 * SEG + 37, 3, 3, 2, True, 0.3, False)]
        return [Problem(agp, 10 + i, *r) for i, r in enumerate(rows)]
    n, d = SEG + 1, 3  # one (x, y) object for every problem: the nx = ny = 1 route
    X = np.random.default_rng(6999).uniform(-2, 2, (n, d))
    data = (agp.RowVecs(X), np.cos(X.sum(1)))
    rows = [(1, 0, 0, False, None, True), (64, 1, 1, False, None, False), (128, 2, 2, False, None, False), (65, 3, 1, False, None, True)]
    return [Problem(agp, 30 + i, m, n, d, kind, tr, vec, mean, dtc, data=data) for i, (m, kind, tr, vec, mean, dtc) in enumerate(rows)]


def _call(agp, ps, **kw):
    return agp.elbo_batch([p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps], return_alpha=True, return_m_eps=True, **kw)


@pytest.mark.parametrize("name", ["per_problem", "shared"])
def test_batch_matches_oracle(agp, kernels_on, name):
    ps = _batch(agp, name, kernels_on)
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    obj, alphas, m_eps = _call(agp, ps)
    assert ctx.get_param(COUNTER) - served == len(ps)
    for b, p in enumerate(ps):
        p.check(obj[b], alphas[b], m_eps[b], f"{name}[{b}] m={p.m} n={len(p.y)}")


def test_routing_mixes_kernel_and_single_path(agp, kernels_on):
    ps = [Problem(agp, 50, 40, 300, 2, 0, 1, False, None, False), Problem(agp, 51, 129, 300, 2, 1, 0, True, 0.2, True),
          Problem(agp, 52, 64, 200, 3, 2, 2, False, None, False)]
    p32 = Problem(agp, 53, 20, 150, 2, 0, 0, False, None, False)
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    fx32, y32 = p32.f(agp.RowVecs(p32.x.X.astype(np.float32)), p32.sig), p32.y.astype(np.float32)
    obj, alphas, m_eps = agp.elbo_batch([p.approx for p in ps + [p32]], [p.fx for p in ps] + [fx32], [p.y for p in ps] + [y32], return_alpha=True,
                                        return_m_eps=True)
    assert ctx.get_param(COUNTER) - served == 2
    for b in (0, 2):
        ps[b].check(obj[b], alphas[b], m_eps[b], f"kernel-served[{b}]")
    # the routed problems ARE their single calls: the same path, the same bits
    single = agp.posterior(ps[1].approx, ps[1].fx, ps[1].y)
    assert obj[1] == single.objective and np.array_equal(alphas[1], single.data.alpha) and np.array_equal(m_eps[1], single.data["m_eps"])
    s32 = agp.posterior(p32.approx, fx32, y32)
    assert alphas[3].dtype == np.float32 and np.float32(obj[3]) == s32.objective and np.array_equal(alphas[3], s32.data.alpha)
    assert np.array_equal(m_eps[3], s32.data["m_eps"])


def test_bits_do_not_depend_on_the_batch(agp, kernels_on):
    SEG = kernels_on
    ps = [Problem(agp, 60 + i, m, n, 2, i % 4, i % 3, i % 2 == 0, None, i % 2 == 1)
          for i, (m, n) in enumerate([(100, 2 * SEG + 37), (1, 5), (64, 64), (33, 700), (128, 130), (65, SEG), (17, 90)])]
    alone = _call(agp, ps[:1])
    first = _call(agp, ps)
    last = _call(agp, ps[1:] + ps[:1])
    again = _call(agp, ps)
    for r, b in ((first, 0), (last, 6), (again, 0)):
        assert r[0][b] == alone[0][0] and np.array_equal(r[1][b], alone[1][0]) and np.array_equal(r[2][b], alone[2][0])


def test_failure_is_data(agp, kernels_on):
    good = [Problem(agp, 70, 30, 200, 2, 0, 1, False, None, False), Problem(agp, 71, 70, 500, 3, 3, 0, True, 0.5, True)]
    bad = Problem(agp, 72, 40, 300, 2, 0, 0, False, None, False, jitter=0.0, dup_z=True, variance=1.0)  # K_zz[:2, :2] is exactly [[1, 1], [1, 1]]
    with pytest.raises(o.PosDefException):  # a genuine failure: the oracle's Cholesky of K_zz refuses it too
        o.vfe_posterior(bad.of, bad.z, 0.0, bad.ofx, bad.y)
    ps = [good[0], bad, good[1]]
    with pytest.raises(agp.PosDefException):
        _call(agp, ps)
    obj, alphas, m_eps = _call(agp, ps, on_error="nan")
    assert np.isnan(obj[1]) and np.isnan(alphas[1]).all() and np.isnan(m_eps[1]).all()
    approxs, fxs, ys = [p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps]
    with pytest.raises(agp.PosDefException) as e:
        agp.elbo_batch(approxs, fxs, ys)
    assert e.value.info > 0 and e.value.index == 1
    for b in (0, 2):
        alone = _call(agp, [ps[b]])
        assert obj[b] == alone[0][0] and np.array_equal(alphas[b], alone[1][0]) and np.array_equal(m_eps[b], alone[2][0])
