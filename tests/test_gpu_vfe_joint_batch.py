"""GPU: agp.approx_joint_batch (gp_vfe_joint_batch: vfe_predict_kernel<false, true>, vfe_jcov_kernel, batch_jfact_kernel behind the sparse fit) — mean, latent
covariance, held-out logpdf and joint samples of many small sparse GPs in one call — against the oracle alone: vfe_posterior(...).mean_and_cov(xs),
logpdf(FiniteGP(post, xs, Σy*), ys) and rand_from(...) (src/sparse_approximations.jl:183-217, src/finite_gp_projection.jl:233-237, 306-311).

Bounds.  mean 1e-7 and covariance entries 1e-8 absolute: what the project grants gp_vfe_predict (tests/test_gpu_vfe_predict_batch.py).  Held-out logpdf: the
larger of 1e-8 relative to max(|ref|, 1) (the sparse objective's bound) and 4 × the worst error of the SINGLE path (agp.posterior(approx, fx, y) -> agp.logpdf /
agp.rand of post(xs, Σy*)) against the oracle on the same table; samples: the larger of 1e-7 (the mean's bound) and 4 × the single path's.  Σy* is 1.3e-2 σ² or a
vector in [1e-2, 5e-2] σ², so the joint matrix's condition number stays below 1 + 100 ns (λ_max <= tr C* <= ns σ², λ_min >= min Σy*).
Measured on the MI355X over the two tables: single path 1.3e-14 (held-out logpdf) and 3.7e-13 (samples), so 4 × stays below both floors; gp_vfe_joint_batch
itself 4.0e-14 (mean), 2.9e-14 (covariance), 1.4e-13 (held-out logpdf) and 1.5e-13 (samples)."""
import functools

import numpy as np
import pytest

from oracle import gp_oracle as o
from tests.test_gpu_vfe_batch import Problem
from tests.test_gpu_vfe_predict_batch import _points

pytestmark = pytest.mark.gpu
COUNTER = "vfe_joint_batch_kernel_problems"
NSAMP = 3
SINGLE_HL, SINGLE_S = 1.3e-14, 3.7e-13  # the single path's worst errors against the oracle on the tables below (docstring)
M_TOL, C_TOL, HL_TOL, S_TOL = 1e-7, 1e-8, max(1e-8, 4 * SINGLE_HL), max(1e-7, 4 * SINGLE_S)


@pytest.fixture()
def pseg(agp, monkeypatch):
    """The measurement overrides: the kernels take every n and ns of this file whatever the header's thresholds route to them.  Returns the predict SEG."""
    for name, v in (("GPMI_VFE_JOINT_BATCH_MAX_N", "4096"), ("GPMI_VFE_PREDICT_BATCH_MAX_N", "4096"), ("GPMI_VFE_JOINT_BATCH_MAX_NS", "1024")):
        monkeypatch.setenv(name, v)
    return agp._lib.vfe_predict_batch_limits()["SEG"]


class Joint:
    """The test side of problem p: ns test points (pseudo-inputs and training inputs first), Σy* (scalar, or a vector with vec), y*, ξ, and the oracle's answers."""

    def __init__(self, agp, p, ns, seed, vec, t=None):
        rng = np.random.default_rng(seed)
        s2 = p.of.kernel.variance
        self.p, self.ns = p, ns
        self.t = _points(p, ns, seed) if t is None else t
        self.xs = agp.RowVecs(self.t)
        self.nz = rng.uniform(1e-2, 5e-2, ns) * s2 if vec else 1.3e-2 * s2
        self.ys, self.xi = rng.standard_normal(ns), rng.standard_normal((ns, NSAMP))
        self.ref = None

    def oracle(self):
        if self.ref is None:
            post = o.vfe_posterior(self.p.of, self.p.z, self.p.jitter, self.p.ofx, self.p.y)
            m, C = post.mean_and_cov(self.t) if self.ns else (np.empty(0), np.empty((0, 0)))
            fs = o.FiniteGP(post, self.t, self.nz)
            self.ref = (m, C, o.logpdf(fs, self.ys) if self.ns else 0.0, o.rand_from(fs, self.xi) if self.ns else self.xi)
        return self.ref

    def errs(self, q):
        """largest deviations of (mean, cov, held-out logpdf, samples) from the oracle, None for what q does not hold"""
        r = self.oracle()
        e = [None if v is None else float(np.max(np.abs(np.asarray(v) - w), initial=0.0)) for v, w in zip(q, r)]
        if e[2] is not None:
            e[2] /= max(abs(r[2]), 1.0)
        return e


@functools.lru_cache(None)  # the table's problems are built once, and so are their oracle answers (Joint.oracle)
def _table(agp, name, P):
    """(m, n, d, kind, transform, diagonal noise, mean, DTC, ns, vector Σy*) per problem: every M, ns, D, kind, transform, noise, mean and approximation of the issue"""
    if name == "per_problem":
        rows = [(1, 1, 1, 0, 0, False, None, False, 1, False), (63, 63, 3, 1, 1, True, 0.7, True, 31, True), (64, 64, 16, 2, 2, False, None, False, 32, False),
                (65, 65, 3, 3, 0, True, None, True, 33, True), (128, 300, 1, 0, 1, False, -0.4, False, 63, False), (65, 200, 3, 1, 2, True, None, False, 64, True),
                (63, 400, 16, 2, 0, False, 1.1, True, 65, False), (128, 400, 3, 3, 2, True, 0.3, False, 129, True), (64, 150, 2, 0, 2, False, None, False, 300, False),
                (128, 250, 3, 2, 1, False, None, True, P + 1, True), (40, 100, 2, 0, 0, False, None, False, 0, False)]
        ps = [Problem(agp, 410 + i, *r[:8]) for i, r in enumerate(rows)]
        return [Joint(agp, p, r[8], 500 + i, r[9]) for i, (p, r) in enumerate(zip(ps, rows))]
    X = np.random.default_rng(6997).uniform(-2, 2, (300, 3))  # one (x, y) object and ONE set of test points for every problem: nx = ny = nxs = 1
    data = (agp.RowVecs(X), np.cos(X.sum(1)))
    rows = [(1, 0, 0, False, None, True), (64, 1, 1, False, 0.5, False), (128, 2, 2, False, None, False), (65, 3, 1, False, None, True)]
    ps = [Problem(agp, 430 + i, m, 300, 3, kind, tr, vec, mean, dtc, data=data) for i, (m, kind, tr, vec, mean, dtc) in enumerate(rows)]
    t = _points(ps[2], 129, 530)
    js = [Joint(agp, p, 129, 531 + i, i % 2 == 1, t=t) for i, p in enumerate(ps)]
    for j in js:
        j.xs = js[0].xs
    return js


def _call(agp, js, what=29, **kw):
    ps = [j.p for j in js]
    if what & 8:
        kw["ys_heldout"] = [j.ys for j in js]
    if what & 16:
        kw["xi"] = [j.xi for j in js]
    return agp.approx_joint_batch([p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps], [j.xs for j in js], noise=[j.nz for j in js], what=what, **kw)


def same_bits(p, q):
    return all((a is None and b is None) or np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(p, q))


@pytest.mark.parametrize("name,what", [("per_problem", 29), ("shared", 29), ("per_problem", 5), ("shared", 8)])
def test_batch_matches_oracle(agp, pseg, name, what):
    js = _table(agp, name, pseg)
    ps = [j.p for j in js]
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    quads, obj = _call(agp, js, what, return_objective=True)
    assert ctx.get_param(COUNTER) - served == len(js)
    assert np.array_equal(obj, agp.elbo_batch([p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps]))
    means, vars_ = agp.approx_mean_and_var_batch([p.approx for p in ps], [p.fx for p in ps], [p.y for p in ps], [j.xs for j in js])
    for b, (j, q) in enumerate(zip(js, quads)):
        assert [v is None for v in q] == [not what & bit for bit in (1, 4, 8, 16)]
        e = j.errs(q)
        print(f"{name}[{b}] what={what} m={j.p.m} ns={j.ns}: mean, cov, held-out logpdf, samples {e}")
        for v, tol in zip(e, (M_TOL, C_TOL, HL_TOL, S_TOL)):
            assert v is None or v <= tol, (b, e)
        if what & 1:
            assert q[0].shape == (j.ns,) and q[0].tobytes() == means[b].tobytes(), b
        if what & 4:
            assert q[1].shape == (j.ns, j.ns) and np.array_equal(q[1], q[1].T), b
            assert np.max(np.abs(np.diag(q[1]) - vars_[b]), initial=0.0) <= 1e-8, b
        assert q[3] is None or q[3].shape == (j.ns, NSAMP)


def test_routing_mixes_kernel_and_single_path(agp, pseg):
    ps = [Problem(agp, 450, 40, 300, 2, 0, 1, False, None, False), Problem(agp, 451, 129, 300, 2, 1, 0, True, 0.2, True),
          Problem(agp, 452, 64, 200, 3, 2, 2, False, None, False)]
    p32 = Problem(agp, 453, 20, 150, 2, 0, 0, False, None, False)
    js = [Joint(agp, p, ns, 550 + i, i == 2) for i, (p, ns) in enumerate(zip(ps + [p32], (70, 40, 33, 35)))]
    fx32, y32 = p32.f(agp.RowVecs(p32.x.X.astype(np.float32)), p32.sig), p32.y.astype(np.float32)
    js[3].xs = agp.RowVecs(js[3].t.astype(np.float32))
    fxs, ys = [p.fx for p in ps] + [fx32], [p.y for p in ps] + [y32]
    ctx = agp.default_context()
    served = ctx.get_param(COUNTER)
    quads = agp.approx_joint_batch([j.p.approx for j in js], fxs, ys, [j.xs for j in js], noise=[j.nz for j in js], ys_heldout=[j.ys for j in js],
                                   xi=[j.xi for j in js])
    assert ctx.get_param(COUNTER) - served == 2
    for b in (0, 2):
        assert all(v <= tol for v, tol in zip(js[b].errs(quads[b]), (M_TOL, C_TOL, HL_TOL, S_TOL))), b
    # the routed problems ARE their single calls: the same path, the same bits
    for b in (1, 3):
        j, post = js[b], agp.posterior(js[b].p.approx, fxs[b], ys[b])
        dt, fs = (np.float32 if b == 3 else np.float64), post(j.xs, j.nz)
        single = (*post.mean_and_cov(j.xs), agp.logpdf(fs, j.ys.astype(dt)), agp.rand(fs, NSAMP, xi=j.xi))
        assert quads[b][0].dtype == dt and same_bits(quads[b], single), b


def test_bits_do_not_depend_on_the_company(agp, pseg):
    ps = [Problem(agp, 460 + i, m, n, 2, i % 4, i % 3, i % 2 == 0, None, i % 2 == 1) for i, (m, n) in enumerate([(100, 400), (1, 5), (64, 64), (128, 130)])]
    js = [Joint(agp, p, ns, 560 + i, i % 2 == 0) for i, (p, ns) in enumerate(zip(ps, [193, 3, 65, 64]))]
    (alone,), obj0 = _call(agp, js[:1], return_objective=True)
    for batch, pos in ((js, 0), (js[1:] + js[:1], 3), (js[2:] + js[:2], 2), (js, 0)):
        quads, obj = _call(agp, batch, return_objective=True)
        assert same_bits(quads[pos], alone) and obj[pos].tobytes() == obj0[0].tobytes(), pos


def test_failure_is_data(agp, pseg):
    good = [Joint(agp, Problem(agp, 470, 30, 200, 2, 0, 1, False, None, False), 40, 570, False),
            Joint(agp, Problem(agp, 471, 70, 300, 3, 3, 0, True, 0.5, True), 70, 571, True)]
    bad = Problem(agp, 472, 40, 300, 2, 0, 0, False, None, False, jitter=0.0, dup_z=True, variance=1.0)  # K_zz[:2, :2] is exactly [[1, 1], [1, 1]]
    with pytest.raises(o.PosDefException):  # a genuine failure: the oracle's Cholesky of K_zz refuses it too
        o.vfe_posterior(bad.of, bad.z, 0.0, bad.ofx, bad.y)
    bad_fit = Joint(agp, bad, 33, 572, False)
    # a joint covariance that is not positive definite: every test point eight times, no Σy*
    pj = Problem(agp, 473, 50, 200, 2, 0, 1, False, 0.3, False)
    bad_joint = Joint(agp, pj, 32, 573, False, t=np.repeat(np.random.default_rng(574).uniform(-2, 2, (4, 2)), 8, axis=0))
    bad_joint.nz = None
    post = o.vfe_posterior(pj.of, pj.z, pj.jitter, pj.ofx, pj.y)
    with pytest.raises(o.PosDefException):  # the oracle's Cholesky of C* refuses it too
        o.logpdf(o.FiniteGP(post, bad_joint.t, 0.0), bad_joint.ys)
    js = [good[0], bad_fit, bad_joint, good[1]]
    with pytest.raises(agp.PosDefException) as e:
        _call(agp, js)
    assert e.value.info > 0 and e.value.index == 1
    with pytest.raises(agp.PosDefException) as e:
        _call(agp, js[2:])
    assert 1 < e.value.info <= 32 and e.value.index == 0
    quads, obj = _call(agp, js, return_objective=True, on_error="nan")
    assert np.isnan(obj[1]) and all(np.isnan(np.asarray(v)).all() for v in quads[1]) and quads[1][1].shape == (33, 33)
    q, (m_o, C_o) = quads[2], post.mean_and_cov(bad_joint.t)
    assert np.isfinite(obj[2]) and np.isnan(q[2]) and np.isnan(q[3]).all()  # NaN in the held-out logpdf and the samples only
    assert np.max(np.abs(q[0] - m_o)) <= M_TOL and np.max(np.abs(q[1] - C_o)) <= C_TOL and np.array_equal(q[1], q[1].T)
    for b in (0, 3):
        (alone,), obj1 = _call(agp, [js[b]], return_objective=True)
        assert same_bits(quads[b], alone) and obj[b].tobytes() == obj1[0].tobytes(), b
