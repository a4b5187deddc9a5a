"""GPU: exact GPs with composite kernels Σ_t σ_t² Π_f κ_f (include/gpmi355.h gp_ksum) — kmat_sum_kernel / kvec_sum_kernel / kgrad_sum_kernel and the
*_sum entry points, against the fp64 NumPy reference of tests/test_composite_cpu.py, SciPy factorisations on the host and scikit-learn."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from tests.composite_ref import dense_data as _dense_data, mauna_loa_kernel, ml_kernel as _ml_kernel, ref_kernelmatrix

pytestmark = pytest.mark.gpu

SE, M12, M32, M52 = agp.SqExponentialKernel, agp.Matern12Kernel, agp.Matern32Kernel, agp.Matern52Kernel


def _base(kind, d):
    return {0: SE(), 1: M12(), 2: M32(), 3: M52(), 4: agp.PeriodicKernel(r=np.linspace(0.6, 1.1, d)), 5: agp.RationalQuadraticKernel(alpha=1.3),
            6: agp.WhiteKernel()}[kind]


def _transformed(kind, tr, d):
    k = 1.7 * _base(kind, d)
    if tr == "scale":
        return k @ agp.ScaleTransform(0.8)
    if tr == "ard":
        return k @ agp.ARDTransform(np.linspace(0.5, 1.2, d))
    return k


def _mauna_loa_data(n, seed=0):
    """Seeded monthly series: x in years since 1958, trend + seasonal + noise (the shape of examples/1-mauna-loa)."""
    rng = np.random.default_rng(seed)
    x = np.arange(n) / 12.0
    y = 0.02 * x**2 + 1.3 * x + 3.0 * np.sin(2 * np.pi * x) + 0.8 * np.cos(4 * np.pi * x) + 0.3 * rng.standard_normal(n)
    return x, y - y.mean()


def _host_fit(K, noise, y):
    C = K + np.diag(np.broadcast_to(noise, (K.shape[0],)))
    L = sla.cholesky(C, lower=True)
    alpha = sla.cho_solve((L, True), y)
    lp = -0.5 * (len(y) * math.log(2 * math.pi) + 2 * np.sum(np.log(np.diag(L))) + y @ alpha)
    return lp, alpha, L


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


# ---- 1. kernel matrix -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 16])
@pytest.mark.parametrize("kind", range(7))
@pytest.mark.parametrize("tr", ["none", "scale", "ard"])
def test_kernelmatrix_of_each_base_kind(agp, kind, tr, d):
    rng = np.random.default_rng(kind * 100 + d)
    X = rng.uniform(1, 10, size=(150, d)) / math.sqrt(d)
    Z = rng.uniform(1, 10, size=(70, d)) / math.sqrt(d)
    k = agp.KernelSum((_transformed(kind, tr, d),))  # a one-term sum: kinds 0..3 take the composite path too
    scale = agp.api._prior_variance(k)
    Kd = agp.kernelmatrix(k, agp.RowVecs(X))
    np.testing.assert_allclose(Kd, ref_kernelmatrix(k, X), rtol=0, atol=1e-13 * scale)
    assert np.array_equal(Kd, Kd.T)
    np.testing.assert_allclose(agp.kernelmatrix(k, agp.RowVecs(X), agp.RowVecs(Z)), ref_kernelmatrix(k, X, Z), rtol=0, atol=1e-13 * scale)


def test_kernelmatrix_of_the_mauna_loa_form_and_white_on_duplicates(agp):
    x, _ = _mauna_loa_data(700)
    k = mauna_loa_kernel()
    scale = agp.api._prior_variance(k)
    np.testing.assert_allclose(agp.kernelmatrix(k, x), ref_kernelmatrix(k, x), rtol=0, atol=1e-13 * scale)
    z = np.concatenate([x[::7], x[5:40] + 0.01])
    np.testing.assert_allclose(agp.kernelmatrix(k, x, z), ref_kernelmatrix(k, x, z), rtol=0, atol=1e-13 * scale)
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 2, size=(90, 3))
    X[40:60] = X[:20]  # duplicates: White is 1 wherever two inputs are equal in every coordinate
    kw = 0.5 * SE() @ agp.ScaleTransform(1.5) + 0.3 * agp.WhiteKernel()
    Kd = agp.kernelmatrix(kw, agp.RowVecs(X))
    np.testing.assert_allclose(Kd, ref_kernelmatrix(kw, X), rtol=0, atol=1e-13)
    assert Kd[45, 5] == pytest.approx(0.8, abs=1e-14)


# ---- 2. agreement with the single-kind path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(4))
@pytest.mark.parametrize("tr", ["none", "scale", "ard"])
def test_one_factor_composite_agrees_with_the_single_kind_path(agp, kind, tr):
    rng = np.random.default_rng(10 + kind)
    X = rng.uniform(0, 3, size=(700, 3))
    y = rng.standard_normal(700)
    k = _transformed(kind, tr, 3)
    ks = agp.KernelSum((k,))
    f, fs = agp.GP(k), agp.GP(ks)
    lp, lps = agp.logpdf(f(agp.RowVecs(X), 0.05), y), agp.logpdf(fs(agp.RowVecs(X), 0.05), y)
    assert lps == pytest.approx(lp, rel=1e-12)
    p, ps = agp.posterior(f(agp.RowVecs(X), 0.05), y), agp.posterior(fs(agp.RowVecs(X), 0.05), y)
    assert _rel(ps.data.alpha, p.data.alpha) <= 1e-9
    assert ps.logpdf_value == pytest.approx(lp, rel=1e-12)
    xs = agp.RowVecs(rng.uniform(0, 3, size=(90, 3)))  # D = 3: the predictive mean of kvec_sum_kernel's D <= 4 instance
    assert _rel(ps.mean(xs), p.mean(xs)) <= 1e-9
    np.testing.assert_allclose(ps.var(xs), p.var(xs), rtol=0, atol=1e-9 * 1.7)


# ---- 3. logpdf and α against the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 4096, 12288])
def test_logpdf_and_alpha_against_a_host_cholesky(agp, n):
    x, y = _dense_data(n, seed=n)
    k = _ml_kernel()
    lp_h, a_h, _ = _host_fit(ref_kernelmatrix(k, x), 0.1, y)
    f = agp.GP(k)
    lp = agp.logpdf(f(x, 0.1), y)
    assert lp == pytest.approx(lp_h, rel=1e-10)
    post = agp.posterior(f(x, 0.1), y)
    assert _rel(post.data.alpha, a_h) <= 1e-8
    assert post.logpdf_value == pytest.approx(lp_h, rel=1e-10)


def test_logpdf_against_sklearn_gaussian_process_regressor(agp):
    gpr_mod = pytest.importorskip("sklearn.gaussian_process")
    skk = pytest.importorskip("sklearn.gaussian_process.kernels")
    x, y = _mauna_loa_data(2000, seed=7)
    k = (4.0 * agp.with_lengthscale(SE(), 20.0) + 2.0 * agp.with_lengthscale(agp.PeriodicKernel(r=[0.6]), 1.0) * agp.with_lengthscale(SE(), 50.0)
         + 0.5 * agp.with_lengthscale(agp.RationalQuadraticKernel(alpha=0.9), 1.5))
    theirs = (skk.ConstantKernel(4.0) * skk.RBF(20.0) + skk.ConstantKernel(2.0) * skk.ExpSineSquared(1.2, 1.0) * skk.RBF(50.0)
              + skk.ConstantKernel(0.5) * skk.RationalQuadratic(1.5, alpha=0.9))
    gpr = gpr_mod.GaussianProcessRegressor(theirs, alpha=0.04, optimizer=None).fit(x[:, None], y)
    lp = agp.logpdf(agp.GP(k)(x, 0.04), y)
    assert lp == pytest.approx(gpr.log_marginal_likelihood(gpr.kernel_.theta), rel=1e-10)


# ---- 4. composite posterior ------------------------------------------------------------------------------------------------------------
def test_composite_posterior_predictions_logpdf_rand_and_update(agp):
    x, y = _mauna_loa_data(1500, seed=11)
    k = mauna_loa_kernel()
    s2 = 0.02
    f = agp.GP(k)
    post = agp.posterior(f(x, s2), y)
    rng = np.random.default_rng(12)
    xs = np.concatenate([x[rng.choice(len(x), 60, replace=False)], rng.uniform(0, x[-1] + 2, 240)])  # some equal to training inputs
    Kxx, Ksx, Kss = ref_kernelmatrix(k, x), ref_kernelmatrix(k, xs, x), ref_kernelmatrix(k, xs)
    _, a_h, L = _host_fit(Kxx, s2, y)
    V = sla.solve_triangular(L, Ksx.T, lower=True)
    m_h, C_h = Ksx @ a_h, Kss - V.T @ V
    m, c = post.mean_and_cov(xs)
    v = post.var(xs)
    sc = agp.api._prior_variance(k)
    np.testing.assert_allclose(m, m_h, rtol=0, atol=1e-8 * np.abs(m_h).max())
    np.testing.assert_allclose(c, C_h, rtol=0, atol=1e-9 * sc)
    np.testing.assert_allclose(v, np.diag(C_h), rtol=0, atol=1e-9 * sc)
    # held-out logpdf under post(x*, σ²*) and the sampling transform
    ys = m_h + 0.1 * rng.standard_normal(len(xs))
    lp_h = -0.5 * (len(xs) * math.log(2 * math.pi) + np.linalg.slogdet(C_h + 0.05 * np.eye(len(xs)))[1]
                   + (ys - m_h) @ np.linalg.solve(C_h + 0.05 * np.eye(len(xs)), ys - m_h))
    assert agp.logpdf(post(xs, 0.05), ys) == pytest.approx(lp_h, rel=1e-9)
    xi = rng.standard_normal((len(xs), 2))
    Lh = np.linalg.cholesky(C_h + 0.05 * np.eye(len(xs)))
    np.testing.assert_allclose(agp.rand(post(xs, 0.05), 2, xi=xi), m_h[:, None] + Lh @ xi, rtol=0, atol=1e-7)
    # sequential conditioning equals the batch fit
    p1 = agp.posterior(f(x[:900], s2), y[:900])
    p2 = agp.posterior(p1(x[900:], s2), y[900:])
    assert _rel(p2.data.alpha, post.data.alpha) <= 1e-8
    assert p2.logpdf_value == pytest.approx(post.logpdf_value, rel=1e-8)
    assert _rel(p2.mean(xs), m) <= 1e-8


def test_conformance_suite_on_a_composite_prior_and_posterior(agp):
    from tests.test_gpu_api import _internal_interface

    rng = np.random.default_rng(123456)
    k = (agp.with_lengthscale(SE(), 1.3) + 0.5 * agp.with_lengthscale(agp.PeriodicKernel(r=[0.8]), 0.9) * M32()
         + 0.3 * agp.RationalQuadraticKernel(alpha=2.0))
    f = agp.GP(k)
    x, z = rng.random(31) * 3, rng.random(17) * 3
    _internal_interface(agp, rng, f, x, z, np.float64, atol=1e-9, s2=1e-1, vfe_checks=False)
    y = np.sin(x) + 0.1 * rng.standard_normal(31)
    post = agp.posterior(f(x, 0.1), y)
    _internal_interface(agp, rng, post, rng.random(17) * 3, rng.random(11) * 3, np.float64, atol=1e-9, s2=1e-1, vfe_checks=False)


# ---- 5. gradient ---------------------------------------------------------------------------------------------------------------------
def test_gradient_against_sklearn_log_marginal_likelihood(agp):
    skk = pytest.importorskip("sklearn.gaussian_process.kernels")
    gpr_mod = pytest.importorskip("sklearn.gaussian_process")
    x, y = _mauna_loa_data(2000, seed=21)
    c1, l1, c2, r, per, l3, c3, a, l4, s2 = 4.0, 20.0, 2.0, 0.6, 1.0, 50.0, 0.5, 0.9, 1.5, 0.04
    k = (c1 * agp.with_lengthscale(SE(), l1) + c2 * agp.with_lengthscale(agp.PeriodicKernel(r=[r]), per) * agp.with_lengthscale(SE(), l3)
         + c3 * agp.with_lengthscale(agp.RationalQuadraticKernel(alpha=a), l4))
    theirs = (skk.ConstantKernel(c1) * skk.RBF(l1) + skk.ConstantKernel(c2) * skk.ExpSineSquared(2 * r, per) * skk.RBF(l3)
              + skk.ConstantKernel(c3) * skk.RationalQuadratic(l4, alpha=a) + skk.WhiteKernel(s2))
    gpr = gpr_mod.GaussianProcessRegressor(theirs, alpha=0.0, optimizer=None).fit(x[:, None], y)
    lml, G = gpr.log_marginal_likelihood(gpr.kernel_.theta, eval_gradient=True)
    lp, g = agp.logpdf_and_grad(agp.GP(k)(x, s2), y)
    assert lp == pytest.approx(lml, rel=1e-10)
    th = g["theta"]  # C-ABI θ: c1, s1 | c2, s_per, r, s3 | c3, s4, α
    # sklearn (log-parameters, by name within each kernel): c1, l1 | c2, l_ess, p | l3 | c3, α, l4 | noise
    mine = [c1 * th[0], -th[1] / l1, c2 * th[2], r * th[4], -th[3] / per, -th[5] / l3, c3 * th[6], a * th[8], -th[7] / l4, s2 * g["noise"]]
    gi = np.abs(G).max()
    for p, (ours, ref) in enumerate(zip(mine, G)):
        assert abs(ours - ref) <= 1e-7 * max(abs(ref), 1e-3 * gi), (p, ours, ref)
    # ∂/∂y = −α
    np.testing.assert_allclose(g["y"], -gpr.alpha_, rtol=0, atol=1e-8 * np.abs(gpr.alpha_).max())


def _host_grad(k, X, s2, y):
    K, dK = ref_kernelmatrix(k, X, grad=True)
    _, a, L = _host_fit(K, s2, y)
    Ci = sla.cho_solve((L, True), np.eye(len(y)))
    W = np.outer(a, a) - Ci
    return np.array([0.5 * np.sum(W * D) for D in dK]), 0.5 * (a @ a - np.trace(Ci))


def test_gradient_against_the_host_formula_with_periodic_ard_and_white(agp):
    rng = np.random.default_rng(31)
    X = rng.uniform(0, 4, size=(3000, 3))
    X[2000:2100] = X[:100]
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(3000)
    k = (1.5 * agp.PeriodicKernel(r=[0.7, 0.9, 1.1]) @ agp.ARDTransform([0.5, 0.8, 0.6]) * agp.with_lengthscale(M52(), 2.0)
         + 0.7 * agp.RationalQuadraticKernel(alpha=1.2) @ agp.ARDTransform([0.9, 1.1, 0.7]) + 0.05 * agp.WhiteKernel())
    gt, gn = _host_grad(k, X, 0.05, y)
    lp, g = agp.logpdf_and_grad(agp.GP(k)(agp.RowVecs(X), 0.05), y)
    gi = np.abs(gt).max()
    np.testing.assert_allclose(g["theta"], gt, rtol=1e-7, atol=1e-9 * gi)
    assert g["noise"] == pytest.approx(gn, rel=1e-8)
    nf = agp.api._NormalForm(k)
    np.testing.assert_allclose(g["kernel"], nf.chain(gt), rtol=1e-7, atol=1e-9 * gi)


@pytest.mark.parametrize("d", [8, 16])
def test_posterior_and_gradient_in_many_dimensions(agp, d):
    """D = 8 and 16: the D <= 16 instances of kmat_sum_kernel, kvec_sum_kernel and kgrad_sum_kernel, in fp64 against the host and in fp32
    (Float32 in -> Float32 out) with the fp32 tolerances of test_fp32_composite_fit.  θ has 29 / 53 entries: two / four gradient launches."""
    rng = np.random.default_rng(100 + d)
    n, s2 = 1000, 0.1
    X = rng.uniform(0, 2, size=(n, d))
    y = np.sin(X.sum(1) / 2) + 0.1 * rng.standard_normal(n)
    k = (1.2 * (agp.PeriodicKernel(r=np.linspace(0.8, 1.4, d)) @ agp.ARDTransform(np.linspace(0.2, 0.5, d))) * agp.with_lengthscale(M32(), 3.0)
         + 0.5 * agp.RationalQuadraticKernel(alpha=1.1) @ agp.ARDTransform(np.linspace(0.3, 0.6, d)) + 0.05 * agp.WhiteKernel())
    Xs = np.concatenate([X[:20], rng.uniform(0, 2, size=(180, d))])
    Kxx, Ksx, Kss = ref_kernelmatrix(k, X), ref_kernelmatrix(k, Xs, X), ref_kernelmatrix(k, Xs)
    lp_h, a_h, L = _host_fit(Kxx, s2, y)
    V = sla.solve_triangular(L, Ksx.T, lower=True)
    m_h, v_h = Ksx @ a_h, np.diag(Kss) - np.sum(V * V, axis=0)
    sc = agp.api._prior_variance(k)
    f = agp.GP(k)
    post = agp.posterior(f(agp.RowVecs(X), s2), y)
    m, v = post.mean_and_var(agp.RowVecs(Xs))
    np.testing.assert_allclose(m, m_h, rtol=0, atol=1e-8 * np.abs(m_h).max())
    np.testing.assert_allclose(v, v_h, rtol=0, atol=1e-9 * sc)
    gt, gn = _host_grad(k, X, s2, y)
    lp, g = agp.logpdf_and_grad(f(agp.RowVecs(X), s2), y)
    assert lp == pytest.approx(lp_h, rel=1e-10)
    np.testing.assert_allclose(g["theta"], gt, rtol=1e-7, atol=1e-9 * np.abs(gt).max())
    assert g["noise"] == pytest.approx(gn, rel=1e-8)
    X32, y32 = X.astype(np.float32), y.astype(np.float32)
    p32 = agp.posterior(f(agp.RowVecs(X32), s2), y32)
    m32 = p32.mean(agp.RowVecs(Xs.astype(np.float32)))
    assert m32.dtype == np.float32 and _rel(m32, m_h) <= 5e-3
    lp32, g32 = agp.logpdf_and_grad(f(agp.RowVecs(X32), s2), y32)
    assert isinstance(lp32, np.float32) and float(lp32) == pytest.approx(lp_h, rel=2e-4)
    np.testing.assert_allclose(g32["theta"], gt, rtol=5e-3, atol=5e-3 * np.abs(gt).max())


def test_gradient_longer_than_one_launch_and_a_shared_parameter(agp):
    """θ of 25 entries (two 16-entry launches) and a variance shared by two terms."""
    rng = np.random.default_rng(41)
    X = rng.uniform(0, 3, size=(1200, 4))
    y = np.cos(X[:, 0]) + 0.1 * rng.standard_normal(1200)
    k = (0.9 * (SE() @ agp.ARDTransform([0.6, 0.7, 0.8, 0.9]) + M32() @ agp.ARDTransform([0.5, 0.4, 0.3, 0.6]))
         * (agp.PeriodicKernel(r=[1.0, 1.1, 1.2, 1.3]) @ agp.ARDTransform([0.3, 0.2, 0.25, 0.35]))
         + 0.2 * agp.RationalQuadraticKernel(alpha=0.8) @ agp.ScaleTransform(0.9))
    nf = agp.api._NormalForm(k)
    assert len(nf.theta()) > 16
    gt, _ = _host_grad(k, X, 0.1, y)
    lp, g = agp.logpdf_and_grad(agp.GP(k)(agp.RowVecs(X), 0.1), y)
    np.testing.assert_allclose(g["theta"], gt, rtol=1e-7, atol=1e-9 * np.abs(gt).max())
    np.testing.assert_allclose(g["kernel"], nf.chain(gt), rtol=1e-7, atol=1e-9 * np.abs(gt).max())


def test_gradient_against_a_central_difference_at_16384(agp):
    x, y = _mauna_loa_data(16384, seed=51)
    k = mauna_loa_kernel()
    s2 = 0.02
    lp, g = agp.logpdf_and_grad(agp.GP(k)(x, s2), y)
    p0 = agp.params(k)
    v = np.random.default_rng(52).standard_normal(len(p0))
    h = 1e-5
    lpp = agp.logpdf(agp.GP(agp.with_params(k, p0 * np.exp(h * v)))(x, s2), y)  # along a direction in log-parameter space
    lpm = agp.logpdf(agp.GP(agp.with_params(k, p0 * np.exp(-h * v)))(x, s2), y)
    fd = (lpp - lpm) / (2 * h)
    an = float(np.dot(g["kernel"] * p0, v))
    assert an == pytest.approx(fd, rel=1e-5)


# ---- 6. fp32 -------------------------------------------------------------------------------------------------------------------------
def test_fp32_composite_fit(agp):
    rng = np.random.default_rng(61)
    n = 4096
    x = np.sort(rng.uniform(0, 6, n))
    y = np.sin(2 * x) + 0.5 * np.cos(7 * x) + 0.1 * rng.standard_normal(n)
    k = (agp.with_lengthscale(SE(), 1.5) + 0.5 * agp.with_lengthscale(agp.PeriodicKernel(r=[0.8]), 0.9) * agp.with_lengthscale(SE(), 3.0)
         + 0.2 * agp.RationalQuadraticKernel(alpha=1.5))
    s2 = 0.05
    lp_h, a_h, L = _host_fit(ref_kernelmatrix(k, x), s2, y)
    f = agp.GP(k)
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    lp = agp.logpdf(f(x32, s2), y32)
    assert isinstance(lp, np.float32)
    assert float(lp) == pytest.approx(lp_h, rel=2e-4)
    post = agp.posterior(f(x32, s2), y32)
    assert post.data.alpha.dtype == np.float32
    assert _rel(post.data.alpha, a_h) <= 5e-3
    xs = rng.uniform(0, 6, 200)
    m_h = ref_kernelmatrix(k, xs, x) @ a_h
    m = post.mean(xs.astype(np.float32))
    assert m.dtype == np.float32
    assert _rel(m, m_h) <= 5e-3
    gt, _ = _host_grad(k, x, s2, y)
    lp32, g32 = agp.logpdf_and_grad(f(x32, s2), y32)
    np.testing.assert_allclose(g32["theta"], gt, rtol=5e-3, atol=5e-3 * np.abs(gt).max())


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_mode", ["no_atomics"], indirect=True)
def test_composite_fits_are_bitwise_repeatable_without_atomics(agp, exact_mode):
    x, y = _mauna_loa_data(3000, seed=71)
    f = agp.GP(mauna_loa_kernel())
    a, b = agp.logpdf(f(x, 0.02), y), agp.logpdf(f(x, 0.02), y)
    assert a.tobytes() == b.tobytes()
    post = agp.posterior(f(x, 0.02), y)
    xs = np.linspace(0, 260, 333)
    m1, c1 = post.mean_and_cov(xs)
    m2, c2 = post.mean_and_cov(xs)
    assert m1.tobytes() == m2.tobytes() and c1.tobytes() == c2.tobytes()


# ---- 8. statuses ---------------------------------------------------------------------------------------------------------------------
def test_negative_noise_raises_the_single_kind_minor(agp):
    rng = np.random.default_rng(81)
    x = np.sort(rng.uniform(0, 5, 300))
    y = rng.standard_normal(300)
    noise = np.full(300, 0.01)
    noise[137] = -5.0
    k = 2.0 * agp.with_lengthscale(SE(), 0.7)
    with pytest.raises(agp.PosDefException) as single:
        agp.logpdf(agp.GP(k)(x, noise), y)
    with pytest.raises(agp.PosDefException) as comp:
        agp.logpdf(agp.GP(agp.KernelSum((k,)))(x, noise), y)
    assert comp.value.info == single.value.info


def test_multi_device_context_runs_composites_on_its_first_device(agp):
    from tests.conftest import rank_devices

    x, y = _dense_data(2500, seed=91)
    k = _ml_kernel()
    xs = np.linspace(0, 66, 150)
    single = agp.GP(k)
    multi = agp.GP(k, ctx=agp.Context(devices=rank_devices(2), P=2, Q=1))
    assert agp.logpdf(multi(x, 0.1), y) == pytest.approx(agp.logpdf(single(x, 0.1), y), rel=1e-12)
    pm, ps = agp.posterior(multi(x, 0.1), y), agp.posterior(single(x, 0.1), y)
    assert _rel(pm.data.alpha, ps.data.alpha) <= 1e-12
    mm, vm = pm.mean_and_var(xs)
    ms, vs = ps.mean_and_var(xs)
    assert _rel(mm, ms) <= 1e-12 and _rel(vm, vs) <= 1e-12


def test_vfe_with_a_composite_kernel_is_refused(agp):
    x, y = _mauna_loa_data(200)
    f = agp.GP(mauna_loa_kernel())
    with pytest.raises(NotImplementedError, match="composite"):
        agp.posterior(agp.VFE(f(x[::10], 1e-6)), f(x, 0.1), y)
    with pytest.raises(NotImplementedError, match="composite"):
        agp.elbo(agp.VFE(f(x[::10], 1e-6)), f(x, 0.1), y)


# ---- the C ABI's own validation of gp_ksum (the Julia shim relies on it) -------------------------------------------------------------------
def _raw_ksum(terms, dtype=0):
    """gp_ksum from [(variance, [(kind, scale, param), ...]), ...] as given — no mirror-side checks; (struct, buffers to keep alive)."""
    keep = []
    dp = C.POINTER(C.c_double)
    cterms = (agp._lib.gp_kterm * max(len(terms), 1))()
    for t, (var, facs) in enumerate(terms):
        cf = (agp._lib.gp_kfactor * max(len(facs), 1))()
        for j, (kind, sc, par) in enumerate(facs):
            sv, pv = np.array(sc, dtype=np.float64), np.array(par, dtype=np.float64)
            keep += [sv, pv]
            cf[j] = agp._lib.gp_kfactor(kind, len(sc), sv.ctypes.data_as(dp) if len(sc) else None, len(par), pv.ctypes.data_as(dp) if len(par) else None)
        keep.append(cf)
        cterms[t] = agp._lib.gp_kterm(var, len(facs), cf)
    keep.append(cterms)
    return agp._lib.gp_ksum(dtype, len(terms), cterms), keep


SE_F = (0, [], [])


@pytest.mark.parametrize("terms,d,text", [
    ([(1.0, [(6, [2.0], [])])], 2, "WhiteKernel takes no transform"),
    ([(1.0, [(4, [], [1.0])])], 2, "param holds D entries"),
    ([(1.0, [(5, [], [])])], 2, "param holds D entries"),
    ([(1.0, [(0, [], [1.0])])], 2, "param holds D entries"),
    ([(1.0, [(4, [], [1.0, 0.0])])], 2, "must be > 0"),
    ([(1.0, [(5, [], [-1.0])])], 2, "must be > 0"),
    ([(0.0, [SE_F])], 2, "variance must be > 0"),
    ([(1.0, [(7, [], [])])], 2, "kind must be 0..6"),
    ([(1.0, [(0, [1.0, 2.0, 3.0], [])])], 2, "nscale must be 0, 1 or D"),
    ([], 2, "1..8 terms"),
    ([(1.0, [SE_F])] * 9, 2, "1..8 terms"),
    ([(1.0, [])], 2, "1..4 factors per term"),
    ([(1.0, [SE_F] * 5)], 2, "1..4 factors per term"),
    ([(1.0, [SE_F] * 4)] * 4 + [(1.0, [SE_F])], 2, "at most 16 factors"),
    ([(1.0, [(4, [1.0] * 16, [1.0] * 16)])] * 2, 16, "at most 64 entries in theta"),
    ([(1.0, [SE_F])], 17, "D must be <= 16"),
])
def test_malformed_descriptors_are_refused_by_the_library(agp, terms, d, text):
    """include/gpmi355.h gp_ksum: limits and malformed descriptors return −2 (the descriptor argument) with the reason in gp_last_error(), from every
    *_sum entry point, before anything reaches the device."""
    ctx = agp.default_context(0)
    lib = ctx.lib
    ks, keep = _raw_ksum(terms)
    m = agp.api._Marshal(np.float64)
    X = np.random.default_rng(0).uniform(0, 1, size=(40, d))
    px = m.points(agp.RowVecs(X))
    nz = m.noise(0.1, 40)
    y = np.ones(40)
    out = np.empty((40, 40), order="F")
    lp = np.empty(1)
    dth = (C.c_double * 80)()
    h = C.c_void_p()
    calls = [
        lambda: lib.gp_kernelmatrix_sum(ctx.handle, C.byref(ks), C.byref(px), None, out.ctypes.data),
        lambda: lib.gp_logpdf_sum(ctx.handle, C.byref(ks), C.byref(px), C.byref(nz), None, y.ctypes.data, 40, 1, lp.ctypes.data),
        lambda: lib.gp_posterior_fit_sum(ctx.handle, C.byref(ks), C.byref(px), C.byref(nz), None, y.ctypes.data, C.byref(h), None, None),
        lambda: lib.gp_logpdf_grad_sum(ctx.handle, C.byref(ks), C.byref(px), C.byref(nz), None, y.ctypes.data, lp.ctypes.data, dth, None, None),
    ]
    for call in calls:
        assert call() == -2
        assert text in lib.gp_last_error().decode()
    assert not h.value
