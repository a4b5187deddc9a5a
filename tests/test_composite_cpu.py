"""CPU: composite kernels of the Python mirror — the normal form Σ_t σ_t² Π_f κ_f, the θ order of include/gpmi355.h gp_ksum, the chain rule
back to params(k), the limits — and the fp64 NumPy reference of tests/composite_ref.py (what tests/test_gpu_composite.py measures the device
against), pinned here to scikit-learn wherever the two agree."""
import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests.composite_ref import mauna_loa_kernel, ref_from_theta, ref_kernelmatrix


# ---- normal form --------------------------------------------------------------------------------------------------------------------
def test_product_distributes_over_sums_and_collects_variances():
    se, m32 = agp.SqExponentialKernel(), agp.Matern32Kernel()
    per = agp.PeriodicKernel(r=[0.7])
    k = 3.0 * ((2.0 * se + per) * (0.5 * m32 + agp.WhiteKernel()))
    nf = agp.api._NormalForm(k)
    assert len(nf.terms) == 4
    assert [[f[0] for f in fs] for _, fs in nf.terms] == [[0, 2], [0, 6], [4, 2], [4, 6]]
    # params depth-first: ScaledKernel 3, se 2, per (1, r 0.7), m32 0.5, white 1
    np.testing.assert_array_equal(agp.params(k), [3.0, 2.0, 1.0, 0.7, 0.5, 1.0])
    th = nf.theta()
    # term by term σ_t², then each factor's scale and param entries
    assert th == pytest.approx([3 * 2 * 0.5, 3 * 2 * 1, 3 * 1 * 0.5, 0.7, 3 * 1 * 1, 0.7])
    assert agp.api._prior_variance(k) == pytest.approx(3.0 + 6.0 + 1.5 + 3.0)


def test_theta_order_with_transforms():
    k = (2.0 * agp.PeriodicKernel(r=[0.5, 0.25]) @ agp.ARDTransform([1.0, 2.0])) * agp.with_lengthscale(agp.RationalQuadraticKernel(alpha=3.0), 4.0)
    nf = agp.api._NormalForm(k)
    # params: per variance, r (2), ARD v (2); rq variance, α, scale
    np.testing.assert_allclose(agp.params(k), [2.0, 0.5, 0.25, 1.0, 2.0, 1.0, 3.0, 0.25])
    # θ: σ², per scale (2), per r (2), rq scale, rq α
    np.testing.assert_allclose(nf.theta(), [2.0, 1.0, 2.0, 0.5, 0.25, 0.25, 3.0])
    assert agp.with_params(k, agp.params(k)) == k
    k2 = agp.with_params(k, agp.params(k) * 2)
    np.testing.assert_allclose(agp.params(k2), agp.params(k) * 2)
    with pytest.raises(ValueError):
        agp.with_params(k, np.ones(9))


def test_chain_rule_back_to_params_with_a_shared_parameter():
    """A parameter that lands in several terms sums its contributions: (a·SE)·(b·M12 + c·RQ) puts a in two terms; the chain rule of the
    mirror against a central difference of f(params) = w · θ(params)."""
    k = (1.3 * agp.with_lengthscale(agp.SqExponentialKernel(), 0.7)) * (0.4 * agp.Matern12Kernel() + 2.2 * agp.RationalQuadraticKernel(alpha=0.9))
    nf = agp.api._NormalForm(k)
    assert len(nf.terms) == 2
    p0 = agp.params(k)
    w = np.random.default_rng(1).standard_normal(len(nf.theta()))
    g = nf.chain(w)
    for i in range(len(p0)):
        e = np.zeros_like(p0)
        e[i] = 1e-6 * max(1.0, abs(p0[i]))
        fp = np.dot(w, agp.api._NormalForm(agp.with_params(k, p0 + e)).theta())
        fm = np.dot(w, agp.api._NormalForm(agp.with_params(k, p0 - e)).theta())
        assert g[i] == pytest.approx((fp - fm) / (2 * e[i]), rel=1e-7, abs=1e-9), i


def test_transforms_on_composites_are_refused_and_white_drops_its_transform():
    se = agp.SqExponentialKernel()
    with pytest.raises(TypeError):
        (se + se) @ agp.ScaleTransform(2.0)
    with pytest.raises(TypeError):
        agp.with_lengthscale(se * agp.Matern32Kernel(), 2.0)
    w = agp.with_lengthscale(agp.WhiteKernel(), 3.0)
    assert w == agp.WhiteKernel() and agp.params(w).tolist() == [1.0]
    # the single-kind objects keep their fields and their own path
    k = 2.0 * agp.with_lengthscale(agp.Matern32Kernel(), 2.0)
    assert (k.kind, k.variance, k.transform.s) == (2, 2.0, 0.5)
    assert not agp.api._is_composite(k) and agp.api._is_composite(se + se) and agp.api._is_composite(agp.WhiteKernel())


def test_out_of_limit_descriptors_are_refused_by_the_mirror():
    m = agp.api._Marshal(np.float64)
    se = agp.SqExponentialKernel()
    nine = se
    for _ in range(8):
        nine = nine + se
    with pytest.raises(TypeError, match="terms"):
        m.ksum(nine, 1)
    five = se * se * se * se * se
    with pytest.raises(TypeError, match="factors"):
        m.ksum(five, 1)
    seventeen = se * se * se * se
    for _ in range(4):
        seventeen = seventeen + se * se * se * se
    with pytest.raises(TypeError, match="factors in all"):
        m.ksum(seventeen + se, 1)
    big = agp.PeriodicKernel(r=np.ones(16)) @ agp.ARDTransform(np.ones(16))
    with pytest.raises(TypeError, match="theta"):
        m.ksum(big * big, 16)
    with pytest.raises(TypeError, match="D = 17"):
        m.ksum(se + se, 17)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        m.ksum(agp.PeriodicKernel(r=[1.0, 1.0]) + se, 3)
    with pytest.raises(ValueError):
        agp.PeriodicKernel(r=[1.0, -1.0])
    with pytest.raises(ValueError):
        agp.RationalQuadraticKernel(alpha=0.0)
    ks, nf = m.ksum(mauna_loa_kernel(), 1)
    assert (ks.nterms, len(nf.theta())) == (5, 12)


# ---- the NumPy reference against scikit-learn -----------------------------------------------------------------------------------------
def _sk():
    """scikit-learn's kernels, or a skip of the one test that pins against them (nothing else in this module needs them)."""
    return pytest.importorskip("sklearn.gaussian_process.kernels")


def _inputs(n, d, seed=0):
    return np.random.default_rng(seed).uniform(0, 3, size=(n, d))


@pytest.mark.parametrize("d", [1, 3])
def test_reference_matches_sklearn_stationary_kernels(d):
    sk = _sk()
    X, Z = _inputs(40, d, 1), _inputs(31, d, 2)
    ell = 0.8
    pairs = [
        (agp.with_lengthscale(agp.SqExponentialKernel(), ell), sk.RBF(ell)),
        (agp.with_lengthscale(agp.Matern12Kernel(), ell), sk.Matern(ell, nu=0.5)),
        (agp.with_lengthscale(agp.Matern32Kernel(), ell), sk.Matern(ell, nu=1.5)),
        (agp.with_lengthscale(agp.Matern52Kernel(), ell), sk.Matern(ell, nu=2.5)),
        (agp.with_lengthscale(agp.RationalQuadraticKernel(alpha=1.7), ell), sk.RationalQuadratic(ell, alpha=1.7)),
        (2.0 * agp.with_lengthscale(agp.SqExponentialKernel(), ell) + 0.5 * agp.with_lengthscale(agp.Matern32Kernel(), 2.0),
         sk.ConstantKernel(2.0) * sk.RBF(ell) + sk.ConstantKernel(0.5) * sk.Matern(2.0, nu=1.5)),
        (3.0 * agp.with_lengthscale(agp.SqExponentialKernel(), ell) * agp.with_lengthscale(agp.RationalQuadraticKernel(alpha=0.6), 1.5),
         sk.ConstantKernel(3.0) * sk.RBF(ell) * sk.RationalQuadratic(1.5, alpha=0.6)),
    ]
    for ours, theirs in pairs:
        np.testing.assert_allclose(ref_kernelmatrix(ours, X, Z), theirs(X, Z), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ref_kernelmatrix(ours, X), theirs(X), rtol=1e-12, atol=1e-14)


def test_reference_matches_sklearn_periodic_in_one_dimension_and_white_on_distinct_inputs():
    sk = _sk()
    X, Z = _inputs(40, 1, 3), _inputs(25, 1, 4)
    r, period = 0.6, 1.3
    ours = agp.with_lengthscale(agp.PeriodicKernel(r=[r]), period)
    theirs = sk.ExpSineSquared(length_scale=2 * r, periodicity=period)
    np.testing.assert_allclose(ref_kernelmatrix(ours, X, Z), theirs(X, Z), rtol=1e-12, atol=1e-14)
    w = 0.3 * agp.WhiteKernel()
    np.testing.assert_array_equal(ref_kernelmatrix(w, X, Z), sk.WhiteKernel(0.3)(X, Z))  # distinct inputs: zero
    np.testing.assert_allclose(ref_kernelmatrix(w, X), sk.WhiteKernel(0.3)(X))         # x == x' on the diagonal


def test_reference_gradients_match_sklearn_eval_gradient():
    sk = _sk()
    X = _inputs(30, 1, 5)
    # c·SE(ℓ): θ = (c, s = 1/ℓ);  sklearn: (log c, log ℓ):  ∂/∂log c = c ∂/∂c,  ∂/∂log ℓ = −s ∂/∂s
    c, ell = 1.7, 0.9
    K, dK = ref_kernelmatrix(c * agp.with_lengthscale(agp.SqExponentialKernel(), ell), X, grad=True)
    Ks, G = (sk.ConstantKernel(c) * sk.RBF(ell))(X, eval_gradient=True)
    np.testing.assert_allclose(K, Ks, rtol=1e-12)
    np.testing.assert_allclose(c * dK[0], G[..., 0], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(-(1 / ell) * dK[1], G[..., 1], rtol=1e-10, atol=1e-13)
    # RQ(ℓ, α): θ = (c, s, α);  sklearn orders hyperparameters by name: (log α, log ℓ)
    a = 0.8
    K, dK = ref_kernelmatrix(agp.with_lengthscale(agp.RationalQuadraticKernel(alpha=a), ell), X, grad=True)
    Ks, G = sk.RationalQuadratic(ell, alpha=a)(X, eval_gradient=True)
    np.testing.assert_allclose(K, Ks, rtol=1e-12)
    np.testing.assert_allclose(a * dK[2], G[..., 0], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(-(1 / ell) * dK[1], G[..., 1], rtol=1e-10, atol=1e-13)
    # Per(r)∘Scale(1/p): θ = (c, s, r);  sklearn ExpSineSquared(l = 2r, p): (log l, log p);  ∂/∂log l = r ∂/∂r, ∂/∂log p = −s ∂/∂s
    r, period = 0.6, 1.3
    K, dK = ref_kernelmatrix(agp.with_lengthscale(agp.PeriodicKernel(r=[r]), period), X, grad=True)
    Ks, G = sk.ExpSineSquared(2 * r, period)(X, eval_gradient=True)
    np.testing.assert_allclose(K, Ks, rtol=1e-12)
    np.testing.assert_allclose(r * dK[2], G[..., 0], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(-(1 / period) * dK[1], G[..., 1], rtol=1e-9, atol=1e-13)
    # Matern 3/2 and 5/2
    for kern, nu in ((agp.Matern32Kernel(), 1.5), (agp.Matern52Kernel(), 2.5)):
        K, dK = ref_kernelmatrix(agp.with_lengthscale(kern, ell), X, grad=True)
        Ks, G = sk.Matern(ell, nu=nu)(X, eval_gradient=True)
        np.testing.assert_allclose(K, Ks, rtol=1e-12)
        np.testing.assert_allclose(-(1 / ell) * dK[1], G[..., 0], rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("d", [1, 3])
def test_reference_gradients_match_central_differences(d):
    X = _inputs(20, d, 6)
    k = (1.2 * agp.PeriodicKernel(r=np.linspace(0.5, 0.9, d)) @ agp.ARDTransform(np.linspace(0.8, 1.2, d))
         * agp.with_lengthscale(agp.Matern52Kernel(), 1.4)
         + 0.7 * agp.RationalQuadraticKernel(alpha=1.1) @ agp.ScaleTransform(0.9)
         + 0.3 * agp.Matern12Kernel() @ agp.ARDTransform(np.linspace(0.5, 1.5, d)) + 0.1 * agp.WhiteKernel())
    nf = agp.api._NormalForm(k)
    th = np.array(nf.theta())
    _, dK = ref_kernelmatrix(k, X, grad=True)
    assert len(dK) == len(th)
    # one θ entry at a time, on the descriptor the device reads
    for j in range(len(th)):
        h = 1e-6 * max(1.0, abs(th[j]))
        Kp = ref_from_theta(nf, th + h * np.eye(len(th))[j], X)
        Km = ref_from_theta(nf, th - h * np.eye(len(th))[j], X)
        np.testing.assert_allclose(dK[j], (Kp - Km) / (2 * h), rtol=1e-5, atol=1e-8, err_msg=str(j))
