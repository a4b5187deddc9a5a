"""GPU: exact GPs with a dense observation-noise covariance Σy (include/gpmi355.h gp_noise kinds 2 / 3) — the streamed upload, dense_add_rows_kernel /
dense_add_cols_kernel / dense_grad_rows_kernel and every entry point that takes a gp_noise — against NumPy / SciPy on the host: Cholesky of K + Σy with K
from oracle.kernelmatrix / tests.composite_ref.ref_kernelmatrix.  Tolerances are the project's (tests/test_gpu_composite.py).

Test noise: Σy = D^½ (0.05·0.6^|i−j|) D^½ + 0.01·I, D = diag(0.5 + U(0, 1)), symmetrised explicitly, on 1.3·SE(ℓ = 0.7) over U(0, 3)³ inputs:
λ_min(Σy) ≈ 0.017, cond(K + Σy) = 5.6e3 at n = 700 and 2.7e4 at n = 3 000.

The mirror reads the UPPER triangle of the array it is given (Symmetric(Σy)): a C-ordered array goes out as kind 3 (lower triangle of the column-major
view), a Fortran-ordered one as kind 2."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests.composite_ref import ref_kernelmatrix

pytestmark = pytest.mark.gpu

VAR, ELL = 1.3, 0.7


def _kernel():
    return VAR * agp.with_lengthscale(agp.SqExponentialKernel(), ELL)


OK = o.Kernel(o.SE, VAR, 1.0 / ELL)


def _ar1(n, rho=0.6):
    idx = np.arange(n, dtype=np.float64)
    A = np.abs(np.subtract.outer(idx, idx))
    return np.power(rho, A, out=A)


def _sigma(n, seed, rho=0.6):
    """(Σy, sqrt(D)): the test noise, exactly symmetric."""
    rng = np.random.default_rng(1000 + seed)
    sd = np.sqrt(0.5 + rng.uniform(0, 1, n))
    S = _ar1(n, rho)
    S *= 0.05
    S *= sd[:, None]
    S *= sd[None, :]
    S[np.diag_indices(n)] += 0.01
    S += S.T.copy()
    S *= 0.5
    return S, sd


def _data(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 3, size=(n, 3)), rng.standard_normal(n)


def _host_fit(K, S, y):
    Cm = K + S
    L = sla.cholesky(Cm, lower=True, overwrite_a=True, check_finite=False)
    alpha = sla.cho_solve((L, True), y, check_finite=False)
    lp = -0.5 * (len(y) * math.log(2 * math.pi) + 2 * np.sum(np.log(np.diag(L))) + y @ alpha)
    return lp, alpha, L


@functools.lru_cache(maxsize=2)
def _case(n):
    """(X, y, Σy, host logpdf, host α) — the host reference of one size, shared by the two memory orders."""
    X, y = _data(n, n)
    S, _ = _sigma(n, n)
    lp, alpha, _ = _host_fit(o.kernelmatrix(OK, X, threads=8), S, y)
    return X, y, S, lp, alpha


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def _ordered(S, order):
    return np.ascontiguousarray(S) if order == "C" else np.asfortranarray(S)


def _check_fit(X, y, S_in, lp_h, a_h, f=None):
    f = f or agp.GP(_kernel())
    fx = f(agp.RowVecs(X), S_in)
    lp = agp.logpdf(fx, y)
    post = agp.posterior(fx, y)
    print(f"n={len(y)} logpdf rel {abs(lp - lp_h) / abs(lp_h):.2e} alpha rel {_rel(post.data.alpha, a_h):.2e}")
    assert lp == pytest.approx(lp_h, rel=1e-10)
    assert post.logpdf_value == pytest.approx(lp_h, rel=1e-10)
    assert _rel(post.data.alpha, a_h) <= 1e-8
    return post


# ---- 1. logpdf / α against the host, both memory orders ------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 257, 1000, 4096, 12288])
def test_logpdf_and_alpha_against_a_host_cholesky(agp, n, order):
    X, y, S, lp_h, a_h = _case(n)
    S_in = _ordered(S, order)
    m = agp.api._Marshal(np.float64)
    assert m.noise(S_in, n).kind == (3 if order == "C" or n == 1 else 2)  # (a 1×1 array is both C- and F-contiguous)
    _check_fit(X, y, S_in, lp_h, a_h)


# ---- 2. a dense diagonal matrix is the vector-noise fit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["C", "F"])
def test_dense_diagonal_matrix_equals_the_vector_noise_fit(agp, order):
    n = 700
    X, y = _data(n, 21)
    v = 0.02 + np.random.default_rng(22).uniform(0, 0.1, n)
    f = agp.GP(_kernel())
    lp_v = agp.logpdf(f(agp.RowVecs(X), v), y)
    pv = agp.posterior(f(agp.RowVecs(X), v), y)
    S_in = _ordered(np.diag(v), order)
    lp_d = agp.logpdf(f(agp.RowVecs(X), S_in), y)
    pd = agp.posterior(f(agp.RowVecs(X), S_in), y)
    assert lp_d == pytest.approx(lp_v, rel=1e-12)
    assert pd.logpdf_value == pytest.approx(lp_v, rel=1e-12)
    assert _rel(pd.data.alpha, pv.data.alpha) <= 1e-9


# ---- 3. only the documented triangle is read ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("n", [300, 1000])
def test_only_the_upper_triangle_of_the_array_is_read(agp, n, order):
    X, y = _data(n, 31)
    S, _ = _sigma(n, 31)
    f = agp.GP(_kernel())
    lp_sym = agp.logpdf(f(agp.RowVecs(X), _ordered(S, order)), y)
    Sn = S.copy()
    Sn[np.tril_indices(n, -1)] = np.nan
    Sn = _ordered(Sn, order)
    lp = agp.logpdf(f(agp.RowVecs(X), Sn), y)
    post = agp.posterior(f(agp.RowVecs(X), Sn), y)
    assert np.isfinite(lp) and np.all(np.isfinite(post.data.alpha))
    assert lp == pytest.approx(lp_sym, rel=1e-12)
    g = agp.logpdf_and_grad(f(agp.RowVecs(X), Sn), y)[1]["noise"]
    assert np.all(np.isfinite(g))


# ---- 4. several panels, the look-ahead schedule, several staging pieces; byte offsets beyond 2³¹ -------------------------------------------------
@pytest.mark.parametrize("order", ["C", "F"])
def test_several_panels_with_lookahead_and_small_staging_pieces(agp, order):
    n = 3001
    X, y, S, lp_h, a_h = _case(n)
    c = agp.default_context(0)
    c.set_param("nb", 512)
    c.set_param("lookahead_min_n", 0)
    c.set_param("dense_stage_mb", 4)  # 128-row / 128-column pieces: 24 of them
    try:
        _check_fit(X, y, _ordered(S, order), lp_h, a_h)
    finally:
        c.set_param("nb", -1)
        c.set_param("lookahead_min_n", 24576)
        c.set_param("dense_stage_mb", 64)


@pytest.mark.parametrize("order", ["C", "F"])
def test_n_16384_byte_offsets_beyond_2_31(agp, order):
    """2.1 GB of Σy, 32 staging pieces, element offsets up to 2.7e8 (byte offsets beyond 2³¹).  Beyond 2³² ELEMENTS (n >= 65 536: 34 GB of host array and a
    two-minute host reference) is not covered by the suite."""
    X, y, S, lp_h, a_h = _case(16384)
    _check_fit(X, y, _ordered(S, order), lp_h, a_h)
    if order == "F":
        _case.cache_clear()  # 6 GB of host arrays


# ---- 5. everything downstream of a dense fit ---------------------------------------------------------------------------------------------------
def test_posterior_predictions_joint_logpdf_and_rand(agp):
    n, ns = 1500, 300
    X, y = _data(n, 51)
    S, _ = _sigma(n, 51)
    rng = np.random.default_rng(52)
    Xs = rng.uniform(0, 3, size=(ns, 3))
    Ss, _ = _sigma(ns, 53)
    K = o.kernelmatrix(OK, X)
    lp_h, a_h, L = _host_fit(K, S, y)
    Ks = o.kernelmatrix(OK, Xs, X)
    m_h = Ks @ a_h
    V = sla.solve_triangular(L, Ks.T, lower=True)
    cov_h = o.kernelmatrix(OK, Xs) - V.T @ V
    f = agp.GP(_kernel())
    post = agp.posterior(f(agp.RowVecs(X), S), y)
    xs = agp.RowVecs(Xs)
    np.testing.assert_allclose(post.mean(xs), m_h, rtol=0, atol=1e-8 * np.max(np.abs(m_h)))
    np.testing.assert_allclose(post.var(xs), np.diag(cov_h), rtol=0, atol=1e-9 * VAR)
    np.testing.assert_allclose(post.cov(xs), cov_h, rtol=0, atol=1e-9 * VAR)
    mm, cc = post.mean_and_cov(xs)
    np.testing.assert_allclose(mm, m_h, rtol=0, atol=1e-8 * np.max(np.abs(m_h)))
    np.testing.assert_allclose(cc, cov_h, rtol=0, atol=1e-9 * VAR)
    # logpdf(post(x*, Σ*), Y*) and rand(post(x*, Σ*)) with a dense Σ*, both memory orders
    Cs = cov_h + Ss
    Ls = sla.cholesky(Cs, lower=True)
    Y = rng.standard_normal((ns, 3)) + m_h[:, None]

    def lp_host(col):
        z = sla.solve_triangular(Ls, col - m_h, lower=True)
        return -0.5 * (ns * math.log(2 * math.pi) + 2 * np.sum(np.log(np.diag(Ls))) + z @ z)

    xi = rng.standard_normal((ns, 2))
    for order in ("C", "F"):
        fxs = post(xs, _ordered(Ss, order))
        assert agp.logpdf(fxs, Y[:, 0]) == pytest.approx(lp_host(Y[:, 0]), rel=1e-9)
        np.testing.assert_allclose(agp.logpdf(fxs, Y), [lp_host(Y[:, j]) for j in range(3)], rtol=1e-9)
        np.testing.assert_allclose(agp.rand(fxs, 2, xi=xi), m_h[:, None] + Ls @ xi, rtol=0, atol=1e-7)
        np.testing.assert_allclose(agp.cov(fxs), Cs, rtol=0, atol=1e-9 * VAR)
        np.testing.assert_allclose(agp.var(fxs), np.diag(Cs), rtol=0, atol=1e-9 * VAR)


def test_prior_finite_gp_accessors_and_logpdf_terms(agp):
    n = 900
    X, y = _data(n, 55)
    S, _ = _sigma(n, 55)
    K = o.kernelmatrix(OK, X)
    lp_h, a_h, L = _host_fit(K, S, y)
    f = agp.GP(0.3, _kernel())
    fx = f(agp.RowVecs(X), np.asfortranarray(S))
    m, sd = agp.marginals(fx)
    np.testing.assert_allclose(m, 0.3)
    np.testing.assert_allclose(sd, np.sqrt(VAR + np.diag(S)), rtol=1e-14)
    m, v = agp.mean_and_var(fx)
    np.testing.assert_allclose(v, VAR + np.diag(S), rtol=1e-14)
    np.testing.assert_allclose(agp.cov(fx), K + S, rtol=0, atol=1e-13 * VAR)
    m, Cm = agp.mean_and_cov(fx)
    np.testing.assert_allclose(Cm, K + S, rtol=0, atol=1e-13 * VAR)
    xi = np.random.default_rng(56).standard_normal((n, 2))
    np.testing.assert_allclose(agp.rand(fx, 2, xi=xi), 0.3 + L @ xi, rtol=0, atol=1e-7)
    # zero-mean terms against the host factor
    f0 = agp.GP(_kernel())
    for order in ("C", "F"):
        fx0 = f0(agp.RowVecs(X), _ordered(S, order))
        assert agp.sqmahal(fx0, y) == pytest.approx(y @ a_h, rel=1e-10)
        assert agp.logdetcov(fx0) == pytest.approx(2 * np.sum(np.log(np.diag(L))), rel=1e-10)
        assert _rel(agp.gradlogpdf(fx0, y), -a_h) <= 1e-8


def test_joint_calls_on_a_vfe_posterior_with_a_dense_noise(agp):
    n, ns, mz = 2000, 200, 64
    X, y = _data(n, 57)
    rng = np.random.default_rng(58)
    Z = rng.uniform(0, 3, size=(mz, 3))
    Xs = rng.uniform(0, 3, size=(ns, 3))
    Ss, _ = _sigma(ns, 59)
    f = agp.GP(_kernel())
    ap = agp.posterior(agp.VFE(f(agp.RowVecs(Z), 1e-6)), f(agp.RowVecs(X), 0.1), y)
    of = o.GP(OK)
    oap = o.vfe_posterior(of, Z, 1e-6, o.FiniteGP(of, X, 0.1), y)
    m_h, c_h = oap.mean_and_cov(Xs)
    Ls = sla.cholesky(c_h + Ss, lower=True)
    Y = rng.standard_normal((ns, 3)) + m_h[:, None]
    xi = rng.standard_normal((ns, 2))
    for order in ("C", "F"):
        fxs = ap(agp.RowVecs(Xs), _ordered(Ss, order))
        ref = []
        for j in range(3):
            z = sla.solve_triangular(Ls, Y[:, j] - m_h, lower=True)
            ref.append(-0.5 * (ns * math.log(2 * math.pi) + 2 * np.sum(np.log(np.diag(Ls))) + z @ z))
        np.testing.assert_allclose(agp.logpdf(fxs, Y), ref, rtol=1e-9)
        np.testing.assert_allclose(agp.rand(fxs, 2, xi=xi), m_h[:, None] + Ls @ xi, rtol=0, atol=1e-7)


# ---- 6. sequential conditioning --------------------------------------------------------------------------------------------------------------
def test_sequential_posterior_equals_the_batch_fit_with_a_block_diagonal_noise(agp):
    n1, n2 = 1000, 333
    n = n1 + n2
    X, y = _data(n, 61)
    S11, _ = _sigma(n1, 61)
    S22, _ = _sigma(n2, 62)
    Sb = np.zeros((n, n))
    Sb[:n1, :n1] = S11
    Sb[n1:, n1:] = S22
    f = agp.GP(_kernel())
    batch = agp.posterior(f(agp.RowVecs(X), Sb), y)
    xs = agp.RowVecs(np.random.default_rng(63).uniform(0, 3, size=(50, 3)))
    for order in ("C", "F"):
        p1 = agp.posterior(f(agp.RowVecs(X[:n1]), _ordered(S11, order)), y[:n1])
        p2 = agp.posterior(p1(agp.RowVecs(X[n1:]), _ordered(S22, order)), y[n1:])
        assert _rel(p2.data.alpha, batch.data.alpha) <= 1e-8
        assert p2.logpdf_value == pytest.approx(batch.logpdf_value, rel=1e-8)
        assert _rel(p2.mean(xs), batch.mean(xs)) <= 1e-8
        assert _rel(p2.var(xs), batch.var(xs)) <= 1e-8


# ---- 7. gradient -----------------------------------------------------------------------------------------------------------------------------
def _host_grad(X, S, y):
    """logpdf, G = ½(ααᵀ − C⁻¹), ∂/∂variance, ∂/∂scale (ScaleTransform s = 1/ℓ), α on the host."""
    K = o.kernelmatrix(OK, X)
    lp, alpha, L = _host_fit(K, S, y)
    Ci = sla.cho_solve((L, True), np.eye(len(y)))
    G = 0.5 * (np.outer(alpha, alpha) - Ci)
    s = 1.0 / ELL
    D2 = -2.0 * np.log(K / VAR)  # s²‖x − x'‖²
    dK_ds = K * (-0.5) * D2 * 2.0 / s
    return lp, G, float(np.sum(G * K) / VAR), float(np.sum(G * dK_ds)), alpha


@pytest.mark.parametrize("order", ["C", "F"])
def test_gradient_against_the_host_formulas(agp, order):
    n = 700
    X, y = _data(n, 71)
    S, _ = _sigma(n, 71)
    lp_h, G_h, dvar_h, dscale_h, a_h = _host_grad(X, S, y)
    f = agp.GP(_kernel())
    lp, g = agp.logpdf_and_grad(f(agp.RowVecs(X), _ordered(S, order)), y)
    assert lp == pytest.approx(lp_h, rel=1e-10)
    G = g["noise"]
    assert G.shape == (n, n)
    assert np.array_equal(G, G.T)
    np.testing.assert_allclose(G, G_h, rtol=1e-7, atol=1e-9 * np.max(np.abs(G_h)))
    assert g["variance"] == pytest.approx(dvar_h, rel=1e-7)
    assert g["scale"] == pytest.approx(dscale_h, rel=1e-7)
    assert _rel(g["y"], -a_h) <= 1e-8


def test_gradient_directional_derivative_and_ar1_chain_rule(agp):
    n = 4096
    X, y = _data(n, 73)
    S, sd = _sigma(n, 73)
    f = agp.GP(_kernel())
    c = agp.default_context(0)
    c.set_param("dense_stage_mb", 8)  # the gradient's download in 16 row blocks
    try:
        _, g = agp.logpdf_and_grad(f(agp.RowVecs(X), S), y)
    finally:
        c.set_param("dense_stage_mb", 64)
    G = g["noise"]
    assert np.array_equal(G, G.T)
    rng = np.random.default_rng(74)
    E = rng.standard_normal((n, n))
    E = 0.5 * (E + E.T)
    E /= np.max(np.abs(np.linalg.eigvalsh(E)))  # unit spectral norm
    h = 1e-5
    fd = (agp.logpdf(f(agp.RowVecs(X), S + h * E), y) - agp.logpdf(f(agp.RowVecs(X), S - h * E), y)) / (2 * h)
    an = float(np.sum(G * E))
    print(f"<G, E> = {an:.10e}, central difference {fd:.10e}, rel {abs(an - fd) / abs(fd):.2e}")
    assert an == pytest.approx(fd, rel=1e-5)
    # Σy(ρ) = D^½ (0.05 ρ^|i−j|) D^½ + 0.01 I:  ∂Σy/∂ρ = D^½ (0.05 |i−j| ρ^(|i−j|−1)) D^½
    rho = 0.6
    idx = np.arange(n, dtype=np.float64)
    A = np.abs(np.subtract.outer(idx, idx))
    dS = 0.05 * A * np.power(rho, np.maximum(A - 1, 0)) * sd[:, None] * sd[None, :]
    an = float(np.sum(G * dS))

    def lp_rho(r):
        Sr = 0.05 * _ar1(n, r) * sd[:, None] * sd[None, :]
        Sr[np.diag_indices(n)] += 0.01
        return agp.logpdf(f(agp.RowVecs(X), 0.5 * (Sr + Sr.T)), y)

    fd = (lp_rho(rho + h) - lp_rho(rho - h)) / (2 * h)
    print(f"d logpdf / d rho = {an:.10e}, central difference {fd:.10e}, rel {abs(an - fd) / abs(fd):.2e}")
    assert an == pytest.approx(fd, rel=1e-5)


# ---- 8. composite kernel + dense Σy ----------------------------------------------------------------------------------------------------------
def test_composite_kernel_with_a_dense_noise(agp):
    from tests.test_gpu_composite import _dense_data, _ml_kernel

    n = 1000
    x, y = _dense_data(n, seed=81)
    S, _ = _sigma(n, 81)
    S += 0.09 * np.eye(n)  # the noise level of the composite tests (0.1) on the diagonal
    k = _ml_kernel()
    K, dK = ref_kernelmatrix(k, x, grad=True)
    lp_h, a_h, L = _host_fit(K, S, y)
    Ci = sla.cho_solve((L, True), np.eye(n))
    G_h = 0.5 * (np.outer(a_h, a_h) - Ci)
    f = agp.GP(k)
    for order in ("C", "F"):
        S_in = _ordered(S, order)
        assert agp.logpdf(f(x, S_in), y) == pytest.approx(lp_h, rel=1e-10)
        post = agp.posterior(f(x, S_in), y)
        assert _rel(post.data.alpha, a_h) <= 1e-8
        lp, g = agp.logpdf_and_grad(f(x, S_in), y)
        assert lp == pytest.approx(lp_h, rel=1e-10)
        th_h = np.array([np.sum(G_h * d) for d in dK])
        np.testing.assert_allclose(g["theta"], th_h, rtol=1e-7, atol=1e-9 * np.max(np.abs(th_h)))
        np.testing.assert_allclose(g["noise"], G_h, rtol=1e-7, atol=1e-9 * np.max(np.abs(G_h)))


# ---- 9. fp32 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["C", "F"])
def test_fp32_dense_fit(agp, order):
    n = 1000
    X, y, S, lp_h, a_h = _case(n)
    X32, y32, S32 = X.astype(np.float32), y.astype(np.float32), _ordered(S.astype(np.float32), order)
    f = agp.GP(_kernel())
    fx = f(agp.RowVecs(X32), S32)
    lp = agp.logpdf(fx, y32)
    post = agp.posterior(fx, y32)
    assert lp.dtype == np.float32 and post.data.alpha.dtype == np.float32
    assert float(lp) == pytest.approx(lp_h, rel=2e-4)
    assert _rel(post.data.alpha, a_h) <= 5e-3
    g = agp.logpdf_and_grad(fx, y32)[1]["noise"]
    assert g.dtype == np.float32 and g.shape == (n, n) and np.array_equal(g, g.T)
    # a float64 Σy beside float32 inputs is converted once (one C-ordered copy)
    assert float(agp.logpdf(f(agp.RowVecs(X32), S), y32)) == pytest.approx(lp_h, rel=2e-4)


# ---- 10. not positive definite -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["C", "F"])
def test_not_positive_definite_reports_the_first_failing_minor(agp, order):
    n = 1000
    X, y = _data(n, 101)
    S, _ = _sigma(n, 101)
    S[400, 400] = -100.0  # row 401 (1-based)
    _, info = sla.lapack.dpotrf(o.kernelmatrix(OK, X) + S, lower=1)
    assert info == 401
    f = agp.GP(_kernel())
    with pytest.raises(agp.PosDefException) as ei:
        agp.logpdf(f(agp.RowVecs(X), _ordered(S, order)), y)
    assert ei.value.info == info
    with pytest.raises(agp.PosDefException) as ei:
        agp.posterior(f(agp.RowVecs(X), _ordered(S, order)), y)
    assert ei.value.info == info


# ---- 11. no atomics: bitwise repeatable ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_mode", ["no_atomics"], indirect=True)
@pytest.mark.parametrize("order", ["C", "F"])
def test_dense_fits_are_bitwise_repeatable_without_atomics(agp, exact_mode, order):
    n = 2500
    X, y = _data(n, 111)
    S, _ = _sigma(n, 111)
    S_in = _ordered(S, order)
    xs = agp.RowVecs(np.random.default_rng(112).uniform(0, 3, size=(200, 3)))
    f = agp.GP(_kernel())
    p1, p2 = agp.posterior(f(agp.RowVecs(X), S_in), y), agp.posterior(f(agp.RowVecs(X), S_in), y)
    assert np.array_equal(p1.data.alpha, p2.data.alpha) and p1.logpdf_value == p2.logpdf_value
    (m1, c1), (m2, c2) = p1.mean_and_cov(xs), p2.mean_and_cov(xs)
    assert np.array_equal(m1, m2) and np.array_equal(c1, c2)


# ---- 12. multi-device context ------------------------------------------------------------------------------------------------------------------
def test_multi_device_context_runs_dense_fits_on_its_first_device(agp):
    from tests.conftest import rank_devices

    n = 2500
    X, y = _data(n, 121)
    S, _ = _sigma(n, 121)
    xs = agp.RowVecs(np.random.default_rng(122).uniform(0, 3, size=(150, 3)))
    single = agp.GP(_kernel())
    multi = agp.GP(_kernel(), ctx=agp.Context(devices=rank_devices(2), P=2, Q=1))
    for order in ("C", "F"):
        S_in = _ordered(S, order)
        assert agp.logpdf(multi(agp.RowVecs(X), S_in), y) == pytest.approx(agp.logpdf(single(agp.RowVecs(X), S_in), y), rel=1e-12)
        pm, ps = agp.posterior(multi(agp.RowVecs(X), S_in), y), agp.posterior(single(agp.RowVecs(X), S_in), y)
        assert _rel(pm.data.alpha, ps.data.alpha) <= 1e-12
        mm, vm = pm.mean_and_var(xs)
        ms, vs = ps.mean_and_var(xs)
        assert _rel(mm, ms) <= 1e-12 and _rel(vm, vs) <= 1e-12
    # a vector-noise fit of the multi-device ctx (distributed factor) followed by a sequential update with a dense Σy2
    v = np.full(n, 0.05)
    p1 = agp.posterior(multi(agp.RowVecs(X[:2000]), v[:2000]), y[:2000])
    p2 = agp.posterior(p1(agp.RowVecs(X[2000:]), S[2000:, 2000:].copy()), y[2000:])
    Sb = np.diag(v)
    Sb[2000:, 2000:] = S[2000:, 2000:]
    pb = agp.posterior(single(agp.RowVecs(X), Sb), y)
    assert _rel(p2.data.alpha, pb.data.alpha) <= 1e-8


# ---- 13. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_vfe_fits_and_bad_noise_descriptors_are_refused(agp):
    n = 200
    X, y = _data(n, 131)
    S, _ = _sigma(n, 131)
    f = agp.GP(_kernel())
    vfe = agp.VFE(f(agp.RowVecs(X[::10]), 1e-6))
    with pytest.raises(NotImplementedError, match="dense Σy"):
        agp.posterior(vfe, f(agp.RowVecs(X), S), y)
    with pytest.raises(NotImplementedError, match="dense Σy"):
        agp.elbo(vfe, f(agp.RowVecs(X), S), y)
    # the C ABI's own checks
    ctx = agp.default_context(0)
    lib = ctx.lib
    m = agp.api._Marshal(np.float64)
    px, pz = m.points(agp.RowVecs(X)), m.points(agp.RowVecs(X[::10]))
    kk = m.kernel(_kernel(), 3)
    Sf = np.asfortranarray(S)
    lp = np.empty(1)
    h = C.c_void_p()
    nz = agp._lib.gp_noise(2, 0.0, Sf.ctypes.data)
    assert lib.gp_vfe_fit(ctx.handle, C.byref(kk), C.byref(px), C.byref(pz), C.byref(nz), 1e-6, None, y.ctypes.data, 0, C.byref(h), lp.ctypes.data) == -4
    assert "dense noise" in lib.gp_last_error().decode() and not h.value
    nz = agp._lib.gp_noise(4, 0.0, Sf.ctypes.data)
    assert lib.gp_logpdf(ctx.handle, C.byref(kk), C.byref(px), C.byref(nz), None, y.ctypes.data, n, 1, lp.ctypes.data) == -4
    assert "noise kind" in lib.gp_last_error().decode()
    nz = agp._lib.gp_noise(-1, 0.0, Sf.ctypes.data)
    assert lib.gp_logpdf(ctx.handle, C.byref(kk), C.byref(px), C.byref(nz), None, y.ctypes.data, n, 1, lp.ctypes.data) == -4
    nz = agp._lib.gp_noise(2, 0.0, None)
    assert lib.gp_logpdf(ctx.handle, C.byref(kk), C.byref(px), C.byref(nz), None, y.ctypes.data, n, 1, lp.ctypes.data) == -4
    assert "NULL" in lib.gp_last_error().decode()
