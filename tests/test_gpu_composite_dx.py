"""GPU: ∂logpdf/∂x and the logdet / sqmahal terms of exact GPs with composite kernels — kgradx_sum_kernel behind gp_logpdf_grad_sum_x, and
gp_logpdf_terms_sum — against the fp64 host reference of tests/composite_dx_ref.py (central-difference checked in tests/test_composite_dx_cpu.py).

Input-gradient tolerances are those of tests/test_gpu_api.py::test_logpdf_grad_wrt_inputs, with g_ref from the HOST reference:
    fp64: rtol 1e-7, atol 1e-8·max(1, max|g_ref|)        fp32: rtol 2e-2, atol 2e-2·max(1, max|g_ref|)
"rel" of a vector is the norm-wise ‖a − b‖ / ‖b‖ the composite tests use throughout (tests/test_gpu_composite.py `_rel`)."""
import ctypes as C
import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests.composite_dx_ref import host_fit, many_dim_kernel, ref_logpdf_grad_x, six_term_data, six_term_kernel
from tests.composite_ref import dense_data, ml_kernel, ref_kernelmatrix

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def _assert_gx(g, g_ref, what=""):
    """the project's input-gradient tolerance for g's dtype; prints the measured error first"""
    tol = 2e-2 if g.dtype == np.float32 else 1e-7
    atol = (2e-2 if g.dtype == np.float32 else 1e-8) * max(1.0, float(np.abs(g_ref).max()))
    assert g.shape == g_ref.shape, (g.shape, g_ref.shape)
    err = float(np.max(np.abs(g.astype(np.float64) - g_ref)))
    print(f"[dx] {what} {g.dtype.name}: max|g - g_ref| = {err:.3e}, max|g_ref| = {np.abs(g_ref).max():.3e}, rel-norm = {_rel(g, g_ref):.3e}")
    assert np.all(np.isfinite(g))
    np.testing.assert_allclose(g, g_ref, rtol=tol, atol=atol)


# ---- the six-term kernel, D = 3 (DR = 4 instance) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _six(n, vector_noise):
    X, y = six_term_data(n, seed=n)
    noise = np.random.default_rng(n + 1).uniform(0.03, 0.1, n) if vector_noise else 0.05
    mean = 0.2 if vector_noise else 0.0  # the prior mean is constant in x
    g = ref_logpdf_grad_x(six_term_kernel(), X, y, noise, mean)
    for a in (X, y, g):
        a.setflags(write=False)
    return X, y, noise, mean, g


@pytest.mark.parametrize("vector_noise", [False, True], ids=["scalar-noise", "vector-noise"])
@pytest.mark.parametrize("n", [333, 130])
def test_six_term_kernel_every_container_and_the_other_gradients_unchanged(n, vector_noise):
    """n = 333: three tile rows, the last with 77 valid rows, tiles above the diagonal reading the mirrored entry; n = 130: two valid rows in the second tile."""
    X, y, noise, mean, g_ref = _six(n, vector_noise)
    k = six_term_kernel()
    f = agp.GP(mean, k) if mean else agp.GP(k)
    lp, g = agp.logpdf_and_grad(f(agp.RowVecs(X), noise), y, wrt_x=True)
    _assert_gx(g["x"], g_ref, f"six-term n={n} RowVecs")
    assert g["x"].shape == (n, 3) and g["x"].dtype == np.float64
    lpc, gc = agp.logpdf_and_grad(f(agp.ColVecs(X.T.copy()), noise), y, wrt_x=True)
    assert gc["x"].shape == (3, n)
    _assert_gx(gc["x"].T, g_ref, f"six-term n={n} ColVecs")
    lp0, g0 = agp.logpdf_and_grad(f(agp.RowVecs(X), noise), y)
    assert "x" not in g0 and set(g) == set(g0) | {"x"}
    # two calls on the default context: the stream-K tails of the factorisation and the backward sweep behind α add with fp64 atomics, so lp, dy and dmean
    # of two calls agree to rounding, not to the bit (profiles/README.md r15: 3 of 60 repeats differed in dy)
    assert lp == pytest.approx(lp0, rel=1e-12) and _rel(g["y"], g0["y"]) <= 1e-12 and _rel(g["mean"], g0["mean"]) <= 1e-12
    assert _rel(g["kernel"], g0["kernel"]) <= 1e-12 and _rel(g["theta"], g0["theta"]) <= 1e-12  # sums by fp64 atomics: not bitwise
    assert _rel(g["noise"], g0["noise"]) <= 1e-12
    lp_h = host_fit(k, X, y, noise, mean)[0]
    assert lp == pytest.approx(lp_h, rel=1e-10)
    # "deterministic" = 1 promises the bits of the fit (include/gpmi355.h): with and without wrt_x, lp, dy and dmean are the same numbers
    ctx = agp.Context(0)
    try:
        ctx.set_param("deterministic", 1)
        fd = agp.GP(mean, k, ctx=ctx) if mean else agp.GP(k, ctx=ctx)
        lpd, gd = agp.logpdf_and_grad(fd(agp.RowVecs(X), noise), y, wrt_x=True)
        lpd0, gd0 = agp.logpdf_and_grad(fd(agp.RowVecs(X), noise), y)
    finally:
        ctx.close()
    assert lpd == lpd0 and np.array_equal(gd["y"], gd0["y"]) and np.array_equal(gd["mean"], gd0["mean"])
    assert lpd == pytest.approx(lp_h, rel=1e-10)
    _assert_gx(gd["x"], g_ref, f"six-term n={n} RowVecs deterministic")


def test_six_term_kernel_in_fp32():
    X, y, noise, mean, g_ref = _six(333, False)
    lp, g = agp.logpdf_and_grad(agp.GP(six_term_kernel())(agp.RowVecs(X.astype(np.float32)), np.float32(noise)), y.astype(np.float32), wrt_x=True)
    assert g["x"].dtype == np.float32
    _assert_gx(g["x"], g_ref, "six-term n=333")


# ---- D = 1 vector input (DR = 1) ---------------------------------------------------------------------------------------------------------
def test_vector_input_of_the_mauna_loa_form():
    x, y = dense_data(200)
    k = ml_kernel()
    g_ref = ref_logpdf_grad_x(k, x, y, 0.1)[:, 0]
    _, g = agp.logpdf_and_grad(agp.GP(k)(x, 0.1), y, wrt_x=True)
    assert g["x"].shape == (200,)
    _assert_gx(g["x"], g_ref, "ml_kernel D=1 n=200")


# ---- D = 8 and D = 16 (DR = 16) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 16])
def test_many_dimensions_fp64_and_fp32(d):
    rng = np.random.default_rng(200 + d)
    n = 260
    X = rng.uniform(0, 2, size=(n, d))
    y = np.sin(X.sum(1) / 2) + 0.1 * rng.standard_normal(n)
    k = many_dim_kernel(d)
    g_ref = ref_logpdf_grad_x(k, X, y, 0.1)
    f = agp.GP(k)
    _, g = agp.logpdf_and_grad(f(agp.RowVecs(X), 0.1), y, wrt_x=True)
    _assert_gx(g["x"], g_ref, f"many-dim D={d}")
    _, g32 = agp.logpdf_and_grad(f(agp.RowVecs(X.astype(np.float32)), np.float32(0.1)), y.astype(np.float32), wrt_x=True)
    assert g32["x"].dtype == np.float32
    _assert_gx(g32["x"], g_ref, f"many-dim D={d}")


# ---- one-term composites against the single-kind path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,okind", [(0, o.SE), (1, o.MATERN12), (2, o.MATERN32), (3, o.MATERN52)])
@pytest.mark.parametrize("tr", ["none", "scale", "ard"])
def test_one_term_composite_agrees_with_the_single_kind_path_and_the_oracle(kind, okind, tr):
    rng = np.random.default_rng(300 + kind)
    n = 200
    X = rng.standard_normal((n, 3))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
    scale = {"none": None, "scale": 0.8, "ard": np.array([0.5, 1.1, 0.9])}[tr]
    k = 1.4 * agp.Kernel(kind)
    if scale is not None:
        k = k @ (agp.ScaleTransform(scale) if tr == "scale" else agp.ARDTransform(scale))
    _, gs = agp.logpdf_and_grad(agp.GP(k)(agp.RowVecs(X), 0.05), y, wrt_x=True)               # kgradx_kernel
    _, gc = agp.logpdf_and_grad(agp.GP(agp.KernelSum((k,)))(agp.RowVecs(X), 0.05), y, wrt_x=True)  # kgradx_sum_kernel
    dev = float(np.max(np.abs(gc["x"] - gs["x"])) / np.abs(gs["x"]).max())
    print(f"[dx] one-term kind={kind} {tr}: max|composite - single| / max|g| = {dev:.3e}")
    assert dev <= 1e-9
    go = o.logpdf_grad(o.FiniteGP(o.GP(o.Kernel(okind, 1.4, scale)), X, 0.05), y)["x"]
    _assert_gx(gc["x"], go, f"one-term kind={kind} {tr} vs oracle")


# ---- duplicated inputs with White (no Matern12: its derivative is not defined at coincident points) ------------------------------------
def test_duplicated_inputs_with_a_white_term():
    rng = np.random.default_rng(401)
    n = 200
    X = rng.uniform(0, 3, size=(n, 3))
    X[11] = X[10]
    X[170] = X[40]  # across tiles
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
    k = agp.SqExponentialKernel() @ agp.ScaleTransform(0.9) + 0.05 * agp.WhiteKernel()
    g_ref = ref_logpdf_grad_x(k, X, y, 0.05)
    _, g = agp.logpdf_and_grad(agp.GP(k)(agp.RowVecs(X), 0.05), y, wrt_x=True)
    assert np.all(np.isfinite(g["x"]))
    _assert_gx(g["x"], g_ref, "duplicates + White")


# ---- dense Σy -----------------------------------------------------------------------------------------------------------------------------
def test_dense_noise_covariance():
    n = 130
    X, y, _, _, _ = _six(n, False)
    k = six_term_kernel()
    B = np.random.default_rng(501).standard_normal((n, 4))
    S = 0.05 * np.eye(n) + 0.01 * B @ B.T
    g_ref = ref_logpdf_grad_x(k, X, y, S)
    _, a, L = host_fit(k, X, y, S)
    G_ref = 0.5 * (np.outer(a, a) - sla.cho_solve((L, True), np.eye(n)))
    _, g = agp.logpdf_and_grad(agp.GP(k)(agp.RowVecs(X), S), y, wrt_x=True)
    _assert_gx(g["x"], g_ref, "dense Σy n=130")
    assert g["noise"].shape == (n, n)
    np.testing.assert_allclose(g["noise"], G_ref, rtol=1e-7, atol=1e-8 * np.abs(G_ref).max())


# ---- logdetcov / sqmahal ------------------------------------------------------------------------------------------------------------------
def test_logdetcov_and_sqmahal_of_a_composite_kernel():
    n = 333
    X, y, _, _, _ = _six(n, False)
    k = six_term_kernel()
    mean, s2 = 0.3, 0.05
    L = sla.cholesky(ref_kernelmatrix(k, X) + s2 * np.eye(n), lower=True)
    Y = np.stack([y, np.cos(3 * y), y[::-1]], axis=1)
    Z = sla.solve_triangular(L, Y - mean, lower=True)
    ld_h, sq_h = 2 * np.sum(np.log(np.diag(L))), np.sum(Z * Z, axis=0)
    fx = agp.GP(mean, k)(agp.RowVecs(X), s2)
    ld, sq, SQ = agp.logdetcov(fx), agp.sqmahal(fx, y), agp.sqmahal(fx, Y)
    print(f"[terms] logdet rel {abs(ld - ld_h) / abs(ld_h):.2e}, sqmahal rel {abs(sq - sq_h[0]) / sq_h[0]:.2e}, matrix {np.max(np.abs(SQ - sq_h) / sq_h):.2e}")
    assert ld == pytest.approx(ld_h, rel=1e-10)
    assert sq == pytest.approx(sq_h[0], rel=1e-10)
    assert SQ.shape == (3,)
    np.testing.assert_allclose(SQ, sq_h, rtol=1e-10)
    assert agp.logpdf(fx, y) == pytest.approx(-0.5 * (n * math.log(2 * math.pi) + ld + sq), rel=1e-13)
    fx32 = agp.GP(mean, k)(agp.RowVecs(X.astype(np.float32)), np.float32(s2))
    ld32, sq32 = agp.logdetcov(fx32), agp.sqmahal(fx32, y.astype(np.float32))
    print(f"[terms] fp32 logdet rel {abs(float(ld32) - ld_h) / abs(ld_h):.2e}, sqmahal rel {abs(float(sq32) - sq_h[0]) / sq_h[0]:.2e}")
    assert isinstance(ld32, np.float32) and isinstance(sq32, np.float32)
    assert float(ld32) == pytest.approx(ld_h, rel=2e-3) and float(sq32) == pytest.approx(sq_h[0], rel=2e-3)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_abi_null_dx_equals_grad_sum_and_argument_errors():
    from tests.test_gpu_composite import _raw_ksum

    ctx = agp.default_context(0)
    lib = ctx.lib
    n = 130
    X, y, _, _, _ = _six(n, False)
    m = agp.api._Marshal(np.float64)
    px = m.points(agp.RowVecs(X))
    ks, nf = m.ksum(six_term_kernel(), 3)
    nth = len(nf.theta())
    nz = m.noise(0.05, n)
    yv = m.arr(y)
    lp_a, lp_b = np.empty(1), np.empty(1)
    th_a, th_b = (C.c_double * nth)(), (C.c_double * nth)()
    dn_a, dn_b, dy_a, dy_b = np.empty(1), np.empty(1), np.empty(n), np.empty(n)
    assert lib.gp_logpdf_grad_sum(ctx.handle, C.byref(ks), C.byref(px), C.byref(nz), None, yv.ctypes.data, lp_a.ctypes.data, th_a, dn_a.ctypes.data, dy_a.ctypes.data) == 0
    assert lib.gp_logpdf_grad_sum_x(ctx.handle, C.byref(ks), C.byref(px), C.byref(nz), None, yv.ctypes.data, lp_b.ctypes.data, th_b, dn_b.ctypes.data,
                                    dy_b.ctypes.data, None) == 0
    assert lp_a[0] == lp_b[0] and np.array_equal(dy_a, dy_b)
    assert _rel(np.array(th_b[:]), np.array(th_a[:])) <= 1e-12 and dn_b[0] == pytest.approx(dn_a[0], rel=1e-12)
    # a dead / NULL ctx
    dx = np.empty((n, 3))
    assert lib.gp_logpdf_grad_sum_x(None, C.byref(ks), C.byref(px), C.byref(nz), None, yv.ctypes.data, lp_b.ctypes.data, th_b, None, None, dx.ctypes.data) == -1
    assert lib.gp_logpdf_terms_sum(None, C.byref(ks), C.byref(px), C.byref(nz), None, yv.ctypes.data, n, 1, lp_b.ctypes.data, lp_b.ctypes.data) == -1
    # a malformed descriptor: −2 with the reason, from both
    bad, keep = _raw_ksum([(1.0, [(7, [], [])])])
    for call in (lambda: lib.gp_logpdf_grad_sum_x(ctx.handle, C.byref(bad), C.byref(px), C.byref(nz), None, yv.ctypes.data, lp_b.ctypes.data, th_b, None, None,
                                                  dx.ctypes.data),
                 lambda: lib.gp_logpdf_terms_sum(ctx.handle, C.byref(bad), C.byref(px), C.byref(nz), None, yv.ctypes.data, n, 1, lp_b.ctypes.data, lp_b.ctypes.data)):
        assert call() == -2
        assert "kind must be 0..6" in lib.gp_last_error().decode()
    # sqmahal without Y: the status of gp_logpdf_terms
    kk = m.kernel(agp.SqExponentialKernel(), 3)
    single = lib.gp_logpdf_terms(ctx.handle, C.byref(kk), C.byref(px), C.byref(nz), None, None, n, 1, None, lp_a.ctypes.data)
    comp = lib.gp_logpdf_terms_sum(ctx.handle, C.byref(ks), C.byref(px), C.byref(nz), None, None, n, 1, None, lp_b.ctypes.data)
    assert single == comp == -6
    assert "sqmahal needs Y" in lib.gp_last_error().decode()


# ---- the deep-kernel bridge (tools/train_deep_kernel_example.py) -------------------------------------------------------------------------
def test_deep_kernel_bridge_backpropagates_the_input_gradient():
    """The gradient of −logpdf against every parameter of an MLP 1 -> 4 -> 2 (fp64, CPU) through NegLogpdf, against central differences (h = 1e-5) of the
    device's own logpdf value: rel <= 1e-5 of the largest entry, the tolerance of test_gradient_against_a_central_difference_at_16384.  σ² = 0.01 here, not
    the tool's 1e-4: the N = 60 feature vectors are smooth functions of one scalar, K has a numerical rank near 10 and cond(K + σ²I) ≈ N/σ²; a central
    difference of a value with rounding error cond·ε·|logpdf| resolves (6e3·1e-16·1e2)/1e-5 ≈ 6e-6 absolute at σ² = 0.01 — far below 1e-5 of a gradient of
    order 10 or more — and a hundred times less of it at σ² = 1e-4.  Then 20 Adam steps lower the loss."""
    import torch

    import train_deep_kernel_example as dk

    x, y = dk.make_data(60, noise_std=0.1)
    kernel = dk.make_kernel("composite")
    net = dk.make_mlp((1, 4, 2), dtype=torch.float64, seed=1)
    x_t = torch.from_numpy(x)[:, None]
    loss = dk.loss_fn(net, x_t, y, kernel, 0.01)
    loss.backward()
    params = list(net.parameters())
    g = np.concatenate([p.grad.numpy().ravel() for p in params])
    fd, h = [], 1e-5
    with torch.no_grad():
        for p in params:
            flat = p.view(-1)
            for i in range(flat.numel()):
                v = float(flat[i])
                flat[i] = v + h
                lp_p = float(dk.loss_fn(net, x_t, y, kernel, 0.01))
                flat[i] = v - h
                lp_m = float(dk.loss_fn(net, x_t, y, kernel, 0.01))
                flat[i] = v
                fd.append((lp_p - lp_m) / (2 * h))
    fd = np.array(fd)
    err = float(np.max(np.abs(g - fd)) / np.abs(fd).max())
    print(f"[dkl] {len(fd)} parameters: max|g - fd| / max|fd| = {err:.3e}, max|fd| = {np.abs(fd).max():.3e}")
    assert err <= 1e-5
    losses = dk.train(net, x_t, y, kernel, 0.01, 20, log_every=0)
    print(f"[dkl] loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert losses[-1] < losses[0]
