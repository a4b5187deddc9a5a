"""GPU: gradients of the predictive mean and variance w.r.t. the test inputs — kpgrad_kernel / kpgrad_sum_kernel and the backward solve X ← X L⁻¹ behind
gp_posterior_predict_grad and gp_vfe_predict_grad — against the fp64 host references of tests/predict_grad_ref.py (central-difference checked in
tests/test_predict_grad_cpu.py).

Tolerance: the project's input-gradient tolerance (tests/test_gpu_composite_dx.py, test_gpu_api.py::test_logpdf_grad_wrt_inputs), g_ref from the HOST:
    fp64: rtol 1e-7, atol 1e-8·max(1, max|g_ref|)        fp32: rtol 2e-2, atol 2e-2·max(1, max|g_ref|)
Every check prints its measured error first ("[pg] ..." lines)."""
import ctypes as C
import functools

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests.composite_dx_ref import many_dim_kernel, six_term_data, six_term_kernel
from tests.conftest import rank_devices
from tests.predict_grad_ref import HostPosterior, central_differences, sparse_grads

pytestmark = pytest.mark.gpu

OKIND = {0: o.SE, 1: o.MATERN12, 2: o.MATERN32, 3: o.MATERN52}


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def _assert_g(g, g_ref, what=""):
    """the project's input-gradient tolerance for g's dtype; prints the measured error first"""
    f32 = g.dtype == np.float32
    tol = 2e-2 if f32 else 1e-7
    atol = (2e-2 if f32 else 1e-8) * max(1.0, float(np.abs(g_ref).max()))
    assert g.shape == g_ref.shape, (g.shape, g_ref.shape)
    err = float(np.max(np.abs(g.astype(np.float64) - g_ref)))
    print(f"[pg] {what} {g.dtype.name}: max|g - g_ref| = {err:.3e}, max|g_ref| = {np.abs(g_ref).max():.3e}, rel-norm = {_rel(g, g_ref):.3e}")
    assert np.all(np.isfinite(g))
    np.testing.assert_allclose(g, g_ref, rtol=tol, atol=atol)


def _assert_all(res, host, Xs, what):
    """(mean, var, dmean, dvar) of the device against the host posterior at Xs (rows)"""
    m, v, dm, dv = res
    mr, vr = host.mean_and_var(Xs)
    gm, gv = host.grads(Xs)
    if dm.ndim == 1:
        gm, gv = gm[:, 0], gv[:, 0]
    _assert_g(dm, gm, what + " dmean")
    _assert_g(dv, gv, what + " dvar")
    vtol = 2e-3 if m.dtype == np.float32 else 1e-8
    print(f"[pg] {what} values: max|mean - ref| = {np.abs(m - mr).max():.3e}, max|var - ref| = {np.abs(v - vr).max():.3e}")
    assert np.abs(m - mr).max() <= vtol * max(1.0, np.abs(mr).max()) and np.abs(v - vr).max() <= vtol * max(1.0, np.abs(vr).max())


def _single(kind, tr, d, var=1.3):
    """(device kernel, oracle kernel) of one kind behind no transform, a ScaleTransform or an ARDTransform"""
    if tr == "none":
        return var * agp.Kernel(kind), o.Kernel(OKIND[kind], var)
    if tr == "scale":
        return var * agp.Kernel(kind) @ agp.ScaleTransform(0.7), o.Kernel(OKIND[kind], var, 0.7)
    v = np.linspace(0.5, 1.1, d)
    return var * agp.Kernel(kind) @ agp.ARDTransform(v), o.Kernel(OKIND[kind], var, v)


def _data(n, d, seed, ns):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 3, size=(n, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
    return X, y, rng.uniform(0, 3, size=(ns, d))


def _own_ctx(**kw):
    ctx = agp.Context(0)
    for k, v in kw.items():
        ctx.set_param(k, v)
    return ctx


# ---- 1. kinds and transforms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("tr", ["none", "scale", "ard"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_kinds_and_transforms(kind, tr, d):
    X, y, Xs = _data(300, d, 10 * kind + d, 37)
    k, ok = _single(kind, tr, d)
    host = HostPosterior(ok, X, y, 0.05)
    xin, xsin = (X[:, 0], Xs[:, 0]) if d == 1 else (agp.RowVecs(X), agp.RowVecs(Xs))  # D = 1: the vector container
    res = agp.posterior(agp.GP(k)(xin, 0.05), y).mean_and_var_grad(xsin)
    assert res[2].shape == ((37,) if d == 1 else (37, 3))
    _assert_all(res, host, Xs, f"kind {kind} {tr} D={d}")


# ---- 2. shapes on the default context -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 129, 300])
def test_shapes_on_the_default_context(n):
    k, ok = _single(2, "ard", 3)
    X, y, _ = _data(n, 3, 40 + n, 1)
    host = HostPosterior(ok, X, y, 0.05)
    post = agp.posterior(agp.GP(k)(agp.RowVecs(X), 0.05), y)
    for ns in (1, 127, 129):
        Xs = np.random.default_rng(ns).uniform(0, 3, size=(ns, 3))
        _assert_all(post.mean_and_var_grad(agp.RowVecs(Xs)), host, Xs, f"n={n} ns={ns}")


# ---- 3. several inverse blocks ----------------------------------------------------------------------------------------------------------------
def test_backward_sweep_across_several_inverse_blocks():
    """n = 700 (768 padded) with dib_nb = 256: the partition of the forward solve (dib_ranges: halves until a block fits) gives FOUR inverse blocks of 192
    columns, not three of 256 — the backward sweep crosses three block boundaries"""
    k, ok = _single(3, "ard", 3)
    X, y, Xs = _data(700, 3, 50, 129)
    host = HostPosterior(ok, X, y, 0.05)
    ctx = _own_ctx(dib_nb=256)
    try:
        res = agp.posterior(agp.GP(k, ctx=ctx)(agp.RowVecs(X), 0.05), y).mean_and_var_grad(agp.RowVecs(Xs))
    finally:
        ctx.close()
    _assert_all(res, host, Xs, "n=700 dib_nb=256")


# ---- 4. the 4 096-row chunk boundary ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dib_nb", [2048, 128], ids=["substitution", "two-inverse-blocks"])
def test_more_test_points_than_one_chunk(dib_nb):
    """ns = 4 099 at n = 200 (256 padded points): a chunk of 4 096 rows and one of 3 valid rows, through the back-substitution (no blocks below 2 048 points)
    and through the blocked sweep (dib_nb = 128: two inverse blocks)"""
    k, ok = _single(0, "scale", 2)
    X, y, Xs = _data(200, 2, 60, 4099)
    host = HostPosterior(ok, X, y, 0.05)
    ctx = _own_ctx(dib_nb=dib_nb)
    try:
        res = agp.posterior(agp.GP(k, ctx=ctx)(agp.RowVecs(X), 0.05), y).mean_and_var_grad(agp.RowVecs(Xs))
    finally:
        ctx.close()
    _assert_all(res, host, Xs, f"n=200 ns=4099 dib_nb={dib_nb}")


# ---- 5. dimensions ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 16])
def test_composite_kernel_in_many_dimensions(d):
    rng = np.random.default_rng(200 + d)
    X = rng.uniform(0, 2, size=(300, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(300)
    Xs = rng.uniform(0, 2, size=(37, d))
    k = many_dim_kernel(d)
    host = HostPosterior(k, X, y, 0.05)
    _assert_all(agp.posterior(agp.GP(k)(agp.RowVecs(X), 0.05), y).mean_and_var_grad(agp.RowVecs(Xs)), host, Xs, f"many-dim D={d}")


@pytest.mark.parametrize("d,dtype", [(20, np.float64), (17, np.float32)])
def test_single_kind_beyond_sixteen_dimensions(d, dtype):
    """two passes of 16 dimensions (the second with 4 / 1 of them)"""
    rng = np.random.default_rng(300 + d)
    X = rng.uniform(0, 2, size=(300, d)).astype(dtype)
    y = (np.sin(X.sum(1)) + 0.1 * rng.standard_normal(300)).astype(dtype)
    Xs = rng.uniform(0, 2, size=(37, d)).astype(dtype)
    v = np.linspace(0.3, 0.6, d)
    host = HostPosterior(o.Kernel(o.SE, 1.2, v), X.astype(np.float64), y.astype(np.float64), 0.05)
    res = agp.posterior(agp.GP(1.2 * agp.SqExponentialKernel() @ agp.ARDTransform(v))(agp.RowVecs(X), dtype(0.05)), y).mean_and_var_grad(agp.RowVecs(Xs))
    assert res[2].dtype == dtype
    _assert_all(res, host, Xs.astype(np.float64), f"SE∘ARD D={d}")


# ---- 6. the six-term kernel, every container -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _six(n=300):
    X, y = six_term_data(n, seed=n)
    Xs = np.concatenate([np.random.default_rng(n + 1).uniform(0, 3, size=(34, 3)), X[[0, 77, n - 1]]])  # three test points ON training points
    host = HostPosterior(six_term_kernel(), X, y, 0.05)
    for a in (X, y, Xs):
        a.setflags(write=False)
    return X, y, Xs, host


def test_six_term_kernel_every_container():
    X, y, Xs, host = _six()
    k = six_term_kernel()
    res = agp.posterior(agp.GP(k)(agp.RowVecs(X), 0.05), y).mean_and_var_grad(agp.RowVecs(Xs))
    assert res[2].shape == (37, 3) and res[3].shape == (37, 3) and res[0].shape == (37,)
    _assert_all(res, host, Xs, "six-term RowVecs")
    resc = agp.posterior(agp.GP(k)(agp.ColVecs(X.T.copy()), 0.05), y).mean_and_var_grad(agp.ColVecs(Xs.T.copy()))
    assert resc[2].shape == (3, 37) and resc[3].shape == (3, 37)
    _assert_all((resc[0], resc[1], resc[2].T, resc[3].T), host, Xs, "six-term ColVecs")
    # a vector: the six-term form needs D = 3, so the D = 1 container runs a two-term composite with a White term and a Matern12 term
    k1 = 1.1 * agp.SqExponentialKernel() @ agp.ScaleTransform(0.8) + 0.3 * agp.Matern12Kernel() + 0.01 * agp.WhiteKernel()
    x1, xs1 = X[:, 0].copy(), np.concatenate([Xs[:30, 0], X[[3, 5, 9], 0]])
    h1 = HostPosterior(k1, x1, y, 0.05)
    r1 = agp.posterior(agp.GP(k1)(x1, 0.05), y).mean_and_var_grad(xs1)
    assert r1[2].shape == (33,) and r1[3].shape == (33,)
    _assert_all(r1, h1, xs1[:, None], "composite vector")


# ---- 7. fp32 handles --------------------------------------------------------------------------------------------------------------------------
def test_fp32_handles():
    """If a variance gradient misses the bound, the message carries the measured figure and the factor's max|L_ii| / min|L_ii|."""
    X, y, Xs, _ = _six()
    X32, y32, Xs32 = X.astype(np.float32), y.astype(np.float32), Xs[:34].astype(np.float32)
    for name, k, hk in (("six-term", six_term_kernel(), six_term_kernel()), ("Matern52∘ARD",) + _single(3, "ard", 3)):
        host = HostPosterior(hk, X32.astype(np.float64), y32.astype(np.float64), 0.05)
        print(f"[pg] fp32 {name}: host factor max|L_ii| / min|L_ii| = {host.diag_ratio():.3e}")
        res = agp.posterior(agp.GP(k)(agp.RowVecs(X32), np.float32(0.05)), y32).mean_and_var_grad(agp.RowVecs(Xs32))
        assert all(r.dtype == np.float32 for r in res)
        _assert_all(res, host, Xs32.astype(np.float64), f"fp32 {name} (diag ratio {host.diag_ratio():.2e})")


# ---- raw calls through the C ABI (8, 9, 10) ----------------------------------------------------------------------------------------------------
def _raw(fn, handle, Xs, what, outs=(True, True, True, True), dtype=np.float64):
    """one raw call; outs: which of (mean, var, dmean, dvar) get a buffer (NULL otherwise).  Returns (status, buffers)."""
    m = agp.api._Marshal(dtype)
    px = m.points(agp.RowVecs(Xs))
    shapes = [(px.n,), (px.n,), (px.n, px.d), (px.n, px.d)]
    bufs = [np.full(s, np.nan, dtype=dtype) if on else None for s, on in zip(shapes, outs)]
    rc = fn(handle, C.byref(px), None, what, *[m.ptr(b) for b in bufs])
    return rc, bufs


@pytest.fixture(scope="module")
def fitted():
    k, ok = _single(2, "ard", 3)
    X, y, Xs = _data(300, 3, 80, 37)
    post = agp.posterior(agp.GP(k)(agp.RowVecs(X), 0.05), y)
    return post, HostPosterior(ok, X, y, 0.05), Xs


def test_values_equal_those_of_predict(fitted):
    post, _, Xs = fitted
    m, v, _, _ = post.mean_and_var_grad(agp.RowVecs(Xs))
    m0, v0 = post.mean_and_var(agp.RowVecs(Xs))
    print(f"[pg] values vs gp_posterior_predict: rel mean {_rel(m, m0):.2e}, rel var {_rel(v, v0):.2e}")
    assert _rel(m, m0) <= 1e-12 and _rel(v, v0) <= 1e-12


def test_each_side_alone_and_each_pointer_null(fitted):
    post, host, Xs = fitted
    lib, h = post.data.C.ctx.lib, post.data.C.handle
    mr, vr = host.mean_and_var(Xs)
    gm, gv = host.grads(Xs)
    for what, outs in ((1, (True, False, True, False)), (1, (False, False, True, False)), (1, (True, False, False, False)),
                       (2, (False, True, False, True)), (2, (False, False, False, True)), (2, (False, True, False, False)),
                       (3, (False, False, True, True)), (3, (True, True, False, False))):
        rc, (m, v, dm, dv) = _raw(lib.gp_posterior_predict_grad, h, Xs, what, outs)
        assert rc == 0, (what, outs, lib.gp_last_error())
        if m is not None:
            assert np.abs(m - mr).max() <= 1e-8
        if v is not None:
            assert np.abs(v - vr).max() <= 1e-8
        if dm is not None:
            _assert_g(dm, gm, f"what={what} outs={outs} dmean")
        if dv is not None:
            _assert_g(dv, gv, f"what={what} outs={outs} dvar")
    # the thin wrappers
    m, dm = post.mean_grad(agp.RowVecs(Xs))
    v, dv = post.var_grad(agp.RowVecs(Xs))
    _assert_g(dm, gm, "mean_grad")
    _assert_g(dv, gv, "var_grad")


def test_argument_errors_have_statuses_and_reasons(fitted):
    post, _, Xs = fitted
    lib, h = post.data.C.ctx.lib, post.data.C.handle
    fn = lib.gp_posterior_predict_grad
    for what in (0, 4, 7, -1):
        rc, _ = _raw(fn, h, Xs, what)
        assert rc == -4 and b"what must be a combination of 1|2" in lib.gp_last_error(), (what, rc, lib.gp_last_error())
    rc, _ = _raw(fn, h, Xs[:, :2].copy(), 3)
    assert rc == -2 and b"xs has a different D than the training inputs" in lib.gp_last_error()
    rc, _ = _raw(fn, h, Xs, 1, (False, True, False, True))
    assert rc == -5 and b"mean_out and dmean_out are both NULL" in lib.gp_last_error()
    rc, _ = _raw(fn, h, Xs, 2, (True, False, True, False))
    assert rc == -6 and b"var_out and dvar_out are both NULL" in lib.gp_last_error()
    k, _ = _single(0, "none", 3)
    X, y, _ = _data(20, 3, 81, 1)
    dead = agp.posterior(agp.GP(k)(agp.RowVecs(X), 0.05), y)
    hd = C.c_void_p(dead.data.C.handle.value)
    dead.data.C.free()
    rc, _ = _raw(fn, hd, Xs, 3)
    assert rc == -1 and b"not a live gp_post" in lib.gp_last_error()
    rc, _ = _raw(lib.gp_vfe_predict_grad, hd, Xs, 3)
    assert rc == -1 and b"not a live gp_vfe" in lib.gp_last_error()


def test_custom_mean_needs_its_gradient():
    k, ok = _single(0, "scale", 3)
    X, y, Xs = _data(100, 3, 82, 9)
    f = agp.GP(lambda x: 0.5 * float(np.sum(x)), k)
    post = agp.posterior(f(agp.RowVecs(X), 0.05), y)
    with pytest.raises(TypeError):
        post.mean_and_var_grad(agp.RowVecs(Xs))
    host = HostPosterior(ok, X, y - 0.5 * X.sum(1), 0.05)
    m, v, dm, dv = post.mean_and_var_grad(agp.RowVecs(Xs), mean_grad=lambda x: np.full((9, 3), 0.5))
    gm, gv = host.grads(Xs)
    _assert_g(dm, gm + 0.5, "custom mean dmean")
    _assert_g(dv, gv, "custom mean dvar")
    _assert_g(post.var_grad(agp.RowVecs(Xs))[1], gv, "custom mean var_grad (no mean gradient needed)")
    c = agp.posterior(agp.GP(0.7, k)(agp.RowVecs(X), 0.05), y)   # ConstMean: exact without anything
    hc = HostPosterior(ok, X, y, 0.05, mean=0.7)
    _assert_all(c.mean_and_var_grad(agp.RowVecs(Xs)), hc, Xs, "ConstMean")


# ---- 11. bitwise repeat -------------------------------------------------------------------------------------------------------------------------
def test_two_identical_calls_give_identical_bits_when_deterministic():
    k, _ = _single(3, "ard", 3)
    X, y, Xs = _data(700, 3, 90, 129)
    ctx = _own_ctx(deterministic=1, dib_nb=256)
    try:
        post = agp.posterior(agp.GP(k, ctx=ctx)(agp.RowVecs(X), 0.05), y)
        a = post.mean_and_var_grad(agp.RowVecs(Xs))
        b = post.mean_and_var_grad(agp.RowVecs(Xs))
    finally:
        ctx.close()
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


# ---- 12. poisoned blocks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dib_nb", [2048, 256])
def test_results_do_not_depend_on_recycled_blocks(dib_nb):
    k, _ = _single(2, "ard", 3)
    X, y, Xs = _data(700, 3, 91, 129)
    out = []
    for poison in (0, 1):
        ctx = _own_ctx(alloc_poison=poison, dib_nb=dib_nb)
        try:
            post = agp.posterior(agp.GP(k, ctx=ctx)(agp.RowVecs(X), 0.05), y)
            post.mean_and_var_grad(agp.RowVecs(Xs[:5]))            # leaves released blocks in the pool for the second call
            out.append(post.mean_and_var_grad(agp.RowVecs(Xs)))
        finally:
            ctx.close()
    for name, p, q in zip(("mean", "var", "dmean", "dvar"), out[0], out[1]):
        print(f"[pg] poisoned vs clean dib_nb={dib_nb} {name}: rel = {_rel(q, p):.2e}")
        assert np.all(np.isfinite(q)) and _rel(q, p) <= 1e-12


# ---- 13. substitution path ----------------------------------------------------------------------------------------------------------------------
def test_substitution_path_without_inverse_blocks():
    """dib_nb = 0: the backward solve is the vector back-substitution, once per test point (the branch the conditioning guard nbi = −1 takes as well)"""
    k, ok = _single(1, "scale", 3)
    X, y, Xs = _data(300, 3, 92, 5)
    host = HostPosterior(ok, X, y, 0.05)
    ctx = _own_ctx(dib_nb=0)
    try:
        res = agp.posterior(agp.GP(k, ctx=ctx)(agp.RowVecs(X), 0.05), y).mean_and_var_grad(agp.RowVecs(Xs))
    finally:
        ctx.close()
    _assert_all(res, host, Xs, "dib_nb=0")


# ---- 14. sequential conditioning ---------------------------------------------------------------------------------------------------------------
def test_handle_from_sequential_conditioning():
    k, ok = _single(0, "ard", 3)
    X, y, Xs = _data(350, 3, 93, 37)
    host = HostPosterior(ok, X, y, 0.05)
    p1 = agp.posterior(agp.GP(k)(agp.RowVecs(X[:200]), 0.05), y[:200])
    p2 = agp.posterior(p1(agp.RowVecs(X[200:]), 0.05), y[200:])
    _assert_all(p2.mean_and_var_grad(agp.RowVecs(Xs)), host, Xs, "200 + 150 sequential")


# ---- 15. multi-device context -------------------------------------------------------------------------------------------------------------------
def test_multi_device_context_equals_the_single_device_result():
    k, _ = _single(2, "ard", 3)
    X, y, Xs = _data(700, 3, 94, 129)
    single = agp.posterior(agp.GP(k)(agp.RowVecs(X), 0.05), y).mean_and_var_grad(agp.RowVecs(Xs))
    ctx = agp.Context(devices=rank_devices(2), P=2, Q=1, nb=256)
    try:
        post = agp.posterior(agp.GP(k, ctx=ctx)(agp.RowVecs(X), 0.05), y)
        _, dm_only = post.mean_grad(agp.RowVecs(Xs))                # the mean side needs no factor: no gather
        multi = post.mean_and_var_grad(agp.RowVecs(Xs))
    finally:
        ctx.close()
    for name, p, q in zip(("mean", "var", "dmean", "dvar"), single, multi):
        print(f"[pg] multi-device vs single {name}: rel = {_rel(q, p):.2e}")
        assert _rel(q, p) <= 1e-12
    assert _rel(dm_only, single[2]) <= 1e-12


# ---- 16. sparse posteriors -----------------------------------------------------------------------------------------------------------------------
def _sparse_case(approx, kind, m, dtype, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, size=(500, 3)).astype(dtype)
    y = (np.sin(X.sum(1)) + 0.1 * rng.standard_normal(500)).astype(dtype)
    Z = rng.uniform(-2, 2, size=(m, 3)).astype(dtype)
    v = np.array([0.5, 1.1, 0.9])
    k, ok = 1.3 * agp.Kernel(kind) @ agp.ARDTransform(v), o.Kernel(OKIND[kind], 1.3, v)
    return X, y, Z, k, ok


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("m", [37, 129, 300])
def test_sparse_posteriors(m, dtype):
    """VFE and DTC, N = 500, kinds 0 / 2 / 3, ns = 1 and 130; M = 300 on a context with dib_nb = 128 (384 padded pseudo-points: blocks of 64 and 128 columns).
    jitter 1e-4: the fp32 handles stream the N-long side in fp32, and cond(K_zz + jitter I) multiplies that rounding."""
    ctx = _own_ctx(dib_nb=128) if m == 300 else None
    try:
        for approx in (agp.VFE, agp.DTC):
            for kind in (0, 2, 3):
                X, y, Z, k, ok = _sparse_case(approx, kind, m, dtype, 100 + kind + m)
                f = agp.GP(k, ctx=ctx) if ctx else agp.GP(k)
                post = agp.posterior(approx(f(agp.RowVecs(Z), 1e-4)), f(agp.RowVecs(X), dtype(0.05)), y)
                fo = o.GP(ok)
                ref = o.vfe_posterior(fo, Z.astype(np.float64), 1e-4, o.FiniteGP(fo, X.astype(np.float64), 0.05), y.astype(np.float64))
                for ns in (1, 130):
                    Xs = np.random.default_rng(ns).uniform(-2, 2, size=(ns, 3)).astype(dtype)
                    mean, var, dm, dv = post.mean_and_var_grad(agp.RowVecs(Xs))
                    assert dm.dtype == dtype and dm.shape == (ns, 3)
                    gm, gv = sparse_grads(ref, Xs.astype(np.float64))
                    tag = f"{approx.__name__} kind {kind} M={m} ns={ns}"
                    _assert_g(dm, gm, tag + " dmean")
                    _assert_g(dv, gv, tag + " dvar")
                    m0, v0 = post.mean_and_var(agp.RowVecs(Xs))
                    assert _rel(mean, m0) <= 1e-6 and np.abs(var.astype(np.float64) - v0).max() <= 1e-6
    finally:
        if ctx:
            ctx.close()


# ---- 17. sparse posteriors after extending ---------------------------------------------------------------------------------------------------
def test_sparse_posterior_after_new_observations_and_new_pseudo_points():
    X, y, Z, k, ok = _sparse_case(agp.VFE, 2, 60, np.float64, 170)
    Xs = np.random.default_rng(171).uniform(-2, 2, size=(37, 3))
    f, fo = agp.GP(k), o.GP(ok)
    post = agp.posterior(agp.VFE(f(agp.RowVecs(Z[:40]), 1e-4)), f(agp.RowVecs(X[:300]), 0.05), y[:300])
    post = agp.update_posterior(post, f(agp.RowVecs(X[300:]), 0.05), y[300:])
    ref = o.vfe_posterior(fo, Z[:40], 1e-4, o.FiniteGP(fo, X, 0.05), y)
    _, _, dm, dv = post.mean_and_var_grad(agp.RowVecs(Xs))
    gm, gv = sparse_grads(ref, Xs)
    _assert_g(dm, gm, "after gp_vfe_update dmean")
    _assert_g(dv, gv, "after gp_vfe_update dvar")
    post2 = agp.update_posterior(post, f(agp.RowVecs(Z[40:]), 1e-4))
    # the reference's append gives the NEW pseudo-points no jitter (src/sparse_approximations.jl:138; tests/test_gpu_vfe_grad.py): the oracle's own
    # update over all the observations, not a refit with one jitter for every pseudo-point
    ref2 = o.vfe_update_z(ref, Z[40:])
    _, _, dm, dv = post2.mean_and_var_grad(agp.RowVecs(Xs))
    gm, gv = sparse_grads(ref2, Xs)
    _assert_g(dm, gm, "after gp_vfe_append dmean")
    _assert_g(dv, gv, "after gp_vfe_append dvar")


# ---- 18. end to end: an acquisition function --------------------------------------------------------------------------------------------------
def test_gradient_of_an_acquisition_function_against_differences_of_the_device():
    """a(x) = mean + 2·sqrt(var) at 20 points, n = 300: the gradient assembled from ONE call against central differences (h = 1e-5) of the device's OWN
    mean_and_var.  Bound 1e-7·max|g| + 2δ/h with δ the largest |device − host reference| of a on the perturbed points (a value error of δ on each side
    moves the difference quotient by at most δ/h; the factor 2 is margin), δ computed here from the host reference."""
    k, ok = _single(3, "ard", 3)
    X, y, Xs = _data(300, 3, 180, 20)
    host = HostPosterior(ok, X, y, 0.05)
    post = agp.posterior(agp.GP(k)(agp.RowVecs(X), 0.05), y)
    m, v, dm, dv = post.mean_and_var_grad(agp.RowVecs(Xs))
    g = dm + dv / np.sqrt(v)[:, None]
    h, delta = 1e-5, [0.0]

    def acq(P):
        md, vd = post.mean_and_var(agp.RowVecs(P))
        mh, vh = host.mean_and_var(P)
        ad, ah = md + 2 * np.sqrt(vd), mh + 2 * np.sqrt(vh)
        delta[0] = max(delta[0], float(np.abs(ad - ah).max()))
        return ad, ad

    fd = central_differences(acq, Xs, h)[0]
    bound = 1e-7 * np.abs(g).max() + 2 * delta[0] / h
    err = float(np.abs(fd - g).max())
    print(f"[pg] acquisition: max|fd - g| = {err:.3e}, max|g| = {np.abs(g).max():.3e}, delta = {delta[0]:.3e}, bound = {bound:.3e}")
    assert err <= bound
