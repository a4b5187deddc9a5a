"""GPU: one factorisation for a matrix of observations — gp_posterior_fit_cols / gp_posterior_predict_cols / gp_logpdf_grad_cols and their *_sum forms
through the mirror (posterior_columns, logpdf_and_grad_columns) against the fp64 reference column by column (tests/cols_cases.py), at the tolerances the
single-column calls are held to: logpdf 1e-10, α and dY 1e-8, mean 1e-8, var / cov 1e-9, gradients rtol 1e-7 / atol 1e-9 of the largest entry; fp32 at
the tolerances of the fp32 fits.  Then the properties of the new kernel: one column equals the old calls, a column's bits do not depend on the other
columns, two calls return the same bits, which launches split the training range, nothing depends on what a recycled block held, and what a handle with
more than one column serves and refuses."""
import ctypes as C

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import cols_cases as cc

pytestmark = pytest.mark.gpu


def _with_ctx(fx, ctx):
    f = fx.f
    g = agp.GP(f.kernel, ctx=ctx) if f.mean_fn is None else agp.GP(f.mean_fn, f.kernel, ctx=ctx)
    return g(fx.x, fx.sigma2)


def _check_fit_and_predict(c, post, ref, f32=False):
    lp_tol, a_tol, m_tol, v_tol = (cc.LP_TOL32, cc.A_TOL32, cc.M_TOL32, cc.V_TOL32) if f32 else (cc.LP_TOL, cc.A_TOL, cc.M_TOL, cc.V_TOL)
    n, ns, S = c["n"], c["ns"], c["S"]
    dt = np.float32 if f32 else np.float64
    assert post.ncols == S and post.data.alpha.shape == (n, S) and post.logpdf_values.shape == (S,)
    assert post.data.alpha.dtype == dt and post.logpdf_values.dtype == dt
    lp_err = np.max(np.abs(post.logpdf_values.astype(np.float64) - ref["lp"]) / np.maximum(np.abs(ref["lp"]), 1.0))
    a_err = max(cc.rel(post.data.alpha[:, s], ref["alpha"][:, s]) for s in range(S))
    m, v = post.mean_and_var(c["xs"])
    m2, cov = post.mean_and_cov(c["xs"])
    assert m.shape == (ns, S) and v.shape == (ns,) and cov.shape == (ns, ns) and m.dtype == dt
    m_err, v_err, c_err = np.max(np.abs(m - ref["mean"])), np.max(np.abs(v - ref["var"])), np.max(np.abs(cov - ref["cov"]))
    print(f"COLS {c['id']} {dt.__name__}: logpdf {lp_err:.2e} alpha {a_err:.2e} mean {m_err:.2e} var {v_err:.2e} cov {c_err:.2e}")
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v)) and np.all(np.isfinite(cov))
    assert lp_err <= lp_tol and a_err <= a_tol
    assert m_err <= m_tol and v_err <= v_tol and c_err <= v_tol
    assert np.array_equal(m, m2) and np.array_equal(post.mean(c["xs"]), m)          # two calls, the same bits
    assert np.array_equal(post.var(c["xs"]), v) or np.max(np.abs(post.var(c["xs"]) - v)) <= v_tol  # (the variance path is the old one)


def _check_grad(c, lp, g, ref, f32=False, wrt_x=True):
    n, S = c["n"], c["S"]
    rg = ref["grad"]

    def close(name, got, want):
        want = np.asarray(want, dtype=np.float64)
        got = np.asarray(got, dtype=np.float64)
        big = max(1.0, float(np.max(np.abs(want))))
        err = float(np.max(np.abs(got - want)))
        print(f"COLSGRAD {c['id']} {name}: max abs err {err:.2e} (largest entry {big:.2e})")
        assert got.shape == want.shape, name
        if f32:
            assert err <= cc.G_TOL32 * big, name
        else:
            np.testing.assert_allclose(got, want, rtol=cc.G_RTOL, atol=cc.G_ATOL * big, err_msg=name)

    lp_err = np.max(np.abs(lp.astype(np.float64) - ref["lp"]) / np.maximum(np.abs(ref["lp"]), 1.0))
    assert lp.shape == (S,) and lp_err <= (cc.LP_TOL32 if f32 else cc.LP_TOL)
    assert g["y"].shape == (n, S)
    assert max(cc.rel(-g["y"][:, s], ref["alpha"][:, s]) for s in range(S)) <= (cc.A_TOL32 if f32 else cc.A_TOL)
    assert np.array_equal(g["mean"], -g["y"])
    if c["composite"]:
        close("theta", g["theta"], rg["theta"])
    else:
        close("variance", g["variance"], rg["variance"])
        if rg["scale"] is None:
            assert g["scale"] is None
        else:
            close("scale", g["scale"], rg["scale"])
    close("noise", g["noise"], rg["noise"])
    if wrt_x:
        close("x", g["x"], cc.grad_x_shaped(c, rg["x"]))


@pytest.mark.parametrize("cid", [c[0] for c in cc.SINGLE])
def test_single_kind_columns_against_the_oracle(agp, cid):
    c = cc.single_case(cid)
    ref = cc.reference(c)
    post = agp.posterior_columns(c["fx"], c["Y"])
    _check_fit_and_predict(c, post, ref)
    lp, g = agp.logpdf_and_grad_columns(c["fx"], c["Y"], wrt_x=True)
    _check_grad(c, lp, g, ref)
    lp2, g2 = agp.logpdf_and_grad_columns(c["fx"], c["Y"])  # dx_out NULL
    assert "x" not in g2 and np.max(np.abs(lp2 - lp)) <= 1e-10 * np.max(np.abs(lp))
    post.data.C.free()


@pytest.mark.parametrize("cid", [c[0] for c in cc.COMPOSITE])
def test_composite_columns_against_the_numpy_reference(agp, cid):
    c = cc.composite_case(cid)
    ref = cc.reference(c)
    post = agp.posterior_columns(c["fx"], c["Y"])
    _check_fit_and_predict(c, post, ref)
    lp, g = agp.logpdf_and_grad_columns(c["fx"], c["Y"], wrt_x=True)
    _check_grad(c, lp, g, ref)
    post.data.C.free()


@pytest.mark.parametrize("cid", [c[0] for c in cc.F32])
def test_fp32_columns(agp, cid):
    c = cc.single_case(cid, np.float32)
    ref = cc.reference(c, np.float32)
    post = agp.posterior_columns(c["fx"], c["Y"])
    _check_fit_and_predict(c, post, ref, f32=True)
    lp, g = agp.logpdf_and_grad_columns(c["fx"], c["Y"], wrt_x=True)
    assert lp.dtype == np.float32 and g["y"].dtype == np.float32 and g["x"].dtype == np.float32
    _check_grad(c, lp, g, ref, f32=True)
    post.data.C.free()


@pytest.mark.parametrize("cid", ["n63", "n300_cap", "n300_d17", "mauna_loa"])
def test_one_column_equals_the_single_column_calls(agp, cid):
    """S = 1 through the column calls against gp_posterior_fit + gp_posterior_predict / gp_logpdf_grad on the same inputs, and gp_posterior_predict_cols on the
    handle of gp_posterior_fit (which it serves: ncols = 1)"""
    c = cc.composite_case(cid) if cid == "mauna_loa" else cc.single_case(cid)
    y = c["Y"][:, 0].copy()
    one = agp.posterior(c["fx"], y)
    cols = agp.posterior_columns(c["fx"], y[:, None])
    assert cols.ncols == 1
    assert abs(float(cols.logpdf_values[0]) - float(one.logpdf_value)) <= cc.LP_TOL * max(1.0, abs(float(one.logpdf_value)))
    assert cc.rel(cols.data.alpha[:, 0], one.data.alpha) <= cc.A_TOL
    m1, v1 = one.mean_and_var(c["xs"])
    mc, vc = cols.mean_and_var(c["xs"])
    assert mc.shape == (c["ns"], 1) and np.max(np.abs(mc[:, 0] - m1)) <= cc.M_TOL and np.max(np.abs(vc - v1)) <= cc.V_TOL
    # the old handle through the new call
    ns = c["ns"]
    m = agp.api._Marshal(np.float64)
    px = m.points(c["xs"])
    pm = agp.api._mean_vector(c["fx"].f.mean_fn, c["xs"], np.float64)
    out = np.full(ns, np.nan)
    nc = C.c_int32(-1)
    lib = one.data.C.ctx.lib
    agp._lib.check(lib.gp_posterior_ncols(one.data.C.handle, C.byref(nc)))
    agp._lib.check(lib.gp_posterior_predict_cols(one.data.C.handle, C.byref(px), m.ptr(None if pm is None else m.arr(pm)), 1, out.ctypes.data, None, None))
    assert nc.value == 1 and np.max(np.abs(out - m1)) <= cc.M_TOL
    lp1, g1 = agp.logpdf_and_grad(c["fx"], y, wrt_x=True)
    lpc, gc = agp.logpdf_and_grad_columns(c["fx"], y[:, None], wrt_x=True)
    assert abs(float(lpc[0]) - float(lp1)) <= cc.LP_TOL * max(1.0, abs(float(lp1)))
    for key in g1:
        if g1[key] is None:
            assert gc[key] is None
            continue
        a, b = np.asarray(gc[key], dtype=np.float64), np.asarray(g1[key], dtype=np.float64)
        np.testing.assert_allclose(a.reshape(b.shape), b, rtol=cc.G_RTOL, atol=cc.G_ATOL * max(1.0, float(np.max(np.abs(b)))), err_msg=key)
    one.data.C.free()
    cols.data.C.free()


@pytest.mark.parametrize("cid", ["n129", "n300_cap", "persewhite_d2"])
def test_a_columns_bits_do_not_depend_on_the_other_columns_and_repeat(agp, cid):
    """On a ctx of its own with "deterministic" = 1 (no atomics in the fit's backward sweep either): column 0 of the fit and of the means keeps its bits when
    every other column is replaced, and a second fit + predict returns the bits of the first."""
    c = cc.composite_case(cid) if c_is_composite(cid) else cc.single_case(cid)
    ctx = agp.Context(0)
    ctx.set_param("deterministic", 1)
    try:
        fx = _with_ctx(c["fx"], ctx)
        Y = np.asfortranarray(c["Y"])
        Y2 = np.asfortranarray(np.random.default_rng(5).standard_normal(Y.shape) * 7.0)
        Y2[:, 0] = Y[:, 0]
        a = agp.posterior_columns(fx, Y)
        b = agp.posterior_columns(fx, Y2)
        a2 = agp.posterior_columns(fx, Y)
        ma, mb, ma2 = a.mean(c["xs"]), b.mean(c["xs"]), a2.mean(c["xs"])
        assert np.array_equal(a.data.alpha, a2.data.alpha) and np.array_equal(ma, ma2) and np.array_equal(a.logpdf_values, a2.logpdf_values)
        assert np.array_equal(a.data.alpha[:, 0], b.data.alpha[:, 0]) and a.logpdf_values[0] == b.logpdf_values[0]
        assert np.array_equal(ma[:, 0], mb[:, 0])
        assert not np.array_equal(ma[:, 1], mb[:, 1])
        for p in (a, b, a2):
            p.data.C.free()
    finally:
        ctx.close()


def c_is_composite(cid):
    return cid in [c[0] for c in cc.COMPOSITE]


def test_which_launches_split_the_training_range(agp):
    """"cols_kernel_calls" / "cols_kernel_splits" (include/gpmi355.h): n = 225 is the smallest problem whose 8 strips of 32 training points go to two
    workgroups (ns = 1); n = 224 stays one; single-kind D = 17 takes the kvec launches and does not count.  Both sides against a NumPy product."""
    ctx = agp.Context(0)
    try:
        rng = np.random.default_rng(3)
        f = agp.GP(1.3 * agp.Matern32Kernel() @ agp.ScaleTransform(0.7), ctx=ctx)
        from oracle import gp_oracle as o

        for n, ns, want in ((224, 1, 1), (225, 1, 2), (300, 200, 2), (129, 65, 1)):
            x = rng.uniform(0, 4, size=n)
            xs = rng.uniform(0, 4, size=ns)
            Y = rng.standard_normal((n, 3))
            calls = ctx.get_param("cols_kernel_calls")
            post = agp.posterior_columns(f(x, 0.05), Y)
            assert ctx.get_param("cols_kernel_calls") == calls      # the fit launches no kmul
            m = post.mean(xs)
            assert ctx.get_param("cols_kernel_calls") == calls + 1 and ctx.get_param("cols_kernel_splits") == want, (n, ns)
            ref = o.kernelmatrix(o.Kernel(o.MATERN32, 1.3, 0.7), xs, x) @ post.data.alpha
            assert np.max(np.abs(m - ref)) <= cc.M_TOL * max(1.0, np.max(np.abs(ref)))
            post.var(xs)
            assert ctx.get_param("cols_kernel_calls") == calls + 1  # variances use no α: no kmul
            post.data.C.free()
        c = cc.single_case("n129_d17")
        calls = ctx.get_param("cols_kernel_calls")
        post = agp.posterior_columns(_with_ctx(c["fx"], ctx), c["Y"])
        post.mean(c["xs"])
        assert ctx.get_param("cols_kernel_calls") == calls
        post.data.C.free()
        with pytest.raises(ValueError):
            ctx.set_param("cols_kernel_calls", 0)                   # read-only
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", ["n65", "n300_cap", "n300_dense", "persewhite_d2", "n129_d17"])
def test_nothing_depends_on_what_a_recycled_block_held(agp, cid):
    """"alloc_poison" = 1 on a ctx of its own: every block handed out holds NaNs first; fit, means (split and unsplit), variances and gradients stay finite and
    inside the tolerances."""
    c = cc.composite_case(cid) if c_is_composite(cid) else cc.single_case(cid)
    ref = cc.reference(c)
    ctx = agp.Context(0)
    ctx.set_param("alloc_poison", 1)
    try:
        fx = _with_ctx(c["fx"], ctx)
        for _ in range(2):  # the second round takes recycled blocks
            post = agp.posterior_columns(fx, c["Y"])
            _check_fit_and_predict(c, post, ref)
            post.data.C.free()
            lp, g = agp.logpdf_and_grad_columns(fx, c["Y"], wrt_x=True)
            assert all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for v in g.values() if v is not None)
            _check_grad(c, lp, g, ref)
    finally:
        ctx.close()


def test_what_a_handle_with_several_columns_serves_and_refuses(agp):
    c = cc.single_case("n65")
    ref = cc.reference(c)
    post = agp.posterior_columns(c["fx"], c["Y"])
    one = agp.posterior(c["fx"], c["Y"][:, 0])
    h, lib, ns, n = post.data.C.handle, post.data.C.ctx.lib, c["ns"], c["n"]
    m = agp.api._Marshal(np.float64)
    px = m.points(c["xs"])
    # ---- served unchanged: everything that uses no α
    var, cov = np.empty(ns), np.empty((ns, ns), order="F")
    agp._lib.check(lib.gp_posterior_predict(h, C.byref(px), None, 6, None, var.ctypes.data, cov.ctypes.data))
    assert np.max(np.abs(var - ref["var"])) <= cc.V_TOL and np.max(np.abs(cov - ref["cov"])) <= cc.V_TOL
    v1, dv1 = one.var_grad(c["xs"])
    v2, dv2 = post.var_grad(c["xs"])
    assert np.max(np.abs(v2 - v1)) <= cc.V_TOL and np.max(np.abs(dv2 - dv1)) <= cc.G_RTOL * max(1.0, np.max(np.abs(dv1)))
    B = np.random.default_rng(1).standard_normal((n, 3))
    assert cc.rel(post.data.C.solve(B), one.data.C.solve(B)) <= cc.A_TOL
    assert cc.rel(post.data.C.Ut_mul(B), one.data.C.Ut_mul(B)) <= 1e-12
    assert cc.rel(post.data.C.U, one.data.C.U) <= 1e-12
    ld_a, ld_b = C.c_double(), C.c_double()
    agp._lib.check(lib.gp_posterior_logdet(h, C.byref(ld_a)))
    agp._lib.check(lib.gp_posterior_logdet(one.data.C.handle, C.byref(ld_b)))
    assert abs(ld_a.value - ld_b.value) <= 1e-12 * max(1.0, abs(ld_b.value)) and lib.gp_posterior_n(h) == n
    # ---- refused: argument error −1, the reason in gp_last_error(), the output buffers untouched
    sent = 12345.5
    nz = agp._lib.gp_noise(0, 0.1, None)

    def refused(rc, *bufs):
        assert rc == -1, rc
        msg = lib.gp_last_error().decode()
        assert "more than one column" in msg and "gp_posterior_predict_cols" in msg
        for b in bufs:
            assert np.all(b == sent)

    mean, var = np.full(ns, sent), np.full(ns, sent)
    refused(lib.gp_posterior_predict(h, C.byref(px), None, 3, mean.ctypes.data, var.ctypes.data, None), mean, var)
    refused(lib.gp_posterior_predict(h, C.byref(px), None, 1, mean.ctypes.data, None, None), mean)
    dmean = np.full(agp.api._dx_buffer(px, np.float64).shape, sent)
    refused(lib.gp_posterior_predict_grad(h, C.byref(px), None, 3, mean.ctypes.data, var.ctypes.data, dmean.ctypes.data, None), mean, var, dmean)
    out = np.full(2, sent)
    Yh = np.zeros((ns, 2), order="F")
    refused(lib.gp_posterior_logpdf(h, C.byref(px), None, C.byref(nz), Yh.ctypes.data, ns, 2, out.ctypes.data), out)
    draws = np.full((ns, 2), sent, order="F")
    refused(lib.gp_posterior_rand(h, C.byref(px), None, C.byref(nz), Yh.ctypes.data, 2, draws.ctypes.data), draws)
    h2 = C.c_void_p(777)
    alpha2, lp2 = np.full(n + ns, sent), np.full(1, sent)
    delta = np.zeros(n + ns)
    refused(lib.gp_posterior_update(h, C.byref(px), C.byref(nz), delta.ctypes.data, C.byref(h2), alpha2.ctypes.data, lp2.ctypes.data), alpha2, lp2)
    assert h2.value == 777
    for meth in (post.mean_grad, post.mean_and_var_grad):
        with pytest.raises(TypeError):
            meth(c["xs"])
    with pytest.raises(TypeError):
        post(c["xs"], 0.1)
    # the handle still works after the refusals
    assert np.max(np.abs(post.mean(c["xs"]) - ref["mean"])) <= cc.M_TOL
    post.data.C.free()
    one.data.C.free()


def test_argument_errors_and_a_matrix_that_is_not_positive_definite(agp):
    c = cc.single_case("n63")
    ctx = c["fx"].f.context()
    lib = ctx.lib
    a = agp.api._cols_marshal(c["fx"], c["Y"], "t")
    h = C.c_void_p(777)
    alpha = np.full((c["n"], 2), 5.0, order="F")
    lp = np.full(2, 5.0)
    args = lambda ldy, S: (ctx.handle, C.byref(a.kk), C.byref(a.px), C.byref(a.nz), a.m.ptr(a.mean), a.Y.ctypes.data, ldy, S)  # noqa: E731
    assert lib.gp_posterior_fit_cols(*args(a.ldy, 129), C.byref(h), alpha.ctypes.data, lp.ctypes.data) == -8 and "GPMI355_COLS_MAX" in lib.gp_last_error().decode()
    assert lib.gp_posterior_fit_cols(*args(a.ldy, 0), C.byref(h), alpha.ctypes.data, lp.ctypes.data) == -8
    assert lib.gp_posterior_fit_cols(*args(a.ldy - 1, 2), C.byref(h), alpha.ctypes.data, lp.ctypes.data) == -7
    assert lib.gp_logpdf_grad_cols(*args(a.ldy, 129), lp.ctypes.data, None, None, None, None, None) == -8
    assert lib.gp_logpdf_grad_cols(*args(a.ldy, 2), None, None, None, None, None, None) == -9
    assert h.value == 777 and np.all(alpha == 5.0) and np.all(lp == 5.0)
    f = agp.GP(agp.SqExponentialKernel())
    x = np.linspace(0, 1, 300)
    with pytest.raises(agp.PosDefException) as e:
        agp.posterior_columns(f(x, -0.5), np.zeros((300, 3)))     # K − 0.5 I is indefinite: the LAPACK info, no handle
    assert 1 <= e.value.info <= 300
    with pytest.raises(agp.PosDefException):
        agp.logpdf_and_grad_columns(f(x, -0.5), np.zeros((300, 3)))
    nc = C.c_int32()
    assert lib.gp_posterior_ncols(None, C.byref(nc)) == -1 and lib.gp_posterior_predict_cols(None, None, None, 1, None, None, None) == -1
