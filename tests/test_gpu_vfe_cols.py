"""GPU: sparse (VFE / DTC) GPs for a matrix of observations — gp_vfe_fit_cols / _update_cols / _append_cols / _predict_cols / _get_cols / _get_by_cols /
_grad_cols through the mirror's posterior_columns(approx, fx, Y) — against oracle/gp_oracle.py column by column (tests/vfe_cols_cases.py).

Tolerances are those of the single-column sparse tests (tests/test_gpu_random_vfe.py, tests/test_gpu_vfe_grad.py): objectives rel 1e-8, means atol 1e-7,
var / cov atol 1e-8, α rel 1e-8, gradients max(1e-7, 1e-11 / jitter) relative to the largest component of a block (`_close`); fp32 handles: objective rel
1e-4, predictions atol 1e-3, gradients rel 5e-3 against the fp64 call."""
import ctypes as C

import numpy as np
import pytest

from oracle import gp_oracle as o
from tests import vfe_cols_cases as vc

pytestmark = pytest.mark.gpu


def _close(a, b, tol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 1 and b.size == 1:
        a, b = a.reshape(()), b.reshape(())
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1.0)
    print(f"    {what}: err {err:.2e} (tol {tol:.0e})")
    assert err <= tol, (what, err)
    return err


def _ctx_for(agp, c, ordered=False):
    """A private Context with the case's chunk, or None (the default context).  ordered: for the bitwise comparisons of a fit of several chunks — the chunk
    SYRKs into B Bᵀ take the stream-K GEMM by default, whose partial sums arrive in no fixed order (two single-column fits differ in the last bits of
    Λ_ε as well); "gemm_streamk" = 0 with "deterministic" = 1 is the engine's ordered mode."""
    if not c["chunk"]:
        return None
    ctx = agp.Context(0)
    ctx.set_param("vfe_chunk", c["chunk"])
    if ordered:
        ctx.set_param("gemm_streamk", 0)
        ctx.set_param("deterministic", 1)
    return ctx


def _approx(agp, name, fz):
    return (agp.VFE if name == "VFE" else agp.DTC)(fz)


def _check_fit(c, post, ref, key):
    S = c["S"]
    assert post.ncols == S and post.objective.shape == (S,)
    print(f"  {c['id']} {key}: objective rel {np.max(np.abs(post.objective - ref[key]) / np.abs(ref[key])):.2e}")
    np.testing.assert_allclose(post.objective, ref[key], rtol=vc.OBJ_RTOL)
    d = post.data
    a, me = d.alpha, d["m_eps"]
    assert a.shape == (c["M"], S) and me.shape == (c["M"], S)
    for s in range(S):
        assert vc.rel(a[:, s], ref["alpha"][:, s]) <= vc.A_RTOL, (s, vc.rel(a[:, s], ref["alpha"][:, s]))
        assert vc.rel(me[:, s], ref["m_eps"][:, s]) <= vc.A_RTOL, s
    np.testing.assert_allclose(d.U, ref["U"], atol=1e-8)
    np.testing.assert_allclose(d.Lam_U, ref["Lam_U"], rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(d.b_y, ref["b_y"], rtol=1e-12, atol=1e-12)


def _check_predict(post, xs, ref):
    m, v = post.mean_and_var(xs)
    assert m.shape == ref["mean"].shape
    print(f"    mean abs {np.max(np.abs(m - ref['mean'])):.2e} var abs {np.max(np.abs(v - ref['var'])):.2e}")
    np.testing.assert_allclose(m, ref["mean"], atol=vc.M_ATOL)
    np.testing.assert_allclose(v, ref["var"], atol=vc.V_ATOL)
    m2, cv = post.mean_and_cov(xs)
    np.testing.assert_array_equal(m2, m)
    np.testing.assert_allclose(cv, ref["cov"], atol=vc.V_ATOL)
    np.testing.assert_allclose(post.mean(xs), ref["mean"], atol=vc.M_ATOL)
    np.testing.assert_allclose(post.var(xs), ref["var"], atol=vc.V_ATOL)
    np.testing.assert_allclose(post.cov(xs), ref["cov"], atol=vc.V_ATOL)


@pytest.mark.parametrize("approx", ["VFE", "DTC"])
@pytest.mark.parametrize("cid", vc.IDS)
def test_fit_data_and_predictions_against_the_oracle(agp, cid, approx):
    c = vc.case(cid)
    ref = vc.reference(cid)
    ctx = _ctx_for(agp, c)
    try:
        _, fz, fx, _, _, xs = vc.mirror(c, ctx)
        Y = c["Y"][:c["n"]]
        post = agp.posterior_columns(_approx(agp, approx, fz), fx, Y)
        key = "elbo" if approx == "VFE" else "dtc"
        _check_fit(c, post, ref, key)
        _check_predict(post, xs, ref)
        val = agp.elbo_columns(_approx(agp, approx, fz), fx, Y) if approx == "VFE" else agp.approx_log_evidence_columns(_approx(agp, approx, fz), fx, Y)
        if c["chunk"]:  # (a second fit of several chunks: see _ctx_for)
            np.testing.assert_allclose(val, post.objective, rtol=1e-12)
        else:
            np.testing.assert_array_equal(val, post.objective)
    finally:
        if ctx is not None:
            ctx.close()


@pytest.mark.parametrize("cid", vc.UPDATE_IDS)
def test_new_observations_and_new_pseudo_points(agp, cid):
    """update_posterior(cols_post, fx2, Y2) and update_posterior(cols_post, fz2) against the oracle's vfe_update_obs / vfe_update_z column by column (one case
    after a fit of three chunks)."""
    c = vc.case(cid)
    ref = vc.reference(cid)
    of, z, ofx, ofx2, z2, xs_o, ofx_all = vc.oracle_parts(c)
    n, S = c["n"], c["S"]
    Y = np.asarray(c["Y"], dtype=np.float64)
    ctx = _ctx_for(agp, c)
    try:
        _, fz, fx, fx2, fz2, xs = vc.mirror(c, ctx)
        post = agp.posterior_columns(agp.VFE(fz), fx, Y[:n])
        p2 = agp.update_posterior(post, fx2, Y[n:])
        assert p2.ncols == S and int(p2._state.ctx.lib.gp_vfe_n(p2._state.handle)) == n + vc.N2
        o2 = [o.vfe_update_obs(ref["posts"][s], ofx2, Y[n:, s]) for s in range(S)]
        np.testing.assert_allclose(p2.objective, [o.elbo(of, z, c["jitter"], ofx_all, Y[:, s]) for s in range(S)], rtol=vc.OBJ_RTOL)
        for s in range(S):
            assert vc.rel(p2.data.alpha[:, s], o2[s].alpha) <= vc.A_RTOL, s
        m, v = p2.mean_and_var(xs)
        np.testing.assert_allclose(m, np.stack([p.mean(xs_o) for p in o2], axis=1), atol=vc.M_ATOL)
        np.testing.assert_allclose(v, o2[0].var(xs_o), atol=vc.V_ATOL)
        np.testing.assert_allclose(p2.data.b_y, np.stack([p.b_y for p in o2], axis=1), rtol=1e-12, atol=1e-12)
        # new pseudo-points on the updated posterior
        p3 = agp.update_posterior(p2, fz2)
        o3 = [o.vfe_update_z(p, z2) for p in o2]
        assert p3.data.alpha.shape == (c["M"] + vc.M2, S)
        jit = np.concatenate([np.full(c["M"], c["jitter"]), np.zeros(vc.M2)])  # the reference gives the appended block no jitter (:138)
        zall = np.concatenate([o.as_points(z), o.as_points(z2)], axis=0)
        zall = zall[:, 0] if c["container"] == "vector" else zall
        np.testing.assert_allclose(p3.objective, [o.elbo(of, zall, jit, ofx_all, Y[:, s]) for s in range(S)], rtol=vc.OBJ_RTOL)
        m, v = p3.mean_and_var(xs)
        np.testing.assert_allclose(m, np.stack([p.mean(xs_o) for p in o3], axis=1), atol=vc.M_ATOL)
        np.testing.assert_allclose(v, o3[0].var(xs_o), atol=vc.V_ATOL)
        np.testing.assert_allclose(p3.cov(xs), o3[0].cov(xs_o), atol=vc.V_ATOL)
    finally:
        if ctx is not None:
            ctx.close()


def _compare_grad(c, g, ref, tol):
    _close(g["variance"], ref["variance"], tol, "variance")
    if ref["scale"] is None:
        assert g["scale"] is None
    else:
        _close(g["scale"], ref["scale"], tol, "scale")
    rn = np.asarray(ref["noise"])
    if rn.ndim == 1:
        _close(g["noise_diag"], rn, tol, "noise_diag")
    _close(g["noise"], np.sum(rn), tol, "noise sum")
    _close(g["y"], ref["y"], tol, "dY")
    _close(g["mean"], ref["mean"], tol, "mean")
    gz = g["z"].T if c["container"] == "colvecs" else g["z"]
    _close(np.reshape(gz, (-1, c["d"])), np.reshape(ref["z"], (-1, c["d"])), tol, "z")
    _close(np.reshape(g["x"], (-1, c["d"])), np.reshape(ref["x"], (-1, c["d"])), tol, "x")


# (the oracle's gradient costs 2.6 s per column at n = 4 500: the chunked case runs with VFE only)
@pytest.mark.parametrize("cid,approx", [(i, a) for i in vc.GRAD_IDS for a in ("VFE", "DTC") if not (a == "DTC" and i == "m129_s2_n4500")])
def test_gradient_of_the_sum_against_the_oracle(agp, cid, approx):
    c = vc.case(cid)
    tol = max(1e-7, 1e-11 / c["jitter"])
    ctx = _ctx_for(agp, c)
    try:
        _, fz, fx, _, _, _ = vc.mirror(c, ctx)
        val, g = agp.elbo_and_grad_columns(_approx(agp, approx, fz), fx, c["Y"][:c["n"]], wrt_x=True)
        np.testing.assert_allclose(val, vc.reference(cid)["elbo" if approx == "VFE" else "dtc"], rtol=vc.OBJ_RTOL)
        if c["container"] == "colvecs":
            g["x"] = g["x"].T
        print(f"  {cid} {approx}")
        _compare_grad(c, g, vc.grad_reference(cid, approx == "VFE"), tol)
    finally:
        if ctx is not None:
            ctx.close()


@pytest.mark.parametrize("cid", ["m63_s2", "m129_s16", "m200_s17"])
def test_gradient_after_an_update_and_after_an_append(agp, cid):
    """The gradient of the sum on the handle after new observations, and after appended pseudo-points on top of them.  The appended block of K_zz carries NO
    jitter (src/sparse_approximations.jl:138), so the bound 1e-11 / jitter — the growth of the entries of K_zz⁻¹ that the jitter caps — has no finite value for
    it: the append stage is held to max(that bound, 1e-6), the tolerance the single-column test of this stage uses
    (tests/test_gpu_vfe_grad.py::test_objective_grad_after_updates).  Where K_zz stays well conditioned on its own (the Matérn kinds in D = 3) the stage measures
    ≈ 1e-12; on m63_s2 (SqExponential, D = 1 as a plain vector, 63 + 10 pseudo-points in [−2, 2]) the variance component measured 8.2e-7 after the append
    against 2.4e-10 before it."""
    c = vc.case(cid)
    of, z, ofx, ofx2, z2, _, ofx_all = vc.oracle_parts(c)
    n, S = c["n"], c["S"]
    Y = np.asarray(c["Y"], dtype=np.float64)
    tol = max(1e-7, 1e-11 / c["jitter"])
    _, fz, fx, fx2, fz2, _ = vc.mirror(c)
    post = agp.update_posterior(agp.posterior_columns(agp.VFE(fz), fx, Y[:n]), fx2, Y[n:])
    print(f"  {cid} after update")
    _compare_grad(c, post.objective_grad(wrt_x=True), vc.sum_grads([o.elbo_grad(of, z, c["jitter"], ofx_all, Y[:, s]) for s in range(S)]), tol)
    post2 = agp.update_posterior(post, fz2)
    jit = np.concatenate([np.full(c["M"], c["jitter"]), np.zeros(vc.M2)])
    zall = np.concatenate([o.as_points(z), o.as_points(z2)], axis=0)
    zall = zall[:, 0] if c["container"] == "vector" else zall
    print(f"  {cid} after append")
    _compare_grad(c, post2.objective_grad(wrt_x=True), vc.sum_grads([o.elbo_grad(of, zall, jit, ofx_all, Y[:, s]) for s in range(S)]), max(tol, 1e-6))


@pytest.mark.parametrize("cid,S", vc.F32)
def test_fp32_handles(agp, cid, S):
    c32, c64 = vc.case(cid, np.float32, S), vc.case(cid, np.float64, S)
    ref = vc.reference(cid, np.float32, S)  # the oracle in fp64 on the fp32-rounded data
    _, fz, fx, _, _, xs = vc.mirror(c32)
    Y32 = c32["Y"][:c32["n"]]
    post = agp.posterior_columns(agp.VFE(fz), fx, Y32)
    assert post.objective.dtype == np.float32 and post.ncols == S
    np.testing.assert_allclose(post.objective, ref["elbo"], rtol=vc.OBJ_RTOL32)
    m, v = post.mean_and_var(xs)
    assert m.dtype == np.float32 and m.shape == (vc.NS, S)
    np.testing.assert_allclose(m, ref["mean"], atol=vc.P_ATOL32)
    np.testing.assert_allclose(v, ref["var"], atol=vc.P_ATOL32)
    np.testing.assert_allclose(post.cov(xs), ref["cov"], atol=vc.P_ATOL32)
    g32 = post.objective_grad(wrt_x=True)
    assert "z" not in g32  # ∂/∂z stays refused on fp32 handles
    dz = np.empty((c32["M"], c32["d"]))
    lib, h = post._state.ctx.lib, post._state.handle
    assert lib.gp_vfe_grad_cols(h, None, None, None, None, None, dz.ctypes.data, 2, None, 1) == -7
    # against the fp64 call on the same (fp32-rounded) data
    c = c32
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    k = c["kernel"]
    f = agp.GP(k) if c["mean_fn"] is None else agp.GP(c["mean_fn"], k)
    s2 = float(c["s2_1"]) if np.ndim(c["s2_1"]) == 0 else f64(c["s2_1"])
    fx64 = f(vc.container(f64(c["X"][:c["n"]]), c["container"]), s2)
    fz64 = f(vc.container(f64(c["Z"][:c["M"]]), c["container"]), c["jitter"])
    g64 = agp.posterior_columns(agp.VFE(fz64), fx64, f64(Y32)).objective_grad(wrt_x=True)
    for key in ("variance", "scale", "noise", "noise_diag", "y", "x"):
        if g64[key] is not None:
            r = vc.rel(g32[key], f64(g64[key]))
            print(f"  fp32 {cid} S={S} {key}: rel {r:.2e}")
            assert r <= vc.G_RTOL32, (key, r)
    assert c64["S"] == S


def test_one_column_is_the_single_column_call_bitwise(agp):
    c = vc.case("m129_s16")
    _, fz, fx, fx2, fz2, xs = vc.mirror(c)
    n = c["n"]
    y, y2 = c["Y"][:n, 3], c["Y"][n:, 3]
    one = agp.posterior(agp.VFE(fz), fx, y)
    col = agp.posterior_columns(agp.VFE(fz), fx, y[:, None])
    assert col.ncols == 1

    def same(pc, p1):
        np.testing.assert_array_equal(pc.objective, [p1.objective])
        for k in ("alpha", "m_eps", "b_y"):
            np.testing.assert_array_equal(pc.data[k][:, 0], p1.data[k])
        np.testing.assert_array_equal(pc.mean(xs)[:, 0], p1.mean(xs))
        np.testing.assert_array_equal(pc.var(xs), p1.var(xs))
        np.testing.assert_array_equal(pc.cov(xs), p1.cov(xs))
        # the gradient: the same launches, but vgrad's sums go through floating-point atomics, so no two calls need agree in the last bits (this comparison
        # was bitwise in one run and off by 1.4e-14 on ∂/∂z in the next) — held to 1e-12 of the largest component instead
        gc, g1 = pc.objective_grad(wrt_x=True), p1.objective_grad(wrt_x=True)
        for k in ("variance", "scale", "noise", "noise_diag", "z", "x"):
            if g1[k] is not None:
                _close(gc[k], g1[k], 1e-12, k)
        _close(gc["y"][:, 0], g1["y"], 1e-12, "y")

    same(col, one)
    same(agp.update_posterior(col, fx2, y2[:, None]), agp.update_posterior(one, fx2, y2))
    same(agp.update_posterior(col, fz2), agp.update_posterior(one, fz2))


@pytest.mark.parametrize("cid", ["m129_s16", "m200_s17", "m129_s2_n4500"])
def test_y_free_outputs_are_those_of_a_single_column_handle_bitwise(agp, cid):
    c = vc.case(cid)
    ctx = _ctx_for(agp, c, ordered=True)
    try:
        _, fz, fx, _, _, xs = vc.mirror(c, ctx)
        Y = c["Y"][:c["n"]]
        post = agp.posterior_columns(agp.VFE(fz), fx, Y)
        s = c["S"] - 1
        one = agp.posterior(agp.VFE(fz), fx, Y[:, s])
        np.testing.assert_array_equal(post.var(xs), one.var(xs))
        np.testing.assert_array_equal(post.cov(xs), one.cov(xs))
        np.testing.assert_array_equal(post.data.U, one.data.U)
        np.testing.assert_array_equal(post.data.Lam_U, one.data.Lam_U)
        np.testing.assert_array_equal(post.var_grad(xs)[1], one.var_grad(xs)[1])
        # each column agrees with its single-column fit within the tolerances (not bitwise: the summation order over the chunk differs)
        np.testing.assert_allclose(post.objective[s], one.objective, rtol=vc.OBJ_RTOL)
        assert vc.rel(post.data.alpha[:, s], one.data.alpha) <= vc.A_RTOL
        np.testing.assert_allclose(post.mean(xs)[:, s], one.mean(xs), atol=vc.M_ATOL)
    finally:
        if ctx is not None:
            ctx.close()


@pytest.mark.parametrize("cid", ["m200_s17", "m63_s128", "m129_s2_n4500"])
def test_a_column_does_not_depend_on_the_other_columns_and_repeats_bitwise(agp, cid):
    c = vc.case(cid)
    ctx = _ctx_for(agp, c, ordered=True)
    try:
        _, fz, fx, _, _, xs = vc.mirror(c, ctx)
        Y = c["Y"][:c["n"]].copy()
        a = agp.posterior_columns(agp.VFE(fz), fx, Y)
        b = agp.posterior_columns(agp.VFE(fz), fx, Y)
        np.testing.assert_array_equal(a.objective, b.objective)
        np.testing.assert_array_equal(a.data.alpha, b.data.alpha)
        np.testing.assert_array_equal(a.mean(xs), b.mean(xs))
        s = c["S"] // 2
        Yo = 3.0 * np.random.default_rng(5).standard_normal(Y.shape) + 1e3
        Yo[:, s] = Y[:, s]
        d = agp.posterior_columns(agp.VFE(fz), fx, Yo)
        np.testing.assert_array_equal(d.objective[s], a.objective[s])
        np.testing.assert_array_equal(d.data.alpha[:, s], a.data.alpha[:, s])
        np.testing.assert_array_equal(d.mean(xs)[:, s], a.mean(xs)[:, s])
        assert not np.array_equal(d.data.alpha[:, s - 1], a.data.alpha[:, s - 1])
    finally:
        if ctx is not None:
            ctx.close()


@pytest.mark.parametrize("cid", ["m129_s16", "m129_s2_n4500"])
def test_nothing_depends_on_what_a_recycled_block_held(agp, cid):
    """"alloc_poison" = 1 on a ctx of its own: every block handed out holds NaNs first; fit, predictions, updates and gradients stay finite and inside the
    tolerances."""
    c = vc.case(cid)
    ref = vc.reference(cid)
    ctx = agp.Context(0)
    ctx.set_param("alloc_poison", 1)
    if c["chunk"]:
        ctx.set_param("vfe_chunk", c["chunk"])
    try:
        _, fz, fx, fx2, fz2, xs = vc.mirror(c, ctx)
        n = c["n"]
        tol = max(1e-7, 1e-11 / c["jitter"])
        for _ in range(2):  # the second round takes recycled blocks
            post = agp.posterior_columns(agp.VFE(fz), fx, c["Y"][:n])
            _check_fit(c, post, ref, "elbo")
            _check_predict(post, xs, ref)
            g = post.objective_grad(wrt_x=True)
            assert all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for v in g.values() if v is not None)
            _compare_grad(c, g, vc.grad_reference(cid, True), tol)
            p3 = agp.update_posterior(agp.update_posterior(post, fx2, c["Y"][n:]), fz2)
            assert np.all(np.isfinite(p3.objective)) and np.all(np.isfinite(p3.mean(xs))) and np.all(np.isfinite(p3.data.alpha))
            del post, p3
    finally:
        ctx.close()


def test_what_a_handle_with_several_columns_serves_and_refuses(agp):
    c = vc.case("m129_s16")
    ref = vc.reference("m129_s16")
    _, fz, fx, fx2, fz2, xs = vc.mirror(c)
    n, M, S, ns = c["n"], c["M"], c["S"], vc.NS
    post = agp.posterior_columns(agp.VFE(fz), fx, c["Y"][:n])
    one = agp.posterior(agp.VFE(fz), fx, c["Y"][:n, 0])
    lib, h = post._state.ctx.lib, post._state.handle
    m = agp.api._Marshal(np.float64)
    px, px2, pz2 = m.points(xs), m.points(fx2.x), m.points(fz2.x)
    nz2 = m.noise(fx2.sigma2, px2.n)
    nc = C.c_int32(-1)
    agp._lib.check(lib.gp_vfe_ncols(h, C.byref(nc)))
    assert nc.value == S
    agp._lib.check(lib.gp_vfe_ncols(one._state.handle, C.byref(nc)))
    assert nc.value == 1
    # ---- served unchanged: everything that uses no α
    var, cov = np.empty(ns), np.empty((ns, ns), order="F")
    agp._lib.check(lib.gp_vfe_predict(h, C.byref(px), None, 6, None, var.ctypes.data, cov.ctypes.data))
    np.testing.assert_allclose(var, ref["var"], atol=vc.V_ATOL)
    np.testing.assert_allclose(cov, ref["cov"], atol=vc.V_ATOL)
    v2, dv = post.var_grad(xs)
    np.testing.assert_allclose(v2, var, atol=vc.V_ATOL)
    np.testing.assert_array_equal(v2, one.var_grad(xs)[0])
    np.testing.assert_array_equal(dv, one.var_grad(xs)[1])
    assert lib.gp_vfe_m(h) == M and lib.gp_vfe_n(h) == n
    np.testing.assert_allclose(post.data.U, ref["U"], atol=1e-8)
    # a one-column handle serves the column calls
    mc = np.empty((ns, 1), order="F")
    agp._lib.check(lib.gp_vfe_predict_cols(one._state.handle, C.byref(px), None, 1, mc.ctypes.data, None, None))
    np.testing.assert_array_equal(mc[:, 0], one.mean(xs))
    # ---- refused: −1, sentinel-filled outputs untouched
    SENT = -777.25
    buf = lambda *shape: np.full(shape, SENT)
    mean, dmean, a1, by, lp, dy = buf(ns), buf(ns, c["d"]), buf(M), buf(n), buf(4), buf(n)
    hout = C.c_void_p(12345)
    obj = buf(S)
    ys = np.zeros((ns, 1), order="F")
    nzs = m.noise(0.1, ns)
    dvar = C.c_double(SENT)
    calls = [
        lib.gp_vfe_predict(h, C.byref(px), None, 1, mean.ctypes.data, None, None),
        lib.gp_vfe_predict(h, C.byref(px), None, 3, mean.ctypes.data, var.ctypes.data, None),
        lib.gp_vfe_predict_grad(h, C.byref(px), None, 1, mean.ctypes.data, None, dmean.ctypes.data, None),
        lib.gp_vfe_get(h, a1.ctypes.data, a1.ctypes.data),
        lib.gp_vfe_get_by(h, by.ctypes.data),
        lib.gp_vfe_logpdf(h, C.byref(px), None, C.byref(nzs), ys.ctypes.data, ns, 1, lp.ctypes.data),
        lib.gp_vfe_rand(h, C.byref(px), None, C.byref(nzs), ys.ctypes.data, 1, mean.ctypes.data),
        lib.gp_vfe_update(h, C.byref(px2), C.byref(nz2), None, np.zeros(px2.n).ctypes.data, C.byref(hout), obj.ctypes.data),
        lib.gp_vfe_append(h, C.byref(pz2), C.byref(hout), obj.ctypes.data),
        lib.gp_vfe_grad(h, C.byref(dvar), None, None, None, dy.ctypes.data, None, 0, None, 0),
    ]
    assert calls == [-1] * len(calls), calls
    assert "more than one column" in lib.gp_last_error().decode()
    for b in (mean, dmean, a1, by, lp, dy, obj):
        assert np.all(b == SENT)
    assert hout.value == 12345 and dvar.value == SENT
    with pytest.raises(TypeError):
        post.mean_and_var_grad(xs)
    with pytest.raises(TypeError):
        post.mean_grad(xs)
    with pytest.raises(TypeError):
        post(xs, 0.1)
    # ---- the handle works afterwards
    np.testing.assert_allclose(post.mean(xs), ref["mean"], atol=vc.M_ATOL)


def test_argument_errors(agp):
    c = vc.case("m63_s2")
    _, fz, fx, fx2, _, _ = vc.mirror(c)
    n = c["n"]
    Y = np.asfortranarray(c["Y"][:n])
    ctx = fx.f.context()
    lib = ctx.lib
    m = agp.api._Marshal(np.float64)
    px, pz = m.points(fx.x), m.points(fz.x)
    kk = m.kernel(fx.f.kernel, px.d)
    nz = m.noise(fx.sigma2, px.n)
    mean = m.arr(np.full(n, 0.4))
    obj = np.zeros(129)

    def fit(ldy, ncols, approx=0, jitter=1e-4, pzz=pz):
        h = C.c_void_p()
        rc = lib.gp_vfe_fit_cols(ctx.handle, C.byref(kk), C.byref(px), C.byref(pzz), C.byref(nz), jitter, mean.ctypes.data, Y.ctypes.data, ldy, ncols, approx,
                                 C.byref(h), obj.ctypes.data)
        return rc, h.value

    assert fit(n, 0) == (-10, None) and fit(n, 129) == (-10, None)
    assert fit(n - 1, 2) == (-9, None)
    assert fit(n, 2, approx=2) == (-11, None)
    rc, h = fit(n, 2)
    assert rc == 0 and h
    lib.gp_vfe_free(C.c_void_p(h))
    # a K_zz that is not positive definite: ten copies of one pseudo-point without jitter -> the LAPACK info, no handle
    Zd = np.full(10, c["Z"][0, 0])
    rc, h = fit(n, 2, jitter=0.0, pzz=m.points(Zd))
    assert 1 <= rc <= 10 and h is None, rc
    with pytest.raises(agp.PosDefException):
        agp.posterior_columns(agp.VFE(fx.f(Zd, 0.0)), fx, Y)
    # a Y2 of another width
    post = agp.posterior_columns(agp.VFE(fz), fx, Y)
    with pytest.raises(ValueError):
        agp.update_posterior(post, fx2, c["Y"][n:, :1])
    with pytest.raises(ValueError):
        agp.update_posterior(post, fx2, np.zeros((vc.N2, 3)))
    nc = C.c_int32()
    assert lib.gp_vfe_ncols(None, C.byref(nc)) == -1 and lib.gp_vfe_predict_cols(None, None, None, 1, None, None, None) == -1
    assert lib.gp_vfe_ncols(post._state.handle, None) == -2
