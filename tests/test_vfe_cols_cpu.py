"""CPU: the context-free half of the sparse column calls (posterior_columns(approx, fx, Y) and its companions): the declared / exported / bound symbols and
their guard, the ABI version, the argument checks of the mirror (raised before any library call), the new kernel's sums free of atomics — and the
self-consistency of the reference in tests/vfe_cols_cases.py: its stacked columns are the single-column oracle calls."""
import numpy as np
import pytest

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import test_abi_guard_static as gs
from tests import test_shim_static as ss
from tests import vfe_cols_cases as vc

NEW = ("gp_vfe_fit_cols", "gp_vfe_update_cols", "gp_vfe_append_cols", "gp_vfe_ncols", "gp_vfe_predict_cols", "gp_vfe_get_cols", "gp_vfe_get_by_cols",
       "gp_vfe_grad_cols")


def test_the_symbols_are_declared_exported_bound_and_the_abi_version_stays(agp):
    lib = agp._lib.load()
    assert all(hasattr(lib, s) for s in NEW) and set(NEW) <= set(agp._lib.header_functions()) and set(NEW) <= set(agp._lib.PROTOTYPES)
    assert lib.gp_abi_version() == 4
    protos = ss.header_prototypes()
    fit, fit1 = protos["gp_vfe_fit_cols"], protos["gp_vfe_fit"]
    assert fit[1] == fit1[1][:8] + ["i64", "i32"] + fit1[1][8:]          # Y, ldy, ncols in place of y
    up, up1 = protos["gp_vfe_update_cols"], protos["gp_vfe_update"]
    assert up[1] == up1[1][:5] + ["i64"] + up1[1][5:]                     # Y2, ldy2
    assert protos["gp_vfe_append_cols"] == protos["gp_vfe_append"]
    assert protos["gp_vfe_predict_cols"] == protos["gp_vfe_predict"]
    assert protos["gp_vfe_get_cols"] == protos["gp_vfe_get"] and protos["gp_vfe_get_by_cols"] == protos["gp_vfe_get_by"]
    assert protos["gp_vfe_grad_cols"] == protos["gp_vfe_grad"]
    for name in ("posterior_columns", "ApproxColumnsPosteriorGP", "elbo_columns", "approx_log_evidence_columns", "elbo_and_grad_columns"):
        assert getattr(agp, name) is getattr(agp.api, name)


def test_every_new_entry_point_starts_with_the_guard():
    src = gs.strip_comments((gs.CSRC / "gpmi355.hip").read_text())
    defs = gs.definitions(src)
    want = gs.header_handle_functions(gs.HEADER.read_text())
    for name in NEW:
        assert want[name] == ("gp_ctx" if name == "gp_vfe_fit_cols" else "gp_vfe")
        assert gs.guard_problem(name, want[name], defs) is None, name


def test_the_new_kernel_sums_without_atomics():
    src = gs.strip_comments((gs.CSRC / "kernels.hpp").read_text())
    a = src.index("void ystats_cols_kernel")
    body = src[a:src.index("\n}\n", a)]
    assert "atomic" not in body and "mfma" in body and "__builtin_nontemporal_load" in body


def _parts(n=12, m=4, dtype=np.float64, kernel=None, sigma2=0.1, mean=None):
    x = np.linspace(0.0, 1.0, n).astype(dtype)
    z = np.linspace(0.1, 0.9, m).astype(dtype)
    k = kernel or 1.3 * agp.SqExponentialKernel()
    f = agp.GP(k) if mean is None else agp.GP(mean, k)
    return f, f(z, 1e-4), f(x, sigma2)


def test_marshalling_of_Y_the_shared_mean_and_dtype_promotion():
    rng = np.random.default_rng(0)
    f, fz, fx = _parts(mean=0.4)
    Y = rng.standard_normal((12, 3))
    a = agp.api._vfe_cols_marshal(agp.VFE(fz), fx, Y, "t")
    assert a.Y.flags.f_contiguous and a.ldy == 12 and a.ncols == 3 and np.array_equal(a.Y, Y) and a.dt is np.float64 and a.approx == 0 and a.jitter == 1e-4
    assert a.mean.shape == (12,) and np.all(a.mean == 0.4) and a.px.n == 12 and a.pz.n == 4
    assert agp.api._vfe_cols_marshal(agp.DTC(fz), fx, Y[:, :1], "t").approx == 1
    f32 = _parts(dtype=np.float32)
    a = agp.api._vfe_cols_marshal(agp.VFE(f32[1]), f32[2], Y.astype(np.float32), "t")
    assert a.dt is np.float32 and a.Y.dtype == np.float32 and a.kk.dtype == 1
    assert agp.api._vfe_cols_marshal(agp.VFE(f32[1]), f32[2], Y, "t").dt is np.float64


def test_argument_checks_of_the_mirror_raise_before_any_library_call(monkeypatch):
    f, fz, fx = _parts()
    Y = np.zeros((12, 3))

    def no_library(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(agp.GP, "context", no_library)
    calls = (lambda a, fx_, Y_: agp.posterior_columns(a, fx_, Y_), agp.elbo_columns, agp.approx_log_evidence_columns, agp.elbo_and_grad_columns)
    for fn in calls:
        with pytest.raises(ValueError):
            fn(agp.VFE(fz), fx, np.zeros((12, 0)))             # S out of range
        with pytest.raises(ValueError):
            fn(agp.VFE(fz), fx, np.zeros((12, 129)))
        with pytest.raises(TypeError):
            fn(agp.VFE(fz), fx, Y[:, 0])                        # Y not 2-D
        with pytest.raises(TypeError):
            fn(agp.VFE(fz), fx, np.zeros((12, 3, 1)))
        with pytest.raises(ValueError):
            fn(agp.VFE(fz), fx, np.zeros((11, 3)))              # row mismatch
        fc = _parts(kernel=agp.SqExponentialKernel() + 0.1 * agp.WhiteKernel())
        with pytest.raises(NotImplementedError):
            fn(agp.VFE(fc[1]), fc[2], Y)                        # composite kernel
        with pytest.raises(NotImplementedError):
            fn(agp.VFE(fz), f(fx.x, 0.1 * np.eye(12)), Y)       # dense Σy
        with pytest.raises(AssertionError):
            fn(agp.VFE(_parts()[1]), fx, Y)                     # vfe.fz.f === fx.f
    with pytest.raises(TypeError):
        agp.elbo_columns(agp.DTC(fz), fx, Y)
    with pytest.raises(TypeError):
        agp.posterior_columns(fx, fx, Y)
    with pytest.raises(TypeError):
        agp.posterior_columns(fx)
    with pytest.raises(TypeError):
        agp.posterior_columns(agp.VFE(fz), fx, Y, Y)
    with pytest.raises(TypeError):
        agp.posterior_columns(fx=fx, Y=Y[:, 0])                 # the two-argument form still takes its arguments by name (a vector: refused by that form)
    # Y2 with a different S, a vector, other rows: refused on a column posterior before the library is asked
    post = agp.ApproxColumnsPosteriorGP(agp.VFE(fz), f, None, np.float64, 4, 3, np.zeros(3))
    fx2 = f(np.linspace(1.0, 2.0, 5), 0.1)
    for bad in (np.zeros((5, 2)), np.zeros((5, 4)), np.zeros(5), np.zeros((4, 3))):
        with pytest.raises((ValueError, TypeError)):
            agp.update_posterior(post, fx2, bad)
    with pytest.raises(NotImplementedError):
        agp.update_posterior(post, f(fx2.x, 0.1 * np.eye(5)), np.zeros((5, 3)))
    for single_only in (post.mean_and_var_grad, post.mean_grad):
        with pytest.raises(TypeError):
            single_only(fx2.x)
    with pytest.raises(TypeError):
        post(fx2.x, 0.1)
    assert post.ncols == 3


@pytest.mark.parametrize("cid", ["m63_s2", "m1_s17", "m128_s128_n1"])
def test_the_reference_stacks_single_column_oracle_calls(cid):
    c = vc.case(cid)
    ref = vc.reference(cid)
    of, z, ofx, _, _, xs, _ = vc.oracle_parts(c)
    Y = np.asarray(c["Y"], dtype=np.float64)[:c["n"]]
    assert ref["alpha"].shape == (c["M"], c["S"]) and ref["mean"].shape == (vc.NS, c["S"]) and ref["b_y"].shape == (c["n"], c["S"])
    for s in {0, c["S"] // 2, c["S"] - 1}:
        p = o.vfe_posterior(of, z, c["jitter"], ofx, Y[:, s])
        assert np.array_equal(ref["alpha"][:, s], p.alpha) and np.array_equal(ref["m_eps"][:, s], p.m_eps) and np.array_equal(ref["mean"][:, s], p.mean(xs))
        assert ref["elbo"][s] == o.elbo(of, z, c["jitter"], ofx, Y[:, s]) and ref["dtc"][s] == o.dtc_log_evidence(of, z, c["jitter"], ofx, Y[:, s])
        assert np.array_equal(ref["var"], p.var(xs)) and np.array_equal(ref["U"], p.U)      # y-free: the same for every column
    if cid == "m63_s2":
        g = vc.grad_reference(cid)
        gs_ = [o.elbo_grad(of, z, c["jitter"], ofx, Y[:, s]) for s in range(c["S"])]
        assert g["variance"] == gs_[0]["variance"] + gs_[1]["variance"] and np.array_equal(g["y"][:, 1], gs_[1]["y"]) and g["y"].shape == (c["n"], 2)


def test_the_cases_cover_the_edges_the_kernels_have():
    cs = vc.CASES
    assert {c[1] for c in cs} == {1, 63, 128, 129, 200} and {c[2] for c in cs} == {1, 2, 15, 16, 17, 128}
    assert {c[3] for c in cs} == {1, 65, 300, 4500} and {c[4] for c in cs} == {1, 3, 17}
    assert {c[5] for c in cs} == {0, 1, 2, 3} and {c[6] for c in cs} == {"none", "scale", "ard"} and {c[7] for c in cs} == {"vector", "colvecs", "rowvecs"}
    assert {c[8] for c in cs} == {"scalar", "vector"} and {c[9] for c in cs} == {"zero", "const", "custom"}
    assert all(1e-6 <= c[10] <= 1e-4 for c in cs)
    (chunked,) = [c for c in cs if c[11]]
    assert chunked[3] == 4500 and chunked[11] == 2048 and chunked[2] == 2   # three chunks, the last ragged; S = 2 where the gradient reference runs
