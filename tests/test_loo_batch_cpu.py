"""CPU: the context-free half of loo_logpdf_batch / loo_mean_and_var_batch / loo_logpdf_and_grad_batch — the reference of every case of
tests/loo_batch_cases.py against brute-force refits and its conditioning, the declared, exported and bound gp_loo_batch / gp_loo_batch_sum /
gp_loo_grad_batch / gp_loo_grad_batch_sum, the two size limits, the static side of the entry points' guard, the marshalling and the mirror's argument
checks."""
import re
from pathlib import Path

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import loo_batch_cases as lb
from tests import loo_cases as lc
from tests import loo_ref as lr
from tests import test_abi_guard_static as gs
from tests import test_shim_static as ss

ROOT = Path(__file__).resolve().parent.parent
VALUE = ("gp_loo_batch", "gp_loo_batch_sum")
GRAD = ("gp_loo_grad_batch", "gp_loo_grad_batch_sum")
NEW = VALUE + GRAD


@pytest.mark.parametrize("cid", lb.SINGLE_IDS + lb.COMPOSITE_IDS + lb.SHARED)
def test_every_case_is_well_conditioned_and_its_reference_matches_brute_force_refits(cid):
    """cond(C) ≤ 1e3 (the bound of tests/test_loo_cpu.py) and the closed form against n refits at 1e-11: the reference alone sits far inside the GPU
    tolerances (L 1e-10 relative, μ 1e-8, v 1e-9)"""
    for c in (lb.shared_batch(cid) if cid in lb.SHARED else [lb.case(cid)]):
        C, m = lc.covariance(c)
        cond = float(np.linalg.cond(C))
        ref = lb.reference(c)
        y = np.asarray(c["y"], dtype=np.float64)
        mu, v, lp = lr.brute_force(C, m, y)
        e_mu, e_v = float(np.max(np.abs(ref["mean"] - mu))), float(np.max(np.abs(ref["var"] - v) / v))
        e_lp, e_L = float(np.max(np.abs(ref["lp"] - lp))), abs(ref["L"] - lp.sum()) / abs(lp.sum())
        print(f"{c['id']}: n = {c['n']}, cond(C) = {cond:.3g}, mean abs {e_mu:.1e}, var rel {e_v:.1e}, lp abs {e_lp:.1e}, L rel {e_L:.1e}")
        assert cond <= 1e3
        assert e_mu <= 1e-11 and e_v <= 1e-11 and e_lp <= 1e-11 and e_L <= 1e-11
        nz = agp.api._Marshal(np.float64).noise(c["s2"], c["n"])
        assert nz.kind == {"scalar": 0, "vector": 1}[c["noise"]]


def test_the_cases_cover_the_shapes_the_kernels_branch_on():
    cases = lb.all_cases()
    assert {c["n"] for c in cases} >= {1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 320}
    singles = lb.ragged_batch()
    assert {c["d"] for c in singles} == {1, 3, 16}
    assert {(c["kind"], c["tr"]) for c in singles} == {(k, t) for k in range(4) for t in ("none", "scale", "ard")}
    assert {c["noise"] for c in singles} == {"scalar", "vector"} and {c["mean"] for c in singles} == {"zero", "const", "custom"}
    assert {c["container"] for c in singles} == {"vector", "colvecs", "rowvecs"}
    nths = [len(agp.api._NormalForm(c["kernel"]).theta()) for c in lb.composite_batch()]
    assert max(nths) > 16 and min(nths) <= 16  # one and two passes of GRAD_NP entries
    assert len(singles) <= 24 and len(lb.composite_batch()) <= 24
    for which, (nx, ny) in zip(lb.SHARED, ((1, 4), (4, 1), (1, 1))):
        b = lb.shared_batch(which)
        (g,) = agp.api._batch_groups([c["fx"] for c in b], [c["y"] for c in b])
        assert (g.nx, g.ny) == (nx, ny), which


def test_the_four_symbols_are_declared_exported_and_bound_with_the_leading_arguments_of_gp_logpdf_batch(agp):
    lib = agp._lib.load()
    assert all(hasattr(lib, s) for s in NEW) and set(NEW) <= set(agp._lib.header_functions()) and set(NEW) <= set(agp._lib.PROTOTYPES)
    assert lib.gp_abi_version() == 4
    protos = ss.header_prototypes()
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gpmi355.h").read_text(), flags=re.S)
    names = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(r"\b" + fn + r"\s*\(([^()]*)\)\s*;", hdr).group(1).split(",")]  # noqa: E731
    for new, old, nargs in (("gp_loo_batch", "gp_logpdf_batch", 14), ("gp_loo_batch_sum", "gp_logpdf_batch_sum", 14),
                            ("gp_loo_grad_batch", "gp_logpdf_batch", 16), ("gp_loo_grad_batch_sum", "gp_logpdf_batch_sum", 15)):
        res, args = agp._lib.PROTOTYPES[new]
        res_old, args_old = agp._lib.PROTOTYPES[old]
        assert res is res_old and args[:9] == args_old[:9] and args[9:11] == args_old[9:11] and len(args) == nargs
        assert protos[new] == ("i32", ["ptr", "i32", "ptr", "i32", "ptr", "ptr", "ptr", "i32", "ptr"] + ["ptr"] * (nargs - 9))
        assert names(new)[:9] == names(old)[:9] and names(new)[9:11] == ["value_out", "info_out"]
    for fn in VALUE:
        assert names(fn)[11:] == ["lp_out_or_null", "mean_out_or_null", "var_out_or_null"]
    assert names("gp_loo_grad_batch")[11:] == names("gp_logpdf_grad_batch_x")[11:]
    assert names("gp_loo_grad_batch_sum")[11:] == names("gp_logpdf_grad_batch_sum_x")[11:]
    assert agp._lib.PROTOTYPES["gp_loo_grad_batch"] == agp._lib.PROTOTYPES["gp_logpdf_grad_batch_x"]
    assert agp._lib.PROTOTYPES["gp_loo_grad_batch_sum"] == agp._lib.PROTOTYPES["gp_logpdf_grad_batch_sum_x"]
    for name in ("loo_logpdf_batch", "loo_mean_and_var_batch", "loo_logpdf_and_grad_batch"):
        assert name in dir(agp) and getattr(agp, name) is getattr(agp.api, name)
    shim = (ROOT / "abstractgps.jl_amd" / "julia" / "HipGPs.jl").read_text()
    for name in NEW:
        assert f"(:{name}, libgpmi355)" in shim, name
    integ = (ROOT / "INTEGRATION.md").read_text()
    assert all(f"`{name}`" in integ for name in NEW)


def test_both_size_limits_are_multiples_of_128_within_the_kernels_and_the_mirror_reads_them(agp):
    txt = (ROOT / "include" / "gpmi355.h").read_text()
    src = (gs.CSRC / "batch.hip").read_text()
    for macro, read, env in (("GPMI355_BATCH_LOO_MAX_N", agp._lib.batch_loo_max_n, "GPMI_BATCH_LOO_MAX_N"),
                             ("GPMI355_BATCH_LOO_GRAD_MAX_N", agp._lib.batch_loo_grad_max_n, "GPMI_BATCH_LOO_GRAD_MAX_N")):
        (v,) = re.findall(r"^#define " + macro + r" (\d+)$", txt, flags=re.M)
        assert int(v) % 128 == 0 and 0 <= int(v) <= 2048 and int(v) == read()
        assert f'env_capped(getenv("{env}"), {macro})' in src
    for name, field in (("batch_loo_kernel_problems", "batch_loo_problems"), ("batch_loo_grad_kernel_problems", "batch_loo_grad_problems")):
        assert f'"{name}"' in txt and f'"{name}"' in (gs.CSRC / "gpmi355.hip").read_text()
        assert field in (gs.CSRC / "engine.hpp").read_text() and f"c->{field}" in src
    assert "profiles/r32/batch_loo_profile.json" in txt


def test_the_new_bodies_have_guards_of_their_own_behind_gradx_batch_impl_and_the_kernels_use_no_atomics():
    src = gs.strip_comments((gs.CSRC / "batch.hip").read_text())
    defs = gs.definitions(src)
    want = gs.header_handle_functions(gs.HEADER.read_text())
    for names, impl, single in ((VALUE, "loo_batch_impl", "gp_loo("), (GRAD, "loo_grad_batch_impl", "gp_loo_grad(")):
        for name in names:
            assert want[name] == "gp_ctx" and gs.guard_problem(name, "gp_ctx", defs) is None
            h, body = defs[name]
            assert impl + "(" + h in body and "grad_batch_impl(" not in body.replace("loo_grad_batch_impl(", "")
        body = defs[impl][1]
        assert body.lstrip("{ \n").startswith("Guard gd(c);")
        assert "grad_batch_impl(" not in body and "gradx_batch_impl(" not in body and " batch_impl(" not in body  # no delegation
        assert body.index("Guard gd(c);") < body.index("for_each_wave(") < body.index("gd.lk.unlock()") < body.index(single)  # the single path locks itself
    assert src.index("int32_t gradx_batch_impl(") < src.index("int32_t loo_batch_impl(") < src.index("int32_t loo_grad_batch_impl(")
    # without the guard of one new body exactly its two entry points are reported
    for names, impl in ((VALUE, "loo_batch_impl"), (GRAD, "loo_grad_batch_impl")):
        cut = src.index(f"int32_t {impl}(")
        defs_m = gs.definitions(src[:cut] + src[cut:].replace("Guard gd(c);", "", 1))
        assert sorted(n for n in want if n in defs_m and gs.guard_problem(n, want[n], defs_m) and n not in gs.RELEASING) == sorted(names)
    assert "atomic" not in src  # no floating-point atomics (none of any kind) anywhere in the unit
    for k in ("batch_loo_kernel", "batch_loo_sum_kernel", "batch_loo_z_kernel", "batch_loo_beta_kernel", "batch_grad_kernel", "batch_inv_kernel"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", src), k
    assert "template <bool SUM, bool LOO>" in src and "batch_grad_kernel<true, false>" in src and "batch_grad_kernel<false, true>" in src


def _fx(n, seed, dtype=np.float64, kernel=None, mean=None, d=1, noise=0.02):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 3, size=n).astype(dtype) if d == 1 else agp.RowVecs(rng.uniform(0, 3, size=(n, d)).astype(dtype))
    k = kernel or 1.3 * agp.SqExponentialKernel()
    return (agp.GP(k) if mean is None else agp.GP(mean, k))(x, noise), rng.standard_normal(n).astype(dtype)


def test_marshalling_of_shared_inputs_ragged_outputs_and_the_callers_order():
    ard = 0.9 * agp.Matern32Kernel() @ agp.ARDTransform([0.5, 0.6, 0.7])
    pairs = [_fx(6, 0), _fx(9, 1, mean=0.4), _fx(4, 2, kernel=ard, d=3, noise=np.full(4, 0.03)), _fx(5, 3, noise=np.full(5, 0.02))]
    fxs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    (g,) = agp.api._batch_groups(fxs, ys)
    call = agp.api._loo_batch_marshal(g)
    nb, karr, nx, pts, narr, marr, ny, yarr, out, info, lparr, muarr, vararr = call.args
    assert (call.entry, nb, nx, ny, len(pts), len(yarr)) == ("gp_loo_batch", 4, 4, 4, 4, 4)
    for bufs, arr in ((call.lp, lparr), (call.mean, muarr), (call.var, vararr)):
        assert [a.shape for a in bufs] == [(6,), (9,), (4,), (5,)] and all(arr[b] == bufs[b].ctypes.data for b in range(4))
    assert len({a.ctypes.data for a in call.lp + call.mean + call.var}) == 12 and marr[0] is None and marr[1] is not None
    # what is not asked for is a NULL array
    only_lp, only_pred = agp.api._loo_batch_marshal(g, True, False), agp.api._loo_batch_marshal(g, False, True)
    assert only_lp.args[-2:] == (None, None) and only_lp.args[-3] is not None and only_lp.mean is None and only_lp.var is None
    assert only_pred.args[-3] is None and only_pred.args[-1] is not None and only_pred.lp is None
    # a shared x and a shared y are sent once
    x = np.linspace(0, 3, 7)
    y = np.sin(x)
    shared = [agp.GP((1.0 + 0.1 * b) * agp.SqExponentialKernel())(x, 0.02) for b in range(5)]
    (g1,) = agp.api._batch_groups(shared, y)
    c1 = agp.api._loo_batch_marshal(g1)
    assert (c1.nb, c1.nx, c1.ny, len(c1.args[3]), len(c1.args[7])) == (5, 1, 1, 1, 1) and len(c1.lp) == 5 and c1.args[5] is None
    gcall = agp.api._loo_grad_batch_marshal(g1)
    assert gcall.entry == "gp_loo_grad_batch" and len(gcall.args) == 15 and gcall.args[-1] is None and gcall.dx is None and len(gcall.dy) == 5
    gx = agp.api._loo_grad_batch_marshal(g1, True)
    assert gx.entry == "gp_loo_grad_batch" and len(gx.args) == 15 and len(gx.dx) == 5 and len({a.ctypes.data for a in gx.dx}) == 5
    assert all(gx.args[-1][b] == gx.dx[b].ctypes.data for b in range(5))
    # dtype and kernel family split the call; the caller's order is kept in the groups' indices
    comp = agp.SqExponentialKernel() @ agp.ScaleTransform(0.5) + 0.5 * agp.Matern32Kernel() * agp.PeriodicKernel(r=[0.9])
    specs = [(5, np.float64, None), (7, np.float32, None), (4, np.float64, comp), (9, np.float64, None), (6, np.float64, comp)]
    pairs = [_fx(n, i, dt, k) for i, (n, dt, k) in enumerate(specs)]
    groups = agp.api._batch_groups([p[0] for p in pairs], [p[1] for p in pairs])
    assert [(gr.dtype, gr.composite, gr.index) for gr in groups] == [(np.float64, False, [0, 3]), (np.float32, False, [1]), (np.float64, True, [2, 4])]
    assert [agp.api._loo_batch_marshal(gr).entry for gr in groups] == ["gp_loo_batch", "gp_loo_batch", "gp_loo_batch_sum"]
    calls = [agp.api._loo_grad_batch_marshal(gr) for gr in groups]
    assert [c.entry for c in calls] == ["gp_loo_grad_batch", "gp_loo_grad_batch", "gp_loo_grad_batch_sum"] and len(calls[2].args) == 14
    assert agp.api._loo_batch_marshal(groups[1]).lp[0].dtype == np.float32 and calls[1].dy[0].dtype == np.float32


def test_argument_checks_of_the_mirror_raise_before_any_library_call(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("the mirror asked for a context before it had checked its arguments")

    monkeypatch.setattr(agp.api, "default_context", no_context)
    fx, y = _fx(5, 0)
    assert agp.loo_logpdf_batch([], []).shape == (0,) and agp.loo_logpdf_batch([], [], pointwise=True)[1] == []
    assert agp.loo_mean_and_var_batch([], []) == ([], [])
    L, grads = agp.loo_logpdf_and_grad_batch([], [], wrt_x=True)
    assert L.shape == (0,) and grads == []
    for fn in (agp.loo_logpdf_batch, agp.loo_mean_and_var_batch, agp.loo_logpdf_and_grad_batch):
        with pytest.raises(ValueError, match="on_error"):
            fn([fx], [y], on_error="ignore")
        with pytest.raises(ValueError, match="DimensionMismatch"):
            fn([fx, fx], [y])
        with pytest.raises(ValueError, match="DimensionMismatch"):
            fn([fx], [np.zeros(4)])
        with pytest.raises(TypeError):
            fn([object()], [y])
    with pytest.raises(TypeError, match="wrt_x"):
        agp.loo_logpdf_and_grad_batch([fx], [y], wrt_x="yes")
