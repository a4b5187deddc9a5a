"""CPU: the context-free half of mean_and_var_batch (grouping, shared test points, marshalling, order), the declared and exported gp_predict_batch
symbols and their prototypes, and the static side of the entry points' guard."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import test_abi_guard_static as gs
from tests import test_shim_static as ss

ROOT = Path(__file__).resolve().parent.parent
NEW = ("gp_predict_batch", "gp_predict_batch_sum")


def _fx(n, seed, dtype=np.float64, kernel=None, mean=None):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 3, size=n).astype(dtype)
    k = kernel or 1.3 * agp.SqExponentialKernel()
    return (agp.GP(k) if mean is None else agp.GP(mean, k))(x, 0.02), rng.standard_normal(n).astype(dtype)


def test_both_symbols_are_declared_exported_and_bound_with_the_leading_arguments_of_gp_logpdf_batch(agp):
    lib = agp._lib.load()
    assert all(hasattr(lib, s) for s in NEW) and set(NEW) <= set(agp._lib.header_functions()) and set(NEW) <= set(agp._lib.PROTOTYPES)
    assert lib.gp_abi_version() == 4
    protos = ss.header_prototypes()
    for new, old in (("gp_predict_batch", "gp_logpdf_batch"), ("gp_predict_batch_sum", "gp_logpdf_batch_sum")):
        res, args = agp._lib.PROTOTYPES[new]
        res_old, args_old = agp._lib.PROTOTYPES[old]
        assert res is res_old and args[:9] == args_old[:9] and len(args) == 17     # ctx, nb, k, nx, x, noise, mean, ny, y | then the new ones
        assert protos[new][1][:9] == protos[old][1][:9]
        assert protos[new] == ("i32", ["ptr", "i32", "ptr", "i32", "ptr", "ptr", "ptr", "i32", "ptr", "i32", "ptr", "ptr", "i32", "ptr", "ptr", "ptr", "ptr"])
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gpmi355.h").read_text(), flags=re.S)
    names = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(fn + r"\s*\(([^()]*)\)\s*;", hdr).group(1).split(",")]  # noqa: E731
    assert names("gp_predict_batch")[:9] == names("gp_logpdf_batch")[:9]
    assert names("gp_predict_batch")[9:] == ["nxs", "xs", "prior_mean_xs_or_null", "what", "mean_out", "var_out", "logpdf_out_or_null", "info_out"]
    assert names("gp_predict_batch_sum") == names("gp_predict_batch")
    assert "mean_and_var_batch" in dir(agp) and agp.mean_and_var_batch is agp.api.mean_and_var_batch


def test_the_new_entry_points_are_guarded_by_a_body_of_their_own_behind_batch_impl():
    src = gs.strip_comments((gs.CSRC / "batch.hip").read_text())
    defs = gs.definitions(src)
    want = gs.header_handle_functions(gs.HEADER.read_text())
    for name in NEW:
        assert want[name] == "gp_ctx" and gs.guard_problem(name, "gp_ctx", defs) is None
        h, body = defs[name]
        assert "batch_impl(" not in body.replace("predict_batch_impl(", "") and "predict_batch_impl(" + h in body
    assert src.index("int32_t batch_impl(") < src.index("int32_t predict_batch_impl(")
    assert "batch_impl(" not in defs["predict_batch_impl"][1]
    # without the guard of the new body exactly the two new names are reported
    cut = src.index("int32_t predict_batch_impl(")
    mutated = src[:cut] + src[cut:].replace("Guard gd(c);", "", 1)
    defs_m = gs.definitions(mutated)
    assert sorted(n for n in want if n in defs_m and gs.guard_problem(n, want[n], defs_m) and n not in gs.RELEASING and "batch" in n) == sorted(NEW)


def test_marshalling_of_shared_and_ragged_test_points_and_of_the_prior_mean():
    rng = np.random.default_rng(1)
    pairs = [_fx(6, 0), _fx(9, 1, mean=0.4), _fx(4, 2), _fx(5, 3, mean=lambda v: 2.0 * float(v))]
    fxs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    xss = [rng.uniform(0, 3, size=k) for k in (3, 0, 7, 2)]  # ragged, one problem without test points
    (g,) = agp.api._predict_groups(fxs, ys, xss)
    assert (g.nx, g.ny, g.nxs, g.index) == (4, 4, 4, [0, 1, 2, 3])
    pc = agp.api._predict_marshal(g, 3)
    nb, karr, nx, pts, narr, marr, ny, yarr, nxs, xpts, pmarr, what, moarr, voarr, out, info = pc.args
    assert (pc.entry, nb, nx, ny, nxs, what, len(xpts), len(moarr), len(voarr)) == ("gp_predict_batch", 4, 4, 4, 4, 3, 4, 4, 4)
    assert [xpts[b].n for b in range(4)] == [3, 0, 7, 2] and all(xpts[b].d == 1 and xpts[b].layout == 0 for b in range(4))
    assert [a.shape for a in pc.means] == [(3,), (0,), (7,), (2,)] == [a.shape for a in pc.vars]
    assert pmarr[0] is None and pmarr[2] is None and pmarr[1] is not None  # NULL for a zero mean
    pm3 = np.ctypeslib.as_array(C.cast(pmarr[3], C.POINTER(C.c_double)), shape=(2,))
    assert np.array_equal(pm3, 2.0 * xss[3])  # m(x*) evaluated on the host
    assert marr[0] is None and marr[1] is not None
    # zero means throughout: no prior-mean array at all; one side only: the other output array is NULL
    (g0,) = agp.api._predict_groups(fxs[:1] + fxs[2:3], ys[:1] + ys[2:3], xss[:1] + xss[2:3])
    p0 = agp.api._predict_marshal(g0, 1)
    assert p0.args[10] is None and p0.args[13] is None and p0.vars is None and len(p0.args[12]) == 2
    p2 = agp.api._predict_marshal(g0, 2)
    assert p2.args[12] is None and p2.means is None and len(p2.args[13]) == 2


def test_shared_test_points_are_detected_by_identity_and_groups_keep_the_callers_order():
    comp = agp.SqExponentialKernel() + 0.5 * agp.Matern32Kernel()
    specs = [(5, np.float64, None), (7, np.float32, None), (4, np.float64, comp), (9, np.float64, None), (6, np.float64, comp)]
    pairs = [_fx(n, i, dt, k) for i, (n, dt, k) in enumerate(specs)]
    xs = np.linspace(0, 3, 8)
    groups = agp.api._predict_groups([p[0] for p in pairs], [p[1] for p in pairs], xs)  # ONE array for all
    assert [(g.dtype, g.composite, g.index, g.nxs) for g in groups] == [(np.float64, False, [0, 3], 1), (np.float32, False, [1], 1), (np.float64, True, [2, 4], 1)]
    calls = [agp.api._predict_marshal(g, 3) for g in groups]
    assert [c.entry for c in calls] == ["gp_predict_batch", "gp_predict_batch", "gp_predict_batch_sum"]
    assert all(len(c.args[9]) == 1 and c.args[9][0].n == 8 for c in calls) and calls[1].means[0].dtype == np.float32
    # equal values in distinct objects are not shared
    (g2, _, _) = agp.api._predict_groups([p[0] for p in pairs], [p[1] for p in pairs], [xs.copy() for _ in pairs])
    assert g2.nxs == 2 and [v is not g2.xss[0] for v in g2.xss[1:]] == [True]
    rv = agp.RowVecs(np.zeros((3, 1)))
    (g3,) = agp.api._predict_groups([pairs[0][0], pairs[3][0]], [pairs[0][1], pairs[3][1]], rv)
    assert g3.nxs == 1 and g3.xss[0] is rv


def test_argument_checks_of_the_mirror_need_no_device():
    fx, y = _fx(5, 0)
    xs = np.linspace(0, 1, 3)
    assert agp.mean_and_var_batch([], [], []) == []
    pairs, lp = agp.mean_and_var_batch([], [], [], return_logpdf=True)
    assert pairs == [] and lp.shape == (0,)
    with pytest.raises(ValueError, match="sets of test points"):
        agp.api._predict_groups([fx, fx], [y, y], [xs])
    with pytest.raises(ValueError):
        agp.api._predict_groups([fx, fx], [y], [xs, xs])
    with pytest.raises(ValueError, match="what"):
        agp.mean_and_var_batch([fx], [y], [xs], what=0)
    with pytest.raises(ValueError, match="what"):
        agp.mean_and_var_batch([fx], [y], [xs], what=4)
    with pytest.raises(ValueError, match="on_error"):
        agp.mean_and_var_batch([fx], [y], [xs], on_error="ignore")
    with pytest.raises(TypeError):
        agp.api._predict_groups([object()], [y], [xs])
