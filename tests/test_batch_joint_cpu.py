"""CPU: the context-free half of joint_batch (grouping, marshalling, order), the declared, exported and bound gp_joint_batch symbols, the static side of the
entry points' guard, the routing constants — and the check that the reference the GPU tests compare against is itself far inside their tolerances."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_joint_cases as jc
from tests import test_abi_guard_static as gs
from tests import test_shim_static as ss

ROOT = Path(__file__).resolve().parent.parent
NEW = ("gp_joint_batch", "gp_joint_batch_sum")
M_TOL, V_TOL, LP_TOL = 1e-8, 1e-9, 1e-10  # tests/test_gpu_batch_joint.py; the held-out logpdf and the samples are held to LP_TOL and M_TOL at least


def _fx(n, seed, dtype=np.float64, kernel=None, mean=None):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 3, size=n).astype(dtype)
    k = kernel or 1.3 * agp.SqExponentialKernel()
    return (agp.GP(k) if mean is None else agp.GP(mean, k))(x, 0.02), rng.standard_normal(n).astype(dtype)


def test_both_symbols_are_declared_exported_and_bound_with_the_leading_arguments_of_gp_predict_batch(agp):
    lib = agp._lib.load()
    assert all(hasattr(lib, s) for s in NEW) and set(NEW) <= set(agp._lib.header_functions()) and set(NEW) <= set(agp._lib.PROTOTYPES)
    assert lib.gp_abi_version() == 4
    protos = ss.header_prototypes()
    for new, old in (("gp_joint_batch", "gp_predict_batch"), ("gp_joint_batch_sum", "gp_predict_batch_sum")):
        res, args = agp._lib.PROTOTYPES[new]
        res_old, args_old = agp._lib.PROTOTYPES[old]
        assert res is res_old and args[:12] == args_old[:12] and len(args) == 24  # ctx … prior_mean_xs_or_null | then the new ones
        assert protos[new][1][:12] == protos[old][1][:12]
        assert protos[new][1][12:] == ["ptr", "i32", "ptr", "ptr", "ptr", "ptr", "i32", "ptr", "ptr", "ptr", "ptr", "ptr"]
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gpmi355.h").read_text(), flags=re.S)
    names = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(fn + r"\s*\(([^()]*)\)\s*;", hdr).group(1).split(",")]  # noqa: E731
    assert names("gp_joint_batch")[:12] == names("gp_predict_batch")[:12]
    assert names("gp_joint_batch")[12:] == ["noise_xs_or_null", "what", "mean_out_or_null", "cov_out_or_null", "ys_or_null", "hlogpdf_out_or_null", "nsamp", "xi_or_null",
                                            "samples_out_or_null", "logpdf_out_or_null", "info_out", "info_joint_out_or_null"]
    assert names("gp_joint_batch_sum") == names("gp_joint_batch")
    for f in ("joint_batch", "mean_and_cov_batch", "logpdf_heldout_batch", "rand_batch"):
        assert f in dir(agp) and getattr(agp, f) is getattr(agp.api, f)
    bound = {c["sym"] for c in ss.shim_ccalls()}
    assert set(NEW) <= bound, "the Julia shim does not bind the new entry points"


def test_the_new_entry_points_are_guarded_by_a_body_of_their_own():
    src = gs.strip_comments((gs.CSRC / "batch.hip").read_text())
    defs = gs.definitions(src)
    want = gs.header_handle_functions(gs.HEADER.read_text())
    for name in NEW:
        assert want[name] == "gp_ctx" and gs.guard_problem(name, "gp_ctx", defs) is None
        h, body = defs[name]
        assert "joint_batch_impl(" + h in body
    assert src.index("int32_t batch_impl(") < src.index("int32_t joint_batch_impl(")
    for other in ("batch_impl(", "predict_batch_impl(", "predict_grad_batch_impl("):
        assert other not in defs["joint_batch_impl"][1]
    # without the guard of the new body exactly the two new names are reported
    cut = src.index("int32_t joint_batch_impl(")
    mutated = src[:cut] + src[cut:].replace("Guard gd(c);", "", 1)
    defs_m = gs.definitions(mutated)
    assert sorted(n for n in want if n in defs_m and gs.guard_problem(n, want[n], defs_m) and n not in gs.RELEASING and "batch" in n) == sorted(NEW)


def test_the_limits_are_multiples_of_128_and_the_counter_is_read_only():
    max_n, max_ns = agp._lib.batch_joint_max()
    assert max_n % 128 == 0 and max_ns % 128 == 0 and 128 <= max_n <= 2048 and 128 <= max_ns <= 2048
    hdr = (ROOT / "include" / "gpmi355.h").read_text()
    main, batch, engine = ((gs.CSRC / f).read_text() for f in ("gpmi355.hip", "batch.hip", "engine.hpp"))
    assert '"batch_joint_kernel_problems"' in hdr and '"batch_joint_kernel_problems"' in main
    assert "batch_joint_problems" in engine and "c->batch_joint_problems += nw" in batch and "c->batch_joint_problems" in main
    defaults = re.search(r"#define GPMI355_PARAM_DEFAULTS(.*?)\nint32_t", hdr, flags=re.S).group(1)
    assert "batch_joint" not in defaults
    assert 'getenv("GPMI_BATCH_JOINT_MAX_N")' in batch and 'getenv("GPMI_BATCH_JOINT_MAX_NS")' in batch
    assert "batch_jcov_kernel" in batch and "batch_jfact_kernel" in batch
    # the Cholesky loop has one definition, and both kernels call it
    assert batch.count("int batch_chol(") == 1 and batch.count("batch_chol(A, ") == 2


def test_marshalling_of_ragged_test_points_noise_forms_heldout_observations_and_draws():
    rng = np.random.default_rng(1)
    pairs = [_fx(6, 0), _fx(9, 1, mean=0.4), _fx(4, 2), _fx(5, 3, mean=lambda v: 2.0 * float(v))]
    fxs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    ns = (3, 0, 7, 2)
    xss = [rng.uniform(0, 3, size=k) for k in ns]  # ragged, one problem without test points
    noises = [0.1, None, rng.uniform(0.1, 0.2, size=7), 0.05 * np.eye(2)]
    ysh = [rng.standard_normal(k) for k in ns]
    xis = [rng.standard_normal((k, 5)) for k in ns]
    (g,) = agp.api._predict_groups(fxs, ys, xss)
    jcall = agp.api._joint_marshal(g, 29, noises, ysh, xis)
    assert jcall.entry == "gp_joint_batch" and len(jcall.args) == 23 == len(agp._lib.PROTOTYPES["gp_joint_batch"][1]) - 1
    (nb, karr, nx, pts, narr, marr, ny, yarr, nxs, xpts, pmarr, nzarr, what, moarr, coarr, ysarr, hl, nsamp, xiarr, soarr, out, info, ij) = jcall.args
    assert (nb, nx, ny, nxs, what, nsamp) == (4, 4, 4, 4, 29, 5)
    assert [xpts[b].n for b in range(4)] == list(ns)
    assert [(nzarr[b].kind, nzarr[b].s) for b in range(4)] == [(0, 0.1), (0, 0.0), (1, 0.0), (3, 0.0)]  # scalar, absent = zero, vector, dense (C order: lower)
    assert [a.shape for a in jcall.means] == [(k,) for k in ns] and [a.shape for a in jcall.covs] == [(k, k) for k in ns]
    assert [a.shape for a in jcall.samples] == [(k, 5) for k in ns] and all(a.flags.f_contiguous for a in jcall.samples + jcall.covs)
    assert jcall.heldout.shape == (4,) and jcall.info_joint.dtype == np.int32 and len(coarr) == len(ysarr) == len(xiarr) == len(soarr) == 4
    x2 = np.ctypeslib.as_array(C.cast(xiarr[2], C.POINTER(C.c_double)), shape=(35,))
    assert np.array_equal(x2, xis[2].ravel(order="F"))  # column-major, leading dimension ns
    pm3 = np.ctypeslib.as_array(C.cast(pmarr[3], C.POINTER(C.c_double)), shape=(2,))
    assert np.array_equal(pm3, 2.0 * xss[3])
    # only what is asked for is marshalled; no Σy* at all: a NULL array
    one = agp.api._joint_marshal(g, 4, None, None, None)
    assert one.args[11] is None and one.args[13] is None and one.args[15] is None and one.args[16] is None and one.args[17] == 0 and one.args[18] is None
    assert one.means is None and one.heldout is None and one.samples is None and len(one.args[14]) == 4
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.api._joint_marshal(g, 8, None, [v[:-1] if len(v) else v for v in ysh][::-1], None)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.api._joint_marshal(g, 16, None, None, xis[:2] + [rng.standard_normal((7, 4))] + xis[3:])


def test_groups_keep_the_callers_order_and_share_what_is_shared():
    comp = agp.SqExponentialKernel() + 0.5 * agp.Matern32Kernel()
    specs = [(5, np.float64, None), (7, np.float32, None), (4, np.float64, comp), (9, np.float64, None), (6, np.float64, comp)]
    pairs = [_fx(n, i, dt, k) for i, (n, dt, k) in enumerate(specs)]
    xs = np.linspace(0, 3, 8)
    groups = agp.api._predict_groups([p[0] for p in pairs], [p[1] for p in pairs], xs)  # ONE array for all
    assert [(g.dtype, g.composite, g.index, g.nxs) for g in groups] == [(np.float64, False, [0, 3], 1), (np.float32, False, [1], 1), (np.float64, True, [2, 4], 1)]
    calls = [agp.api._joint_marshal(g, 5, None, None, None) for g in groups]
    assert [c.entry for c in calls] == ["gp_joint_batch", "gp_joint_batch", "gp_joint_batch_sum"]
    assert all(len(c.args[9]) == 1 and c.args[9][0].n == 8 for c in calls) and calls[1].covs[0].dtype == np.float32


def test_argument_checks_of_the_mirror_need_no_device():
    fx, y = _fx(5, 0)
    xs = np.linspace(0, 1, 3)
    assert agp.joint_batch([], [], []) == []
    quads, lp = agp.joint_batch([], [], [], return_logpdf=True)
    assert quads == [] and lp.shape == (0,)
    for bad in (0, 2, 3, 32, 64):
        with pytest.raises(ValueError, match="what"):
            agp.joint_batch([fx], [y], [xs], what=bad)
    with pytest.raises(ValueError, match="ys_heldout"):
        agp.joint_batch([fx], [y], [xs], what=8)
    with pytest.raises(ValueError, match="xi"):
        agp.joint_batch([fx], [y], [xs], what=16)
    with pytest.raises(ValueError, match="on_error"):
        agp.joint_batch([fx], [y], [xs], on_error="ignore")
    with pytest.raises(ValueError, match="entries of noise"):
        agp.joint_batch([fx, fx], [y, y], [xs, xs], noise=[0.1])


def _host_route(case):
    """SciPy cho_factor / cho_solve on K + Σy, then cholesky(C* + Σy*): independent of the oracle's own factorisation and solves"""
    ofx = case["ofx"]
    k, X, XS, n = ofx.f.kernel, case["X"] if case["container"] != "vector" else case["X"][:, 0], case["oxs"], case["n"]
    Cm = o.kernelmatrix(k, X) + np.diag(np.broadcast_to(np.asarray(case["s2"], dtype=np.float64), (n,)))
    cf = sla.cho_factor(Cm, lower=True)
    delta = case["y"] - o.mean_vector(ofx.f.mean, X)
    alpha = sla.cho_solve(cf, delta)
    lp = -0.5 * (n * np.log(2 * np.pi) + 2.0 * np.sum(np.log(np.diag(cf[0]))) + delta @ alpha)
    Kxs = o.kernelmatrix(k, X, XS)
    mean = o.mean_vector(ofx.f.mean, XS) + Kxs.T @ alpha
    cov = o.kernelmatrix(k, XS) - Kxs.T @ sla.cho_solve(cf, Kxs)
    Ls = np.linalg.cholesky(cov + np.diag(np.broadcast_to(np.asarray(case["nz"], dtype=np.float64), (case["ns"],))))
    z = sla.solve_triangular(Ls, case["ys"] - mean, lower=True)
    hl = -0.5 * (case["ns"] * np.log(2 * np.pi) + 2.0 * np.sum(np.log(np.diag(Ls))) + z @ z)
    return {"lp": lp, "mean": mean, "cov": cov, "hl": hl, "samples": mean[:, None] + Ls @ case["xi"]}


def test_the_reference_is_itself_far_inside_the_tolerances_on_these_very_cases():
    """Within 0.1 × each tolerance of tests/test_gpu_batch_joint.py (the held-out logpdf and the samples at 0.1 × the floors LP_TOL and M_TOL of theirs)."""
    cases, refs = jc.joint_cases(), jc.joint_refs()
    assert {c["ns"] for c in cases} == set(jc.NS_SIZES) and {c["n"] for c in cases} == set(jc.N_SIZES)
    assert sum(1 for b, c in enumerate(cases) if b % 3 == 0 and c["ns"] >= 2 and (c["XS"][0] == c["X"]).all(axis=1).any()) >= 6  # coincident points are there
    worst = [0.0] * 5
    for c, ref in zip(cases, refs):
        h = _host_route(c)
        e = jc.errs((h["mean"], h["cov"], h["hl"], h["samples"]), h["lp"], ref)
        worst = [max(w, v) for w, v in zip(worst, e)]
    print("oracle against the host route, worst: mean %.1e cov %.1e logpdf %.1e held-out logpdf %.1e samples %.1e" % tuple(worst))
    assert worst[0] <= 0.1 * M_TOL and worst[1] <= 0.1 * V_TOL and worst[2] <= 0.1 * LP_TOL and worst[3] <= 0.1 * LP_TOL and worst[4] <= 0.1 * M_TOL, worst
