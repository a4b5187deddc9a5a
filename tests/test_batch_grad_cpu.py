"""CPU: the context-free half of logpdf_and_grad_batch (marshalling, shared inputs, ragged outputs, order), the declared and exported
gp_logpdf_grad_batch symbols and their prototypes, GPMI355_BATCH_GRAD_MAX_N, the static side of the entry points' guard — and the oracle's own gradient
against one built from SciPy's Cholesky on the cases the GPU tests use (the reference is itself far inside the tolerances it is used with)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import batch_cases as bc
from tests import batch_grad_cases as gc
from tests import test_abi_guard_static as gs
from tests import test_shim_static as ss

ROOT = Path(__file__).resolve().parent.parent
NEW = ("gp_logpdf_grad_batch", "gp_logpdf_grad_batch_sum")


def _fx(n, seed, dtype=np.float64, kernel=None, mean=None, d=1, noise=0.02):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 3, size=n).astype(dtype) if d == 1 else agp.RowVecs(rng.uniform(0, 3, size=(n, d)).astype(dtype))
    k = kernel or 1.3 * agp.SqExponentialKernel()
    return (agp.GP(k) if mean is None else agp.GP(mean, k))(x, noise), rng.standard_normal(n).astype(dtype)


def test_both_symbols_are_declared_exported_and_bound_with_the_leading_arguments_of_gp_logpdf_batch(agp):
    lib = agp._lib.load()
    assert all(hasattr(lib, s) for s in NEW) and set(NEW) <= set(agp._lib.header_functions()) and set(NEW) <= set(agp._lib.PROTOTYPES)
    assert lib.gp_abi_version() == 4
    protos = ss.header_prototypes()
    for new, old, nargs in (("gp_logpdf_grad_batch", "gp_logpdf_batch", 15), ("gp_logpdf_grad_batch_sum", "gp_logpdf_batch_sum", 14)):
        res, args = agp._lib.PROTOTYPES[new]
        res_old, args_old = agp._lib.PROTOTYPES[old]
        assert res is res_old and args[:9] == args_old[:9] and len(args) == nargs  # ctx, nb, k, nx, x, noise, mean, ny, y | logpdf, info, the gradients
        assert args[9:11] == args_old[9:11]
        assert protos[new][1][:9] == protos[old][1][:9]
        assert protos[new] == ("i32", ["ptr", "i32", "ptr", "i32", "ptr", "ptr", "ptr", "i32", "ptr"] + ["ptr"] * (nargs - 9))
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gpmi355.h").read_text(), flags=re.S)
    names = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(fn + r"\s*\(([^()]*)\)\s*;", hdr).group(1).split(",")]  # noqa: E731
    assert names("gp_logpdf_grad_batch")[:11] == names("gp_logpdf_batch")[:11]
    assert names("gp_logpdf_grad_batch")[11:] == ["dvariance_out_or_null", "dscale_out_or_null", "dnoise_out_or_null", "dy_out_or_null"]
    assert names("gp_logpdf_grad_batch_sum")[:11] == names("gp_logpdf_batch_sum")[:11]
    assert names("gp_logpdf_grad_batch_sum")[11:] == ["dtheta_out_or_null", "dnoise_out_or_null", "dy_out_or_null"]
    assert "logpdf_and_grad_batch" in dir(agp) and agp.logpdf_and_grad_batch is agp.api.logpdf_and_grad_batch


def test_the_size_limit_is_a_multiple_of_128_within_the_kernels_and_the_mirror_reads_it(agp):
    txt = (ROOT / "include" / "gpmi355.h").read_text()
    (v,) = re.findall(r"^#define GPMI355_BATCH_GRAD_MAX_N (\d+)$", txt, flags=re.M)
    assert int(v) % 128 == 0 and 0 < int(v) <= 2048 and int(v) == agp._lib.batch_grad_max_n()
    src = (gs.CSRC / "batch.hip").read_text()
    assert 'getenv("GPMI_BATCH_GRAD_MAX_N")' in src and "GPMI355_BATCH_GRAD_MAX_N" in src
    assert '"batch_grad_kernel_problems"' in txt and '"batch_grad_kernel_problems"' in (gs.CSRC / "gpmi355.hip").read_text()


def test_the_new_entry_points_are_guarded_by_a_body_of_their_own_behind_predict_batch_impl():
    src = gs.strip_comments((gs.CSRC / "batch.hip").read_text())
    defs = gs.definitions(src)
    want = gs.header_handle_functions(gs.HEADER.read_text())
    for name in NEW:
        assert want[name] == "gp_ctx" and gs.guard_problem(name, "gp_ctx", defs) is None
        h, body = defs[name]
        assert "grad_batch_impl(" + h in body and "predict_batch_impl(" not in body and " batch_impl(" not in body
    assert src.index("int32_t batch_impl(") < src.index("int32_t predict_batch_impl(") < src.index("int32_t grad_batch_impl(")
    body = defs["grad_batch_impl"][1]
    assert "Guard gd(c);" in body and "predict_batch_impl(" not in body and " batch_impl(" not in body
    assert body.index("gd.lk.unlock()") < body.index("gp_logpdf_grad(")  # the single path takes the lock itself
    # without the guard of the new body exactly the two new names are reported
    cut = src.index("int32_t grad_batch_impl(")
    mutated = src[:cut] + src[cut:].replace("Guard gd(c);", "", 1)
    defs_m = gs.definitions(mutated)
    assert sorted(n for n in want if n in defs_m and gs.guard_problem(n, want[n], defs_m) and n not in gs.RELEASING and "batch" in n) == sorted(NEW)


def test_the_gradient_kernels_use_no_atomics_and_leave_the_other_kernels_alone():
    src = gs.strip_comments((gs.CSRC / "batch.hip").read_text())
    assert "atomic" not in src  # no floating-point atomics (none of any kind) anywhere in the unit
    for k in ("batch_inv_kernel", "batch_grad_kernel", "batch_gsum_kernel", "batch_logpdf_kernel", "batch_predict_kernel"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", src), k
    kf = gs.strip_comments((gs.CSRC / "kfun.hpp").read_text())
    kh = gs.strip_comments((gs.CSRC / "kernels.hpp").read_text())
    for fn in ("void ksum_grad(", "void ksum_factor_grad(", "void kappa_and_dr2("):  # ONE copy of the derivative code, shared by both translation units
        assert kf.count(fn) == 1 and kh.count(fn) == 0, fn


def test_marshalling_of_shared_inputs_ragged_outputs_and_scales():
    ard = 0.9 * agp.Matern32Kernel() @ agp.ARDTransform([0.5, 0.6, 0.7])
    sc = 1.1 * agp.Matern52Kernel() @ agp.ScaleTransform(0.7)
    pairs = [_fx(6, 0), _fx(9, 1, mean=0.4, kernel=sc), _fx(4, 2, kernel=ard, d=3, noise=np.full(4, 0.03)), _fx(5, 3, noise=np.full(5, 0.02))]
    fxs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    (g,) = agp.api._batch_groups(fxs, ys)
    gcall = agp.api._grad_batch_marshal(g)
    nb, karr, nx, pts, narr, marr, ny, yarr, out, info, dvar, dsarr, dnarr, dyarr = gcall.args
    assert (gcall.entry, nb, nx, ny, len(dsarr), len(dnarr), len(dyarr)) == ("gp_logpdf_grad_batch", 4, 4, 4, 4, 4, 4)
    assert dsarr[0] is None and dsarr[3] is None and dsarr[1] is not None and dsarr[2] is not None  # NULL where nscale = 0
    assert [None if a is None else a.shape for a in gcall.dscale] == [None, (1,), (3,), None]
    assert [a.shape for a in gcall.dnoise] == [(1,), (1,), (4,), (5,)] and [a.shape for a in gcall.dy] == [(6,), (9,), (4,), (5,)]
    assert gcall.noise_kind == [0, 0, 1, 1] and gcall.dvar.shape == (4,) and gcall.dvar.dtype == np.float64
    assert all(dnarr[b] == gcall.dnoise[b].ctypes.data and dyarr[b] == gcall.dy[b].ctypes.data for b in range(4))
    assert marr[0] is None and marr[1] is not None
    # a shared x and a shared y are sent once
    x = np.linspace(0, 3, 7)
    y = np.sin(x)
    shared = [agp.GP((1.0 + 0.1 * b) * agp.SqExponentialKernel())(x, 0.02) for b in range(5)]
    (g1,) = agp.api._batch_groups(shared, y)
    c1 = agp.api._grad_batch_marshal(g1)
    assert (c1.nb, c1.nx, c1.ny, len(c1.args[3]), len(c1.args[7])) == (5, 1, 1, 1, 1) and len(c1.dy) == 5 and c1.args[5] is None  # no mean array at all
    # float32 problems: noise and y gradients in the call's dtype, kernel gradients always double
    (g32,) = agp.api._batch_groups(*zip(*[_fx(5, 7, dtype=np.float32)]))
    c32 = agp.api._grad_batch_marshal(g32)
    assert c32.dy[0].dtype == np.float32 and c32.dnoise[0].dtype == np.float32 and c32.dvar.dtype == np.float64


def test_composite_marshalling_against_the_single_kind_entry_and_the_callers_order():
    comp = agp.SqExponentialKernel() @ agp.ScaleTransform(0.5) + 0.5 * agp.Matern32Kernel() * agp.PeriodicKernel(r=[0.9])
    specs = [(5, np.float64, None), (7, np.float32, None), (4, np.float64, comp), (9, np.float64, None), (6, np.float64, comp)]
    pairs = [_fx(n, i, dt, k) for i, (n, dt, k) in enumerate(specs)]
    groups = agp.api._batch_groups([p[0] for p in pairs], [p[1] for p in pairs])
    assert [(g.dtype, g.composite, g.index) for g in groups] == [(np.float64, False, [0, 3]), (np.float32, False, [1]), (np.float64, True, [2, 4])]
    calls = [agp.api._grad_batch_marshal(g) for g in groups]
    assert [c.entry for c in calls] == ["gp_logpdf_grad_batch", "gp_logpdf_grad_batch", "gp_logpdf_grad_batch_sum"]
    cs = calls[2]
    nth = len(agp.api._NormalForm(comp).theta())
    assert len(cs.args) == 13 and [a.shape for a in cs.dtheta] == [(nth,), (nth,)] and cs.dvar is None and cs.dscale is None and len(cs.nfs) == 2
    assert len(calls[0].args) == 14 and calls[0].dtheta is None
    assert all(cs.args[10][b] == cs.dtheta[b].ctypes.data for b in range(2))


def test_argument_checks_of_the_mirror_need_no_device():
    fx, y = _fx(5, 0)
    lp, grads = agp.logpdf_and_grad_batch([], [])
    assert lp.shape == (0,) and grads == []
    with pytest.raises(ValueError, match="on_error"):
        agp.logpdf_and_grad_batch([fx], [y], on_error="ignore")
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.logpdf_and_grad_batch([fx, fx], [y])
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.logpdf_and_grad_batch([fx], [np.zeros(4)])
    with pytest.raises(TypeError):
        agp.logpdf_and_grad_batch([object()], [y])


def test_the_oracle_gradient_is_far_inside_the_gpu_tolerances_on_the_ragged_cases():
    """oracle.logpdf_grad (explicit inverse) against a gradient from SciPy's Cholesky (L⁻¹, then L⁻ᵀL⁻¹) on bc.ragged_cases(): worst relative error of a
    kernel entry 4.4e-11 (a variance), noise 7.4e-12 of its largest entry, ∂/∂y 1.5e-12 when this test was written; 1e-9 asserted, a hundredth of the
    relative term of the GPU tolerance.  The smallest kernel entry of any case is 6e-6 of that problem's g∞: the relative term governs everywhere."""
    cases, refs = gc.ragged_with_oracle()
    worst = {"kernel": 0.0, "noise": 0.0, "y": 0.0, "smallest": np.inf}
    for c, (_, g) in zip(cases, refs):
        h = gc.scipy_grad(c)
        kg, kh = gc.entries(g, ("variance", "scale")), gc.entries(h, ("variance", "scale"))
        ng, nh = gc.entries(g, ("noise",)), gc.entries(h, ("noise",))
        ginf = max(np.max(np.abs(kh)), np.max(np.abs(nh)))
        worst["kernel"] = max(worst["kernel"], float(np.max(np.abs(kg - kh) / np.abs(kh))))
        worst["noise"] = max(worst["noise"], float(np.max(np.abs(ng - nh)) / np.max(np.abs(nh))))
        worst["y"] = max(worst["y"], bc.vec_err(g["y"], h["y"]))
        worst["smallest"] = min(worst["smallest"], float(np.min(np.abs(kh)) / ginf))
    print("oracle against SciPy: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert worst["kernel"] <= 1e-9 and worst["noise"] <= 1e-9 and worst["y"] <= 1e-9
    assert worst["smallest"] * gc.G_RTOL > 0  # every kernel entry is non-zero: the relative term of the tolerance is never vacuous
