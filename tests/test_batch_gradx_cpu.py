"""CPU: the context-free half of logpdf_and_grad_batch(..., wrt_x=True) — the declared, exported and bound gp_logpdf_grad_batch_x / gp_logpdf_grad_batch_sum_x,
GPMI355_BATCH_GRADX_MAX_N, the marshalling of the dx array, the mirror's argument checks, the static side of the entry points' guard — and the oracle's
own ∂logpdf/∂x against one built from SciPy's Cholesky on the cases the GPU tests use (the reference is itself far inside the tolerance it is used with)."""
import re
from pathlib import Path

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import batch_cases as bc
from tests import batch_grad_cases as gc
from tests import batch_gradx_cases as xc
from tests import test_abi_guard_static as gs
from tests import test_shim_static as ss

ROOT = Path(__file__).resolve().parent.parent
PAIRS = (("gp_logpdf_grad_batch_x", "gp_logpdf_grad_batch", 16), ("gp_logpdf_grad_batch_sum_x", "gp_logpdf_grad_batch_sum", 15))


def test_both_symbols_are_declared_exported_and_bound_with_the_arguments_of_the_entry_points_without_x(agp):
    lib = agp._lib.load()
    protos = ss.header_prototypes()
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gpmi355.h").read_text(), flags=re.S)
    names = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(r"\b" + fn + r"\s*\(([^()]*)\)\s*;", hdr).group(1).split(",")]  # noqa: E731
    for new, old, nargs in PAIRS:
        assert hasattr(lib, new) and new in agp._lib.header_functions() and new in agp._lib.PROTOTYPES
        res, args = agp._lib.PROTOTYPES[new]
        res_old, args_old = agp._lib.PROTOTYPES[old]
        assert res is res_old and len(args) == nargs == len(args_old) + 1 and args[:-1] == args_old and args[-1] is args_old[-1]  # one more void* const*
        assert protos[new] == (protos[old][0], protos[old][1] + ["ptr"])
        assert names(new) == names(old) + ["dx_out_or_null"]
    assert lib.gp_abi_version() == 4
    txt = (ROOT / "include" / "gpmi355.h").read_text()
    assert "There is no ∂/∂x here" not in txt


def test_the_size_limit_is_a_multiple_of_128_within_the_kernels_and_the_mirror_reads_it(agp):
    txt = (ROOT / "include" / "gpmi355.h").read_text()
    (v,) = re.findall(r"^#define GPMI355_BATCH_GRADX_MAX_N (\d+)$", txt, flags=re.M)
    assert int(v) % 128 == 0 and 0 < int(v) <= 2048 and int(v) == agp._lib.batch_gradx_max_n()
    src = (gs.CSRC / "batch.hip").read_text()
    assert 'getenv("GPMI_BATCH_GRADX_MAX_N")' in src and "GPMI355_BATCH_GRADX_MAX_N" in src
    assert '"batch_gradx_kernel_problems"' in txt and '"batch_gradx_kernel_problems"' in (gs.CSRC / "gpmi355.hip").read_text()
    assert "batch_gradx_problems" in (gs.CSRC / "engine.hpp").read_text() and "c->batch_gradx_problems += nwx" in src


def test_the_new_entry_points_start_with_a_guard_of_their_own_and_the_kernels_use_no_atomics():
    src = gs.strip_comments((gs.CSRC / "batch.hip").read_text())
    defs = gs.definitions(src)
    want = gs.header_handle_functions(gs.HEADER.read_text())
    for new, _, _ in PAIRS:
        assert want[new] == "gp_ctx" and gs.guard_problem(new, "gp_ctx", defs) is None
        h, body = defs[new]
        assert "gradx_batch_impl(" + h in body
    body = defs["gradx_batch_impl"][1]
    assert body.index("Guard gd(c);") < body.index("gd.lk.unlock()") < body.index("grad_batch_impl(c")  # grad_batch_impl takes the lock itself
    # the guard is the entry points' own: it holds without the one of grad_batch_impl, and without both all four entry points of the family are reported
    cut_g, cut_x = src.index("int32_t grad_batch_impl("), src.index("int32_t gradx_batch_impl(")
    assert cut_g < cut_x
    no_g = src[:cut_g] + src[cut_g:].replace("Guard gd(c);", "", 1)
    defs_g = gs.definitions(no_g)
    assert all(gs.guard_problem(new, "gp_ctx", defs_g) is None and gs.guard_problem(old, "gp_ctx", defs_g) for new, old, _ in PAIRS)
    cut_x = no_g.index("int32_t gradx_batch_impl(")
    defs_n = gs.definitions(no_g[:cut_x] + no_g[cut_x:].replace("Guard gd(c);", "", 1))
    assert sorted(n for n in want if n in defs_n and gs.guard_problem(n, want[n], defs_n)) == sorted(p[i] for p in PAIRS for i in (0, 1))
    assert "atomic" not in src
    for k in ("batch_gradx_kernel", "batch_gxsum_kernel"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", src), k
    kf = gs.strip_comments((gs.CSRC / "kfun.hpp").read_text())
    assert kf.count("void ksum_gradx(") == 1 and "ksum_gradx<double, BATCH_MAXD>" in src


def _fx(n, seed, container, dtype=np.float64, kernel=None, d=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 3, size=(n, d)).astype(dtype)
    x = X[:, 0].copy() if container == "vector" else (agp.ColVecs(np.ascontiguousarray(X.T)) if container == "colvecs" else agp.RowVecs(X))
    return agp.GP(kernel or 1.3 * agp.SqExponentialKernel())(x, 0.02), rng.standard_normal(n).astype(dtype)


def test_marshalling_of_the_dx_array_for_ragged_sizes_every_container_and_a_shared_x():
    pairs = [_fx(6, 0, "vector"), _fx(9, 1, "colvecs"), _fx(4, 2, "rowvecs"), _fx(5, 3, "rowvecs", d=8), _fx(7, 4, "colvecs", dtype=np.float32)]
    fxs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    g64, g32 = agp.api._batch_groups(fxs, ys)
    plain, call = agp.api._grad_batch_marshal(g64), agp.api._grad_batch_marshal(g64, True)
    assert plain.entry == "gp_logpdf_grad_batch" and plain.dx is None and len(plain.args) == 14  # without wrt_x: the same entry point and arguments
    assert call.entry == "gp_logpdf_grad_batch_x" and len(call.args) == 15 and call.nb == 4
    # the ABI layout of the inputs as they lie (no host copy): (n,) vector; a C-ordered ColVecs array (d, n) is dimension-major = layout 2; a C-ordered
    # RowVecs array (n, d) is point-major = layout 1
    assert [a.shape for a in call.dx] == [(6,), (3, 9), (4, 3), (5, 8)] and all(a.dtype == np.float64 for a in call.dx)
    assert [call.pts[b].layout for b in range(4)] == [0, 2, 1, 1]
    dxarr = call.args[-1]
    assert len(dxarr) == 4 and all(dxarr[b] == call.dx[b].ctypes.data for b in range(4))
    for b, a in enumerate(call.dx):  # what the caller gets back has the shape of the container's array
        a[...] = 0.0
        assert agp.api._dx_shaped(a, call.pts[b], fxs[b].x).shape == np.shape(fxs[b].x.X if hasattr(fxs[b].x, "X") else fxs[b].x)
    c32 = agp.api._grad_batch_marshal(g32, True)
    assert c32.dx[0].dtype == np.float32 and c32.dx[0].shape == (3, 7)
    # a shared x object is sent once, and every problem still has a buffer of its own
    X = agp.RowVecs(np.random.default_rng(5).uniform(0, 3, size=(7, 2)))
    y = np.arange(7.0)
    shared = [agp.GP((1.0 + 0.1 * b) * agp.SqExponentialKernel())(X, 0.02) for b in range(5)]
    (g1,) = agp.api._batch_groups(shared, y)
    c1 = agp.api._grad_batch_marshal(g1, True)
    assert (c1.nb, c1.nx, c1.ny, len(c1.args[3])) == (5, 1, 1, 1) and len(c1.dx) == 5 and len({a.ctypes.data for a in c1.dx}) == 5
    assert all(a.shape == (7, 2) for a in c1.dx)


def test_marshalling_of_the_composite_group():
    comp = agp.SqExponentialKernel() @ agp.ScaleTransform(0.5) + 0.5 * agp.Matern32Kernel() * agp.PeriodicKernel(r=[0.9, 1.0, 1.1])
    pairs = [_fx(5, 0, "rowvecs"), _fx(4, 1, "colvecs", kernel=comp), _fx(6, 2, "rowvecs", kernel=comp)]
    groups = agp.api._batch_groups([p[0] for p in pairs], [p[1] for p in pairs])
    calls = [agp.api._grad_batch_marshal(g, True) for g in groups]
    assert [c.entry for c in calls] == ["gp_logpdf_grad_batch_x", "gp_logpdf_grad_batch_sum_x"]
    cs = calls[1]
    assert len(cs.args) == 14 and [a.shape for a in cs.dx] == [(3, 4), (6, 3)] and cs.args[-1][1] == cs.dx[1].ctypes.data
    assert agp.api._grad_batch_marshal(groups[1]).entry == "gp_logpdf_grad_batch_sum"


def test_argument_checks_of_the_mirror_need_no_device():
    fx, y = _fx(5, 0, "rowvecs")
    lp, grads = agp.logpdf_and_grad_batch([], [], wrt_x=True)
    assert lp.shape == (0,) and grads == []
    with pytest.raises(ValueError, match="on_error"):
        agp.logpdf_and_grad_batch([fx], [y], wrt_x=True, on_error="ignore")
    with pytest.raises(TypeError, match="wrt_x"):
        agp.logpdf_and_grad_batch([fx], [y], wrt_x="yes")
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.logpdf_and_grad_batch([fx, fx], [y], wrt_x=True)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.logpdf_and_grad_batch([fx], [np.zeros(4)], wrt_x=True)
    with pytest.raises(TypeError):
        agp.logpdf_and_grad_batch([object()], [y], wrt_x=True)


def test_the_oracle_input_gradient_is_far_inside_the_gpu_tolerance():
    """oracle.logpdf_grad(...)["x"] (explicit inverse) against ∂/∂x from SciPy's Cholesky (L⁻¹ by a triangular solve, C⁻¹ = L⁻ᵀL⁻¹) on bc.ragged_cases(), the
    boundary cases and the two cases with coincident points, in units of the fp64 tolerance 1e-7·|g_ref| + 1e-8·max(1, max|g_ref|): at most 1e-2 of it in
    every entry.  Worst case when this test was written: 9.8e-4 of the tolerance (n = 1 000, Matern12, ARD, D = 1, max|g| = 1.7e4)."""
    cases, refs = gc.ragged_with_oracle()
    bcases, brefs = xc.boundary_with_oracle()
    dups = [xc.duplicate_case(0, 31), xc.duplicate_case(1, 32)]
    worst = 0.0
    for c, (_, g) in list(zip(cases, refs)) + list(zip(bcases, brefs)) + [(c, gc.oracle_grad(c)) for c in dups]:
        h = xc.scipy_grad_x(c)
        assert g["x"].shape == h.shape == ((c["n"],) if c["container"] == "vector" else (c["n"], c["d"]))
        ex = xc.dx_excess(g["x"], h)
        if ex > 0.5 * worst:
            print(f"n={c['n']} kind={c['kind']} {c['tr']} D={c['d']}: oracle against SciPy {ex:.2e} of the tolerance, max|g| = {np.abs(h).max():.2e}")
        worst = max(worst, ex)
    print(f"worst: {worst:.2e} of the tolerance")
    assert worst <= 1e-2
    assert np.all(bcases[0]["n"] == 1 and brefs[0][1]["x"] == 0.0)  # a single point has no pairs
    for c in dups:  # coincident points: finite, and the pair contributes nothing to either of its points beyond what the other pairs give
        assert np.all(np.isfinite(gc.oracle_grad(c)[1]["x"]))
