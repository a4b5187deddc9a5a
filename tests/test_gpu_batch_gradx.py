"""GPU: gp_logpdf_grad_batch_x / gp_logpdf_grad_batch_sum_x (csrc/batch.hip: the kernels of gp_logpdf_grad_batch, then batch_gradx_kernel and
batch_gxsum_kernel on the S strips and α they leave) through agp.logpdf_and_grad_batch(..., wrt_x=True) — the gradient of logpdf w.r.t. the inputs of many
small exact GPs in one call.  Tolerance of "x": the project's own for input gradients (tests/batch_gradx_cases.py): fp64 |err| <= 1e-7·|ref| +
1e-8·max(1, max|g_ref|), fp32 2e-2 for both; the other outputs keep the tolerances of tests/batch_grad_cases.py.  The read-only ctx parameter
"batch_gradx_kernel_problems" proves which path served a problem."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_cases as bc
from tests import batch_grad_cases as gc
from tests import batch_gradx_cases as xc
from tests.composite_dx_ref import many_dim_kernel, ref_logpdf_grad_x, six_term_data, six_term_kernel

pytestmark = pytest.mark.gpu

COUNTER = "batch_gradx_kernel_problems"


def call(cases, **kw):
    return agp.logpdf_and_grad_batch([c["fx"] for c in cases], [c["y"] for c in cases], **kw)


def without_x(g):
    return {k: v for k, v in g.items() if k != "x"}


def report(tag, c, lp, g, ref):
    """every figure printed, then: all outputs within tolerance of the reference (logpdf, gradient dict with "x" as (n, d) / (n,))"""
    lp_ref, g_ref = ref
    ex, ey = gc.grad_excess(g, g_ref)
    el = bc.lp_err(lp, lp_ref)
    print(f"{tag}: kernel/noise {ex:.2e} of the tolerance, dy {ey:.1e}, logpdf {el:.1e}")
    return xc.report_x(tag, c, g["x"], g_ref["x"]) and ex <= 1.0 and ey <= gc.DY_TOL and el <= gc.LP_TOL


def on(ctx, cases):
    """the same problems with their priors bound to ctx"""
    out = []
    for c in cases:
        f = c["fx"].f
        g = agp.GP(f.kernel, ctx=ctx) if f.mean_fn is None else agp.GP(f.mean_fn, f.kernel, ctx=ctx)
        out.append(dict(c, fx=agp.FiniteGP(g, c["fx"].x, c["fx"].sigma2)))
    return out


# ---- 1. boundary sizes in one call ----------------------------------------------------------------------------------------------------------------
def test_boundary_sizes_in_one_call_against_the_oracle_and_the_loop(agp, ctx):
    cases, refs = xc.boundary_with_oracle()
    assert {c["n"] for c in cases} == set(xc.BOUNDARY_SIZES) and {c["d"] for c in cases} == {1, 3, 8, 16}
    assert {c["kind"] for c in cases} == {0, 1, 2, 3} and {c["tr"] for c in cases} == set(bc.TRANSFORMS) and {c["noise"] for c in cases} == set(bc.NOISES)
    assert {c["mean"] for c in cases} == set(bc.MEANS) and {c["container"] for c in cases} == set(bc.CONTAINERS)
    before = ctx.get_param(COUNTER)
    lp, grads = call(cases, wrt_x=True)
    assert ctx.get_param(COUNTER) - before == len(cases)  # the kernels served every problem
    ok = True
    for b, c in enumerate(cases):
        g = grads[b]
        assert set(g) == {"variance", "scale", "noise", "y", "mean", "x"} and g["x"].dtype == np.float64 and g["x"].shape == xc.x_shape(c)
        ok &= report(f"problem {b} vs oracle", c, lp[b], g, refs[b])
        _, gl = agp.logpdf_and_grad(c["fx"], c["y"], wrt_x=True)
        assert gl["x"].shape == g["x"].shape
        ok &= xc.report_x(f"problem {b} vs single", c, g["x"], xc.rows_of(gl["x"], c))
        if c["n"] == 1:
            assert np.all(g["x"] == 0.0)  # no pairs: exactly zero
    assert ok


# ---- 2. ragged batch ---------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_against_the_oracle(agp, ctx, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_GRADX_MAX_N", "1024")  # every size of the ragged set is kernel-served whatever the constant is
    cases, refs = gc.ragged_with_oracle()
    before = ctx.get_param(COUNTER)
    lp, grads = call(cases, wrt_x=True)
    assert ctx.get_param(COUNTER) - before == len(cases)
    assert all(report(f"problem {b}", c, lp[b], grads[b], refs[b]) for b, c in enumerate(cases))


# ---- 3. outputs that must not change ------------------------------------------------------------------------------------------------------------------
def test_the_other_outputs_are_the_bits_of_the_call_without_wrt_x(agp, ctx):
    limit = min(agp._lib.batch_gradx_max_n(), agp._lib.batch_grad_max_n())
    cases = [c for c in xc.boundary_cases() + bc.small_cases(12, seed=21) if c["n"] <= limit]
    assert len(cases) >= 24
    lp0, g0 = call(cases)
    lp1, g1 = call(cases, wrt_x=True)
    assert lp0.tobytes() == lp1.tobytes()
    for a, b in zip(g0, g1):
        assert "x" not in a and gc.same_bits(a, without_x(b))
    # through ctypes: the _x entry with a NULL dx array equals the plain entry bit for bit
    (g,) = agp.api._batch_groups([c["fx"] for c in cases], [c["y"] for c in cases])
    plain, nulled = agp.api._grad_batch_marshal(g), agp.api._grad_batch_marshal(g)
    served = ctx.get_param(COUNTER)
    assert ctx.lib.gp_logpdf_grad_batch(ctx.handle, *plain.args) == 0
    assert ctx.lib.gp_logpdf_grad_batch_x(ctx.handle, *nulled.args, None) == 0
    assert ctx.get_param(COUNTER) == served  # no dx: the new kernels do not run
    assert plain.out.tobytes() == nulled.out.tobytes() == lp0.tobytes() and plain.dvar.tobytes() == nulled.dvar.tobytes()
    for p, q in zip(plain.dnoise + plain.dy + [a for a in plain.dscale if a is not None], nulled.dnoise + nulled.dy + [a for a in nulled.dscale if a is not None]):
        assert p.tobytes() == q.tobytes()


# ---- 4. the kernels' own limit -----------------------------------------------------------------------------------------------------------------------
def test_the_kernels_serve_every_size_up_to_their_own_limit(agp, ctx, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_GRADX_MAX_N", "2048")
    cases = [bc.make_case(2048, 3, "scale", 3, "colvecs", "vector", "const", seed=92), bc.make_case(1985, 2, "ard", 3, "rowvecs", "scalar", "custom", seed=91)]
    before = ctx.get_param(COUNTER)
    lp, grads = call(cases, wrt_x=True)
    assert ctx.get_param(COUNTER) - before == 2
    assert all(report("kernel-served", c, lp[b], grads[b], gc.oracle_grad(c)) for b, c in enumerate(cases))


# ---- 5. neighbours and repetition --------------------------------------------------------------------------------------------------------------------
def test_a_problem_does_not_see_its_neighbours(agp):
    p = bc.make_case(200, 2, "ard", 3, "rowvecs", "vector", "custom", seed=77)
    lp0, (g0,) = call([p], wrt_x=True)
    assert report("alone", p, lp0[0], g0, gc.oracle_grad(p))
    lp0b, (g0b,) = call([p], wrt_x=True)
    assert gc.same_bits(g0, g0b) and lp0.tobytes() == lp0b.tobytes()  # repetition
    others = bc.small_cases(63, seed=3)
    for total in (2, 64):
        for pos in sorted({0, total // 2, total - 1}):
            batch = others[:total - 1]
            batch = batch[:pos] + [p] + batch[pos:]
            lp, grads = call(batch, wrt_x=True, on_error="nan")
            assert gc.same_bits(grads[pos], g0) and lp[pos].tobytes() == lp0[0].tobytes(), (total, pos)


# ---- 6. coincident points ----------------------------------------------------------------------------------------------------------------------------
def test_coincident_points_contribute_nothing(agp, ctx):
    cases = [xc.duplicate_case(0, 31), xc.duplicate_case(1, 32)]  # SE, Matern12
    before = ctx.get_param(COUNTER)
    lp, grads = call(cases, wrt_x=True)
    assert ctx.get_param(COUNTER) - before == 2
    for b, c in enumerate(cases):
        assert np.all(np.isfinite(grads[b]["x"]))
        assert report(f"duplicates kind={c['kind']}", c, lp[b], grads[b], gc.oracle_grad(c))


# ---- 7. composite kernels ----------------------------------------------------------------------------------------------------------------------------
def _comp(k, X, y, noise, mean=0.0):
    fx = (agp.GP(mean, k) if mean else agp.GP(k))(agp.RowVecs(X), noise)
    return {"fx": fx, "y": y, "n": X.shape[0], "d": X.shape[1], "container": "rowvecs", "ref": ref_logpdf_grad_x(k, X, y, noise, mean)}


def test_composite_kernels_against_the_host_reference_and_a_mixed_call(agp, ctx):
    comps = []
    for n in (130, 333):
        X, y = six_term_data(n, seed=n)
        comps.append(_comp(six_term_kernel(), X, y, 0.05))
        comps.append(_comp(six_term_kernel(), X, y, np.random.default_rng(n + 1).uniform(0.03, 0.1, n), 0.2))
    rng = np.random.default_rng(216)
    X16 = rng.uniform(0, 2, size=(260, 16))
    comps.append(_comp(many_dim_kernel(16), X16, np.sin(X16.sum(1) / 2) + 0.1 * rng.standard_normal(260), 0.1))
    X3, y3 = six_term_data(150, seed=7)
    X3[11] = X3[10]  # the White factor is 1 at coincident points and contributes no derivative
    kw = (0.7 * agp.WhiteKernel() * (agp.Matern32Kernel() @ agp.ScaleTransform(0.6))
          + (agp.PeriodicKernel(r=[1.0, 0.8, 1.2]) @ agp.ARDTransform([0.3, 0.5, 0.4])) * agp.SqExponentialKernel())
    comps.append(_comp(kw, X3, y3, 0.05))
    before = ctx.get_param(COUNTER)
    lp, grads = call(comps, wrt_x=True)
    assert ctx.get_param(COUNTER) - before == len(comps)
    ok = True
    for b, c in enumerate(comps):
        assert set(grads[b]) == {"kernel", "theta", "noise", "y", "mean", "x"}
        ok &= xc.report_x(f"composite {b}", c, grads[b]["x"], c["ref"])
    assert ok
    lpn, gn = call(comps)  # the other outputs: the bits of the call without wrt_x
    assert lpn.tobytes() == lp.tobytes() and all(gc.same_bits(a, without_x(b)) for a, b in zip(gn, grads))
    # composite and single-kind problems in one mirror call: the same bits as each group alone
    singles = bc.small_cases(3, seed=9)
    lps, gs_ = call(singles, wrt_x=True)
    mixed = [comps[0], singles[0], comps[3], singles[1], singles[2], comps[4]]
    lpm, gm = call(mixed, wrt_x=True)
    for pos, b in ((0, 0), (2, 3), (5, 4)):
        assert gc.same_bits(gm[pos], grads[b]) and lpm[pos].tobytes() == lp[b].tobytes()
    for pos, s in ((1, 0), (3, 1), (4, 2)):
        assert gc.same_bits(gm[pos], gs_[s]) and lpm[pos].tobytes() == lps[s].tobytes()


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_a_one_term_composite_agrees_with_the_single_kind_kernel(agp, kind):
    ok = True
    for tr in bc.TRANSFORMS:
        c = bc.make_case(150, kind, tr, 3, "rowvecs", "scalar", "zero", seed=300 + kind)
        wrapped = dict(c, fx=agp.GP(agp.KernelSum((c["fx"].f.kernel,)))(c["fx"].x, c["s2"]))
        (_, (gs_,)), (_, (gk,)) = call([c], wrt_x=True), call([wrapped], wrt_x=True)
        dev = float(np.max(np.abs(gk["x"] - gs_["x"])) / np.abs(gs_["x"]).max())
        print(f"one-term kind={kind} {tr}: max|composite - single| / max|g| = {dev:.3e}")
        ok &= dev <= 1e-9 and xc.report_x(f"one-term kind={kind} {tr} vs oracle", c, gk["x"], gc.oracle_grad(c)[1]["x"])
    assert ok


# ---- 8. routing --------------------------------------------------------------------------------------------------------------------------------------
def test_routed_problems_are_answered_by_the_single_path_inside_the_call(agp, ctx, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_GRADX_MAX_N", "256")
    served = [bc.make_case(n, b % 4, bc.TRANSFORMS[b % 3], 3, "rowvecs", bc.NOISES[b % 2], "const", seed=800 + b) for b, n in enumerate((100, 256, 31))]
    above = bc.make_case(300, 1, "ard", 3, "colvecs", "vector", "const", seed=811)
    d17 = bc.make_case(90, 0, "ard", 17, "rowvecs", "scalar", "zero", seed=812)
    f32 = bc.make_case(120, 2, "scale", 3, "rowvecs", "scalar", "zero", seed=813, dtype=np.float32)
    dn = bc.make_case(80, 3, "ard", 3, "rowvecs", "scalar", "zero", seed=814)
    B = np.random.default_rng(815).standard_normal((80, 4))
    S = 0.05 * np.eye(80) + 0.01 * B @ B.T
    dense = dict(dn, fx=agp.FiniteGP(dn["fx"].f, dn["fx"].x, S))
    batch = [served[0], above, f32, served[1], dense, d17, served[2]]
    before = ctx.get_param(COUNTER)
    lp, grads = call(batch, wrt_x=True)
    assert ctx.get_param(COUNTER) - before == 3  # only the served ones count
    ok = True
    for pos, c in ((0, served[0]), (1, above), (3, served[1]), (5, d17), (6, served[2])):
        ok &= report(f"routing pos {pos}", c, lp[pos], grads[pos], gc.oracle_grad(c))
    assert grads[2]["x"].dtype == np.float32 and grads[2]["x"].shape == (120, 3)
    ok &= xc.report_x("routing fp32", f32, grads[2]["x"], gc.oracle_grad(f32)[1]["x"])
    assert grads[4]["noise"].shape == (80, 80)
    ok &= xc.report_x("routing dense", dense, grads[4]["x"], ref_logpdf_grad_x(dn["fx"].f.kernel, dn["X"], dn["y"], S))
    assert ok


# ---- 9. shared x ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_shared_x_gives_every_problem_its_own_gradient(agp, ctx):
    rng = np.random.default_rng(900)
    n, d = 140, 3
    X = rng.uniform(0.0, 2.5, size=(n, d))
    xin = agp.RowVecs(X)
    cases = []
    for b in range(5):
        scale = np.linspace(0.5, 0.9, d) + 0.05 * b
        k = (1.0 + 0.2 * b) * [agp.SqExponentialKernel, agp.Matern12Kernel, agp.Matern32Kernel, agp.Matern52Kernel][b % 4]() @ agp.ARDTransform(scale)
        y = rng.standard_normal(n)
        cases.append({"fx": agp.GP(k)(xin, 0.05), "ofx": o.FiniteGP(o.GP(o.Kernel(b % 4, 1.0 + 0.2 * b, scale)), X, 0.05), "y": y, "n": n, "d": d,
                      "container": "rowvecs"})
    (g,) = agp.api._batch_groups([c["fx"] for c in cases], [c["y"] for c in cases])
    assert g.nx == 1  # one x object, sent once
    before = ctx.get_param(COUNTER)
    lp, grads = call(cases, wrt_x=True)
    assert ctx.get_param(COUNTER) - before == 5
    assert all(report(f"shared x {b}", c, lp[b], grads[b], gc.oracle_grad(c)) for b, c in enumerate(cases))
    assert len({grads[b]["x"].tobytes() for b in range(5)}) == 5


# ---- 10. failures are per problem ------------------------------------------------------------------------------------------------------------------------
def test_failures_are_per_problem(agp, ctx):
    good = bc.small_cases(9, seed=6, lo=40)
    lp_good, g_good = call(good, wrt_x=True)
    bad = list(good)
    c = good[4]
    s2 = np.array(np.broadcast_to(c["s2"], (c["n"],)), dtype=np.float64)
    i = int(0.6 * (c["n"] - 1))
    s2[i] = -10.0
    bad[4] = dict(c, fx=agp.FiniteGP(c["fx"].f, c["fx"].x, s2))
    lp, grads = call(bad, wrt_x=True, on_error="nan")
    assert np.flatnonzero(np.isnan(lp)).tolist() == [4]
    assert gc.all_nan(grads[4]) and grads[4]["x"].shape == xc.x_shape(c) and np.isnan(grads[4]["x"]).all()
    for b in range(9):
        if b != 4:
            assert gc.same_bits(grads[b], g_good[b]) and lp[b].tobytes() == lp_good[b].tobytes(), b
    with pytest.raises(agp.PosDefException) as e:
        call(bad, wrt_x=True)
    assert (e.value.index, e.value.info) == (4, i + 1)


# ---- 11. recycled blocks ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _poisoned_and_clean():
    cs = [agp.Context(0), agp.Context(0)]
    try:
        cs[0].set_param("alloc_poison", 1)
        assert cs[0].get_param("alloc_poison") == 1 and cs[1].get_param("alloc_poison") == 0
        yield cs
    finally:
        for c in cs:
            c.close()


def test_nothing_depends_on_what_a_recycled_block_held(agp):
    cases = bc.small_cases(16, seed=14) + [bc.make_case(n, 2, "ard", 3, "rowvecs", "vector", "const", seed=140 + n) for n in (1, 63, 65, 129, 193)]
    X, y = six_term_data(150, seed=3)
    comp = [{"fx": agp.GP(six_term_kernel())(agp.RowVecs(X), 0.05), "y": y}]
    results = []
    with _poisoned_and_clean() as ctxs:
        for c in ctxs:
            for batch in (on(c, cases), on(c, comp)):
                first = call(batch, wrt_x=True)
                cached = (c.get_param("pool_cached_mb"), c.get_param("pool_blocks"))
                second = call(batch, wrt_x=True)
                assert (c.get_param("pool_cached_mb"), c.get_param("pool_blocks")) == cached  # the second call runs in the first one's blocks
                assert first[0].tobytes() == second[0].tobytes() and all(gc.same_bits(p, q) for p, q in zip(first[1], second[1]))
                c.trim()
                results.append(first)
            assert c.get_param(COUNTER) == 2 * (len(cases) + len(comp))
    for (lp_p, g_p), (lp_c, g_c) in zip(results[:2], results[2:]):  # poisoned against clean
        assert np.isfinite(lp_p).all() and lp_p.tobytes() == lp_c.tobytes()
        assert all(gc.same_bits(p, q) for p, q in zip(g_p, g_c))
        assert all(np.isfinite(p["x"]).all() for p in g_p)
    for b in (0, 17, 20):
        assert report("recycled", cases[b], results[0][0][b], results[0][1][b], gc.oracle_grad(cases[b]))


# ---- 12. argument errors -------------------------------------------------------------------------------------------------------------------------------
def test_a_null_entry_of_the_dx_array_is_an_argument_error(agp, ctx):
    cases = [bc.make_case(n, 2, tr, 3, "rowvecs", "vector", "const", seed=700 + n) for n, tr in ((20, "ard"), (31, "none"), (12, "scale"))]
    (g,) = agp.api._batch_groups([c["fx"] for c in cases], [c["y"] for c in cases])
    gcall = agp.api._grad_batch_marshal(g, True)
    outs = [gcall.out, gcall.dvar] + [a for a in gcall.dscale if a is not None] + gcall.dnoise + gcall.dy + gcall.dx
    for a in outs:
        a[...] = 123.0
    args = list(gcall.args)
    args[-1] = (C.c_void_p * 3)(args[-1][0], None, args[-1][2])
    assert ctx.lib.gp_logpdf_grad_batch_x(ctx.handle, *args) == -16
    why = ctx.lib.gp_last_error().decode()
    assert why.startswith("invalid argument 16: ") and "dx_out" in why, why
    assert all(np.all(a == 123.0) for a in outs)  # a refused call writes nothing
    assert ctx.lib.gp_logpdf_grad_batch_x(None, *gcall.args) == -1 and "not a live gp_ctx" in ctx.lib.gp_last_error().decode()
    assert ctx.lib.gp_logpdf_grad_batch_x(ctx.handle, *gcall.args) == 0
    assert all(xc.dx_excess(gcall.dx[b], gc.oracle_grad(c)[1]["x"]) <= 1.0 for b, c in enumerate(cases))
    # the composite entry point counts its arguments itself
    X, y = six_term_data(40, seed=1)
    (gs_,) = agp.api._batch_groups([agp.GP(six_term_kernel())(agp.RowVecs(X), s) for s in (0.05, 0.07)], y)
    sc = agp.api._grad_batch_marshal(gs_, True)
    sargs = list(sc.args)
    sargs[-1] = (C.c_void_p * 2)(None, sargs[-1][1])
    assert ctx.lib.gp_logpdf_grad_batch_sum_x(ctx.handle, *sargs) == -15
    why = ctx.lib.gp_last_error().decode()
    assert why.startswith("invalid argument 15: ") and "dx_out" in why, why
    assert ctx.lib.gp_logpdf_grad_batch_sum_x(ctx.handle, *sc.args) == 0 and all(np.isfinite(a).all() for a in sc.dx)
