"""GPU: gp_loo_batch / gp_loo_batch_sum and gp_loo_grad_batch / gp_loo_grad_batch_sum (csrc/batch.hip: batch_logpdf_kernel and batch_inv_kernel, then
batch_loo_kernel and batch_loo_sum_kernel; for the gradient batch_loo_z_kernel, batch_loo_beta_kernel, batch_grad_kernel<SUM, true> and batch_gsum_kernel)
through agp.loo_logpdf_batch / loo_mean_and_var_batch / loo_logpdf_and_grad_batch, against the fp64 host reference of tests/loo_ref.py on the cases of
tests/loo_batch_cases.py (cond(C) ≤ 1e3, asserted in tests/test_loo_batch_cpu.py) and against the loop of single calls.

Tolerances are those of tests/loo_cases.py as tests/test_gpu_loo.py applies them: L rel 1e-10, ℓ 1e-10·max(1, max|ℓ|), μ abs 1e-8, v abs 1e-9, θ, noise and
∂/∂y entries 1e-7·|ref| + 1e-9·g∞.  Every comparison prints its ratio to the bound as a line "LOO_BATCH_RATIO <against> <group> <case> <ratio>".  The
read-only ctx parameters "batch_loo_kernel_problems" and "batch_loo_grad_kernel_problems" prove which path served a problem."""
from pathlib import Path

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import batch_cases as bc
from tests import loo_batch_cases as lb
from tests import loo_cases as lc

pytestmark = pytest.mark.gpu

VALUE, GRAD = "batch_loo_kernel_problems", "batch_loo_grad_kernel_problems"
GOLDEN = Path(__file__).resolve().parent / "golden" / lb.GOLDEN_BATCH_GRAD


@pytest.fixture(autouse=True)
def _limits(monkeypatch):
    """the kernels serve every case of tests/loo_batch_cases.py (n ≤ 320) whatever the header's limits are"""
    monkeypatch.setenv("GPMI_BATCH_LOO_MAX_N", "512")
    monkeypatch.setenv("GPMI_BATCH_LOO_GRAD_MAX_N", "512")


def run(cases, **kw):
    """the three mirror calls on one batch: per problem {"L", "lp", "mean", "var", "L_grad", "grad"}"""
    fxs, ys = [c["fx"] for c in cases], [c["y"] for c in cases]
    if len({id(y) for y in ys}) == 1 and len(ys) > 1:
        ys = ys[0]  # ONE vector shared by all
    L, lp = agp.loo_logpdf_batch(fxs, ys, pointwise=True, **kw)
    mu, var = agp.loo_mean_and_var_batch(fxs, ys, **kw)
    Lg, g = agp.loo_logpdf_and_grad_batch(fxs, ys, **kw)
    assert agp.loo_logpdf_batch(fxs, ys, **kw).tobytes() == L.tobytes()
    return [{"L": L[b], "lp": lp[b], "mean": mu[b], "var": var[b], "L_grad": Lg[b], "grad": g[b]} for b in range(len(cases))]


def singles(c):
    """the same from the loop of single calls, as a reference dict of lb.ratios"""
    mu, var = agp.loo_mean_and_var(c["fx"], c["y"])
    Lg, g = agp.loo_logpdf_and_grad(c["fx"], c["y"])
    return {"L": float(agp.loo_logpdf(c["fx"], c["y"])), "lp": agp.loo_logpdf(c["fx"], c["y"], pointwise=True), "mean": mu, "var": var, "grad": g}


def inside(c, out, ref, against):
    r = lb.ratios(c, ref, out["L"], out["lp"], out["mean"], out["var"], out["grad"])
    r["L_grad_call"] = lb.ratios(c, ref, L=out["L_grad"])["L"]
    for k, v in r.items():
        print(f"LOO_BATCH_RATIO {against} {k} {c['id']} {v:.3e}")
    g = out["grad"]
    assert np.array_equal(g["mean"], -g["y"]) and g["y"].shape == (c["n"],) and np.shape(g["noise"]) == (() if c["noise"] == "scalar" else (c["n"],))
    assert out["lp"].shape == out["mean"].shape == out["var"].shape == (c["n"],)
    return {f"{c['id']}:{k}": v for k, v in r.items() if not v <= 1.0}


def same_bits(p, q):
    return all(np.asarray(p[k]).tobytes() == np.asarray(q[k]).tobytes() for k in ("L", "lp", "mean", "var", "L_grad")) \
        and lb.grad_bytes(p["grad"]) == lb.grad_bytes(q["grad"])


def on(ctx, cases):
    """the same problems with their priors bound to ctx"""
    out = []
    for c in cases:
        f = c["fx"].f
        g = agp.GP(f.kernel, ctx=ctx) if f.mean_fn is None else agp.GP(f.mean_fn, f.kernel, ctx=ctx)
        out.append(dict(c, fx=agp.FiniteGP(g, c["fx"].x, c["fx"].sigma2)))
    return out


# ---- 1. every case against the reference and the loop of single calls ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ragged", "composite"] + lb.SHARED)
def test_every_case_against_the_host_reference_and_the_loop_of_single_calls(agp, ctx, which):
    cases = lb.ragged_batch() if which == "ragged" else (lb.composite_batch() if which == "composite" else lb.shared_batch(which))
    v0, g0 = ctx.get_param(VALUE), ctx.get_param(GRAD)
    outs = run(cases)
    assert ctx.get_param(VALUE) - v0 == 3 * len(cases) and ctx.get_param(GRAD) - g0 == len(cases)  # three value calls and one gradient call in run()
    bad = {}
    for c, out in zip(cases, outs):
        assert set(out["grad"]) == ({"kernel", "theta", "noise", "y", "mean"} if c["composite"] else {"variance", "scale", "noise", "y", "mean"})
        bad.update(inside(c, out, lb.reference(c), "reference"))
        bad.update(inside(c, out, singles(c), "single"))
    assert not bad, f"outside the tolerance (error / bound): {bad}"


def test_one_point_is_the_prior_prediction(agp):
    c = lb.single_case("b_n1")  # ConstMean 0.4, variance 1.3
    (out,) = run([c])
    assert out["mean"].shape == (1,) and abs(out["mean"][0] - 0.4) <= 1e-14 and abs(out["var"][0] - (1.3 + float(c["s2"]))) <= 1e-14
    in_company = run(lb.ragged_batch())[[k["id"] for k in lb.ragged_batch()].index("b_n1")]
    assert same_bits(out, in_company)


# ---- 2. the same bits alone, anywhere in a batch, on repetition and from recycled blocks ----------------------------------------------------------------
@pytest.mark.parametrize("cid", ["b_n193", "b_n64", "b_theta29_130"])
def test_a_problem_returns_the_same_bits_alone_anywhere_in_a_batch_and_twice(agp, cid):
    p = lb.case(cid)
    others = [c for c in (lb.composite_batch() if p["composite"] else lb.ragged_batch()) if c["id"] != cid]
    (alone,) = run([p])
    assert not inside(p, alone, lb.reference(p), "reference")
    (again,) = run([p])
    assert same_bits(alone, again)
    for pos in sorted({0, len(others) // 2, len(others)}):
        batch = others[:pos] + [p] + others[pos:]
        assert same_bits(run(batch)[pos], alone), pos


def test_nothing_depends_on_what_a_recycled_block_held(agp):
    """"alloc_poison" = 1 on a ctx of its own: every block handed out holds NaNs first; the second round takes recycled blocks"""
    batches = [lb.ragged_batch(), lb.composite_batch(), lb.shared_batch("shared_xy")]
    clean = [run(b) for b in batches]
    ctx = agp.Context(0)
    ctx.set_param("alloc_poison", 1)
    try:
        for b, ref in zip(batches, clean):
            for r in range(2):
                outs = run(on(ctx, b))
                assert all(same_bits(p, q) for p, q in zip(outs, ref)), r
                assert all(np.isfinite(o["lp"]).all() and np.isfinite(o["grad"]["y"]).all() for o in outs)
        assert ctx.get_param(GRAD) == 2 * sum(len(b) for b in batches)
    finally:
        ctx.close()


# ---- 3. routing ------------------------------------------------------------------------------------------------------------------------------------
def _lc_inside(c, out, ref, tag):
    """a case of tests/loo_cases.py (dense Σy, D = 17) against its reference"""
    r = {"L": abs(float(out["L"]) - ref["L"]) / (lc.L_TOL * abs(ref["L"])), "mean": float(np.max(np.abs(out["mean"] - ref["mean"]))) / lc.M_TOL,
         "var": float(np.max(np.abs(out["var"] - ref["var"]))) / lc.V_TOL,
         "lp": float(np.max(np.abs(out["lp"] - ref["lp"]))) / (lc.L_TOL * max(1.0, float(np.max(np.abs(ref["lp"]))))),
         "L_grad_call": abs(float(out["L_grad"]) - ref["L"]) / (lc.L_TOL * abs(ref["L"]))}
    g, rg = out["grad"], ref["grad"]
    for k in ("variance", "scale", "noise", "y"):
        if rg[k] is not None:
            r[k] = lc.grad_ratio(g[k], rg[k])
    for k, v in r.items():
        print(f"LOO_BATCH_RATIO reference {k} {tag} {v:.3e}")
    return {f"{tag}:{k}": v for k, v in r.items() if not v <= 1.0}


def test_which_path_serves_a_problem(agp, ctx):
    """fp64 problems with noise kind 0 / 1, D ≤ 16 and n within the limit are the kernels'; fp32, a dense Σy, D = 17 and every problem of a call with
    wrt_x go to gp_loo / gp_loo_grad inside the same call, and their results still match the reference"""
    mine = [lb.single_case("b_n65"), lb.single_case("b_n129")]
    dense, d17 = lc.single_case("n129_dense"), lc.single_case("n129_d17")
    f32 = lc.single_case(lc.F32[0], np.float32)
    batch = [mine[0], dense, d17, f32, mine[1]]
    v0, g0 = ctx.get_param(VALUE), ctx.get_param(GRAD)
    outs = run(batch)
    assert ctx.get_param(VALUE) - v0 == 3 * 2 and ctx.get_param(GRAD) - g0 == 2
    bad = {}
    for c, out in ((mine[0], outs[0]), (mine[1], outs[4])):
        bad.update(inside(c, out, lb.reference(c), "reference"))
    bad.update(_lc_inside(dense, outs[1], lc.reference(dense), "routed_dense"))
    bad.update(_lc_inside(d17, outs[2], lc.reference(d17), "routed_d17"))
    assert not bad, bad
    assert outs[1]["grad"]["noise"].shape == (129, 129)
    ref32 = lc.reference(f32, np.float32)
    assert outs[3]["lp"].dtype == np.float32 and outs[3]["grad"]["y"].dtype == np.float32
    assert abs(float(outs[3]["L"]) - ref32["L"]) <= 1e-4 * abs(ref32["L"]) and abs(float(outs[3]["L_grad"]) - ref32["L"]) <= 1e-4 * abs(ref32["L"])
    assert outs[3]["mean"].dtype == np.float32 and outs[3]["var"].dtype == np.float32  # (the value at the suite's fp32 tolerance, as tests/test_gpu_loo.py)
    # a call that asks for ∂/∂x runs on the single path, every problem of it
    v0, g0 = ctx.get_param(VALUE), ctx.get_param(GRAD)
    cases = [mine[0], mine[1], lb.composite_case("b_theta29_65")]
    L, grads = agp.loo_logpdf_and_grad_batch([c["fx"] for c in cases], [c["y"] for c in cases], wrt_x=True)
    assert ctx.get_param(VALUE) == v0 and ctx.get_param(GRAD) == g0
    for b, c in enumerate(cases):
        ref = lb.reference(c)
        r = lb.ratios(c, ref, L=L[b], g=grads[b])
        r["x"] = lc.gradx_ratio(grads[b]["x"], lc.grad_x_shaped(c, ref["grad"]["x"]))
        print(f"LOO_BATCH_RATIO reference wrt_x {c['id']} {r}")
        assert all(v <= 1.0 for v in r.values()), (c["id"], r)
        assert grads[b]["x"].shape == np.shape(lc.grad_x_shaped(c, ref["grad"]["x"]))


def test_with_the_limits_at_zero_everything_is_routed_and_the_values_agree(agp, ctx, monkeypatch):
    cases = lb.ragged_batch()[:6] + lb.composite_batch()[:2]
    served = run(cases)
    monkeypatch.setenv("GPMI_BATCH_LOO_MAX_N", "0")
    monkeypatch.setenv("GPMI_BATCH_LOO_GRAD_MAX_N", "0")
    v0, g0 = ctx.get_param(VALUE), ctx.get_param(GRAD)
    routed = run(cases)
    assert ctx.get_param(VALUE) == v0 and ctx.get_param(GRAD) == g0
    bad = {}
    for c, out, k in zip(cases, routed, served):
        bad.update(inside(c, out, lb.reference(c), "reference_routed"))
        bad.update(inside(c, out, {"L": float(k["L"]), "lp": k["lp"], "mean": k["mean"], "var": k["var"], "grad": k["grad"]}, "kernels"))
    assert not bad, bad


# ---- 4. failure is data ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["b_n129", "b_ml_128"])
def test_a_failing_problem_is_data_and_its_neighbours_are_untouched(agp, ctx, cid):
    good = [lb.single_case("b_n127"), lb.single_case("b_n192")] if cid == "b_n129" else [lb.composite_case("b_theta29_130"), lb.composite_case("b_ml_193")]
    c = lb.case(cid)
    s2 = np.array(np.broadcast_to(c["s2"], (c["n"],)), dtype=np.float64)
    s2[70] = -10.0 * (1.0 + float(np.max(np.abs(np.diag(c["K"])))))
    bad = dict(c, fx=agp.FiniteGP(c["fx"].f, c["fx"].x, s2), noise="vector")
    batch = [good[0], bad, good[1]]
    base = run(good)
    outs = run(batch, on_error="nan")
    assert same_bits(outs[0], base[0]) and same_bits(outs[2], base[1])
    o = outs[1]
    assert np.isnan(o["L"]) and np.isnan(o["L_grad"]) and all(np.isnan(o[k]).all() and o[k].shape == (c["n"],) for k in ("lp", "mean", "var"))
    assert all(np.isnan(np.asarray(v, dtype=np.float64)).all() for v in o["grad"].values() if v is not None)
    assert np.shape(o["grad"]["noise"]) == (c["n"],) and o["grad"]["y"].shape == (c["n"],)
    # the info of every problem, straight from the ABI: a failing problem is data, not a status
    (g,) = agp.api._batch_groups([k["fx"] for k in batch], [k["y"] for k in batch])
    for call in (agp.api._loo_batch_marshal(g), agp.api._loo_grad_batch_marshal(g)):
        assert getattr(ctx.lib, call.entry)(ctx.handle, *call.args) == 0
        assert call.info.tolist() == [0, 71, 0], call.entry
    for fn in (agp.loo_logpdf_batch, agp.loo_mean_and_var_batch, agp.loo_logpdf_and_grad_batch):
        with pytest.raises(agp.PosDefException) as e:
            fn([k["fx"] for k in batch], [k["y"] for k in batch])
        assert (e.value.index, e.value.info) == (1, 71)


# ---- 5. the generalised tile kernel leaves gp_logpdf_grad_batch its bits -------------------------------------------------------------------------------
def test_gp_logpdf_grad_batch_returns_the_bits_it_returned_before_the_weight_step_was_generalised(agp):
    """tests/golden/bits/batch_grad_bits_r32.npz: every output of lb.batch_grad_outputs() recorded on an MI355X with the library of the commit before
    batch_grad_kernel gained its LOO parameter (np.savez of that dict).  Beside it, what that commit already guaranteed: a problem of the batch returns the
    bits of a batch of one."""
    got = lb.batch_grad_outputs()
    with np.load(GOLDEN) as want:
        assert sorted(want.files) == sorted(got)
        diff = [k for k in got if got[k].dtype != want[k].dtype or got[k].tobytes() != want[k].tobytes()]
    assert not diff, f"outputs of gp_logpdf_grad_batch whose bits changed: {diff}"
    singles_ = bc.small_cases(12, seed=32, lo=40)
    for b in (0, 5, 11):
        lp1, (g1,) = agp.logpdf_and_grad_batch([singles_[b]["fx"]], [singles_[b]["y"]])
        assert lp1[0].tobytes() == got["s_logpdf"][b].tobytes()
        assert all(np.atleast_1d(np.asarray(v)).tobytes() == got[f"s{b}_{k}"].tobytes() for k, v in g1.items() if v is not None)
