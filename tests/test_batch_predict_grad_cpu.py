"""CPU: what gp_predict_grad_batch / gp_predict_grad_batch_sum promise without a device — the symbols (declared, bound with matching prototypes, exported),
the routing constant and the counter's name in header and sources, the static side of the entry points' guard, the context-free half of
mean_and_var_grad_batch — and the reference the GPU tests measure against (tests/predict_grad_ref.HostPosterior.grads): on the exact cases
tests/test_gpu_batch_predict_grad.py uses, its cho_solve form against the device's form through the explicit S = L⁻ᵀ (W = (K* S) Sᵀ), and one case per kind
against central differences of the oracle's mean_and_var.

The S form and the cho_solve form differ by rounding only: both are backward stable solves with a factor whose condition number the cases bound (Σy at
least 1e-2 of the prior variance); the bound asked for is 1e-3 of the gradient tolerance (rtol 1e-7, atol 1e-8·max(1, max|g|)), so that a device failure
at that tolerance is the device's.  Measured here: 1.6e-6 of the tolerance at worst (n = 2 048)."""
import re
from pathlib import Path

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import batch_cases as bc
from tests import batch_pgrad_cases as pg
from tests import test_abi_guard_static as gs
from tests import test_shim_static as ss
from tests.predict_grad_ref import central_differences
from tests.test_gpu_batch_predict import with_points

ROOT = Path(__file__).resolve().parent.parent
NEW = ("gp_predict_grad_batch", "gp_predict_grad_batch_sum")


def test_both_symbols_are_declared_exported_and_bound_with_the_leading_arguments_of_gp_predict_batch(agp):
    lib = agp._lib.load()
    assert all(hasattr(lib, s) for s in NEW) and set(NEW) <= set(agp._lib.header_functions()) and set(NEW) <= set(agp._lib.PROTOTYPES)
    assert lib.gp_abi_version() == 4
    protos = ss.header_prototypes()
    for new, old in (("gp_predict_grad_batch", "gp_predict_batch"), ("gp_predict_grad_batch_sum", "gp_predict_batch_sum")):
        res, args = agp._lib.PROTOTYPES[new]
        res_old, args_old = agp._lib.PROTOTYPES[old]
        # ctx … what, mean_out, var_out | dmean_out, dvar_out | logpdf_out, info_out
        assert res is res_old and args[:15] == args_old[:15] and args[17:] == args_old[15:] and len(args) == 19 and args[15] == args[16] == args[14]
        assert protos[new][1][:15] == protos[old][1][:15] and protos[new][1][17:] == protos[old][1][15:] and protos[new][1][15:17] == ["ptr", "ptr"]
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gpmi355.h").read_text(), flags=re.S)
    names = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(fn + r"\s*\(([^()]*)\)\s*;", hdr).group(1).split(",")]  # noqa: E731
    assert names("gp_predict_grad_batch")[:13] == names("gp_predict_batch")[:13]
    assert names("gp_predict_grad_batch")[13:] == ["mean_out_or_null", "var_out_or_null", "dmean_out_or_null", "dvar_out_or_null", "logpdf_out_or_null", "info_out"]
    assert names("gp_predict_grad_batch_sum") == names("gp_predict_grad_batch")
    assert "mean_and_var_grad_batch" in dir(agp) and agp.mean_and_var_grad_batch is agp.api.mean_and_var_grad_batch


def test_the_constant_and_the_counter_are_in_the_header_and_the_sources(agp):
    hdr = (ROOT / "include" / "gpmi355.h").read_text()
    n = agp._lib.batch_pgrad_max_n()
    assert n % 128 == 0 and 128 <= n <= 2048  # a multiple of 128 of the sweep, within what the kernels admit
    csrc = gs.CSRC
    batch, engine, main = ((csrc / f).read_text() for f in ("batch.hip", "engine.hpp", "gpmi355.hip"))
    assert 'env_capped(getenv("GPMI_BATCH_PGRAD_MAX_N"), GPMI355_BATCH_PGRAD_MAX_N)' in batch and "GPMI_BATCH_PGRAD_MAX_N" in hdr
    assert '"batch_pgrad_kernel_problems"' in hdr and '"batch_pgrad_kernel_problems"' in main
    assert "batch_pgrad_problems" in engine and "c->batch_pgrad_problems += nw" in batch and "c->batch_pgrad_problems" in main
    assert "batch_pgrad_kernel" in batch and "ksum_gradx" in (csrc / "kfun.hpp").read_text()
    assert "void ksum_gradx(" not in (csrc / "kernels.hpp").read_text()  # one definition, in kfun.hpp


def test_the_new_entry_points_are_guarded_by_a_body_of_their_own():
    src = gs.strip_comments((gs.CSRC / "batch.hip").read_text())
    defs = gs.definitions(src)
    want = gs.header_handle_functions(gs.HEADER.read_text())
    for name in NEW:
        assert want[name] == "gp_ctx" and gs.guard_problem(name, "gp_ctx", defs) is None
        h, body = defs[name]
        assert "predict_grad_batch_impl(" + h in body and " predict_batch_impl(" not in body
    body = defs["predict_grad_batch_impl"][1]
    assert "Guard gd(c);" in body and "run_drained" not in body and "run_predict_wave(" in body
    # the lock is released before the routed problems re-enter the single path
    assert body.index("gd.lk.unlock();") < body.index("gp_posterior_fit(") and body.index("gd.lk.unlock();") < body.index("gp_posterior_predict_grad(")
    assert body.index("for_each_wave(") < body.index("gd.lk.unlock();")
    assert "run_drained(" in defs["run_predict_wave"][1]  # the device work of a wave
    # without the guard of the new body exactly the two new names are reported
    cut = src.index("int32_t predict_grad_batch_impl(")
    mutated = src[:cut] + src[cut:].replace("Guard gd(c);", "", 1)
    defs_m = gs.definitions(mutated)
    assert sorted(n for n in want if n in defs_m and gs.guard_problem(n, want[n], defs_m) and n not in gs.RELEASING and "batch" in n) == sorted(NEW)


def test_marshalling_and_argument_checks_of_the_mirror_need_no_device():
    rng = np.random.default_rng(1)

    def fx(n, seed, mean=None):
        r = np.random.default_rng(seed)
        g = agp.GP(1.3 * agp.SqExponentialKernel()) if mean is None else agp.GP(mean, 1.3 * agp.SqExponentialKernel())
        return g(agp.RowVecs(r.uniform(0, 3, size=(n, 2))), 0.02), r.standard_normal(n)

    pairs = [fx(6, 0), fx(9, 1, mean=0.4), fx(4, 2, mean=lambda v: float(np.sum(v)))]
    fxs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    xss = [agp.RowVecs(rng.uniform(0, 3, size=(k, 2))) for k in (3, 0, 7)]
    (g,) = agp.api._predict_groups(fxs, ys, xss)
    pc = agp.api._predict_grad_marshal(g, 3)
    assert pc.entry == "gp_predict_grad_batch" and len(pc.args) == 18 and pc.args[11] == 3
    assert [a.size for a in pc.dmeans] == [6, 0, 14] == [a.size for a in pc.dvars] and pc.dmeans[0].shape == (3, 2) and pc.dvars[2].shape == (7, 2)
    assert [a.shape for a in pc.means] == [(3,), (0,), (7,)]
    p1 = agp.api._predict_grad_marshal(g, 1)
    assert p1.args[13] is None and p1.args[15] is None and p1.dvars is None and len(p1.args[12]) == len(p1.args[14]) == 3
    p2 = agp.api._predict_grad_marshal(g, 2)
    assert p2.args[12] is None and p2.args[14] is None and p2.dmeans is None and len(p2.args[13]) == len(p2.args[15]) == 3
    comp = agp.SqExponentialKernel() + 0.5 * agp.Matern32Kernel()
    (gc,) = agp.api._predict_groups([agp.GP(comp)(np.linspace(0, 1, 5), 0.1)], [np.zeros(5)], np.linspace(0, 1, 4))
    assert agp.api._predict_grad_marshal(gc, 3).entry == "gp_predict_grad_batch_sum"
    # checks that come before any library call
    assert agp.mean_and_var_grad_batch([], [], []) == []
    quads, lp = agp.mean_and_var_grad_batch([], [], [], return_logpdf=True)
    assert quads == [] and lp.shape == (0,)
    with pytest.raises(ValueError, match="what"):
        agp.mean_and_var_grad_batch(fxs, ys, xss, what=0)
    with pytest.raises(ValueError, match="on_error"):
        agp.mean_and_var_grad_batch(fxs, ys, xss, on_error="ignore")
    with pytest.raises(ValueError, match="mean_grads"):
        agp.mean_and_var_grad_batch(fxs, ys, xss, mean_grads=[None])
    with pytest.raises(TypeError, match=r"mean_grads\[2\]"):  # a CustomMean with the mean side: never a silently incomplete gradient
        agp.mean_and_var_grad_batch(fxs, ys, xss)
    with pytest.raises(TypeError, match="CustomMean"):
        agp.mean_and_var_grad_batch(fxs, ys, xss, what=1, mean_grads=[None, None, None])


def test_the_host_reference_through_the_explicit_inverse_factor_agrees_with_its_cho_solve_form():
    """W = (K* S) Sᵀ with S = L⁻ᵀ — the device's form — against cho_solve, on the cases of the GPU tests (the ragged batch and the kernels' own limit)."""
    worst = 0.0
    for c in list(pg.ragged_cases()) + pg.limit_cases():
        if c["ns"] == 0:
            continue
        hp = pg.host(c)
        Xs = pg.xs_rows(c)
        ref, got = hp.grads(Xs), pg.grads_through_S(hp, Xs)
        e = max(float(np.max(np.abs(a - b) / pg.g_bound(b))) for a, b in zip(got, ref))
        print(f"n={c['n']} ns={c['ns']} kind={c['kind']} {c['tr']} D={c['d']}: S form against cho_solve {e:.1e} of the gradient tolerance")
        worst = max(worst, e)
    print(f"worst: {worst:.1e} of the gradient tolerance")
    assert worst <= 1e-3


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_the_host_reference_against_central_differences_of_the_oracle(kind):
    """Bound and error model: tests/test_predict_grad_cpu.py (h = 1e-5: truncation ≈ 2e-11·|f'''|, rounding ≈ 1e-11; 1e-7·max|g| leaves orders over both).
    The test points keep away from the training points (D = 3): Matern12 has a kink there, where the device's convention (0) is not a derivative."""
    c = with_points(bc.make_case(120, kind, "ard", 3, "rowvecs", "vector", "const", seed=40 + kind), 43, seed=140 + kind)
    Xs = pg.xs_rows(c)[3:]  # the first three coincide with training points
    post = bc.o.logpdf_and_posterior(c["ofx"], c["y"])[1]
    g = pg.host(c).grads(Xs)
    fd = central_differences(lambda Z: tuple(np.asarray(a) for a in post.mean_and_var(Z)), Xs)
    for name, a, b in (("mean", g[0], fd[0]), ("var", g[1], fd[1])):
        worst = float(np.abs(a - b).max())
        print(f"kind {kind} d{name}: max |fd - g| / max|g| = {worst / np.abs(a).max():.2e}")
        assert worst <= 1e-7 * np.abs(a).max()
