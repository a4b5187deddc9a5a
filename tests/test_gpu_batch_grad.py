"""GPU: gp_logpdf_grad_batch / gp_logpdf_grad_batch_sum (csrc/batch.hip: batch_logpdf_kernel, then batch_inv_kernel, batch_grad_kernel and batch_gsum_kernel
on the slices it leaves) through agp.logpdf_and_grad_batch — value and gradient of logpdf of many small exact GPs in one call.
Tolerances are the project's own for fp64 gradients (tests/batch_grad_cases.py): kernel and noise entries |err| <= 1e-7·|ref| + 1e-9·g∞, ∂/∂y 1e-8 in the
2-norm, logpdf 1e-10 relative to max(|reference|, 1).  The read-only ctx parameter "batch_grad_kernel_problems" proves which path served a problem."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import batch_cases as bc
from tests import batch_grad_cases as gc
from tests.composite_ref import dense_data, mauna_loa_kernel, ml_kernel

pytestmark = pytest.mark.gpu

COUNTER = "batch_grad_kernel_problems"
COMP = ("theta", "kernel", "noise")


def call(cases, **kw):
    return agp.logpdf_and_grad_batch([c["fx"] for c in cases], [c["y"] for c in cases], **kw)


def report(tag, c, lp, g, ref, keys=("variance", "scale", "noise")):
    """prints every figure, then returns whether all of them are within tolerance"""
    lp_ref, g_ref = ref
    ex, ey = gc.grad_excess(g, g_ref, keys)
    el = bc.lp_err(lp, lp_ref)
    print(f"{tag} n={c['n']} kind={c.get('kind')} {c.get('tr')} D={c.get('d')} {c.get('noise')} {c.get('mean')}: kernel/noise {ex:.2e} of the tolerance, "
          f"dy {ey:.1e}, logpdf {el:.1e}")
    return ex <= 1.0 and ey <= gc.DY_TOL and el <= gc.LP_TOL


def on(ctx, cases):
    """the same problems with their priors bound to ctx"""
    out = []
    for c in cases:
        f = c["fx"].f
        g = agp.GP(f.kernel, ctx=ctx) if f.mean_fn is None else agp.GP(f.mean_fn, f.kernel, ctx=ctx)
        out.append(dict(c, fx=agp.FiniteGP(g, c["fx"].x, c["fx"].sigma2)))
    return out


# ---- 1. ragged batch against the oracle and the single path -----------------------------------------------------------------------------------
def test_ragged_batch_against_the_oracle_and_the_single_path(agp, ctx, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_GRAD_MAX_N", "512")
    cases, refs = gc.ragged_with_oracle()
    served = sum(c["n"] <= 512 for c in cases)
    assert 0 < served < len(cases) and {1, 2, 63, 64, 65, 127, 128, 129, 545, 1000} <= {c["n"] for c in cases}  # both paths run
    before = ctx.get_param(COUNTER)
    lp, grads = call(cases)
    assert ctx.get_param(COUNTER) - before == served
    assert lp.dtype == np.float64 and len(grads) == len(cases)
    ok = True
    for b, c in enumerate(cases):
        g = grads[b]
        assert set(g) == {"variance", "scale", "noise", "y", "mean"} and g["y"].shape == (c["n"],)
        assert (g["scale"] is None) == (c["tr"] == "none") and np.shape(g["noise"]) == (() if c["noise"] == "scalar" else (c["n"],))
        ok &= report(f"problem {b} vs oracle:", c, lp[b], g, refs[b])
        ok &= report(f"problem {b} vs single:", c, lp[b], g, agp.logpdf_and_grad(c["fx"], c["y"]))
    assert ok


# ---- 2. the kernel at its limit ------------------------------------------------------------------------------------------------------------
def test_the_kernels_serve_every_size_up_to_their_own_limit(agp, ctx, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_GRAD_MAX_N", "2048")
    cases = [bc.make_case(1985, 2, "ard", 8, "rowvecs", "scalar", "custom", seed=91),
             bc.make_case(2048, 3, "scale", 3, "colvecs", "vector", "const", seed=92),
             bc.make_case(200, 0, "ard", 16, "rowvecs", "vector", "zero", seed=93)]
    before = ctx.get_param(COUNTER)
    lp, grads = call(cases)
    assert ctx.get_param(COUNTER) - before == 3
    lp2, grads2 = call(cases)
    ok = True
    for b, c in enumerate(cases):
        ok &= report("kernel-served", c, lp[b], grads[b], gc.oracle_grad(c))
        assert gc.same_bits(grads[b], grads2[b]) and lp[b].tobytes() == lp2[b].tobytes()  # a fixed schedule
    assert ok


# ---- 3. company changes nothing ------------------------------------------------------------------------------------------------------------
def test_a_problem_does_not_see_its_neighbours(agp, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_GRAD_MAX_N", "512")
    p = bc.make_case(200, 2, "ard", 3, "rowvecs", "vector", "custom", seed=77)
    lp0, (g0,) = call([p])
    assert report("alone", p, lp0[0], g0, gc.oracle_grad(p))
    others = bc.small_cases(699, seed=3)
    for total in (2, 64, 700):
        for pos in sorted({0, total // 2, total - 1}):
            batch = others[:total - 1]
            batch = batch[:pos] + [p] + batch[pos:]
            lp, grads = call(batch, on_error="nan")
            assert gc.same_bits(grads[pos], g0) and lp[pos].tobytes() == lp0[0].tobytes(), (total, pos)


# ---- 4. composite kernels ------------------------------------------------------------------------------------------------------------------
def test_composite_batch_against_a_host_gradient_and_a_mixed_call(agp, ctx, monkeypatch):
    """16 perturbed Mauna Loa kernels at n = 545, in both parametrisations the suite has: the example's own amplitudes (50² for the trend; K + Σy has a
    condition number near 1e9 — the analytic gradient must still match the host's) and tests/composite_ref.ml_kernel's amplitudes of order 1 over dense
    inputs.  The central differences are taken on the second family: a difference of two logpdf values carries their rounding error divided by 2h, and at
    h = 1e-5 a relative 1e-5 of a derivative of order 1 needs logpdf good to about 1e-10 ABSOLUTE, which only the well-conditioned family gives (measured on
    the first family: the analytic derivative agrees with the host gradient to 1e-11 while the difference quotient is off by up to 1.05e-5)."""
    monkeypatch.setenv("GPMI_BATCH_GRAD_MAX_N", "1024")  # the kernels serve n = 545 whatever the constant is
    ok = True
    for family, k0, (x, y) in (("example", mauna_loa_kernel(), bc.mauna_loa_data(545)), ("order-1", ml_kernel(), dense_data(545))):
        kernels = bc.perturbed_kernels(k0, 16)
        s2 = [1e-2 * agp.api._prior_variance(k) for k in kernels]
        fxs = [agp.GP(k)(x, s) for k, s in zip(kernels, s2)]
        before = ctx.get_param(COUNTER)
        lp, grads = agp.logpdf_and_grad_batch(fxs, y)
        assert ctx.get_param(COUNTER) - before == 16
        for b, k in enumerate(kernels):
            lp_h, g_h = gc.host_grad_composite(k, x, s2[b], y)
            g_h["kernel"] = agp.api._NormalForm(k).chain(g_h["theta"])
            assert set(grads[b]) == {"kernel", "theta", "noise", "y", "mean"}
            ok &= report(f"composite {family} {b}", {"n": 545}, lp[b], grads[b], (lp_h, g_h), COMP)
    assert ok
    # composite and single-kind priors in one mirror call (two ABI calls, merged in the caller's order): the same bits
    singles = bc.small_cases(3, seed=9)
    lps, gs_ = call(singles)
    mixed = [(fxs[0], y), (singles[0]["fx"], singles[0]["y"]), (fxs[3], y), (singles[1]["fx"], singles[1]["y"]), (singles[2]["fx"], singles[2]["y"]), (fxs[7], y)]
    lpm, gm = agp.logpdf_and_grad_batch([t[0] for t in mixed], [t[1] for t in mixed])
    for pos, b in ((0, 0), (2, 3), (5, 7)):
        assert gc.same_bits(gm[pos], grads[b]) and lpm[pos].tobytes() == lp[b].tobytes()
    for pos, s in ((1, 0), (3, 1), (4, 2)):
        assert gc.same_bits(gm[pos], gs_[s]) and lpm[pos].tobytes() == lps[s].tobytes()
    # along a direction in log-parameter space: central differences of agp.logpdf_batch
    h = 1e-5
    rng = np.random.default_rng(52)
    fds = []
    for b in (0, 5, 10, 15):
        p0 = agp.params(kernels[b])
        v = rng.standard_normal(len(p0))
        pm = agp.logpdf_batch([agp.GP(agp.with_params(kernels[b], p0 * np.exp(sg * h * v)))(x, s2[b]) for sg in (1, -1)], y)
        fd = (pm[0] - pm[1]) / (2 * h)
        an = float(np.dot(grads[b]["kernel"] * p0, v))
        print(f"composite {b}: directional derivative {an:.10e}, central difference {fd:.10e}, relative {abs(an - fd) / abs(fd):.1e}")
        fds.append((an, fd))
    for an, fd in fds:
        assert an == pytest.approx(fd, rel=1e-5)


def test_composite_theta_longer_than_one_pass_and_a_shared_parameter(agp, ctx, monkeypatch):
    """The kernel of test_gradient_longer_than_one_launch_and_a_shared_parameter at n = 200: a θ longer than one pass of 16 entries in batch_grad_kernel
    (29 entries: two passes) and a variance shared by two terms — `theta` and the chained `kernel`."""
    monkeypatch.setenv("GPMI_BATCH_GRAD_MAX_N", "512")
    SE, M32 = agp.SqExponentialKernel, agp.Matern32Kernel
    rng = np.random.default_rng(41)
    X = rng.uniform(0, 3, size=(200, 4))
    y = np.cos(X[:, 0]) + 0.1 * rng.standard_normal(200)
    k = (0.9 * (SE() @ agp.ARDTransform([0.6, 0.7, 0.8, 0.9]) + M32() @ agp.ARDTransform([0.5, 0.4, 0.3, 0.6]))
         * (agp.PeriodicKernel(r=[1.0, 1.1, 1.2, 1.3]) @ agp.ARDTransform([0.3, 0.2, 0.25, 0.35]))
         + 0.2 * agp.RationalQuadraticKernel(alpha=0.8) @ agp.ScaleTransform(0.9))
    nf = agp.api._NormalForm(k)
    assert len(nf.theta()) == 29 > 16
    lp_h, g_h = gc.host_grad_composite(k, X, 0.1, y)
    g_h["kernel"] = nf.chain(g_h["theta"])
    before = ctx.get_param(COUNTER)
    lp, (g,) = agp.logpdf_and_grad_batch([agp.GP(k)(agp.RowVecs(X), 0.1)], [y])
    assert ctx.get_param(COUNTER) - before == 1
    assert g["theta"].shape == (29,) and g["kernel"].shape == (len(nf.params),)
    assert report("29 theta entries", {"n": 200}, lp[0], g, (lp_h, g_h), COMP)


# ---- 5. failures are per problem ------------------------------------------------------------------------------------------------------------
def test_failures_are_per_problem(agp, ctx, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_GRAD_MAX_N", "512")
    good = bc.small_cases(24, seed=6, lo=40)
    big = bc.make_case(600, 1, "ard", 3, "rowvecs", "vector", "const", seed=61)  # above the limit: fails on the single path
    good.append(big)
    lp_good, g_good = call(good)
    bad = list(good)
    expect = {}
    for b, at in ((3, 0.4), (17, 0.9), (24, 0.5)):
        c = good[b]
        s2 = np.array(np.broadcast_to(c["s2"], (c["n"],)), dtype=np.float64)
        i = int(at * (c["n"] - 1))
        s2[i] = -10.0
        bad[b] = dict(c, fx=agp.FiniteGP(c["fx"].f, c["fx"].x, s2))
        expect[b] = i + 1
    lp, grads = call(bad, on_error="nan")
    assert sorted(np.flatnonzero(np.isnan(lp)).tolist()) == [3, 17, 24]
    for b in range(25):
        if b in expect:
            assert gc.all_nan(grads[b]) and grads[b]["y"].shape == (good[b]["n"],) and np.shape(grads[b]["noise"]) == (good[b]["n"],), b
        elif b < 24:
            assert gc.same_bits(grads[b], g_good[b]) and lp[b].tobytes() == lp_good[b].tobytes(), b
    # the info of every problem, straight from the ABI
    (g,) = agp.api._batch_groups([c["fx"] for c in bad], [c["y"] for c in bad])
    gcall = agp.api._grad_batch_marshal(g)
    assert getattr(ctx.lib, gcall.entry)(ctx.handle, *gcall.args) == 0  # a failing problem is data, not a status
    assert {b: int(gcall.info[b]) for b in np.flatnonzero(gcall.info)} == expect
    with pytest.raises(agp.PosDefException) as e:
        call(bad)
    assert (e.value.index, e.value.info) == (3, expect[3])


# ---- 6. recycled blocks -----------------------------------------------------------------------------------------------------------------------
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


def test_nothing_depends_on_what_a_recycled_block_held(agp, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_GRAD_MAX_N", "512")
    cases = bc.small_cases(40, seed=14) + [bc.make_case(n, 2, "ard", 3, "rowvecs", "vector", "const", seed=140 + n) for n in (1, 63, 65, 129, 321)]
    x, y = bc.mauna_loa_data(150)
    comp = [dict(fx=agp.GP(k)(x, 1e-2 * agp.api._prior_variance(k)), y=y) for k in bc.perturbed_kernels(mauna_loa_kernel(), 3)]
    results = []
    with _poisoned_and_clean() as ctxs:
        for c in ctxs:
            for batch in (on(c, cases), on(c, comp)):
                blocks0 = c.get_param("pool_blocks")
                first = call(batch)
                cached = (c.get_param("pool_cached_mb"), c.get_param("pool_blocks"))
                second = call(batch)
                assert (c.get_param("pool_cached_mb"), c.get_param("pool_blocks")) == cached  # the second call runs in the first one's blocks
                assert first[0].tobytes() == second[0].tobytes() and all(gc.same_bits(p, q) for p, q in zip(first[1], second[1]))
                assert c.get_param("pool_blocks") >= 3  # after the call every block is back in the cache ...
                c.trim()
                assert c.get_param("pool_blocks") == blocks0 == 0  # ... and nothing is held after the trim
                results.append(first)
            assert c.get_param(COUNTER) == 2 * (len(cases) + len(comp))
    for (lp_p, g_p), (lp_c, g_c) in zip(results[:2], results[2:]):  # poisoned against clean
        assert np.isfinite(lp_p).all() and lp_p.tobytes() == lp_c.tobytes()
        assert all(gc.same_bits(p, q) for p, q in zip(g_p, g_c))
        assert all(np.isfinite(gc.entries(p, list(p))).all() for p in g_p)
    for b in (0, 41, 44):
        assert report("recycled", cases[b], results[0][0][b], results[0][1][b], gc.oracle_grad(cases[b]))


# ---- 7. argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_have_their_statuses_and_reasons(agp, ctx):
    cases = [bc.make_case(n, 2, tr, 3, "rowvecs", "vector", "const", seed=700 + n) for n, tr in ((20, "ard"), (31, "none"), (12, "scale"))]
    (g,) = agp.api._batch_groups([c["fx"] for c in cases], [c["y"] for c in cases])
    gcall = agp.api._grad_batch_marshal(g)
    fn = ctx.lib.gp_logpdf_grad_batch
    good = list(gcall.args)
    NB, K, NX, X, NZ, M, NY, Y, LP, INFO, DVAR, DS, DN, DY = range(14)
    outs = [gcall.out, gcall.dvar] + [a for a in gcall.dscale if a is not None] + gcall.dnoise + gcall.dy

    def status(fn=fn, good=good, **broken):
        args = list(good)
        for name, v in broken.items():
            args[{"nb": NB, "k": K, "nx": NX, "x": X, "nz": NZ, "ny": NY, "y": Y, "lp": LP, "info": INFO, "dvar": DVAR, "ds": DS, "dn": DN, "dy": DY}[name]] = v
        rc = fn(ctx.handle, *args)
        return rc, ctx.lib.gp_last_error().decode()

    def sentinel():
        for a in outs:
            a[...] = 123.0

    def untouched():
        return all(np.all(a == 123.0) for a in outs)

    sentinel()
    assert fn(ctx.handle, 0, None, 0, None, None, None, 0, None, None, None, None, None, None, None) == 0  # nb = 0 touches nothing
    assert status(nb=0)[0] == 0 and untouched()
    y_null = (C.c_void_p * 3)(good[Y][0], None, good[Y][2])
    ds_null = (C.c_void_p * 3)(None, None, good[DS][2])  # problem 0 has three scales
    dn_null = (C.c_void_p * 3)(good[DN][0], None, good[DN][2])
    dy_null = (C.c_void_p * 3)(good[DY][0], good[DY][1], None)
    k_mixed = (type(good[K][0]) * 3)(*good[K])
    k_mixed[1].dtype = 1
    rows = [  # the arguments gp_logpdf_batch has: its numbers and reasons
        (dict(nb=-1), -2, "nb"), (dict(k=None), -3, "kernel array is NULL"), (dict(k=k_mixed), -3, "dtype"), (dict(nx=2), -4, "nx"),
        (dict(x=None), -5, "points array is NULL"), (dict(nz=None), -6, "noise array is NULL"), (dict(ny=2), -8, "ny"), (dict(y=None), -9, "y array is NULL"),
        (dict(y=y_null), -9, "a y pointer is NULL"), (dict(lp=None), -10, "logpdf_out is NULL"), (dict(info=None), -11, "info_out is NULL"),
        # the new ones
        (dict(ds=ds_null), -13, "a dscale_out pointer is NULL where the kernel has scales"), (dict(dn=dn_null), -14, "a dnoise_out pointer is NULL"),
        (dict(dy=dy_null), -15, "a dy_out pointer is NULL")]
    for broken, rc, text in rows:
        got, why = status(**broken)
        assert got == rc and why.startswith(f"invalid argument {-rc}: ") and text in why, (list(broken), got, why)
        assert untouched(), list(broken)  # no refused call wrote a result
    assert fn(None, *good) == -1 and "not a live gp_ctx" in ctx.lib.gp_last_error().decode()
    # the composite entry point counts its arguments itself
    x, y = bc.mauna_loa_data(40)
    kern = bc.perturbed_kernels(mauna_loa_kernel(), 2)
    (gs_,) = agp.api._batch_groups([agp.GP(k)(x, 0.5) for k in kern], y)
    sc = agp.api._grad_batch_marshal(gs_)
    fs, sgood = ctx.lib.gp_logpdf_grad_batch_sum, list(sc.args)
    for idx, rc, text in ((10, -12, "a dtheta_out pointer is NULL"), (11, -13, "a dnoise_out pointer is NULL"), (12, -14, "a dy_out pointer is NULL")):
        args = list(sgood)
        args[idx] = (C.c_void_p * 2)(sgood[idx][0], None)
        assert fs(ctx.handle, *args) == rc
        why = ctx.lib.gp_last_error().decode()
        assert why.startswith(f"invalid argument {-rc}: ") and text in why, why
    assert fs(ctx.handle, *sgood) == 0 and np.isfinite(sc.out).all() and all(np.isfinite(a).all() for a in sc.dtheta)
    # legal: every gradient array may be NULL on its own, and a dscale_out entry where the kernel has no scales
    assert status(dvar=None, ds=None, dn=None, dy=None)[0] == 0 and all(np.all(a == 123.0) for a in outs[1:]) and np.all(gcall.out != 123.0)
    assert good[DS][1] is None and status()[0] == 0
    ok = True
    for b, c in enumerate(cases):
        sc_ = gcall.dscale[b]
        got = {"variance": float(gcall.dvar[b]), "scale": None if sc_ is None else (float(sc_[0]) if sc_.shape[0] == 1 else sc_), "noise": gcall.dnoise[b],
               "y": gcall.dy[b], "mean": -gcall.dy[b]}
        ok &= report("abi", c, gcall.out[b], got, gc.oracle_grad(c))
    assert ok
