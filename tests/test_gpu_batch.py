"""GPU: gp_logpdf_batch / gp_logpdf_batch_sum (csrc/batch.hip) through agp.logpdf_batch — many small exact GPs in one call.
Tolerances are the project's own for fp64 exact fits: logpdf 1e-10 relative to max(|reference|, 1), α 1e-8 in the 2-norm."""
import ctypes as C

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import batch_cases as bc
from tests.composite_ref import mauna_loa_kernel, ref_kernelmatrix

pytestmark = pytest.mark.gpu

LP_TOL, A_TOL = 1e-10, 1e-8


def _call(cases, **kw):
    return agp.logpdf_batch([c["fx"] for c in cases], [c["y"] for c in cases], **kw)


# ---- 1 / 2. parity with the oracle and with the single path, ragged batch ----------------------------------------------------------------
def test_ragged_batch_against_the_oracle_and_the_single_path(agp):
    cases = bc.ragged_cases()
    assert len(cases) >= 32
    lp, alphas = _call(cases, return_alpha=True)
    lp_only = _call(cases)
    served = np.array([c["n"] <= agp._lib.batch_max_n() for c in cases])
    assert served.sum() >= 24 and not served.all()  # both paths inside one call
    assert lp.dtype == np.float64 and np.array_equal(lp[served], lp_only[served])  # the kernel's schedule is fixed; the routed problems repeat to rounding
    assert all(bc.lp_err(u, v) <= LP_TOL for u, v in zip(lp[~served], lp_only[~served]))
    worst = [0.0, 0.0, 0.0]
    for b, c in enumerate(cases):
        lp_o, a_o = bc.oracle_fit(c)
        e_lp, e_a = bc.lp_err(lp[b], lp_o), bc.vec_err(alphas[b], a_o)
        e_single = bc.lp_err(lp[b], agp.logpdf(c["fx"], c["y"]))
        worst = [max(w, e) for w, e in zip(worst, (e_lp, e_a, e_single))]
        print(f"problem {b}: n={c['n']} kind={c['kind']} {c['tr']} D={c['d']} {c['container']} {c['noise']} {c['mean']}: "
              f"logpdf {e_lp:.1e} alpha {e_a:.1e} vs single {e_single:.1e}")
        assert alphas[b].shape == (c["n"],)
        assert e_lp <= LP_TOL and e_a <= A_TOL and e_single <= LP_TOL, (b, c["n"], e_lp, e_a, e_single)
    print(f"worst: logpdf {worst[0]:.1e} alpha {worst[1]:.1e} vs single path {worst[2]:.1e}")


def test_the_kernel_serves_every_size_up_to_its_own_limit(agp, monkeypatch):
    """GPMI355_BATCH_MAX_N routes the larger problems of the ragged batch to the single path; with the library's measurement override
    (environment GPMI_BATCH_MAX_N, read per call) the batch kernel takes them all, n = 2 048 included — same bounds."""
    monkeypatch.setenv("GPMI_BATCH_MAX_N", "2048")
    cases = [c for c in bc.ragged_cases() if c["n"] > 500] + [bc.make_case(2048, 3, "scale", 3, "rowvecs", "vector", "const", seed=99),
                                                               bc.make_case(1985, 0, "ard", 8, "colvecs", "scalar", "custom", seed=98)]
    lp, alphas = _call(cases, return_alpha=True)
    lp2, alphas2 = _call(cases, return_alpha=True)
    for b, c in enumerate(cases):
        lp_o, a_o = bc.oracle_fit(c)
        print(f"kernel-served n={c['n']}: logpdf {bc.lp_err(lp[b], lp_o):.1e} alpha {bc.vec_err(alphas[b], a_o):.1e}")
        assert bc.lp_err(lp[b], lp_o) <= LP_TOL and bc.vec_err(alphas[b], a_o) <= A_TOL
        assert lp[b].tobytes() == lp2[b].tobytes() and alphas[b].tobytes() == alphas2[b].tobytes()  # the kernel's schedule is fixed: same bits


# ---- 3. a problem does not see its neighbours ------------------------------------------------------------------------------------------
def test_a_problem_does_not_see_its_neighbours(agp):
    p = bc.make_case(200, 2, "ard", 3, "rowvecs", "vector", "custom", seed=77)
    assert p["n"] <= agp._lib.batch_max_n()
    lp0, (a0,) = _call([p], return_alpha=True)
    lp_o, a_o = bc.oracle_fit(p)
    assert bc.lp_err(lp0[0], lp_o) <= LP_TOL and bc.vec_err(a0, a_o) <= A_TOL
    others = bc.small_cases(699, seed=3)
    for total in (2, 64, 700):
        for pos in sorted({0, total // 2, total - 1}):
            batch = others[:total - 1]
            batch = batch[:pos] + [p] + batch[pos:]
            for rep in range(2):
                lp, al = _call(batch, return_alpha=True, on_error="nan")
                assert lp[pos].tobytes() == lp0[0].tobytes() and al[pos].tobytes() == a0.tobytes(), (total, pos, rep)


# ---- 4. shared inputs ------------------------------------------------------------------------------------------------------------------------
def test_shared_inputs_are_sent_once_and_change_nothing(agp):
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 4, size=(333, 3))
    x, y = agp.RowVecs(X), rng.standard_normal(333)
    ks = [(0.8 + 0.02 * b) * [agp.SqExponentialKernel, agp.Matern32Kernel][b % 2]() @ agp.ScaleTransform(0.5 + 0.01 * b) for b in range(64)]
    shared = [agp.GP(k)(x, 0.02) for k in ks]
    (g,) = agp.api._batch_groups(shared, y)
    call = agp.api._batch_marshal(g, True)
    assert (call.nb, call.nx, call.ny, call.args[2], call.args[6], len(call.args[3]), len(call.args[7])) == (64, 1, 1, 1, 1, 1, 1)
    repeated = [agp.GP(k)(agp.RowVecs(X.copy()), 0.02) for k in ks]
    (g2,) = agp.api._batch_groups(repeated, [y.copy() for _ in ks])
    assert (g2.nx, g2.ny) == (64, 64)
    lp1, a1 = agp.logpdf_batch(shared, y, return_alpha=True)
    lp2, a2 = agp.logpdf_batch(repeated, [y.copy() for _ in ks], return_alpha=True)
    assert lp1.tobytes() == lp2.tobytes() and all(u.tobytes() == v.tobytes() for u, v in zip(a1, a2))
    for b in (0, 17, 63):
        assert bc.lp_err(lp1[b], agp.logpdf(shared[b], y)) <= LP_TOL


# ---- 5. composite kernels ------------------------------------------------------------------------------------------------------------------
def test_composite_batch_and_a_mixed_call_against_a_host_cholesky(agp):
    x, y = bc.mauna_loa_data(545)
    kernels = bc.perturbed_kernels(mauna_loa_kernel(), 16)
    s2 = [1e-2 * agp.api._prior_variance(k) for k in kernels]
    fxs = [agp.GP(k)(x, s) for k, s in zip(kernels, s2)]
    lp, al = agp.logpdf_batch(fxs, y, return_alpha=True)
    for b, k in enumerate(kernels):
        lp_h, a_h = bc.host_fit(ref_kernelmatrix(k, x) + s2[b] * np.eye(545), y)
        print(f"composite {b}: logpdf {bc.lp_err(lp[b], lp_h):.1e} alpha {bc.vec_err(al[b], a_h):.1e}")
        assert bc.lp_err(lp[b], lp_h) <= LP_TOL and bc.vec_err(al[b], a_h) <= A_TOL
    # composite and single-kind priors in one mirror call (two ABI calls, merged in the caller's order)
    singles = bc.small_cases(5, seed=9)
    mixed_fx = [fxs[0], singles[0]["fx"], fxs[3], singles[1]["fx"], singles[2]["fx"], fxs[7], singles[3]["fx"], singles[4]["fx"]]
    mixed_y = [y, singles[0]["y"], y, singles[1]["y"], singles[2]["y"], y, singles[3]["y"], singles[4]["y"]]
    lpm, alm = agp.logpdf_batch(mixed_fx, mixed_y, return_alpha=True)
    for pos, b in ((0, 0), (2, 3), (5, 7)):
        assert lpm[pos].tobytes() == lp[b].tobytes() and alm[pos].tobytes() == al[b].tobytes()
    for pos, s in ((1, 0), (3, 1), (4, 2), (6, 3), (7, 4)):
        lp_o, a_o = bc.oracle_fit(singles[s])
        assert bc.lp_err(lpm[pos], lp_o) <= LP_TOL and bc.vec_err(alm[pos], a_o) <= A_TOL


# ---- 6. failures are per problem ----------------------------------------------------------------------------------------------------------
def test_failures_are_per_problem(agp):
    good = bc.small_cases(64, seed=6, lo=40)
    lp_good, a_good = _call(good, return_alpha=True)
    bad = list(good)
    expect = {}
    for b, at in ((3, 0.4), (40, 0.9)):
        c = good[b]
        s2 = np.array(np.broadcast_to(c["s2"], (c["n"],)), dtype=np.float64)
        i = int(at * (c["n"] - 1))
        s2[i] = -10.0
        fx = agp.FiniteGP(c["fx"].f, c["fx"].x, s2)
        bad[b] = dict(c, fx=fx)
        with pytest.raises(agp.PosDefException) as e:
            agp.logpdf(fx, c["y"])
        expect[b] = e.value.info
        assert e.value.info == i + 1
    groups = agp.api._batch_groups([c["fx"] for c in bad], [c["y"] for c in bad])
    lp, al = _call(bad, return_alpha=True, on_error="nan")
    assert sorted(np.flatnonzero(np.isnan(lp)).tolist()) == [3, 40]
    assert all(np.isnan(al[b]).all() for b in (3, 40))
    for b in range(64):
        if b not in (3, 40):
            assert lp[b].tobytes() == lp_good[b].tobytes() and al[b].tobytes() == a_good[b].tobytes(), b
    # the info of every problem, straight from the ABI
    (g,) = groups
    call = agp.api._batch_marshal(g, False)
    ctx = agp.default_context()
    assert getattr(ctx.lib, call.entry)(ctx.handle, *call.args) == 0
    assert {b: int(call.info[b]) for b in np.flatnonzero(call.info)} == expect
    with pytest.raises(agp.PosDefException) as e:
        _call(bad)
    assert (e.value.index, e.value.info) == (3, expect[3])


# ---- 7. routing ------------------------------------------------------------------------------------------------------------------------------
def test_problems_the_kernel_does_not_take_are_answered_by_the_single_path(agp):
    big_n = agp._lib.batch_max_n() + 128
    small = bc.make_case(300, 0, "scale", 3, "rowvecs", "scalar", "const", seed=70)
    big = bc.make_case(big_n, 3, "ard", 3, "colvecs", "vector", "zero", seed=71)
    f32 = bc.make_case(400, 2, "scale", 3, "rowvecs", "scalar", "zero", seed=72, dtype=np.float32)
    dn = bc.make_case(350, 1, "none", 3, "rowvecs", "scalar", "custom", seed=73)
    rng = np.random.default_rng(74)
    G = rng.standard_normal((350, 350))
    S = 0.05 * np.eye(350) + 1e-3 * (G @ G.T) / 350
    dn = dict(dn, fx=agp.FiniteGP(dn["fx"].f, dn["fx"].x, S))
    cases = [small, big, f32, dn]
    lp, al = _call(cases, return_alpha=True)
    assert lp.dtype == np.float64 and al[2].dtype == np.float32
    for b in (0, 1):
        lp_o, a_o = bc.oracle_fit(cases[b])
        assert bc.lp_err(lp[b], lp_o) <= LP_TOL and bc.vec_err(al[b], a_o) <= A_TOL
    lp_o, a_o = bc.oracle_fit(f32)  # the fp64 oracle on the fp32 inputs: what tests/test_gpu_parity.py accepts for an fp32 logpdf
    assert bc.lp_err(lp[2], lp_o) <= 1e-4
    m, Cm = bc.o.mean_and_cov(dn["ofx"])
    Cm = Cm - np.diag(np.broadcast_to(dn["s2"], (350,))) + S
    lp_h, a_h = bc.host_fit(Cm, dn["y"] - m)
    assert bc.lp_err(lp[3], lp_h) <= LP_TOL and bc.vec_err(al[3], a_h) <= A_TOL
    # the path depends on the problem alone: alone, the kernel-served problem returns the same bits; the routed ones take the single path again, whose default
    # schedule (stream-K tails) repeats to rounding, not to the bit
    for b, c in enumerate(cases):
        lp1 = _call([c])
        if b == 0:
            assert float(lp1[0]) == float(lp[b])
        else:
            assert bc.lp_err(lp1[0], lp[b]) <= (1e-4 if b == 2 else LP_TOL)


# ---- 8. waves ----------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_larger_than_one_launch_runs_in_waves_and_returns_its_memory(agp, ctx):
    B, n = 3000, 64  # more than the 2 048 problems one launch takes
    rng = np.random.default_rng(8)
    X = rng.uniform(0, 4, size=(B, n, 2))
    Y = rng.standard_normal((B, n))
    kinds = [agp.SqExponentialKernel, agp.Matern12Kernel, agp.Matern32Kernel, agp.Matern52Kernel]
    fxs = [agp.GP((1.0 + 1e-4 * b) * kinds[b % 4]() @ agp.ScaleTransform(0.7))(agp.RowVecs(X[b]), 0.02) for b in range(B)]
    ys = [Y[b] for b in range(B)]
    lp_warm = agp.logpdf_batch(fxs, ys)  # the first call of a shape brings its blocks into the ctx's cache
    before = (ctx.get_param("pool_cached_mb"), ctx.get_param("pool_blocks"))
    lp = agp.logpdf_batch(fxs, ys)
    assert (ctx.get_param("pool_cached_mb"), ctx.get_param("pool_blocks")) == before
    assert lp.tobytes() == lp_warm.tobytes()
    worst = 0.0
    for b in range(B):
        ofx = bc.o.FiniteGP(bc.o.GP(bc.o.Kernel(b % 4, 1.0 + 1e-4 * b, 0.7)), X[b], 0.02)
        worst = max(worst, bc.lp_err(lp[b], bc.o.logpdf(ofx, Y[b])))
    print(f"3000 problems of n = 64 in two waves: worst logpdf error {worst:.1e}")
    assert worst <= LP_TOL


# ---- 9. argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_have_their_statuses_and_reasons(agp, ctx):
    cases = bc.small_cases(3, seed=12)
    (g,) = agp.api._batch_groups([c["fx"] for c in cases], [c["y"] for c in cases])
    call = agp.api._batch_marshal(g, True)
    fn = ctx.lib.gp_logpdf_batch
    nb, karr, nx, pts, narr, marr, ny, yarr, out, info, aarr = call.args

    def status(*args):
        rc = fn(ctx.handle, *args)
        return rc, ctx.lib.gp_last_error().decode()

    call.out[:] = 123.0
    assert fn(ctx.handle, 0, None, 0, None, None, None, 0, None, None, None, None) == 0  # nb = 0 touches nothing
    assert fn(ctx.handle, 0, karr, nx, pts, narr, marr, ny, yarr, out, info, aarr) == 0 and np.all(call.out == 123.0)
    rc, why = status(-1, karr, nx, pts, narr, marr, ny, yarr, out, info, aarr)
    assert rc == -2 and "nb" in why
    rc, why = status(nb, karr, 2, pts, narr, marr, ny, yarr, out, info, aarr)
    assert rc == -4 and "nx" in why
    rc, why = status(nb, karr, nx, pts, narr, marr, 2, yarr, out, info, aarr)
    assert rc == -8 and "ny" in why
    ynull = (C.c_void_p * 3)(yarr[0], None, yarr[2])
    rc, why = status(nb, karr, nx, pts, narr, marr, ny, ynull, out, info, aarr)
    assert rc == -9 and "NULL" in why
    rc, why = status(nb, karr, nx, pts, narr, marr, ny, None, out, info, aarr)
    assert rc == -9
    kmixed = (type(karr[0]) * 3)(karr[0], karr[1], karr[2])
    kmixed[1].dtype = 1
    rc, why = status(nb, kmixed, nx, pts, narr, marr, ny, yarr, out, info, aarr)
    assert rc == -3 and "dtype" in why
    assert np.all(call.out == 123.0)  # none of the refused calls wrote a result
    assert fn(ctx.handle, nb, karr, nx, pts, narr, marr, ny, yarr, out, info, aarr) == 0
    for b, c in enumerate(cases):
        assert bc.lp_err(call.out[b], bc.oracle_fit(c)[0]) <= LP_TOL
