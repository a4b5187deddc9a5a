"""GPU: gp_predict_grad_batch / gp_predict_grad_batch_sum (csrc/batch.hip: batch_logpdf_kernel, batch_inv_kernel, then per launch group
batch_predict_kernel and batch_pgrad_kernel behind it) through agp.mean_and_var_grad_batch — predictive mean and variance of many small exact GPs AND
their gradients w.r.t. the test inputs, in one call.
Tolerances are the project's own.  Values: mean 1e-8 absolute, var 1e-9 absolute, logpdf 1e-10 relative to max(|reference|, 1).
Gradients (tests/test_gpu_predict_grad.py, fp64): rtol 1e-7, atol 1e-8·max(1, max|g_ref|), g_ref from the fp64 host reference
(tests/predict_grad_ref.HostPosterior; tests/test_batch_predict_grad_cpu.py pins it to central differences and to the device's S form).
Worst errors measured over the ragged batch on an MI355X (test 1 prints them): against the host reference dmean 2.6e-12 absolute
(5.6e-5 of the tolerance), dvar 7.2e-15 (6.3e-7 of the tolerance), mean 1.3e-12, var 6.2e-15, logpdf 1.1e-14; against the single path dmean 1.4e-12, dvar 4.7e-15,
mean 1.4e-12, var 4.2e-15; n = 2 048 under the kernels' own limit: dmean 6.1e-12 (1.5e-4 of the tolerance), dvar 9.6e-15."""
import ctypes as C

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import batch_cases as bc
from tests import batch_pgrad_cases as pg
from tests.composite_dx_ref import many_dim_kernel
from tests.composite_ref import dense_data, ml_kernel, ref_kernelmatrix
from tests.predict_grad_ref import HostPosterior
from tests.test_gpu_batch_predict import LAUNCH_POINTS, LP_TOL, M_TOL, V_TOL, _poisoned_and_clean, _tiny_batch, errs, on, oracle_predict, with_points

pytestmark = pytest.mark.gpu

COUNTER = "batch_pgrad_kernel_problems"


def call(cases, **kw):
    kw.setdefault("mean_grads", [pg.mean_grad_of(c) for c in cases])
    return agp.mean_and_var_grad_batch([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases], **kw)


def rows_of(case, g):
    """a gradient in the shape of the case's container as (ns, d) rows"""
    if case["container"] == "vector":
        return g[:, None]
    return g.T if case["container"] == "colvecs" else g


def g_err(g, g_ref):
    """worst error of a gradient in units of its tolerance (<= 1 passes), and absolute"""
    if g_ref.size == 0:
        return 0.0, 0.0
    e = np.abs(g - g_ref)
    return float(np.max(e / pg.g_bound(g_ref))), float(e.max())


def same_bits(p, q):
    return all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(p, q))


def counter(ctx=None):
    return (ctx or agp.default_context()).get_param(COUNTER)


def raw(cases, what=3):
    """the marshalled ABI call of one group of cases"""
    (g,) = agp.api._predict_groups([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases])
    return agp.api._predict_grad_marshal(g, what)


# ---- 1. ragged batch against the host reference and the single path ---------------------------------------------------------------------------
def test_ragged_batch_against_the_host_reference_and_the_single_path(agp):
    cases, refs = pg.ragged_cases(), pg.ragged_refs()
    assert all(c["n"] <= agp._lib.batch_pgrad_max_n() for c in cases)  # every problem goes to the kernels
    assert {c["ns"] for c in cases[:-1]} == set(pg.NS) and {c["n"] for c in cases[:-1]} == set(pg.SIZES) and cases[-1]["d"] == 16
    assert {c["kind"] for c in cases} == {0, 1, 2, 3} and {c["tr"] for c in cases} == set(bc.TRANSFORMS) and {c["mean"] for c in cases} == set(bc.MEANS)
    assert {c["container"] for c in cases} == set(bc.CONTAINERS) and {c["noise"] for c in cases} == set(bc.NOISES) and {1, 3, 8} <= {c["d"] for c in cases}
    n0 = counter()
    quads, lp = call(cases, return_logpdf=True)
    assert counter() - n0 == len(cases)
    pairs, lp_p = agp.mean_and_var_batch([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases], return_logpdf=True)
    worst = [0.0] * 11
    for b, c in enumerate(cases):
        m, v, dm, dv = quads[b]
        assert m.shape == v.shape == (c["ns"],) and dm.shape == dv.shape == np.shape(c["xs"].X if hasattr(c["xs"], "X") else c["xs"]) and dm.dtype == np.float64
        # mean / var / logpdf: the bits of mean_and_var_batch (the same kernels compute them)
        assert m.tobytes() == pairs[b][0].tobytes() and v.tobytes() == pairs[b][1].tobytes() and lp[b].tobytes() == lp_p[b].tobytes(), b
        em, ev, el = errs((m, v), lp[b], refs[b][0])
        gm, gv = refs[b][1]
        if c["mean"] == "custom" and c["ns"]:
            gm = gm + 0.3
        (tm, am), (tv, av) = g_err(rows_of(c, dm), gm), g_err(rows_of(c, dv), gv)
        sm = sv = sdm = sdv = 0.0
        if c["ns"]:  # gp_posterior_fit + gp_posterior_predict_grad on the same inputs
            m1, v1, dm1, dv1 = agp.posterior(c["fx"], c["y"]).mean_and_var_grad(c["xs"], mean_grad=pg.mean_grad_of(c))
            sm, sv = float(np.max(np.abs(m - m1))), float(np.max(np.abs(v - v1)))
            (tsm, sdm), (tsv, sdv) = g_err(dm, dm1), g_err(dv, dv1)
            assert tsm <= 1.0 and tsv <= 1.0, (b, tsm, tsv)
        print(f"problem {b}: n={c['n']} ns={c['ns']} kind={c['kind']} {c['tr']} D={c['d']} {c['container']} {c['noise']} {c['mean']}: mean {em:.1e} var {ev:.1e} "
              f"logpdf {el:.1e} dmean {am:.1e} ({tm:.1e} of tol) dvar {av:.1e} ({tv:.1e} of tol); vs single path mean {sm:.1e} var {sv:.1e} dmean {sdm:.1e} dvar {sdv:.1e}")
        worst = [max(w, e) for w, e in zip(worst, (em, ev, el, am, tm, av, tv, sm, sv, sdm, sdv))]
        assert np.isfinite(dm).all() and np.isfinite(dv).all()
        assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL and tm <= 1.0 and tv <= 1.0 and sm <= M_TOL and sv <= V_TOL, (b, c["n"], c["ns"], em, ev, el, tm, tv, sm, sv)
    print("worst: mean %.1e var %.1e logpdf %.1e dmean %.1e (%.1e of tol) dvar %.1e (%.1e of tol); vs single path mean %.1e var %.1e dmean %.1e dvar %.1e" % tuple(worst))
    # one side at a time: the same bits as with both
    for what, keep in ((1, (0, 2)), (2, (1, 3))):
        one = call(cases, what=what)
        for p, q in zip(one, quads):
            assert all(p[i] is None for i in range(4) if i not in keep) and all(p[i].tobytes() == q[i].tobytes() for i in keep)
    # values only and gradients only, through the ABI: the same bits
    ctx = agp.default_context()
    NBUF = {"values": (12, 13), "gradients": (14, 15)}
    for dropped, keep in (("gradients", ("means", "vars")), ("values", ("dmeans", "dvars"))):
        pc = raw(cases)
        args = list(pc.args)
        for i in NBUF[dropped]:
            args[i] = None
        assert getattr(ctx.lib, pc.entry)(ctx.handle, *args) == 0
        full = raw(cases)
        assert getattr(ctx.lib, full.entry)(ctx.handle, *full.args) == 0
        for name in keep:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(getattr(pc, name), getattr(full, name))), (dropped, name)
        assert pc.out.tobytes() == full.out.tobytes()


# ---- 2. the kernels' own limit ------------------------------------------------------------------------------------------------------------
def test_the_kernels_serve_every_size_up_to_their_own_limit(agp, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_PGRAD_MAX_N", "2048")
    cases = pg.limit_cases()
    n0 = counter()
    quads, lp = call(cases, return_logpdf=True)
    quads2 = call(cases)
    assert counter() - n0 == 2 * len(cases)
    for b, c in enumerate(cases):
        em, ev, el = errs(quads[b][:2], lp[b], oracle_predict(c))
        gm, gv = pg.host_grads(c)
        if c["mean"] == "custom":
            gm = gm + 0.3
        (tm, am), (tv, av) = g_err(rows_of(c, quads[b][2]), gm), g_err(rows_of(c, quads[b][3]), gv)
        print(f"kernel-served n={c['n']}: mean {em:.1e} var {ev:.1e} logpdf {el:.1e} dmean {am:.1e} ({tm:.1e} of tol) dvar {av:.1e} ({tv:.1e} of tol)")
        assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL and tm <= 1.0 and tv <= 1.0
        assert same_bits(quads[b], quads2[b])  # a fixed schedule


# ---- 3. company changes nothing --------------------------------------------------------------------------------------------------------------
def test_a_problem_does_not_see_its_neighbours(agp):
    p = with_points(bc.make_case(200, 2, "ard", 3, "rowvecs", "vector", "custom", seed=77), 70, seed=177)
    (quad0,), lp0 = call([p], return_logpdf=True)
    gm, gv = pg.host_grads(p)
    assert g_err(quad0[2], gm + 0.3)[0] <= 1.0 and g_err(quad0[3], gv)[0] <= 1.0
    others = [with_points(c, 1 + b % 7, seed=500 + b) for b, c in enumerate(bc.small_cases(300, seed=3))]
    for total in (2, 64, 301):
        for pos in sorted({0, total // 2, total - 1}):
            batch = others[:total - 1]
            batch = batch[:pos] + [p] + batch[pos:]
            quads, lp = call(batch, return_logpdf=True, on_error="nan")
            assert same_bits(quads[pos], quad0) and lp[pos].tobytes() == lp0[0].tobytes(), (total, pos)


# ---- 4. a test point does not see the others ----------------------------------------------------------------------------------------------------
def test_a_test_point_does_not_see_the_other_test_points(agp):
    """Each row's arithmetic touches no other row (the weights of a row are one row of the MFMA tiles, its sums one wave's): a difference here is a padding
    leak.  Alone, at any position among 200 others (two tiles), and on either side of the split into two predict launches."""
    c = bc.make_case(200, 3, "scale", 3, "rowvecs", "scalar", "const", seed=78)
    rng = np.random.default_rng(79)
    pt = rng.uniform(0.0, 4.0, size=(1, 3)) / np.sqrt(3)
    (alone,) = call([dict(c, xs=agp.RowVecs(pt), ns=1)])
    others = rng.uniform(0.0, 4.0, size=(200, 3)) / np.sqrt(3)
    for pos in (0, 1, 31, 32, 100, 127, 128, 199, 200):
        XS = np.concatenate([others[:pos], pt, others[pos:]])
        (quad,) = call([dict(c, xs=agp.RowVecs(XS), ns=201)])
        assert all(quad[i][pos].tobytes() == alone[i][0].tobytes() for i in range(4)), pos
        assert all(np.isfinite(quad[i]).all() for i in range(4))
    small = bc.make_case(40, 0, "scale", 3, "rowvecs", "scalar", "const", seed=80)
    (alone,) = call([dict(small, xs=agp.RowVecs(pt), ns=1)])
    ns = LAUNCH_POINTS + 5  # 1 025 tiles: the last one runs in a second launch group, on the first group's strips
    XS = rng.uniform(0.0, 4.0, size=(ns, 3)) / np.sqrt(3)
    spots = (0, LAUNCH_POINTS - 1, LAUNCH_POINTS, ns - 1)
    for pos in spots:
        XS[pos] = pt[0]
    (quad,) = call([dict(small, xs=agp.RowVecs(XS), ns=ns)])
    for pos in spots:
        assert all(quad[i][pos].tobytes() == alone[i][0].tobytes() for i in range(4)), pos
    assert all(np.isfinite(quad[i]).all() for i in range(4))


# ---- 5. shared test points ------------------------------------------------------------------------------------------------------------------
def test_shared_test_points_give_the_bits_of_the_per_problem_form(agp):
    rng = np.random.default_rng(4)
    X, XS = rng.uniform(0, 4, size=(333, 3)), rng.uniform(0, 4, size=(150, 3))
    XS[:3] = X[:3]
    x, xs = agp.RowVecs(X), agp.RowVecs(XS)
    k = 0.8 * agp.Matern52Kernel() @ agp.ScaleTransform(0.6)
    Y = rng.standard_normal((16, 333))
    fxs = [agp.GP(k)(x, 0.02)] * 16
    (g,) = agp.api._predict_groups(fxs, [Y[b] for b in range(16)], xs)
    pc = agp.api._predict_grad_marshal(g, 3)
    assert (pc.nb, g.nx, g.ny, g.nxs, len(pc.args[9])) == (16, 1, 16, 1, 1)
    shared, lp1 = agp.mean_and_var_grad_batch(fxs, [Y[b] for b in range(16)], xs, return_logpdf=True)
    repeated, lp2 = agp.mean_and_var_grad_batch([agp.GP(k)(agp.RowVecs(X.copy()), 0.02) for _ in range(16)], [Y[b].copy() for b in range(16)],
                                                [agp.RowVecs(XS.copy()) for _ in range(16)], return_logpdf=True)
    assert lp1.tobytes() == lp2.tobytes() and all(same_bits(p, q) for p, q in zip(shared, repeated))
    assert all(p[3].tobytes() == shared[0][3].tobytes() for p in shared)  # the variance and its gradient do not depend on y
    host = HostPosterior(bc.o.Kernel(3, 0.8, 0.6), X, Y[9], 0.02)
    gm, gv = host.grads(XS)
    assert g_err(shared[9][2], gm)[0] <= 1.0 and g_err(shared[9][3], gv)[0] <= 1.0


# ---- 6. composite kernels ------------------------------------------------------------------------------------------------------------------
def test_composite_batch_and_a_mixed_call_against_the_host_reference(agp):
    x, y = dense_data(545)
    rng = np.random.default_rng(50)
    xs = rng.uniform(0.0, 65.0, size=100)
    xs[:3] = x[[7, 300, 544]]  # White adds to the cross-covariance exactly here, and contributes 0 to the gradients
    kernels = bc.perturbed_kernels(ml_kernel(), 16)
    s2 = [1e-2 * agp.api._prior_variance(k) for k in kernels]
    fxs = [agp.GP(k)(x, s) for k, s in zip(kernels, s2)]
    n0 = counter()
    quads, lp = agp.mean_and_var_grad_batch(fxs, y, xs, return_logpdf=True)
    assert counter() - n0 == 16
    worst = [0.0] * 5
    for b, k in enumerate(kernels):
        host = HostPosterior(k, x, y, s2[b])
        lp_h, _ = bc.host_fit(ref_kernelmatrix(k, x) + s2[b] * np.eye(545), y)
        m_h, v_h = host.mean_and_var(xs)
        gm, gv = host.grads(xs)
        em, ev, el = errs(quads[b][:2], lp[b], (lp_h, m_h, v_h))
        (tm, _), (tv, _) = g_err(quads[b][2], gm[:, 0]), g_err(quads[b][3], gv[:, 0])
        worst = [max(w, e) for w, e in zip(worst, (em, ev, el, tm, tv))]
        assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL and tm <= 1.0 and tv <= 1.0, (b, em, ev, el, tm, tv)
    print("16 Mauna Loa kernels, n = 545: worst mean %.1e var %.1e logpdf %.1e dmean %.1e of tol dvar %.1e of tol" % tuple(worst))
    # a product of factors behind different transforms, D = 8
    rng = np.random.default_rng(51)
    X, XS = rng.uniform(0, 3, size=(200, 8)), rng.uniform(0, 3, size=(70, 8))
    XS[:3] = X[[0, 77, 199]]
    yk = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(200)
    km = many_dim_kernel(8)
    (qm,) = agp.mean_and_var_grad_batch([agp.GP(km)(agp.ColVecs(np.ascontiguousarray(X.T)), 0.05)], [yk], [agp.ColVecs(np.ascontiguousarray(XS.T))])
    host = HostPosterior(km, X, yk, 0.05)
    m_h, v_h = host.mean_and_var(XS)
    gm, gv = host.grads(XS)
    (tm, am), (tv, av) = g_err(qm[2].T, gm), g_err(qm[3].T, gv)
    print(f"many-dim D=8: mean {np.max(np.abs(qm[0] - m_h)):.1e} var {np.max(np.abs(qm[1] - v_h)):.1e} dmean {am:.1e} ({tm:.1e} of tol) dvar {av:.1e} ({tv:.1e} of tol)")
    assert qm[2].shape == (8, 70) and np.max(np.abs(qm[0] - m_h)) <= M_TOL and np.max(np.abs(qm[1] - v_h)) <= V_TOL and tm <= 1.0 and tv <= 1.0
    # a mixed call: single-kind and composite groups, the caller's order
    singles = [with_points(c, 20 + b, seed=900 + b) for b, c in enumerate(bc.small_cases(3, seed=9))]
    s_quads = call(singles)
    mixed = [(fxs[0], y, xs, None), (singles[0]["fx"], singles[0]["y"], singles[0]["xs"], pg.mean_grad_of(singles[0])), (fxs[3], y, xs, None),
             (singles[1]["fx"], singles[1]["y"], singles[1]["xs"], pg.mean_grad_of(singles[1])),
             (singles[2]["fx"], singles[2]["y"], singles[2]["xs"], pg.mean_grad_of(singles[2])), (fxs[1], y, xs, None)]
    got = agp.mean_and_var_grad_batch([t[0] for t in mixed], [t[1] for t in mixed], [t[2] for t in mixed], mean_grads=[t[3] for t in mixed])
    for pos, b in ((0, 0), (2, 3), (5, 1)):
        assert same_bits(got[pos], quads[b])
    for pos, s in ((1, 0), (3, 1), (4, 2)):
        assert same_bits(got[pos], s_quads[s])


# ---- 7. failures are per problem ------------------------------------------------------------------------------------------------------------
def test_failures_are_per_problem(agp):
    good = [with_points(c, 10 + 9 * b, seed=600 + b) for b, c in enumerate(bc.small_cases(16, seed=6, lo=40))]
    ref, lp_ref = call(good, return_logpdf=True)
    c = good[5]
    s2 = np.array(np.broadcast_to(c["s2"], (c["n"],)), dtype=np.float64)
    i = int(0.6 * (c["n"] - 1))
    s2[i] = -10.0
    bad = list(good)
    bad[5] = dict(c, fx=agp.FiniteGP(c["fx"].f, c["fx"].x, s2))
    quads, lp = call(bad, return_logpdf=True, on_error="nan")
    assert np.flatnonzero(np.isnan(lp)).tolist() == [5]
    assert quads[5][0].shape == (c["ns"],) and quads[5][2].shape == ref[5][2].shape and all(np.isnan(quads[5][j]).all() for j in range(4))
    for b in range(16):
        if b != 5:
            assert same_bits(quads[b], ref[b]) and lp[b].tobytes() == lp_ref[b].tobytes(), b
    pc = raw(bad)
    ctx = agp.default_context()
    assert getattr(ctx.lib, pc.entry)(ctx.handle, *pc.args) == 0  # a failing problem is data, not a status
    assert {b: int(pc.info[b]) for b in np.flatnonzero(pc.info)} == {5: i + 1}
    with pytest.raises(agp.PosDefException) as e:
        call(bad)
    assert (e.value.index, e.value.info) == (5, i + 1)


# ---- 8. routing ----------------------------------------------------------------------------------------------------------------------------
def test_problems_the_kernels_do_not_take_are_answered_by_the_single_path(agp):
    """fp32, a dense Σy, n above the constant and D = 17 run gp_posterior_fit + gp_posterior_predict_grad inside the call; the counter does not move."""
    ctx = agp.Context(0)
    try:
        rng = np.random.default_rng(74)
        G = rng.standard_normal((120, 120))
        dn = bc.make_case(120, 1, "none", 3, "rowvecs", "scalar", "const", seed=73)
        dense = 0.05 * np.eye(120) + 1e-3 * (G @ G.T) / 120
        dn = dict(dn, fx=agp.FiniteGP(dn["fx"].f, dn["fx"].x, dense), s2=dense)
        cases = on(ctx, [with_points(bc.make_case(100, 2, "scale", 3, "rowvecs", "scalar", "zero", seed=72, dtype=np.float32), 30, seed=172),
                         with_points(dn, 31, seed=173),
                         with_points(bc.make_case(agp._lib.batch_pgrad_max_n() + 128, 3, "ard", 3, "colvecs", "vector", "const", seed=71), 32, seed=171),
                         with_points(bc.make_case(100, 0, "ard", 17, "rowvecs", "vector", "zero", seed=75), 33, seed=175)])
        quads, lp = call(cases, return_logpdf=True)
        assert counter(ctx) == 0
        assert all(q.dtype == np.float32 for q in quads[0]) and all(q.dtype == np.float64 for q in quads[1])
        for b, c in enumerate(cases):
            gm, gv = pg.host_grads(c)
            m, v, dm, dv = quads[b]
            assert m.shape == (c["ns"],) and rows_of(c, dm).shape == (c["ns"], c["d"])
            if b == 0:  # fp32: the tolerance of tests/test_gpu_predict_grad.py for fp32
                for g, gr in ((rows_of(c, dm), gm), (rows_of(c, dv), gv)):
                    np.testing.assert_allclose(g, gr, rtol=2e-2, atol=2e-2 * max(1.0, float(np.abs(gr).max())))
                continue
            (tm, _), (tv, _) = g_err(rows_of(c, dm), gm), g_err(rows_of(c, dv), gv)
            post = agp.posterior(c["fx"], c["y"])
            m1, v1 = post.mean_and_var(c["xs"])
            print(f"routed {b}: n={c['n']} D={c['d']}: dmean {tm:.1e} of tol, dvar {tv:.1e} of tol")
            assert tm <= 1.0 and tv <= 1.0 and np.max(np.abs(m - m1)) <= M_TOL and np.max(np.abs(v - v1)) <= V_TOL
            assert bc.lp_err(lp[b], post.logpdf_value) <= LP_TOL
        kernel_served = on(ctx, [with_points(bc.make_case(90, 0, "scale", 3, "rowvecs", "scalar", "const", seed=76), 34, seed=176)])
        call(kernel_served)
        assert counter(ctx) == 1
    finally:
        ctx.close()


# ---- 9. poisoned context and waves -------------------------------------------------------------------------------------------------------------
def test_poisoned_blocks_and_more_problems_than_one_launch(agp):
    B = 2048 + 60  # BATCH_WAVE_PROBLEMS + 60: two waves, and 2 048 tiles in the first one: two launch groups
    build, oracle = _tiny_batch(B)
    with _poisoned_and_clean() as (poisoned, clean):
        quads, lp = agp.mean_and_var_grad_batch(*build(poisoned), return_logpdf=True)
        quads_c, lp_c = agp.mean_and_var_grad_batch(*build(clean), return_logpdf=True)
        assert poisoned.get_param(COUNTER) == clean.get_param(COUNTER) == B
        ragged = [c for c in pg.ragged_cases() if c["n"] <= 129]
        rp, rc = call(on(poisoned, ragged)), call(on(clean, ragged))
    assert all(same_bits(p, q) for p, q in zip(rp, rc))
    assert np.isfinite(lp).all() and all(np.isfinite(a).all() for q in quads for a in q)
    assert lp.tobytes() == lp_c.tobytes() and all(same_bits(p, q) for p, q in zip(quads, quads_c))
    fxs, ys, xss = build(None)
    worst = [0.0, 0.0]
    for b in range(0, B, 97):  # a sample against the single path; every problem's values against the oracle below
        m1, v1, dm1, dv1 = agp.posterior(fxs[b], ys[b]).mean_and_var_grad(xss[b])
        worst = [max(w, e) for w, e in zip(worst, (g_err(quads[b][2], dm1)[0], g_err(quads[b][3], dv1)[0]))]
    wv = [0.0, 0.0, 0.0]
    for b in range(B):
        wv = [max(w, e) for w, e in zip(wv, errs(quads[b][:2], lp[b], oracle(b)))]
    print(f"{B} problems of n = 8, ns = 3: worst mean {wv[0]:.1e} var {wv[1]:.1e} logpdf {wv[2]:.1e}; dmean {worst[0]:.1e} of tol dvar {worst[1]:.1e} of tol")
    assert wv[0] <= M_TOL and wv[1] <= V_TOL and wv[2] <= LP_TOL and worst[0] <= 1.0 and worst[1] <= 1.0


# ---- 10. argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_have_their_statuses_and_reasons(agp, ctx):
    cases = [with_points(c, 4 + b, seed=700 + b) for b, c in enumerate(bc.small_cases(3, seed=12))]
    pc = raw(cases)
    fn = ctx.lib.gp_predict_grad_batch
    good = list(pc.args)
    names = ["nb", "k", "nx", "x", "nz", "m", "ny", "y", "nxs", "xs", "pm", "what", "mo", "vo", "dmo", "dvo", "lp", "info"]
    K, Y, XS, MO, VO, DMO, DVO = (names.index(v) for v in ("k", "y", "xs", "mo", "vo", "dmo", "dvo"))
    bufs = pc.means + pc.vars + pc.dmeans + pc.dvars

    def status(**broken):
        args = list(good)
        for name, v in broken.items():
            args[names.index(name)] = v
        rc = fn(ctx.handle, *args)
        return rc, ctx.lib.gp_last_error().decode()

    def sentinel():
        pc.out[:] = 123.0
        for a in bufs:
            a[...] = 123.0

    def untouched():
        return np.all(pc.out == 123.0) and all(np.all(a == 123.0) for a in bufs)

    sentinel()
    assert fn(ctx.handle, 0, None, 0, None, None, None, 0, None, 0, None, None, 0, None, None, None, None, None, None) == 0  # nb = 0 touches nothing
    assert status(nb=0)[0] == 0 and untouched()
    pts = type(good[XS][0])
    xs_null = (pts * 3)(*good[XS])
    xs_null[1].data = None
    xs_neg = (pts * 3)(*good[XS])
    xs_neg[2].n = -1
    xs_d = (pts * 3)(*good[XS])
    xs_d[0].d += 1
    xs_d[0].layout = 1
    y_null = (C.c_void_p * 3)(good[Y][0], None, good[Y][2])
    hole = lambda i, at: (C.c_void_p * 3)(*[None if b == at else good[i][b] for b in range(3)])  # noqa: E731
    k_mixed = (type(good[K][0]) * 3)(*good[K])
    k_mixed[1].dtype = 1
    rows = [  # the arguments gp_predict_batch has: its numbers and reasons
        (dict(nb=-1), -2, "nb"), (dict(k=None), -3, "kernel array is NULL"), (dict(k=k_mixed), -3, "dtype"), (dict(nx=2), -4, "nx"),
        (dict(x=None), -5, "points array is NULL"), (dict(nz=None), -6, "noise array is NULL"), (dict(ny=2), -8, "ny"), (dict(y=None), -9, "y array is NULL"),
        (dict(y=y_null), -9, "a y pointer is NULL"), (dict(nxs=2), -10, "nxs"), (dict(xs=None), -11, "test points array is NULL"),
        (dict(xs=xs_null), -11, "points NULL"), (dict(xs=xs_neg), -11, "n must be >= 0"), (dict(xs=xs_d), -11, "different D"), (dict(what=0), -13, "what"),
        (dict(what=4), -13, "what"), (dict(what=7), -13, "what"),
        # the outputs: not both arrays of a side that is asked for, no hole in an array that is given
        (dict(mo=None, dmo=None), -14, "mean_out and dmean_out are both NULL"), (dict(vo=None, dvo=None), -15, "var_out and dvar_out are both NULL"),
        (dict(mo=hole(MO, 1)), -14, "a mean_out pointer is NULL"), (dict(vo=hole(VO, 0)), -15, "a var_out pointer is NULL"),
        (dict(dmo=hole(DMO, 2)), -16, "a dmean_out pointer is NULL"), (dict(dvo=hole(DVO, 1)), -17, "a dvar_out pointer is NULL"),
        (dict(info=None), -19, "info_out is NULL")]
    for broken, rc, text in rows:
        got, why = status(**broken)
        assert got == rc and why.startswith(f"invalid argument {-rc}: ") and text in why, (list(broken), got, why)
        assert untouched(), list(broken)  # no refused call wrote a result
    assert fn(None, *good) == -1 and "not a live gp_ctx" in ctx.lib.gp_last_error().decode()
    # legal: the arrays of a side that is not asked for may be NULL, and so may logpdf_out and one array of a side
    assert status(what=1, vo=None, dvo=None, lp=None)[0] == 0 and np.all(pc.out == 123.0) and all(np.all(a == 123.0) for a in pc.vars + pc.dvars)
    assert status(what=2, mo=None, dmo=None)[0] == 0
    assert status(mo=None, dvo=None)[0] == 0
    assert status()[0] == 0
    for b, c in enumerate(cases):
        em, ev, el = errs((pc.means[b], pc.vars[b]), pc.out[b], oracle_predict(c))
        gm, gv = pg.host_grads(c)
        dm, dv = (agp.api._dx_shaped(a[b], pc.xpts[b], c["xs"]) for a in (pc.dmeans, pc.dvars))
        assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL and g_err(rows_of(c, dm), gm)[0] <= 1.0 and g_err(rows_of(c, dv), gv)[0] <= 1.0


# ---- 11. CustomMean -----------------------------------------------------------------------------------------------------------------------------
def test_a_custom_mean_needs_its_derivative(agp):
    c = with_points(bc.make_case(150, 0, "ard", 3, "colvecs", "scalar", "custom", seed=88), 40, seed=188)
    with pytest.raises(TypeError, match="mean_grads"):
        agp.mean_and_var_grad_batch([c["fx"]], [c["y"]], [c["xs"]])
    (only_var,) = agp.mean_and_var_grad_batch([c["fx"]], [c["y"]], [c["xs"]], what=2)  # the variance side does not need it
    (quad,) = call([c])
    gm, gv = pg.host_grads(c)
    assert quad[2].shape == (3, 40)
    assert g_err(quad[2].T, gm + 0.3)[0] <= 1.0 and g_err(quad[3].T, gv)[0] <= 1.0 and only_var[3].tobytes() == quad[3].tobytes()
    assert not g_err(quad[2].T, gm)[0] <= 1.0  # the derivative of the mean function is in dmean
