"""GPU: gp_predict_batch / gp_predict_batch_sum (csrc/batch.hip: batch_logpdf_kernel, then batch_predict_kernel on the slices it leaves) through
agp.mean_and_var_batch — predictive mean and variance of many small exact GPs, each at its own test points, in one call.
Tolerances are the project's own for fp64 exact fits: mean 1e-8 absolute, var 1e-9 absolute, logpdf 1e-10 relative to max(|reference|, 1).
Test points are drawn from the box of the training inputs; the first few coincide exactly with training points."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from tests import batch_cases as bc
from tests.composite_ref import dense_data, ml_kernel, ref_kernelmatrix

pytestmark = pytest.mark.gpu

M_TOL, V_TOL, LP_TOL = 1e-8, 1e-9, 1e-10
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 545, 768]
NS = [0, 1, 63, 64, 65, 200]
LAUNCH_POINTS = 1024 * 128  # BATCH_PRED_TILES tiles of TP test points: what one predict launch takes (csrc/batch.hip)


def draw_points(case, ns, seed):
    """ns test points of a case's dimension and container, and the same as the oracle takes them; the first min(3, ns, n) are training points."""
    rng = np.random.default_rng(seed)
    n, d = case["X"].shape
    XS = (rng.uniform(0.0, 4.0, size=(ns, d)) / np.sqrt(d)).astype(case["X"].dtype)
    k = min(3, ns, n)
    XS[:k] = case["X"][rng.permutation(n)[:k]]
    return as_container(case, XS), (XS[:, 0] if case["container"] == "vector" else XS)


def as_container(case, XS):
    if case["container"] == "vector":
        return XS[:, 0].copy()
    return agp.ColVecs(np.ascontiguousarray(XS.T)) if case["container"] == "colvecs" else agp.RowVecs(XS)


def with_points(case, ns, seed):
    xs, oxs = draw_points(case, ns, seed)
    return dict(case, xs=xs, oxs=oxs, ns=ns)


def oracle_predict(case):
    lp, post = bc.o.logpdf_and_posterior(case["ofx"], case["y"])
    m, v = post.mean_and_var(case["oxs"]) if case["ns"] else (np.empty(0), np.empty(0))
    return float(lp), np.asarray(m), np.asarray(v)


def call(cases, **kw):
    return agp.mean_and_var_batch([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases], **kw)


def errs(pair, lp, ref):
    lp_o, m_o, v_o = ref
    em = float(np.max(np.abs(pair[0] - m_o))) if len(m_o) else 0.0
    ev = float(np.max(np.abs(pair[1] - v_o))) if len(v_o) else 0.0
    return em, ev, bc.lp_err(lp, lp_o)


def same_bits(p, q):
    return p[0].tobytes() == q[0].tobytes() and p[1].tobytes() == q[1].tobytes()


def on(ctx, cases):
    """the same problems with their priors bound to ctx"""
    out = []
    for c in cases:
        f = c["fx"].f
        g = agp.GP(f.kernel, ctx=ctx) if f.mean_fn is None else agp.GP(f.mean_fn, f.kernel, ctx=ctx)
        out.append(dict(c, fx=agp.FiniteGP(g, c["fx"].x, c["fx"].sigma2)))
    return out


@functools.lru_cache(maxsize=None)
def ragged():
    """Every size twice, the numbers of test points cycling against them; the categories cycle as in bc.ragged_cases.  With the oracle's answers."""
    cases = []
    for b, n in enumerate(SIZES + SIZES):
        cont = bc.CONTAINERS[b % 3]
        d = 1 if cont == "vector" else [1, 3, 8][(b // 3) % 3]
        c = bc.make_case(n, b % 4, bc.TRANSFORMS[(b // 4) % 3], d, cont, bc.NOISES[(b // 2) % 2], bc.MEANS[(b // 5) % 3], seed=3000 + b)
        cases.append(with_points(c, NS[(b + b // len(SIZES)) % len(NS)], seed=4000 + b))
    return cases, [oracle_predict(c) for c in cases]


# ---- 1. ragged batch against the oracle and the single path -----------------------------------------------------------------------------------
def test_ragged_batch_against_the_oracle_and_the_single_path(agp):
    cases, refs = ragged()
    assert all(c["n"] <= agp._lib.batch_max_n() for c in cases)  # every problem goes to the batch kernel
    assert {c["ns"] for c in cases} == set(NS) and {c["n"] for c in cases} == set(SIZES)
    pairs, lp = call(cases, return_logpdf=True)
    worst = [0.0] * 5
    for b, c in enumerate(cases):
        assert pairs[b][0].shape == pairs[b][1].shape == (c["ns"],) and pairs[b][0].dtype == np.float64
        em, ev, el = errs(pairs[b], lp[b], refs[b])
        sm = sv = 0.0
        if c["ns"]:
            m1, v1 = agp.posterior(c["fx"], c["y"]).mean_and_var(c["xs"])  # gp_posterior_fit + gp_posterior_predict on the same inputs
            sm, sv = float(np.max(np.abs(pairs[b][0] - m1))), float(np.max(np.abs(pairs[b][1] - v1)))
        print(f"problem {b}: n={c['n']} ns={c['ns']} kind={c['kind']} {c['tr']} D={c['d']} {c['container']} {c['noise']} {c['mean']}: "
              f"mean {em:.1e} var {ev:.1e} logpdf {el:.1e}; vs single path mean {sm:.1e} var {sv:.1e}")
        worst = [max(w, e) for w, e in zip(worst, (em, ev, el, sm, sv))]
        assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL and sm <= M_TOL and sv <= V_TOL, (b, c["n"], c["ns"], em, ev, el, sm, sv)
    print("worst: mean %.1e var %.1e logpdf %.1e; vs single path mean %.1e var %.1e" % tuple(worst))
    # one side at a time: the same bits as with both
    for what, side in ((1, 0), (2, 1)):
        one = call(cases, what=what)
        assert all(p[1 - side] is None and p[side].tobytes() == q[side].tobytes() for p, q in zip(one, pairs))


# ---- 2. the kernel's own limit -----------------------------------------------------------------------------------------------------------
def test_the_kernel_serves_every_size_up_to_its_own_limit(agp, monkeypatch):
    monkeypatch.setenv("GPMI_BATCH_MAX_N", "2048")
    cases = [with_points(bc.make_case(1100, 2, "ard", 3, "rowvecs", "vector", "custom", seed=97), 65, seed=197),
             with_points(bc.make_case(2048, 3, "scale", 3, "colvecs", "scalar", "const", seed=99), 65, seed=199)]
    pairs, lp = call(cases, return_logpdf=True)
    pairs2 = call(cases)
    for b, c in enumerate(cases):
        em, ev, el = errs(pairs[b], lp[b], oracle_predict(c))
        print(f"kernel-served n={c['n']}: mean {em:.1e} var {ev:.1e} logpdf {el:.1e}")
        assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL
        assert same_bits(pairs[b], pairs2[b])  # a fixed schedule


# ---- 3. company changes nothing ------------------------------------------------------------------------------------------------------------
def test_a_problem_does_not_see_its_neighbours(agp):
    p = with_points(bc.make_case(200, 2, "ard", 3, "rowvecs", "vector", "custom", seed=77), 70, seed=177)
    (pair0,), lp0 = call([p], return_logpdf=True)
    em, ev, el = errs(pair0, lp0[0], oracle_predict(p))
    assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL
    others = [with_points(c, 1 + b % 7, seed=500 + b) for b, c in enumerate(bc.small_cases(300, seed=3))]
    for total in (2, 64, 301):
        for pos in sorted({0, total // 2, total - 1}):
            batch = others[:total - 1]
            batch = batch[:pos] + [p] + batch[pos:]
            pairs, lp = call(batch, return_logpdf=True, on_error="nan")
            assert same_bits(pairs[pos], pair0) and lp[pos].tobytes() == lp0[0].tobytes(), (total, pos)


def test_a_test_point_does_not_see_the_other_test_points(agp):
    """Each row's arithmetic touches no other row: a difference here is a padding leak.  Alone, at any position among 200 others (two tiles), and on
    either side of the split into two predict launches."""
    c = bc.make_case(200, 3, "scale", 3, "rowvecs", "scalar", "const", seed=78)
    rng = np.random.default_rng(79)
    pt = rng.uniform(0.0, 4.0, size=(1, 3)) / np.sqrt(3)
    (alone,) = call([dict(c, xs=agp.RowVecs(pt))])
    others = rng.uniform(0.0, 4.0, size=(200, 3)) / np.sqrt(3)
    for pos in (0, 1, 100, 127, 128, 199, 200):
        XS = np.concatenate([others[:pos], pt, others[pos:]])
        (pair,) = call([dict(c, xs=agp.RowVecs(XS))])
        assert pair[0][pos].tobytes() == alone[0].tobytes() and pair[1][pos].tobytes() == alone[1].tobytes(), pos
    small = bc.make_case(40, 0, "scale", 3, "rowvecs", "scalar", "const", seed=80)
    (alone,) = call([dict(small, xs=agp.RowVecs(pt))])
    ns = LAUNCH_POINTS + 5  # 1 025 tiles: the last one runs in a second launch
    XS = rng.uniform(0.0, 4.0, size=(ns, 3)) / np.sqrt(3)
    for pos in (0, LAUNCH_POINTS - 1, LAUNCH_POINTS, ns - 1):
        XS[pos] = pt[0]
    (pair,) = call([dict(small, xs=agp.RowVecs(XS))])
    for pos in (0, LAUNCH_POINTS - 1, LAUNCH_POINTS, ns - 1):
        assert pair[0][pos].tobytes() == alone[0].tobytes() and pair[1][pos].tobytes() == alone[1].tobytes(), pos
    assert np.isfinite(pair[0]).all() and np.isfinite(pair[1]).all()


# ---- 4. shared inputs ----------------------------------------------------------------------------------------------------------------------
def test_shared_inputs_are_sent_once_and_change_nothing(agp):
    rng = np.random.default_rng(4)
    X, XS = rng.uniform(0, 4, size=(333, 3)), rng.uniform(0, 4, size=(150, 3))
    XS[:3] = X[:3]
    x, xs = agp.RowVecs(X), agp.RowVecs(XS)
    k = 0.8 * agp.Matern52Kernel() @ agp.ScaleTransform(0.6)
    Y = rng.standard_normal((16, 333))  # independent outputs over one x, predicted at one xs
    fxs = [agp.GP(k)(x, 0.02)] * 16
    (g,) = agp.api._predict_groups([agp.GP(k)(x, 0.02) for _ in range(16)], [Y[b] for b in range(16)], xs)
    pc = agp.api._predict_marshal(g, 3)
    assert (pc.nb, pc.nx, pc.ny, pc.nxs, len(pc.args[3]), len(pc.args[9])) == (16, 1, 16, 1, 1, 1)
    shared, lp1 = agp.mean_and_var_batch(fxs, [Y[b] for b in range(16)], xs, return_logpdf=True)
    repeated, lp2 = agp.mean_and_var_batch([agp.GP(k)(agp.RowVecs(X.copy()), 0.02) for _ in range(16)], [Y[b].copy() for b in range(16)],
                                           [agp.RowVecs(XS.copy()) for _ in range(16)], return_logpdf=True)
    assert lp1.tobytes() == lp2.tobytes() and all(same_bits(p, q) for p, q in zip(shared, repeated))
    assert all(p[1].tobytes() == shared[0][1].tobytes() for p in shared)  # the variance does not depend on y
    for b in (0, 9, 15):
        m1, v1 = agp.posterior(fxs[b], Y[b]).mean_and_var(xs)
        assert np.max(np.abs(shared[b][0] - m1)) <= M_TOL and np.max(np.abs(shared[b][1] - v1)) <= V_TOL


# ---- 5. composite kernels ------------------------------------------------------------------------------------------------------------------
def test_composite_batch_and_a_mixed_call_against_a_host_cholesky(agp):
    x, y = dense_data(545)
    rng = np.random.default_rng(50)
    xs = rng.uniform(0.0, 65.0, size=100)
    xs[:3] = x[[7, 300, 544]]  # White adds to the cross-covariance exactly here
    kernels = bc.perturbed_kernels(ml_kernel(), 4)
    s2 = [1e-2 * agp.api._prior_variance(k) for k in kernels]
    fxs = [agp.GP(k)(x, s) for k, s in zip(kernels, s2)]
    pairs, lp = agp.mean_and_var_batch(fxs, y, xs, return_logpdf=True)
    for b, k in enumerate(kernels):
        Cm = ref_kernelmatrix(k, x) + s2[b] * np.eye(545)
        lp_h, a_h = bc.host_fit(Cm, y)
        Kxs = ref_kernelmatrix(k, x, xs)
        V = sla.solve_triangular(np.linalg.cholesky(Cm), Kxs, lower=True)
        m_h, v_h = Kxs.T @ a_h, np.diag(ref_kernelmatrix(k, xs)) - np.sum(V * V, axis=0)
        em, ev, el = errs(pairs[b], lp[b], (lp_h, m_h, v_h))
        print(f"composite {b}: mean {em:.1e} var {ev:.1e} logpdf {el:.1e}")
        assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL
    singles = [with_points(c, 20 + b, seed=900 + b) for b, c in enumerate(bc.small_cases(3, seed=9))]
    s_pairs = call(singles)
    mixed = [(fxs[0], y, xs), (singles[0]["fx"], singles[0]["y"], singles[0]["xs"]), (fxs[3], y, xs), (singles[1]["fx"], singles[1]["y"], singles[1]["xs"]),
             (singles[2]["fx"], singles[2]["y"], singles[2]["xs"]), (fxs[1], y, xs)]
    got = agp.mean_and_var_batch([t[0] for t in mixed], [t[1] for t in mixed], [t[2] for t in mixed])
    for pos, b in ((0, 0), (2, 3), (5, 1)):
        assert same_bits(got[pos], pairs[b])
    for pos, s in ((1, 0), (3, 1), (4, 2)):
        assert same_bits(got[pos], s_pairs[s])


# ---- 6. failures are per problem ------------------------------------------------------------------------------------------------------------
def test_failures_are_per_problem(agp):
    good = [with_points(c, 10 + 9 * b, seed=600 + b) for b, c in enumerate(bc.small_cases(16, seed=6, lo=40))]
    ref, lp_ref = call(good, return_logpdf=True)
    c = good[5]
    s2 = np.array(np.broadcast_to(c["s2"], (c["n"],)), dtype=np.float64)
    i = int(0.6 * (c["n"] - 1))
    s2[i] = -10.0
    bad = list(good)
    bad[5] = dict(c, fx=agp.FiniteGP(c["fx"].f, c["fx"].x, s2))
    pairs, lp = call(bad, return_logpdf=True, on_error="nan")
    assert np.flatnonzero(np.isnan(lp)).tolist() == [5]
    assert pairs[5][0].shape == (c["ns"],) and np.isnan(pairs[5][0]).all() and np.isnan(pairs[5][1]).all()
    for b in range(16):
        if b != 5:
            assert same_bits(pairs[b], ref[b]) and lp[b].tobytes() == lp_ref[b].tobytes(), b
    (g,) = agp.api._predict_groups([q["fx"] for q in bad], [q["y"] for q in bad], [q["xs"] for q in bad])
    pc = agp.api._predict_marshal(g, 3)
    ctx = agp.default_context()
    assert getattr(ctx.lib, pc.entry)(ctx.handle, *pc.args) == 0  # a failing problem is data, not a status
    assert {b: int(pc.info[b]) for b in np.flatnonzero(pc.info)} == {5: i + 1}
    with pytest.raises(agp.PosDefException) as e:
        call(bad)
    assert (e.value.index, e.value.info) == (5, i + 1)


# ---- 7. routing ----------------------------------------------------------------------------------------------------------------------------
def test_problems_the_kernel_does_not_take_are_answered_by_the_single_path(agp):
    """fp32, a dense Σy, n above the constant and D = 17 run gp_posterior_fit + gp_posterior_predict inside the call: the same code as the single path, so
    under "deterministic" = 1 the fp64 problems return the same bits."""
    ctx = agp.Context(0)
    try:
        ctx.set_param("deterministic", 1)
        ctx.set_param("gemm_streamk", 0)
        rng = np.random.default_rng(74)
        G = rng.standard_normal((120, 120))
        dn = bc.make_case(120, 1, "none", 3, "rowvecs", "scalar", "custom", seed=73)
        dn = dict(dn, fx=agp.FiniteGP(dn["fx"].f, dn["fx"].x, 0.05 * np.eye(120) + 1e-3 * (G @ G.T) / 120))
        cases = on(ctx, [with_points(bc.make_case(100, 2, "scale", 3, "rowvecs", "scalar", "zero", seed=72, dtype=np.float32), 30, seed=172),
                         with_points(dn, 31, seed=173),
                         with_points(bc.make_case(agp._lib.batch_max_n() + 128, 3, "ard", 3, "colvecs", "vector", "const", seed=71), 32, seed=171),
                         with_points(bc.make_case(100, 0, "ard", 17, "rowvecs", "vector", "zero", seed=75), 33, seed=175),
                         with_points(bc.make_case(90, 0, "scale", 3, "rowvecs", "scalar", "const", seed=76), 34, seed=176)])  # the last one: the batch kernel
        pairs, lp = call(cases, return_logpdf=True)
        assert pairs[0][0].dtype == pairs[0][1].dtype == np.float32 and pairs[1][0].dtype == np.float64
        for b, c in enumerate(cases):
            post = agp.posterior(c["fx"], c["y"])
            m1, v1 = post.mean_and_var(c["xs"])
            assert pairs[b][0].shape == (c["ns"],)
            if b == 0:  # fp32 results of one code path: compared at the fp32 tolerance of the parity tests
                assert np.max(np.abs(pairs[b][0] - m1)) <= 1e-4 and np.max(np.abs(pairs[b][1] - v1)) <= 1e-4
                assert bc.lp_err(lp[b], post.logpdf_value) <= 1e-4
            elif b < 4:
                assert same_bits(pairs[b], (m1, v1)) and float(lp[b]) == float(post.logpdf_value), b
            else:
                assert np.max(np.abs(pairs[b][0] - m1)) <= M_TOL and np.max(np.abs(pairs[b][1] - v1)) <= V_TOL
        for b in (2, 3):  # against the oracle as well
            em, ev, el = errs(pairs[b], lp[b], oracle_predict(cases[b]))
            assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL
    finally:
        ctx.close()


# ---- 8. waves and splitting -----------------------------------------------------------------------------------------------------------------
def _tiny_batch(B):
    rng = np.random.default_rng(8)
    X, XS, Y = rng.uniform(0, 4, size=(B, 8, 2)), rng.uniform(0, 4, size=(B, 3, 2)), rng.standard_normal((B, 8))
    XS[:, 0] = X[:, 0]
    kinds = [agp.SqExponentialKernel, agp.Matern12Kernel, agp.Matern32Kernel, agp.Matern52Kernel]

    def build(c):
        return ([agp.GP((1.0 + 1e-4 * b) * kinds[b % 4]() @ agp.ScaleTransform(0.7), ctx=c)(agp.RowVecs(X[b]), 0.02) for b in range(B)],
                [Y[b] for b in range(B)], [agp.RowVecs(XS[b]) for b in range(B)])

    def oracle(b):
        ofx = bc.o.FiniteGP(bc.o.GP(bc.o.Kernel(b % 4, 1.0 + 1e-4 * b, 0.7)), X[b], 0.02)
        lp, post = bc.o.logpdf_and_posterior(ofx, Y[b])
        return (float(lp),) + tuple(post.mean_and_var(XS[b]))

    return build, oracle


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


def _run_twice_and_trim(ctx, args):
    blocks0 = ctx.get_param("pool_blocks")
    first = agp.mean_and_var_batch(*args, return_logpdf=True)
    cached = (ctx.get_param("pool_cached_mb"), ctx.get_param("pool_blocks"))
    second = agp.mean_and_var_batch(*args, return_logpdf=True)
    assert (ctx.get_param("pool_cached_mb"), ctx.get_param("pool_blocks")) == cached  # the second call runs in the first one's blocks
    assert second[1].tobytes() == first[1].tobytes() and all(same_bits(p, q) for p, q in zip(first[0], second[0]))
    ctx.trim()
    assert ctx.get_param("pool_blocks") == blocks0 == 0  # every block of the call went back to the cache: nothing is held after the trim
    return first


def test_more_problems_than_one_launch_run_in_waves(agp):
    B = 2048 + 60  # BATCH_WAVE_PROBLEMS + 60: two waves, and 2 048 tiles in the first one: two predict launches
    build, oracle = _tiny_batch(B)
    with _poisoned_and_clean() as (poisoned, clean):
        pairs, lp = _run_twice_and_trim(poisoned, build(poisoned))
        pairs_c, lp_c = agp.mean_and_var_batch(*build(clean), return_logpdf=True)
    assert np.isfinite(lp).all() and all(np.isfinite(p[0]).all() and np.isfinite(p[1]).all() for p in pairs)
    assert lp.tobytes() == lp_c.tobytes() and all(same_bits(p, q) for p, q in zip(pairs, pairs_c))
    worst = [0.0, 0.0, 0.0]
    for b in range(B):
        worst = [max(w, e) for w, e in zip(worst, errs(pairs[b], lp[b], oracle(b)))]
    print(f"{B} problems of n = 8, ns = 3: worst mean {worst[0]:.1e} var {worst[1]:.1e} logpdf {worst[2]:.1e}")
    assert worst[0] <= M_TOL and worst[1] <= V_TOL and worst[2] <= LP_TOL


def test_more_test_points_than_one_launch_run_in_several_predict_launches(agp):
    c = bc.make_case(8, 2, "scale", 2, "rowvecs", "scalar", "const", seed=81)
    ns = LAUNCH_POINTS + 300  # 1 027 tiles against the cap of 1 024
    c = with_points(c, ns, seed=181)
    ref = oracle_predict(c)
    with _poisoned_and_clean() as (poisoned, clean):
        (p,) = on(poisoned, [c])
        (pair,), lp = _run_twice_and_trim(poisoned, ([p["fx"]], [p["y"]], [p["xs"]]))
        (q,) = on(clean, [c])
        (pair_c,), lp_c = agp.mean_and_var_batch([q["fx"]], [q["y"]], [q["xs"]], return_logpdf=True)
    assert np.isfinite(pair[0]).all() and np.isfinite(pair[1]).all() and np.isfinite(lp).all()
    assert same_bits(pair, pair_c) and lp.tobytes() == lp_c.tobytes()
    em, ev, el = errs(pair, lp[0], ref)
    print(f"n = 8, ns = {ns}: mean {em:.1e} var {ev:.1e} logpdf {el:.1e}")
    assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL


# ---- 9. argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_have_their_statuses_and_reasons(agp, ctx):
    cases = [with_points(c, 4 + b, seed=700 + b) for b, c in enumerate(bc.small_cases(3, seed=12))]
    (g,) = agp.api._predict_groups([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases])
    pc = agp.api._predict_marshal(g, 3)
    fn = ctx.lib.gp_predict_batch
    good = list(pc.args)
    NB, K, NX, X, NZ, M, NY, Y, NXS, XS, PM, WHAT, MO, VO, LP, INFO = range(16)

    def status(**broken):
        args = list(good)
        for name, v in broken.items():
            args[{"nb": NB, "k": K, "nx": NX, "x": X, "nz": NZ, "ny": NY, "y": Y, "nxs": NXS, "xs": XS, "what": WHAT, "mo": MO, "vo": VO, "lp": LP,
                  "info": INFO}[name]] = v
        rc = fn(ctx.handle, *args)
        return rc, ctx.lib.gp_last_error().decode()

    def sentinel():
        pc.out[:] = 123.0
        for a in pc.means + pc.vars:
            a[:] = 123.0

    def untouched():
        return np.all(pc.out == 123.0) and all(np.all(a == 123.0) for a in pc.means + pc.vars)

    sentinel()
    assert fn(ctx.handle, 0, None, 0, None, None, None, 0, None, 0, None, None, 0, None, None, None, None) == 0  # nb = 0 touches nothing
    assert status(nb=0)[0] == 0 and untouched()
    xs_null = (type(good[XS][0]) * 3)(*good[XS])
    xs_null[1].data = None
    xs_neg = (type(good[XS][0]) * 3)(*good[XS])
    xs_neg[2].n = -1
    xs_d = (type(good[XS][0]) * 3)(*good[XS])
    xs_d[0].d += 1
    xs_d[0].layout = 1
    y_null = (C.c_void_p * 3)(good[Y][0], None, good[Y][2])
    mo_null = (C.c_void_p * 3)(good[MO][0], None, good[MO][2])
    vo_null = (C.c_void_p * 3)(None, good[VO][1], good[VO][2])
    k_mixed = (type(good[K][0]) * 3)(*good[K])
    k_mixed[1].dtype = 1
    rows = [  # the arguments gp_logpdf_batch has: its numbers and reasons
        (dict(nb=-1), -2, "nb"), (dict(k=None), -3, "kernel array is NULL"), (dict(k=k_mixed), -3, "dtype"), (dict(nx=2), -4, "nx"),
        (dict(x=None), -5, "points array is NULL"), (dict(nz=None), -6, "noise array is NULL"), (dict(ny=2), -8, "ny"), (dict(y=None), -9, "y array is NULL"),
        (dict(y=y_null), -9, "a y pointer is NULL"),
        # the new ones
        (dict(nxs=2), -10, "nxs"), (dict(xs=None), -11, "test points array is NULL"), (dict(xs=xs_null), -11, "points NULL"),
        (dict(xs=xs_neg), -11, "n must be >= 0"), (dict(xs=xs_d), -11, "different D"), (dict(what=0), -13, "what"), (dict(what=4), -13, "what"),
        (dict(what=7), -13, "what"), (dict(mo=None), -14, "mean_out is NULL"), (dict(mo=mo_null), -14, "a mean_out pointer is NULL"),
        (dict(vo=None), -15, "var_out is NULL"), (dict(vo=vo_null), -15, "a var_out pointer is NULL"), (dict(info=None), -17, "info_out is NULL")]
    for broken, rc, text in rows:
        got, why = status(**broken)
        assert got == rc and why.startswith(f"invalid argument {-rc}: ") and text in why, (list(broken), got, why)
        assert untouched(), list(broken)  # no refused call wrote a result
    assert fn(None, *good) == -1 and "not a live gp_ctx" in ctx.lib.gp_last_error().decode()
    # legal: an output array that is not asked for may be NULL, and so may logpdf_out
    assert status(what=1, vo=None, lp=None)[0] == 0 and np.all(pc.out == 123.0) and all(np.all(a == 123.0) for a in pc.vars)
    assert status(what=2, mo=None)[0] == 0
    assert status()[0] == 0
    for b, c in enumerate(cases):
        em, ev, el = errs((pc.means[b], pc.vars[b]), pc.out[b], oracle_predict(c))
        assert em <= M_TOL and ev <= V_TOL and el <= LP_TOL
