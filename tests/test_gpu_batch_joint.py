"""GPU: gp_joint_batch / gp_joint_batch_sum (csrc/batch.hip: batch_logpdf_kernel, batch_predict_kernel, then batch_jcov_kernel and batch_jfact_kernel) through
agp.joint_batch and through the raw ABI — mean, latent covariance, held-out logpdf and joint samples of many small exact GPs in one call.

Tolerances.  mean 1e-8 and covariance entries 1e-9 absolute, training logpdf 1e-10 relative to max(|reference|, 1): the project's own for fp64 exact fits
(tests/test_gpu_batch_predict.py).  The held-out logpdf and the samples: the larger of LP_TOL (resp. M_TOL) and 4 × the worst error of the SINGLE path
(agp.logpdf(post(xs, Σy*), y*), agp.rand(post(xs, Σy*), xi = ...)) against the oracle on tests/batch_joint_cases.py, the factor 4 being headroom for a
different, equally stable summation order.  Measured (profiles/r25/batch_joint_errors.txt): single path 1.5e-13 and 9.2e-13, so 4 × stays below the floors and
HL_TOL = LP_TOL, S_TOL = M_TOL; gp_joint_batch itself measured 3.5e-13 and 1.3e-12 there."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import batch_cases as bc
from tests import batch_joint_cases as jc
from tests.composite_ref import ml_kernel, ref_kernelmatrix

pytestmark = pytest.mark.gpu

M_TOL, V_TOL, LP_TOL = 1e-8, 1e-9, 1e-10
HL_TOL, S_TOL = max(LP_TOL, 4 * 1.5e-13), max(M_TOL, 4 * 9.2e-13)
COUNTER = "batch_joint_kernel_problems"


def within(e):
    return e[0] <= M_TOL and e[1] <= V_TOL and e[2] <= LP_TOL and e[3] <= HL_TOL and e[4] <= S_TOL


def same_bits(p, q):
    return all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(p, q))


def on(ctx, cases):
    """the same problems with their priors bound to ctx"""
    out = []
    for c in cases:
        f = c["fx"].f
        g = agp.GP(f.kernel, ctx=ctx) if f.mean_fn is None else agp.GP(f.mean_fn, f.kernel, ctx=ctx)
        out.append(dict(c, fx=agp.FiniteGP(g, c["fx"].x, c["fx"].sigma2)))
    return out


def check_parity(cases, refs, ctx):
    before = ctx.get_param(COUNTER)
    quads, lp = jc.call(cases, return_logpdf=True)
    assert ctx.get_param(COUNTER) - before == len(cases)  # every problem went to the kernels
    worst = [0.0] * 5
    for b, (c, r) in enumerate(zip(cases, refs)):
        q = quads[b]
        assert q[0].shape == (c["ns"],) and q[1].shape == (c["ns"], c["ns"]) and q[3].shape == (c["ns"], jc.NSAMP) and q[0].dtype == np.float64
        e = jc.errs(q, lp[b], r)
        print(f"problem {b}: n={c['n']} ns={c['ns']} kind={c['kind']} {c['tr']} D={c['d']} {c['container']}: mean {e[0]:.1e} cov {e[1]:.1e} logpdf {e[2]:.1e} "
              f"held-out logpdf {e[3]:.1e} samples {e[4]:.1e}")
        worst = [max(w, v) for w, v in zip(worst, e)]
        assert within(e), (b, c["n"], c["ns"], e)
        assert np.array_equal(q[1], q[1].T), b  # exactly symmetric
    print("worst: mean %.1e cov %.1e logpdf %.1e held-out logpdf %.1e samples %.1e" % tuple(worst))
    return quads, lp


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------------
def test_every_output_against_the_oracle_through_the_mirror(agp):
    cases, refs = jc.joint_cases(), jc.joint_refs()
    max_n, max_ns = agp._lib.batch_joint_max()
    assert all(c["n"] <= max_n and c["ns"] <= max_ns for c in cases)
    quads, lp = check_parity(cases, refs, agp.default_context())
    # the thin wrappers and single bits: the same bits as with everything asked for
    args = ([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases])
    nz = [c["nz"] for c in cases]
    pairs = agp.mean_and_cov_batch(*args)
    hl = agp.logpdf_heldout_batch(*args, [c["ys"] for c in cases], noise=nz)
    draws = agp.rand_batch(*args, [c["xi"] for c in cases], noise=nz)
    for b, q in enumerate(quads):
        assert same_bits(pairs[b], q[:2]) and hl[b].tobytes() == q[2].tobytes() and draws[b].tobytes() == q[3].tobytes(), b
    only_cov = jc.call(cases, what=4)
    assert all(q[0] is None and q[2] is None and q[3] is None and q[1].tobytes() == r[1].tobytes() for q, r in zip(only_cov, quads))


def test_every_output_against_the_oracle_through_the_raw_abi(agp, ctx):
    cases, refs = jc.joint_cases()[::3], jc.joint_refs()[::3]
    (g,) = agp.api._predict_groups([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases])
    call = agp.api._joint_marshal(g, 29, [c["nz"] for c in cases], [c["ys"] for c in cases], [c["xi"] for c in cases])
    assert ctx.lib.gp_joint_batch(ctx.handle, *call.args) == 0
    assert not call.info.any() and not call.info_joint.any()
    for b, r in enumerate(refs):
        assert within(jc.errs((call.means[b], call.covs[b], call.heldout[b], call.samples[b]), call.out[b], r)), b


def test_mean_and_logpdf_are_the_bits_of_gp_predict_batch_and_the_diagonal_is_its_variance(agp):
    cases = jc.joint_cases()
    args = ([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases])
    pairs, lp_p = agp.mean_and_var_batch(*args, return_logpdf=True)
    quads, lp_j = agp.joint_batch(*args, return_logpdf=True)  # no Σy*
    assert lp_j.tobytes() == lp_p.tobytes()
    for b, (q, p) in enumerate(zip(quads, pairs)):
        assert q[0].tobytes() == p[0].tobytes(), b
        assert np.max(np.abs(np.diag(q[1]) - p[1])) <= V_TOL, b
        assert np.array_equal(q[1], q[1].T)


# ---- 2. bits -----------------------------------------------------------------------------------------------------------------------------------
def test_a_problem_does_not_see_its_neighbours_and_repeats_its_bits(agp):
    p = jc.with_joint(bc.make_case(200, 2, "ard", 3, "rowvecs", "vector", "custom", seed=77), 193, seed=177, coincide=True, vector_noise=True)
    (alone,), lp0 = jc.call([p], return_logpdf=True)
    assert within(jc.errs(alone, lp0[0], jc.oracle_joint(p)))
    others = [jc.with_joint(c, 1 + 13 * (b % 6), seed=500 + b, vector_noise=b % 2 == 0) for b, c in enumerate(bc.small_cases(40, seed=3))]
    for total in (2, 41):
        for pos in sorted({0, total // 2, total - 1}):
            batch = others[:total - 1]
            batch = batch[:pos] + [p] + batch[pos:]
            for _ in range(2):  # and on repetition
                quads, lp = jc.call(batch, return_logpdf=True)
                assert same_bits(quads[pos], alone) and lp[pos].tobytes() == lp0[0].tobytes(), (total, pos)


def test_shared_test_points_are_sent_once_and_change_nothing(agp):
    rng = np.random.default_rng(4)
    X, XS = rng.uniform(0, 4, size=(150, 3)), rng.uniform(0, 4, size=(129, 3))
    XS[:3] = X[:3]
    x, xs = agp.RowVecs(X), agp.RowVecs(XS)
    k = 0.8 * agp.Matern52Kernel() @ agp.ScaleTransform(0.6)
    Y, YS, XI = rng.standard_normal((8, 150)), rng.standard_normal((8, 129)), rng.standard_normal((8, 129, 2))
    (g,) = agp.api._predict_groups([agp.GP(k)(x, 0.02) for _ in range(8)], [Y[b] for b in range(8)], xs)
    jcall = agp.api._joint_marshal(g, 29, [0.03] * 8, list(YS), list(XI))
    assert (jcall.nb, jcall.nx, jcall.ny, jcall.nxs, len(jcall.args[3]), len(jcall.args[9])) == (8, 1, 8, 1, 1, 1)
    kw = dict(noise=0.03, ys_heldout=list(YS), xi=list(XI), return_logpdf=True)
    shared, lp1 = agp.joint_batch([agp.GP(k)(x, 0.02)] * 8, list(Y), xs, **kw)
    copies, lp2 = agp.joint_batch([agp.GP(k)(agp.RowVecs(X.copy()), 0.02) for _ in range(8)], [Y[b].copy() for b in range(8)],
                                  [agp.RowVecs(XS.copy()) for _ in range(8)], **kw)
    assert lp1.tobytes() == lp2.tobytes() and all(same_bits(p, q) for p, q in zip(shared, copies))
    assert all(p[1].tobytes() == shared[0][1].tobytes() for p in shared)  # the covariance does not depend on y
    post = agp.posterior(agp.GP(k)(x, 0.02), Y[5])
    m1, C1 = post.mean_and_cov(xs)
    assert np.max(np.abs(shared[5][0] - m1)) <= M_TOL and np.max(np.abs(shared[5][1] - C1)) <= V_TOL
    assert bc.lp_err(shared[5][2], agp.logpdf(post(xs, 0.03), YS[5])) <= HL_TOL
    assert np.max(np.abs(shared[5][3] - agp.rand(post(xs, 0.03), 2, xi=XI[5]))) <= S_TOL


# ---- 3. routing ----------------------------------------------------------------------------------------------------------------------------------
def test_problems_the_kernels_do_not_take_are_answered_by_the_single_path(agp, monkeypatch):
    """fp32, a dense Σy, D = 17, n above the limit, ns above the limit and a dense Σy* run the single-path sequence inside the call and are not counted."""
    monkeypatch.setenv("GPMI_BATCH_JOINT_MAX_N", "256")
    monkeypatch.setenv("GPMI_BATCH_JOINT_MAX_NS", "128")
    rng = np.random.default_rng(74)
    G, H = rng.standard_normal((120, 120)), rng.standard_normal((40, 40))
    dn = bc.make_case(120, 1, "none", 3, "rowvecs", "scalar", "custom", seed=73)
    dn = dict(dn, fx=agp.FiniteGP(dn["fx"].f, dn["fx"].x, 0.05 * np.eye(120) + 1e-3 * (G @ G.T) / 120),
              ofx=bc.o.FiniteGP(dn["ofx"].f, dn["ofx"].x, 0.05 * np.eye(120) + 1e-3 * (G @ G.T) / 120))
    dense_star = jc.with_joint(bc.make_case(90, 2, "scale", 3, "rowvecs", "scalar", "const", seed=79), 40, seed=179)
    dense_star["nz"] = 0.03 * np.eye(40) + 1e-3 * (H @ H.T) / 40
    cases = [jc.with_joint(bc.make_case(100, 2, "scale", 3, "rowvecs", "scalar", "zero", seed=72, dtype=np.float32), 30, seed=172),
             jc.with_joint(dn, 31, seed=173, vector_noise=True),
             jc.with_joint(bc.make_case(100, 0, "ard", 17, "rowvecs", "vector", "zero", seed=75), 33, seed=175),
             jc.with_joint(bc.make_case(257, 3, "ard", 3, "colvecs", "vector", "const", seed=71), 32, seed=171, vector_noise=True),
             jc.with_joint(bc.make_case(90, 0, "scale", 3, "rowvecs", "scalar", "const", seed=76), 129, seed=176),
             dense_star,
             jc.with_joint(bc.make_case(256, 1, "scale", 3, "rowvecs", "scalar", "const", seed=78), 128, seed=178, coincide=True)]  # the last one: the kernels, at both limits
    ctx = agp.default_context()
    before = ctx.get_param(COUNTER)
    quads, lp = jc.call(cases, return_logpdf=True)  # two library calls: the fp32 problem travels in a group of its own
    assert ctx.get_param(COUNTER) - before == 1
    assert quads[0][0].dtype == quads[0][1].dtype == quads[0][3].dtype == np.float32 and quads[1][0].dtype == np.float64
    for b, c in enumerate(cases):
        post = agp.posterior(c["fx"], c["y"])
        m1, C1 = post.mean_and_cov(c["xs"])
        fs = post(c["xs"], c["nz"])
        hl1, s1 = agp.logpdf(fs, c["ys"].astype(c["X"].dtype)), agp.rand(fs, jc.NSAMP, xi=c["xi"])
        tol = (1e-4,) * 5 if b == 0 else (M_TOL, V_TOL, LP_TOL, HL_TOL, S_TOL)  # fp32 results of one code path: the fp32 tolerance of the parity tests
        e = jc.errs(quads[b], lp[b], {"mean": m1, "cov": C1, "lp": post.logpdf_value, "hl": hl1, "samples": s1})
        assert all(v <= t for v, t in zip(e, tol)), (b, e)
        if b in (2, 3, 4, 6):  # against the oracle as well (its FiniteGP takes a scalar or a diagonal noise)
            assert within(jc.errs(quads[b], lp[b], jc.oracle_joint(c))), b


def test_single_kind_and_composite_groups_of_one_call_come_back_in_the_callers_order(agp):
    x, y = bc.mauna_loa_data(200)
    rng = np.random.default_rng(51)
    xs = rng.uniform(0.0, 17.0, size=65)
    ysh, xi = rng.standard_normal(65), rng.standard_normal((65, 2))
    kernels = bc.perturbed_kernels(ml_kernel(), 2)
    comp = [dict(fx=agp.GP(k)(x, 1e-2 * agp.api._prior_variance(k)), y=y, xs=xs, nz=0.02, ys=ysh, xi=xi) for k in kernels]
    single = [jc.with_joint(c, 20 + b, seed=900 + b, nsamp=2) for b, c in enumerate(bc.small_cases(3, seed=9))]
    c_quads, s_quads = jc.call(comp), jc.call(single)
    mixed = [comp[0], single[0], single[1], comp[1], single[2]]
    got = jc.call(mixed)
    for pos, ref in zip(range(5), (c_quads[0], s_quads[0], s_quads[1], c_quads[1], s_quads[2])):
        assert same_bits(got[pos], ref), pos


# ---- 4. composite kernels ----------------------------------------------------------------------------------------------------------------------
def test_composite_kernels_against_a_host_cholesky(agp):
    x, y = bc.mauna_loa_data(200)
    rng = np.random.default_rng(50)
    xs = rng.uniform(0.0, 17.0, size=129)
    xs[:40] = x[rng.integers(0, 200, size=40)]  # White adds to the cross-covariance and to K** exactly here
    ysh, xi = rng.standard_normal(129), rng.standard_normal((129, 2))
    kernels = bc.perturbed_kernels(ml_kernel(), 4)
    s2 = [1e-2 * agp.api._prior_variance(k) for k in kernels]
    nz = [1.3e-2, rng.uniform(1e-2, 5e-2, size=129), None, 2e-2]
    nz[2] = 1e-2 * s2[2]
    ctx = agp.default_context()
    before = ctx.get_param(COUNTER)
    quads, lp = agp.joint_batch([agp.GP(k)(x, s) for k, s in zip(kernels, s2)], y, xs, noise=nz, ys_heldout=[ysh] * 4, xi=[xi] * 4, return_logpdf=True)
    assert ctx.get_param(COUNTER) - before == 4
    for b, k in enumerate(kernels):
        Cm = ref_kernelmatrix(k, x) + s2[b] * np.eye(200)
        lp_h, a_h = bc.host_fit(Cm, y)
        Kxs = ref_kernelmatrix(k, x, xs)
        V = np.linalg.solve(np.linalg.cholesky(Cm), Kxs)
        mean, cov = Kxs.T @ a_h, ref_kernelmatrix(k, xs) - V.T @ V
        Ls = np.linalg.cholesky(cov + np.diag(np.broadcast_to(nz[b], (129,))))
        z = np.linalg.solve(Ls, ysh - mean)
        hl = -0.5 * (129 * np.log(2 * np.pi) + 2.0 * np.sum(np.log(np.diag(Ls))) + z @ z)
        e = jc.errs(quads[b], lp[b], {"lp": lp_h, "mean": mean, "cov": cov, "hl": hl, "samples": mean[:, None] + Ls @ xi})
        print(f"composite {b}: mean {e[0]:.1e} cov {e[1]:.1e} logpdf {e[2]:.1e} held-out logpdf {e[3]:.1e} samples {e[4]:.1e}")
        assert within(e), (b, e)
        assert np.array_equal(quads[b][1], quads[b][1].T)


# ---- 5. failure is data ----------------------------------------------------------------------------------------------------------------------------
def test_failures_are_per_problem(agp):
    good = [jc.with_joint(c, 10 + 9 * b, seed=600 + b, vector_noise=b % 2 == 1) for b, c in enumerate(bc.small_cases(8, seed=6, lo=40))]
    ref, lp_ref = jc.call(good, return_logpdf=True)
    rng = np.random.default_rng(61)
    # a training problem that is not positive definite: every input twenty times, no noise
    P3 = rng.uniform(0, 4, size=(3, 2))
    Xd = np.repeat(P3, 20, axis=0)
    k = 1.3 * agp.SqExponentialKernel()
    bad_fit = dict(fx=agp.GP(k)(agp.RowVecs(Xd), 0.0), y=rng.standard_normal(60), xs=agp.RowVecs(rng.uniform(0, 4, size=(33, 2))), nz=0.02,
                   ys=rng.standard_normal(33), xi=rng.standard_normal((33, jc.NSAMP)))
    # a joint covariance that is not: every test point eight times, no Σy*
    c = bc.make_case(70, 0, "scale", 2, "rowvecs", "scalar", "const", seed=62)
    XS = np.repeat(rng.uniform(0, 4, size=(4, 2)) / np.sqrt(2), 8, axis=0)
    bad_joint = dict(c, xs=agp.RowVecs(XS), oxs=XS, ns=32, nz=None, ys=rng.standard_normal(32), xi=rng.standard_normal((32, jc.NSAMP)))
    empty = jc.with_joint(bc.make_case(50, 1, "none", 2, "rowvecs", "scalar", "zero", seed=63), 0, seed=163)
    batch = good[:2] + [bad_fit] + good[2:5] + [bad_joint, empty] + good[5:]
    where = {2: "fit", 6: "joint", 7: "empty"}
    quads, lp = jc.call(batch, return_logpdf=True, on_error="nan")
    it = iter(range(8))
    for pos in range(len(batch)):
        if pos not in where:
            b = next(it)
            assert same_bits(quads[pos], ref[b]) and lp[pos].tobytes() == lp_ref[b].tobytes(), pos  # the neighbours keep their bits
    q = quads[2]
    assert np.isnan(lp[2]) and all(np.isnan(np.asarray(a)).all() for a in q) and q[1].shape == (33, 33) and q[3].shape == (33, jc.NSAMP)
    q = quads[6]
    post = bc.o.posterior(c["ofx"], c["y"])
    m_o, C_o = post.mean_and_cov(XS)
    assert np.isfinite(lp[6]) and np.isnan(q[2]) and np.isnan(q[3]).all()  # NaN in the held-out logpdf and the samples only
    assert np.max(np.abs(q[0] - m_o)) <= M_TOL and np.max(np.abs(q[1] - C_o)) <= V_TOL and np.array_equal(q[1], q[1].T)
    q = quads[7]
    assert np.isfinite(lp[7]) and q[0].shape == (0,) and q[1].shape == (0, 0) and q[3].shape == (0, jc.NSAMP) and q[2] == 0.0
    # the statuses through the raw ABI, and the mirror's exceptions
    (g,) = agp.api._predict_groups([p["fx"] for p in batch], [p["y"] for p in batch], [p["xs"] for p in batch])
    call = agp.api._joint_marshal(g, 29, [p["nz"] for p in batch], [p["ys"] for p in batch], [p["xi"] for p in batch])
    ctx = agp.default_context()
    assert getattr(ctx.lib, call.entry)(ctx.handle, *call.args) == 0  # a failing problem is data, not a status
    assert np.flatnonzero(call.info).tolist() == [2] and 1 < call.info[2] <= 60
    assert np.flatnonzero(call.info_joint).tolist() == [6] and 1 < call.info_joint[6] <= 32
    with pytest.raises(agp.PosDefException) as e:
        jc.call(batch)
    assert (e.value.index, e.value.info) == (2, int(call.info[2]))
    with pytest.raises(agp.PosDefException) as e:
        jc.call(batch[3:])
    assert (e.value.index, e.value.info) == (3, int(call.info_joint[6]))


# ---- 6. recycled blocks ----------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _poisoned():
    c = agp.Context(0)
    try:
        c.set_param("alloc_poison", 1)
        assert c.get_param("alloc_poison") == 1
        yield c
    finally:
        c.close()


def test_nothing_depends_on_what_a_recycled_block_held(agp):
    """Every device block arrives filled with NaN: the strip rows batch_predict_kernel does not write (a last strip with one valid row leaves 96) must reach
    no output.  The same bits as on the default context."""
    cases, refs = jc.joint_cases(), jc.joint_refs()
    clean = jc.call(cases)
    with _poisoned() as ctx:
        quads, lp = check_parity(on(ctx, cases), refs, ctx)
        again = jc.call(on(ctx, cases))  # in the blocks the first call left in the cache
    assert all(same_bits(p, q) and same_bits(p, r) for p, q, r in zip(quads, clean, again))


# ---- 7. argument errors ----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_have_their_statuses_and_reasons(agp, ctx):
    cases = [jc.with_joint(c, 4 + b, seed=700 + b, vector_noise=b == 1) for b, c in enumerate(bc.small_cases(3, seed=12))]
    (g,) = agp.api._predict_groups([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases])
    call = agp.api._joint_marshal(g, 29, [c["nz"] for c in cases], [c["ys"] for c in cases], [c["xi"] for c in cases])
    fn = ctx.lib.gp_joint_batch
    good = list(call.args)
    names = ["nb", "k", "nx", "x", "nz", "m", "ny", "y", "nxs", "xs", "pm", "nzs", "what", "mo", "co", "ys", "hl", "nsamp", "xi", "so", "lp", "info", "ij"]

    def status(**broken):
        args = list(good)
        for name, v in broken.items():
            args[names.index(name)] = v
        rc = fn(ctx.handle, *args)
        return rc, ctx.lib.gp_last_error().decode()

    outputs = call.means + call.covs + call.samples + [call.heldout, call.out]

    def sentinel():
        for a in outputs:
            a[...] = 123.0

    def untouched():
        return all(np.all(a == 123.0) for a in outputs)

    sentinel()
    assert fn(ctx.handle, 0, None, 0, None, None, None, 0, None, 0, None, None, None, 0, None, None, None, None, 0, None, None, None, None, None) == 0  # nb = 0 touches nothing
    assert status(nb=0)[0] == 0 and untouched()
    ptrs3 = lambda arr, hole: (C.c_void_p * 3)(*[None if b == hole else arr[b] for b in range(3)])  # noqa: E731
    xs_neg = (type(good[9][0]) * 3)(*good[9])
    xs_neg[2].n = -1
    nzs_bad = (type(good[11][0]) * 3)(*good[11])
    nzs_bad[0].kind = 7
    rows = [  # the arguments gp_predict_batch has: its numbers and reasons
        (dict(nb=-1), -2, "nb"), (dict(k=None), -3, "kernel array is NULL"), (dict(nx=2), -4, "nx"), (dict(x=None), -5, "points array is NULL"),
        (dict(nz=None), -6, "noise array is NULL"), (dict(ny=2), -8, "ny"), (dict(y=None), -9, "y array is NULL"), (dict(nxs=2), -10, "nxs"),
        (dict(xs=None), -11, "test points array is NULL"), (dict(xs=xs_neg), -11, "n must be >= 0"),
        # the new ones
        (dict(nzs=nzs_bad), -13, "noise kind"), (dict(what=0), -14, "what"), (dict(what=2), -14, "what"), (dict(what=3), -14, "what"), (dict(what=31), -14, "what"),
        (dict(what=32), -14, "what"), (dict(mo=None), -15, "mean_out is NULL"), (dict(mo=ptrs3(good[13], 1)), -15, "a mean_out pointer is NULL"),
        (dict(co=None), -16, "cov_out is NULL"), (dict(co=ptrs3(good[14], 0)), -16, "a cov_out pointer is NULL"), (dict(ys=None), -17, "ys array is NULL"),
        (dict(ys=ptrs3(good[15], 2)), -17, "a ys pointer is NULL"), (dict(hl=None), -18, "hlogpdf_out is NULL"), (dict(nsamp=-1), -19, "nsamp"),
        (dict(xi=None), -20, "xi array is NULL"), (dict(xi=ptrs3(good[18], 1)), -20, "a xi pointer is NULL"), (dict(so=None), -21, "samples_out is NULL"),
        (dict(so=ptrs3(good[19], 0)), -21, "a samples_out pointer is NULL"), (dict(info=None), -23, "info_out is NULL")]
    for broken, rc, text in rows:
        got, why = status(**broken)
        assert got == rc and why.startswith(f"invalid argument {-rc}: ") and text in why, (list(broken), got, why)
        assert untouched(), list(broken)  # no refused call wrote a result
    assert fn(None, *good) == -1 and "not a live gp_ctx" in ctx.lib.gp_last_error().decode()
    # legal: whatever is not asked for may be NULL, and so may Σy*, logpdf_out and info_joint_out; nsamp = 0 draws nothing
    assert status(what=4, mo=None, ys=None, hl=None, xi=None, so=None, lp=None, ij=None, nzs=None)[0] == 0
    assert all(np.all(a == 123.0) for a in call.means + call.samples + [call.heldout, call.out])
    assert status(what=16, nsamp=0, xi=None, so=None)[0] == 0 and all(np.all(a == 123.0) for a in call.samples)
    assert status()[0] == 0
    for b, c in enumerate(cases):
        assert within(jc.errs((call.means[b], call.covs[b], call.heldout[b], call.samples[b]), call.out[b], jc.oracle_joint(c))), b
