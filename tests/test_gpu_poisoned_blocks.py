"""GPU: no result depends on what a device block held before the call wrote it.

Every device buffer of the single-device engine comes from `ctx_alloc` (csrc/gpmi355.hip) — a fresh `hipMalloc` block or one from the ctx's cache — and is
never initialised there; each path has its own rule about which parts it fills itself (identity padding, finite slack rows, "zero above the diagonal on
entry", scratch "zeroed by the caller").  The rest of the suite runs in one process on one warm cache, where a recycled block practically always holds stale
FINITE numbers, so a kernel that multiplies an unwritten tile by a zero mask gets the right answer by accident.  Here every test builds a context of its own
with the ctx parameter "alloc_poison" = 1 (include/gpmi355.h): every block is handed out filled with 0xFF bytes — NaN as fp64 and as fp32, −1 as int32.

For every operation:
  (a) the result against the oracle (oracle/gp_oracle.py) or a SciPy Cholesky on the host, at the tolerance the rest of the suite uses for that operation
      (logpdf 1e-10 relative — to max(|ref|, 1) as tests/batch_cases.py does, a one-point logpdf can be near zero —, α 1e-8 in norm, mean 1e-8, var / cov
      1e-9, rand 1e-7, gradients 1e-7, fp32 logpdf 1e-4; the VFE tolerances of tests/test_gpu_random_vfe.py / test_gpu_vfe_grad.py);
  (b) every host output entirely finite;
  (c) exact path only: with "deterministic" = 1 and "gemm_streamk" = 0 the poisoned context returns the same BITS as a clean context with the same settings
      — a dependence on stale finite data that stays inside the tolerance shows here, NaN only shows what happens to propagate.  The gradient entry points
      (gp_logpdf_grad, gp_logpdf_grad_sum, the dense-noise gradient) and the VFE / DTC path keep their floating-point atomics under "deterministic" = 1
      (include/gpmi355.h), so their tests run on a poisoned context alone, twice, with (a) and (b); the batch kernel's schedule is fixed, so its results are
      compared bit for bit with a clean context as well.

The last test is the production scenario with the parameter OFF: fits that stop with a PosDefException leave NaN in their factor, a failing batch problem
leaves NaN in α, and those blocks go back to the cache; the good calls that follow reuse them."""
import contextlib
import math

import numpy as np
import pytest
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_cases as bc
from tests.composite_ref import dense_data as _dense_data, ml_kernel as _ml_kernel, ref_kernelmatrix
from tests.conftest import rank_devices

pytestmark = pytest.mark.gpu

VAR, ELL, MEAN = 1.3, 0.7, 0.3
OK = o.Kernel(o.SE, VAR, 1.0 / ELL)
DET = {"deterministic": 1, "gemm_streamk": 0}
POOL_MB = 48  # small enough that the cache evicts (a factor of n = 2 500 is 53 MB: it stays as the one oversize block and displaces everything else)


def _kernel():
    return VAR * agp.with_lengthscale(agp.SqExponentialKernel(), ELL)


def _new_ctx(poison, params=None, pool_mb=POOL_MB):
    c = agp.Context(0)
    c.set_param("alloc_poison", 1 if poison else 0)
    c.set_param("pool_cap_mb", pool_mb)
    for k, v in (params or {}).items():
        c.set_param(k, v)
    return c


@contextlib.contextmanager
def _contexts(params=None, pool_mb=POOL_MB):
    """(poisoned ctx in the default schedule, poisoned ctx without atomics, clean ctx without atomics), closed on exit."""
    cs = []
    try:
        cs.append(_new_ctx(True, params, pool_mb))
        cs.append(_new_ctx(True, dict(params or {}, **DET), pool_mb))
        cs.append(_new_ctx(False, dict(params or {}, **DET), pool_mb))
        for c in cs[:2]:
            assert c.get_param("alloc_poison") == 1
        yield cs
    finally:
        for c in cs:
            c.close()


@contextlib.contextmanager
def _poisoned(params=None, pool_mb=POOL_MB):
    c = _new_ctx(True, params, pool_mb)
    try:
        yield c
    finally:
        c.close()


def _leaves(out, prefix=""):
    if isinstance(out, dict):
        for k, v in out.items():
            yield from _leaves(v, f"{prefix}{k}.")
    elif isinstance(out, (list, tuple)):
        for i, v in enumerate(out):
            yield from _leaves(v, f"{prefix}{i}.")
    elif out is not None:
        yield prefix[:-1], np.asarray(out)


def _assert_finite(out):
    for name, a in _leaves(out):
        assert np.all(np.isfinite(a)), f"{name}: {int(np.sum(~np.isfinite(a)))} of {a.size} entries are not finite"


def _assert_same_bits(a, b):
    la, lb = dict(_leaves(a)), dict(_leaves(b))
    assert la.keys() == lb.keys()
    for name in la:
        assert la[name].dtype == lb[name].dtype and la[name].shape == lb[name].shape, name
        if la[name].tobytes() != lb[name].tobytes():
            diff = np.flatnonzero(la[name].ravel().view(np.uint8 if la[name].dtype.itemsize == 1 else f"u{la[name].dtype.itemsize}")
                                  != lb[name].ravel().view(np.uint8 if lb[name].dtype.itemsize == 1 else f"u{lb[name].dtype.itemsize}"))
            raise AssertionError(f"{name}: poisoned and clean context differ in {diff.size} of {la[name].size} entries (first at flat index {diff[0]})")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _three_ways(run, check, params=None, pool_mb=POOL_MB):
    """run(ctx) -> nested dict of host outputs; check(out, det) asserts (a), det = a run without atomics.  (a) + (b) on the poisoned context in the default schedule and without atomics,
    (c) poisoned against clean."""
    with _contexts(params, pool_mb) as (cp, cpd, ccd):
        out = run(cp)
        _assert_finite(out)
        check(out)
        outp = run(cpd)
        _assert_finite(outp)
        check(outp, det=True)
        outc = run(ccd)
        _assert_same_bits(outp, outc)
        again = run(cpd)   # second pass: the blocks of the first one come back from the cache, poisoned again
        _assert_same_bits(again, outc)
        assert cpd.get_param("pool_blocks") >= 1   # blocks did cycle through the cache


# ---- noise forms -----------------------------------------------------------------------------------------------------------------------------------
def _dense_sigma(n, seed):
    """The test noise of tests/test_gpu_dense_noise.py: D^½ (0.05·0.6^|i−j|) D^½ + 0.01 I, exactly symmetric."""
    rng = np.random.default_rng(1000 + seed)
    sd = np.sqrt(0.5 + rng.uniform(0, 1, n))
    idx = np.arange(n, dtype=np.float64)
    S = 0.05 * np.power(0.6, np.abs(np.subtract.outer(idx, idx))) * sd[:, None] * sd[None, :]
    S[np.diag_indices(n)] += 0.01
    return 0.5 * (S + S.T)


def _noise(form, n, seed, dtype):
    """(what the mirror is given, the n×n fp64 matrix the host reference adds)"""
    if form == "scalar":
        return dtype(0.05), 0.05 * np.eye(n) if dtype == np.float64 else float(np.float32(0.05)) * np.eye(n)
    if form == "vector":
        v = (0.02 + np.random.default_rng(seed).uniform(0, 0.1, n)).astype(dtype)
        return v, np.diag(v.astype(np.float64))
    S = _dense_sigma(n, seed).astype(dtype)
    S_in = np.ascontiguousarray(S) if form == "dense_lower" else np.asfortranarray(S)   # C order: gp_noise kind 3, Fortran order: kind 2
    return S_in, S.astype(np.float64)


def _host_fit(K, S, delta):
    L = sla.cholesky(K + S, lower=True, check_finite=False)
    D = delta.reshape(len(delta), -1)
    A = sla.cho_solve((L, True), D, check_finite=False)
    logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
    sq = np.einsum("ij,ij->j", D, A)
    lp = -0.5 * (len(delta) * math.log(2 * math.pi) + logdet + sq)
    return lp, A, L, logdet, sq


# ---- fits ------------------------------------------------------------------------------------------------------------------------------------------
FIT_SIZES = [1, 65, 200, 1025, 2500]   # one leaf, one tile, several tiles, several panels of the nb below — none a multiple of 128


def _fit_case(n, form, dtype, params=None):
    rng = np.random.default_rng(n * 7 + len(form))
    X = rng.uniform(0, 3, size=(n, 3)).astype(dtype)
    Y = rng.standard_normal((n, 130)).astype(dtype)
    s_in, S = _noise(form, n, n, dtype)
    K = o.kernelmatrix(OK, X.astype(np.float64))
    lp_h, A_h, L_h, logdet_h, sq_h = _host_fit(K, S, Y.astype(np.float64) - MEAN)

    def run(ctx):
        f = agp.GP(MEAN, _kernel(), ctx=ctx)
        fx = f(agp.RowVecs(X), s_in)
        out = {"lp1": agp.logpdf(fx, Y[:, 0]), "lp3": agp.logpdf(fx, Y[:, :3]), "lp130": agp.logpdf(fx, Y)}
        post = agp.posterior(fx, Y[:, 0])
        out["alpha"], out["post_lp"], out["U"] = post.data.alpha, post.logpdf_value, post.data.C.U
        post.data.C.free()
        out["logdet"] = agp.logdetcov(fx)
        out["sqmahal"] = agp.sqmahal(fx, Y[:, :3])
        return out

    def check(out, det=False):
        assert not np.any(np.tril(out["U"], -1))   # the strictly lower part of C.U is exactly zero
        if dtype == np.float32:
            for key, cols in (("lp1", slice(0, 1)), ("lp3", slice(0, 3)), ("lp130", slice(0, 130))):
                got = np.atleast_1d(out[key])
                assert got.dtype == np.float32
                assert max(bc.lp_err(u, v) for u, v in zip(got, lp_h[cols])) <= 1e-4, key
            assert bc.lp_err(out["post_lp"], lp_h[0]) <= 1e-4
            return
        for key, cols in (("lp1", slice(0, 1)), ("lp3", slice(0, 3)), ("lp130", slice(0, 130))):
            assert max(bc.lp_err(u, v) for u, v in zip(np.atleast_1d(out[key]), lp_h[cols])) <= 1e-10, key
        assert bc.lp_err(out["post_lp"], lp_h[0]) <= 1e-10
        assert _rel(out["alpha"], A_h[:, 0]) <= 1e-8
        assert bc.lp_err(out["logdet"], logdet_h) <= 1e-10
        assert max(bc.lp_err(u, v) for u, v in zip(out["sqmahal"], sq_h[:3])) <= 1e-10
        assert np.max(np.abs(out["U"] - L_h.T)) <= 1e-10   # the bound tests/test_gpu_multi.py puts on the factor of a fit

    return run, check


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("form", ["scalar", "vector", "dense_upper", "dense_lower"])
@pytest.mark.parametrize("n", FIT_SIZES)
def test_fits(agp, n, form, dtype):
    """gp_logpdf (1, 3 and 130 columns of Y), gp_posterior_fit (+ the whole factor) and gp_logpdf_terms for every noise form; nb = 512, so that n = 1 025 and
    2 500 take several outer panels, and 1 MiB staging buffers, so that a dense Σy is uploaded in several pieces."""
    run, check = _fit_case(n, form, dtype)
    _three_ways(run, check, {"nb": 512, "dense_stage_mb": 1})


@pytest.mark.parametrize("params", [{"nb": 512, "lookahead": 1, "lookahead_min_n": 0}, {"nb": 0}, {"nb": 512, "leaf_cols": 64}, {}],
                         ids=["two-stream-lookahead", "recursive", "leaf_cols64", "defaults"])
@pytest.mark.parametrize("n", [1025, 2500])
def test_fit_schedules(agp, n, params):
    """The same fits under the two-stream look-ahead forced at a small size (as tests/test_gpu_parity.py::test_two_stream_lookahead_forced_at_a_small_size does),
    the purely recursive factorisation, 64-column leaves, and the default parameters."""
    run, check = _fit_case(n, "vector", np.float64)
    _three_ways(run, check, params)


# ---- predictions -----------------------------------------------------------------------------------------------------------------------------------
def _exact_problem(n, d=3, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
    s2 = 0.04 + 0.05 * rng.random(n)
    f = lambda ctx: agp.GP(0.2, 1.4 * agp.Matern52Kernel() @ agp.ScaleTransform(0.8), ctx=ctx)
    of = o.GP(o.Kernel(o.MATERN52, 1.4, 0.8), 0.2)
    return rng, X, y, s2, f, of


def _predict_all(post, xs):
    """every combination of the mean / var / cov bits of gp_posterior_predict"""
    return {f"what{w}": post._predict(agp.RowVecs(xs), w) for w in range(1, 8)}


def _check_predict(out, opost, xs):
    mo, co = opost.mean_and_cov(xs)
    for w in range(1, 8):
        m, v, c = out[f"what{w}"]
        assert (m is not None, v is not None, c is not None) == (bool(w & 1), bool(w & 2), bool(w & 4))
        if m is not None:
            np.testing.assert_allclose(m, mo, rtol=0, atol=1e-8)
        if v is not None:
            np.testing.assert_allclose(v, np.diag(co), rtol=0, atol=1e-9)
        if c is not None:
            np.testing.assert_allclose(c, co, rtol=0, atol=1e-9)


def _factor_outputs(post, B1, B130, xi):
    C = post.data.C
    return {"solve1": C.solve(B1), "solve130": C.solve(B130), "Ut_mul": C.Ut_mul(xi), "U": C.U}


def _check_factor(out, U_ref, B1, B130, xi, tol_u=1e-10):
    """C \\ B at 1e-8 in norm, C.U' ξ at 1e-10 and C.U at 1e-10 (a fit) / 1e-9 (an updated factor): the bounds of tests/test_gpu_multi.py"""
    assert _rel(out["solve1"], sla.cho_solve((U_ref, False), B1)) <= 1e-8
    assert _rel(out["solve130"], sla.cho_solve((U_ref, False), B130)) <= 1e-8
    np.testing.assert_allclose(out["Ut_mul"], U_ref.T @ xi, rtol=0, atol=1e-10)
    assert np.max(np.abs(out["U"] - U_ref)) <= tol_u
    assert not np.any(np.tril(out["U"], -1))


@pytest.mark.parametrize("dib_nb", [0, 512, 2048])
def test_predictions_from_a_posterior(agp, dib_nb):
    """From a posterior of n = 1 025: gp_posterior_predict with every combination of outputs at N* = 1, 37, 129, 1 500; gp_posterior_logpdf and
    gp_posterior_rand at N* = 11, 129, 700; gp_posterior_solve with 1 and 130 columns, gp_posterior_factor_mul, gp_posterior_get_factor — with the forward
    solves through inverse diagonal blocks of two widths and through the substitution leaves."""
    n = 1025
    rng, X, y, s2, f, of = _exact_problem(n)
    opost = o.posterior(o.FiniteGP(of, X, s2), y)
    xs_all = rng.standard_normal((1500, 3))
    B1, B130, xi = rng.standard_normal(n), rng.standard_normal((n, 130)), rng.standard_normal((n, 2))
    joint = {}
    for ns in (11, 129, 700):
        joint[ns] = (rng.standard_normal((ns, 3)), 0.05 + 0.2 * rng.random(ns), rng.standard_normal((ns, 3)), rng.standard_normal((ns, 4)))

    def run(ctx):
        post = agp.posterior(f(ctx)(agp.RowVecs(X), s2), y)
        out = {f"predict{ns}": _predict_all(post, xs_all[:ns]) for ns in (1, 37, 129, 1500)}
        for ns, (xs, s2s, ys, z) in joint.items():
            pfx = post(agp.RowVecs(xs), s2s)
            out[f"joint{ns}"] = {"logpdf1": agp.logpdf(pfx, ys[:, 0]), "logpdf3": agp.logpdf(pfx, ys), "rand": agp.rand(pfx, 4, xi=z)}
        out["factor"] = _factor_outputs(post, B1, B130, xi)
        post.data.C.free()
        return out

    def check(out, det=False):
        for ns in (1, 37, 129, 1500):
            _check_predict(out[f"predict{ns}"], opost, xs_all[:ns])
        for ns, (xs, s2s, ys, z) in joint.items():
            opfx = o.FiniteGP(opost, xs, s2s)
            ref = o.logpdf(opfx, ys)
            assert max(bc.lp_err(u, v) for u, v in zip(out[f"joint{ns}"]["logpdf3"], ref)) <= 1e-9   # what tests/test_gpu_api.py asks of the held-out logpdf
            assert bc.lp_err(out[f"joint{ns}"]["logpdf1"], ref[0]) <= 1e-9
            np.testing.assert_allclose(out[f"joint{ns}"]["rand"], o.rand_from(opfx, z), rtol=0, atol=1e-7)
        _check_factor(out["factor"], opost.U, B1, B130, xi)

    _three_ways(run, check, {"dib_nb": dib_nb})


# ---- sequential updates ----------------------------------------------------------------------------------------------------------------------------
def _update_chain(sizes, seed):
    """Fit sizes[0] points, then condition on sizes[1:] batch by batch.  After every update: predictions (mean / var / cov in every combination), a held-out
    logpdf, C \\ B, C.U' ξ and the whole factor from the UPDATED handle against the oracle's BATCH fit on all points so far; then the old handle again."""
    ntot = sum(sizes)
    rng, X, y, s2, f, of = _exact_problem(ntot, seed=seed)
    xs = rng.standard_normal((150, 3))
    s2s, ys = 0.05 + 0.2 * rng.random(150), rng.standard_normal((150, 2))
    ends = np.cumsum(sizes)
    rhs = {int(e): (rng.standard_normal(int(e)), rng.standard_normal((int(e), 130)), rng.standard_normal((int(e), 2))) for e in ends}
    batch = {int(e): o.posterior(o.FiniteGP(of, X[:e], s2[:e]), y[:e]) for e in ends}
    batch_lp = {int(e): float(o.logpdf(o.FiniteGP(of, X[:e], s2[:e]), y[:e])) for e in ends}

    def stage(post, e):
        pfx = post(agp.RowVecs(xs), s2s)
        return {"alpha": post.data.alpha, "lp": post.logpdf_value, "predict": _predict_all(post, xs), "heldout": agp.logpdf(pfx, ys),
                "factor": _factor_outputs(post, *rhs[e])}

    def run(ctx):
        posts = [agp.posterior(f(ctx)(agp.RowVecs(X[:ends[0]]), s2[:ends[0]]), y[:ends[0]])]
        out = {"stage0": stage(posts[0], int(ends[0]))}
        for i in range(1, len(sizes)):
            a, b = ends[i - 1], ends[i]
            posts.append(agp.posterior(posts[-1](agp.RowVecs(X[a:b]), s2[a:b]), y[a:b]))
            out[f"stage{i}"] = stage(posts[-1], int(b))
        out["old"] = {f"stage{i}": stage(p, int(ends[i])) for i, p in enumerate(posts[:-1])}   # every older handle still answers, unchanged
        for p in posts:
            p.data.C.free()
        return out

    def check_stage(st, e, updated):
        ob = batch[e]
        assert _rel(st["alpha"], ob.alpha) <= 1e-8
        assert bc.lp_err(st["lp"], batch_lp[e]) <= 1e-10
        _check_predict(st["predict"], ob, xs)
        ref = o.logpdf(o.FiniteGP(ob, xs, s2s), ys)
        assert max(bc.lp_err(u, v) for u, v in zip(st["heldout"], ref)) <= 1e-9
        _check_factor(st["factor"], ob.U, *rhs[e], tol_u=1e-9 if updated else 1e-10)

    def check(out, det=False):
        for i, e in enumerate(ends):
            check_stage(out[f"stage{i}"], int(e), i > 0)
        for i, e in enumerate(ends[:-1]):
            check_stage(out["old"][f"stage{i}"], int(e), i > 0)
            if det:
                _assert_same_bits(out["old"][f"stage{i}"], out[f"stage{i}"])

    return run, check


@pytest.mark.parametrize("sizes", [(65, 1), (300, 77), (1000, 500), (127, 129), (200, 9, 130, 64)], ids=lambda s: "+".join(map(str, s)))
@pytest.mark.parametrize("dib_nb", [2048, 0])
def test_sequential_updates(agp, sizes, dib_nb):
    """gp_posterior_update: the extended factor is assembled in a fresh block from L11, U12ᵀ and chol(S) plus the identity padding; the region to the right of
    L11 (rows < n1, columns >= n1) lies inside the diagonal tiles at the seam whenever n1 is not a multiple of the tile size, and is loaded whole by the
    forward-solve leaves and the inverse-diagonal-block build."""
    run, check = _update_chain(sizes, seed=sum(sizes))
    _three_ways(run, check, {"dib_nb": dib_nb})


# ---- gradients -------------------------------------------------------------------------------------------------------------------------------------
def _grad_close(a, ref, what):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    err = np.max(np.abs(a - ref)) / max(np.max(np.abs(ref)), 1.0)
    assert err <= 1e-7, (what, err)


@pytest.mark.parametrize("d,n", [(3, 700), (17, 450)])
def test_logpdf_grad_with_wrt_x(agp, d, n):
    rng = np.random.default_rng(d)
    X = rng.standard_normal((n, d)) / math.sqrt(d / 3)
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
    sc = np.linspace(0.5, 1.1, d)
    sig = rng.uniform(0.03, 0.1, n)
    ofx = o.FiniteGP(o.GP(o.Kernel(o.MATERN52, 1.4, sc), 0.2), X, sig)
    go, lpo = o.logpdf_grad(ofx, y), float(o.logpdf(ofx, y))
    with _poisoned() as ctx:
        f = agp.GP(0.2, 1.4 * agp.Matern52Kernel() @ agp.ARDTransform(sc), ctx=ctx)
        for rep in range(2):
            lp, g = agp.logpdf_and_grad(f(agp.RowVecs(X), sig), y, wrt_x=True)
            _assert_finite({"lp": lp, "g": g})
            assert bc.lp_err(lp, lpo) <= 1e-10
            for key in ("variance", "scale", "noise", "y", "mean", "x"):
                _grad_close(g[key], go[key], key)
        assert ctx.get_param("pool_blocks") >= 1


def test_logpdf_grad_sum_on_the_mauna_loa_form(agp):
    """gp_logpdf_grad_sum on the Mauna Loa form with amplitudes of order 1 (tests/composite_ref.py ml_kernel: the one the suite holds to 1e-10 / 1e-8)."""
    x, y = _dense_data(1000, seed=81)
    k, s2 = _ml_kernel(), 0.1
    K, dK = ref_kernelmatrix(k, x, grad=True)
    lp_h, A_h, L_h, _, _ = _host_fit(K, s2 * np.eye(len(x)), y)
    a = A_h[:, 0]
    W = np.outer(a, a) - sla.cho_solve((L_h, True), np.eye(len(x)))
    gt, gn = np.array([0.5 * np.sum(W * D) for D in dK]), 0.5 * np.trace(W)
    with _poisoned() as ctx:
        for rep in range(2):
            lp, g = agp.logpdf_and_grad(agp.GP(k, ctx=ctx)(x, s2), y)
            _assert_finite({"lp": lp, "g": g})
            assert bc.lp_err(lp, lp_h[0]) <= 1e-10
            np.testing.assert_allclose(g["theta"], gt, rtol=1e-7, atol=1e-9 * np.abs(gt).max())   # the bound of tests/test_gpu_composite.py
            assert g["noise"] == pytest.approx(gn, rel=1e-7)
            assert _rel(g["y"], -a) <= 1e-8
        assert ctx.get_param("pool_blocks") >= 1


@pytest.mark.parametrize("form", ["dense_upper", "dense_lower"])
def test_dense_noise_gradient(agp, form):
    n = 700
    rng = np.random.default_rng(71)
    X, y = rng.uniform(0, 3, size=(n, 3)), rng.standard_normal(n)
    s_in, S = _noise(form, n, 71, np.float64)
    K = o.kernelmatrix(OK, X)
    lp_h, A_h, L_h, _, _ = _host_fit(K, S, y)
    a = A_h[:, 0]
    G_h = 0.5 * (np.outer(a, a) - sla.cho_solve((L_h, True), np.eye(n)))
    s = 1.0 / ELL
    dK_ds = K * (-0.5) * (-2.0 * np.log(K / VAR)) * 2.0 / s
    with _poisoned({"dense_stage_mb": 1}) as ctx:
        for rep in range(2):
            lp, g = agp.logpdf_and_grad(agp.GP(_kernel(), ctx=ctx)(agp.RowVecs(X), s_in), y)
            _assert_finite({"lp": lp, "g": g})   # all of the n×n "noise" block
            assert bc.lp_err(lp, lp_h[0]) <= 1e-10
            assert g["noise"].shape == (n, n) and np.array_equal(g["noise"], g["noise"].T)
            np.testing.assert_allclose(g["noise"], G_h, rtol=1e-7, atol=1e-9 * np.max(np.abs(G_h)))
            assert g["variance"] == pytest.approx(float(np.sum(G_h * K) / VAR), rel=1e-7)
            assert g["scale"] == pytest.approx(float(np.sum(G_h * dK_ds)), rel=1e-7)
            assert _rel(g["y"], -a) <= 1e-8


# ---- composite kernels -----------------------------------------------------------------------------------------------------------------------------
def test_composite_fit_predictions_and_update(agp):
    """gp_posterior_fit_sum / gp_logpdf_sum / gp_kernelmatrix_sum, predictions, and one sequential update on a composite posterior."""
    n, n1 = 1100, 777
    x, y = _dense_data(n, seed=11)
    k, s2 = _ml_kernel(), 0.1
    sc = agp.api._prior_variance(k)
    rng = np.random.default_rng(12)
    xs = np.concatenate([x[rng.choice(n, 40, replace=False)], rng.uniform(0, x[-1] + 2, 160)])
    Kxx, Ksx, Kss = ref_kernelmatrix(k, x), ref_kernelmatrix(k, xs, x), ref_kernelmatrix(k, xs)
    lp_h, A_h, L_h, _, _ = _host_fit(Kxx, s2 * np.eye(n), y)
    V = sla.solve_triangular(L_h, Ksx.T, lower=True)
    m_h, C_h = Ksx @ A_h[:, 0], Kss - V.T @ V

    def run(ctx):
        f = agp.GP(k, ctx=ctx)
        post = agp.posterior(f(x, s2), y)
        p1 = agp.posterior(f(x[:n1], s2), y[:n1])
        p2 = agp.posterior(p1(x[n1:], s2), y[n1:])
        out = {"K": agp.kernelmatrix(k, x[:333], ctx=ctx), "Kxz": agp.kernelmatrix(k, x[:333], xs, ctx=ctx), "lp": agp.logpdf(f(x, s2), y),
               "post_lp": post.logpdf_value, "alpha": post.data.alpha, "predict": {f"what{w}": post._predict(xs, w) for w in range(1, 8)},
               "upd_alpha": p2.data.alpha, "upd_lp": p2.logpdf_value, "upd_predict": {f"what{w}": p2._predict(xs, w) for w in range(1, 8)}, "upd_U": p2.data.C.U}
        for p in (post, p1, p2):
            p.data.C.free()
        return out

    def check(out, det=False):
        np.testing.assert_allclose(out["K"], Kxx[:333, :333], rtol=0, atol=1e-13 * sc)   # the bound of tests/test_gpu_composite.py for gp_kernelmatrix_sum
        np.testing.assert_allclose(out["Kxz"], Ksx.T[:333], rtol=0, atol=1e-13 * sc)
        assert bc.lp_err(out["lp"], lp_h[0]) <= 1e-10 and bc.lp_err(out["post_lp"], lp_h[0]) <= 1e-10
        assert _rel(out["alpha"], A_h[:, 0]) <= 1e-8
        for pre, key_a in (("", "alpha"), ("upd_", "upd_alpha")):
            assert _rel(out[key_a], A_h[:, 0]) <= 1e-8
            for w in range(1, 8):
                m, v, c = out[pre + "predict"][f"what{w}"]
                if m is not None:
                    np.testing.assert_allclose(m, m_h, rtol=0, atol=1e-8 * np.abs(m_h).max())
                if v is not None:
                    np.testing.assert_allclose(v, np.diag(C_h), rtol=0, atol=1e-9 * sc)
                if c is not None:
                    np.testing.assert_allclose(c, C_h, rtol=0, atol=1e-9 * sc)
        assert bc.lp_err(out["upd_lp"], lp_h[0]) <= 1e-10
        assert np.max(np.abs(out["upd_U"] - L_h.T)) <= 1e-9
        assert not np.any(np.tril(out["upd_U"], -1))

    _three_ways(run, check)


# ---- VFE / DTC -------------------------------------------------------------------------------------------------------------------------------------
class Fp32DtcVarianceOff(AssertionError):
    """the known finding below, and nothing else"""


FP32_DTC_FINDING = ("gp_vfe_grad on an fp32 DTC handle with M = 40: d/dvariance is 6.3e-3 from the fp64 oracle (bound 2e-3·max(|ref|, 1), reference 0.86) on a clean "
                    "and on a poisoned context alike.  Not a stale-block dependence: the fp32 chunk SYRK of csrc/vfe.hpp (launch_gemm<float>, gemm_nt_dma, into the fp32 "
                    "scratch that add_lower_batched_kernel sums into D_acc) rounds the M×M accumulator D_acc = B Bᵀ, whose entries are of size tr(B Bᵀ) ≈ 2e4, and "
                    "the backward pass forms tr(C⁻¹ Q_ff) <= M from it by the Woodbury identity; the ELBO's trace term (−3 336) hides the same error for VFE.  "
                    "The fp32 GEMM / SYRK kernels themselves are inside their rounding bounds (tests/test_gpu_units_f32.py: exact on integer operands, at most 0.01 of "
                    "γ_{k+2·CUs}(|C₀| + |A||B|ᵀ) up to k = 20 000), so the miss is rounding amplified by the cancellation, not a kernel fault")


def _sparse_case(m, approx, dtype, variance_against):
    """variance_against = "oracle": every gradient block against the oracle; "clean": ∂/∂variance against the same call on a clean context instead (the other
    blocks still against the oracle)."""
    n, n2, m2, d = 4200, 300, 25, 3
    f64 = dtype == np.float64
    jitter = 1e-4 if f64 else 1e-3
    rng = np.random.default_rng(m)
    X = rng.uniform(-2, 2, (n + n2, d)).astype(dtype)
    y = (np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n + n2)).astype(dtype)
    perm = rng.permutation(n)
    Z = (X[perm[:m]] + 0.01 * rng.standard_normal((m, d))).astype(dtype)
    Z2 = (X[perm[m:m + m2]] + 0.01 * rng.standard_normal((m2, d))).astype(dtype)
    s2 = rng.uniform(0.05, 0.3, n + n2).astype(dtype)
    xs = rng.uniform(-2, 2, (70, d)).astype(dtype)
    s2s, ys, xi = (0.1 + 0.1 * rng.random(70)).astype(dtype), rng.standard_normal(70).astype(dtype), rng.standard_normal((70, 2)).astype(dtype)
    X64, y64, Z64, Z264, s264, xs64 = (a.astype(np.float64) for a in (X, y, Z, Z2, s2, xs))
    of = o.GP(o.Kernel(o.MATERN32, 1.2, 0.7))
    vfe = approx == "VFE"
    ofx1, ofx = o.FiniteGP(of, X64[:n], s264[:n]), o.FiniteGP(of, X64, s264)
    o1 = o.vfe_posterior(of, Z64, jitter, ofx1, y64[:n])
    obj1 = o.elbo(of, Z64, jitter, ofx1, y64[:n]) if vfe else o.dtc_log_evidence(of, Z64, jitter, ofx1, y64[:n])
    g1 = o.elbo_grad(of, Z64, jitter, ofx1, y64[:n], vfe=vfe)
    o2 = o.vfe_posterior(of, Z64, jitter, ofx, y64)
    obj2 = o.elbo(of, Z64, jitter, ofx, y64) if vfe else o.dtc_log_evidence(of, Z64, jitter, ofx, y64)
    o3 = o.vfe_update_z(o.vfe_update_obs(o1, o.FiniteGP(of, X64[n:], s264[n:]), y64[n:]), Z264)
    obj3 = o.objective_from_posterior(o3, ofx, y64, vfe=vfe)
    tol_m, tol_v, tol_lp, tol_r, tol_app = (1e-7, 1e-8, 1e-7, 1e-6, 1e-6) if f64 else (2e-2, 2e-2, None, 2e-2, 2e-2)
    with _poisoned({"vfe_chunk": 2048}) as ctx:
        f = agp.GP(1.2 * agp.Matern32Kernel() @ agp.ScaleTransform(0.7), ctx=ctx)
        A = agp.VFE if vfe else agp.DTC
        for rep in range(2):
            p1 = agp.posterior(A(f(agp.RowVecs(Z), jitter)), f(agp.RowVecs(X[:n]), s2[:n]), y[:n])
            out = {"obj": p1.objective, "predict": {w: p1._predict(agp.RowVecs(xs), w) for w in range(1, 8)}, "data": {k: p1.data[k] for k in p1.data},
                   "grad": p1.objective_grad(wrt_x=True)}
            pfx = p1(agp.RowVecs(xs), s2s)
            out["logpdf"], out["rand"] = agp.logpdf(pfx, ys), agp.rand(pfx, 2, xi=xi)
            p2 = agp.update_posterior(p1, f(agp.RowVecs(X[n:]), s2[n:]), y[n:])
            out["upd"] = {"obj": p2.objective, "predict": p2._predict(agp.RowVecs(xs), 7), "data": {k: p2.data[k] for k in p2.data}}
            p3 = agp.update_posterior(p2, f(agp.RowVecs(Z2), jitter))
            out["app"] = {"obj": p3.objective, "predict": p3._predict(agp.RowVecs(xs), 7), "data": {k: p3.data[k] for k in p3.data}}
            out["old"] = p1._predict(agp.RowVecs(xs), 7)
            _assert_finite(out)
            for key in ("U", "Lam_U"):   # gp_vfe_get_factors: M×M upper factors, strictly lower part exactly zero
                for part in (out["data"], out["upd"]["data"], out["app"]["data"]):
                    assert not np.any(np.tril(part[key], -1)), key
            assert float(out["obj"]) == pytest.approx(obj1, rel=1e-8 if f64 else 1e-4)
            assert float(out["upd"]["obj"]) == pytest.approx(obj2, rel=1e-8 if f64 else 1e-4)
            assert float(out["app"]["obj"]) == pytest.approx(obj3, rel=1e-8 if f64 else 2e-4)   # (tests/test_gpu_api.py::test_vfe_append_pseudo_points)
            mo, co = o1.mean_and_cov(xs64)
            for w, (mu, v, c) in out["predict"].items():
                if mu is not None:
                    np.testing.assert_allclose(mu, mo, rtol=0, atol=tol_m)
                if v is not None:
                    np.testing.assert_allclose(v, np.diag(co), rtol=0, atol=tol_v)
                if c is not None:
                    np.testing.assert_allclose(c, co, rtol=0, atol=tol_v)
            np.testing.assert_allclose(out["old"][0], mo, rtol=0, atol=tol_m)
            mo2, co2 = o2.mean_and_cov(xs64)
            np.testing.assert_allclose(out["upd"]["predict"][0], mo2, rtol=0, atol=tol_m)
            np.testing.assert_allclose(out["upd"]["predict"][1], np.diag(co2), rtol=0, atol=tol_v)
            np.testing.assert_allclose(out["upd"]["predict"][2], co2, rtol=0, atol=tol_v)
            mo3, co3 = o3.mean_and_cov(xs64)
            np.testing.assert_allclose(out["app"]["predict"][0], mo3, rtol=0, atol=tol_app)
            np.testing.assert_allclose(out["app"]["predict"][1], np.diag(co3), rtol=0, atol=tol_app)
            opfx = o.FiniteGP(o1, xs64, s2s.astype(np.float64))
            np.testing.assert_allclose(out["rand"], o.rand_from(opfx, xi.astype(np.float64)), rtol=0, atol=tol_r)
            if f64:
                np.testing.assert_allclose(out["app"]["predict"][2], co3, rtol=0, atol=tol_app)
                assert out["logpdf"] == pytest.approx(float(o.logpdf(opfx, ys)), rel=tol_lp)
            g, tol_g = out["grad"], 1e-7 if f64 else 2e-3
            assert ("z" in g) == f64   # ∂/∂z needs an fp64 handle (include/gpmi355.h gp_vfe_grad)
            for key, ref in (("variance", g1["variance"]), ("scale", g1["scale"]), ("noise_diag", g1["noise"]), ("noise", np.sum(g1["noise"])), ("y", g1["y"]),
                             ("mean", g1["mean"]), ("x", g1["x"])) + ((("z", g1["z"]),) if f64 else ()):
                a, b = np.asarray(g[key], dtype=np.float64), np.asarray(ref, dtype=np.float64)
                assert a.shape == b.shape, key
                err, scale = np.max(np.abs(a - b)), max(np.max(np.abs(b)), 1.0)
                if key == "variance" and variance_against == "clean":
                    # the two runs differ in the order of the fp64 atomic adds of the backward pass only: the suite's fp64 gradient bound
                    with contextlib.closing(_new_ctx(False, {"vfe_chunk": 2048})) as clean:
                        fc = agp.GP(1.2 * agp.Matern32Kernel() @ agp.ScaleTransform(0.7), ctx=clean)
                        gc = agp.posterior(A(fc(agp.RowVecs(Z), jitter)), fc(agp.RowVecs(X[:n]), s2[:n]), y[:n]).objective_grad()["variance"]
                    print(f"d/dvariance: poisoned {float(a):.10e} clean {float(gc):.10e} oracle {float(b):.10e}")
                    assert abs(float(a) - float(gc)) <= 1e-7 * scale, (key, float(a), float(gc))
                    continue
                if key == "variance" and not f64 and err > tol_g * scale:
                    raise Fp32DtcVarianceOff(f"{key}: {err:.2e} > {tol_g * scale:.1e}")
                assert err <= tol_g * scale, (key, err, tol_g * scale)
        assert ctx.get_param("pool_blocks") >= 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("approx", ["VFE", "DTC"])
@pytest.mark.parametrize("m", [40, 130, 700])
def test_sparse_fit_update_append_predict_and_gradient(agp, m, approx, dtype):
    """gp_vfe_fit streamed in three chunks of at most 2 048 points (ragged tail), gp_vfe_update, gp_vfe_append, gp_vfe_predict, gp_vfe_logpdf / gp_vfe_rand,
    gp_vfe_get / gp_vfe_get_factors and gp_vfe_grad with ∂/∂z and ∂/∂x.  fp64 at the tolerances of tests/test_gpu_random_vfe.py (objective 1e-8, mean 1e-7,
    var / cov 1e-8), tests/test_gpu_api.py (held-out logpdf 1e-7, rand 1e-6, append 1e-6) and tests/test_gpu_vfe_grad.py (1e-7); fp32 at theirs (objective 1e-4,
    predictions 2e-2 — rand, the predictive mean plus a factor of the predictive covariance times ξ, on that bound too —, gradient 2e-3; the suite has no fp32 bound
    for a held-out logpdf on a sparse posterior: finite).  One entry of one case misses the oracle bound for a reason that has nothing to do with stale blocks
    (FP32_DTC_FINDING): for it this test requires the poisoned context to agree with a clean one, and
    test_fp32_dtc_variance_gradient_at_few_pseudo_points keeps the oracle bound as a strict xfail."""
    known = (m, approx, dtype) == (40, "DTC", np.float32)
    _sparse_case(m, approx, dtype, "clean" if known else "oracle")


@pytest.mark.xfail(raises=Fp32DtcVarianceOff, strict=True, reason=FP32_DTC_FINDING)
def test_fp32_dtc_variance_gradient_at_few_pseudo_points(agp):
    _sparse_case(40, "DTC", np.float32, "oracle")


# ---- batch -----------------------------------------------------------------------------------------------------------------------------------------
def _on(ctx, cases):
    """the problems of tests/batch_cases.py on a context of the test's own"""
    out = []
    for c in cases:
        f = c["fx"].f
        g = agp.GP(f.kernel, ctx=ctx) if f.mean_fn is None else agp.GP(f.mean_fn, f.kernel, ctx=ctx)
        out.append(dict(c, fx=agp.FiniteGP(g, c["fx"].x, c["fx"].sigma2)))
    return out


def _batch(cases, **kw):
    return agp.logpdf_batch([c["fx"] for c in cases], [c["y"] for c in cases], **kw)


def test_ragged_batch(agp):
    """bc.ragged_cases(): the batch kernel and the problems routed to the single path, in one call."""
    ref = [bc.oracle_fit(c) for c in bc.ragged_cases()]
    with _poisoned() as ctx, contextlib.closing(_new_ctx(False)) as clean:
        cases = _on(ctx, bc.ragged_cases())
        served = np.array([c["n"] <= agp._lib.batch_max_n() for c in cases])
        assert served.any() and not served.all()
        lp_c, al_c = _batch(_on(clean, bc.ragged_cases()), return_alpha=True)
        for rep in range(2):
            lp, al = _batch(cases, return_alpha=True)
            _assert_finite({"lp": lp, "alpha": al})
            for b, (lp_o, a_o) in enumerate(ref):
                assert bc.lp_err(lp[b], lp_o) <= 1e-10 and bc.vec_err(al[b], a_o) <= 1e-8, (b, cases[b]["n"])
            # the batch kernel's schedule is fixed: the same bits as on a clean context
            assert lp[served].tobytes() == lp_c[served].tobytes()
            assert all(al[b].tobytes() == al_c[b].tobytes() for b in np.flatnonzero(served))


def test_two_waves_share_the_workspace(agp):
    """2 200 problems of n = 64: more than the 2 048 one launch takes, so the second wave runs in the first one's workspace."""
    B, n = 2200, 64
    rng = np.random.default_rng(8)
    X = rng.uniform(0, 4, size=(B, n, 2))
    Y = rng.standard_normal((B, n))
    kinds = [agp.SqExponentialKernel, agp.Matern12Kernel, agp.Matern32Kernel, agp.Matern52Kernel]
    ys = [Y[b] for b in range(B)]
    with _poisoned() as ctx, contextlib.closing(_new_ctx(False)) as clean:
        def fxs(c):
            return [agp.GP((1.0 + 1e-4 * b) * kinds[b % 4]() @ agp.ScaleTransform(0.7), ctx=c)(agp.RowVecs(X[b]), 0.02) for b in range(B)]

        lp_c = agp.logpdf_batch(fxs(clean), ys)
        for rep in range(2):
            lp, al = agp.logpdf_batch(fxs(ctx), ys, return_alpha=True)
            _assert_finite({"lp": lp, "alpha": al})
            assert lp.tobytes() == lp_c.tobytes()
        worst = 0.0
        for b in range(B):
            ofx = o.FiniteGP(o.GP(o.Kernel(b % 4, 1.0 + 1e-4 * b, 0.7)), X[b], 0.02)
            worst = max(worst, bc.lp_err(lp[b], o.logpdf(ofx, Y[b])))
        assert worst <= 1e-10


def _with_failures(cases, where):
    bad, idx = list(cases), {}
    for b, at in where:
        c = cases[b]
        s2 = np.array(np.broadcast_to(c["s2"], (c["n"],)), dtype=np.float64)
        i = int(at * (c["n"] - 1))
        s2[i] = -10.0
        bad[b] = dict(c, fx=agp.FiniteGP(c["fx"].f, c["fx"].x, s2))
        idx[b] = i + 1
    return bad, idx


def test_failing_problems_do_not_touch_their_neighbours(agp):
    with _poisoned() as ctx:
        good = _on(ctx, bc.small_cases(64, seed=6, lo=40))
        lp_good, a_good = _batch(good, return_alpha=True)
        _assert_finite({"lp": lp_good, "alpha": a_good})
        bad, _ = _with_failures(good, ((3, 0.4), (40, 0.9)))
        for rep in range(2):
            lp, al = _batch(bad, return_alpha=True, on_error="nan")
            assert sorted(np.flatnonzero(np.isnan(lp)).tolist()) == [3, 40]
            for b in range(64):
                if b in (3, 40):
                    assert np.isnan(al[b]).all()
                else:
                    assert lp[b].tobytes() == lp_good[b].tobytes() and al[b].tobytes() == a_good[b].tobytes(), b
        for b, c in enumerate(good):
            lp_o, a_o = bc.oracle_fit(c)
            assert bc.lp_err(lp_good[b], lp_o) <= 1e-10 and bc.vec_err(a_good[b], a_o) <= 1e-8


# ---- multi-device ----------------------------------------------------------------------------------------------------------------------------------
def test_multi_device_rank_contexts(agp, monkeypatch):
    """The rank contexts of a multi-device ctx allocate their matrix pieces and operand buffers through ctx_alloc too: GPMI_PARAMS carries the parameter into
    gp_ctx_create (the workspaces a rank context creates when it is primed), gp_ctx_set_param forwards it like every other single-device parameter.
    2×2 virtual ranks, n = 2 300, nb = 256: fit, predictive variance on the pieces, one update."""
    n, n2, d = 2300, 333, 3
    x, y = o.synth_inputs(n + n2, d, 64)
    rng = np.random.default_rng(29)
    s2 = 0.03 + 0.05 * rng.random(n + n2)
    of = o.GP(o.Kernel(o.MATERN32, 1.7, 0.7), -0.3)
    ofx = o.FiniteGP(of, x[:n], s2[:n])
    opost, opost2 = o.posterior(ofx, y[:n]), o.posterior(o.FiniteGP(of, x, s2), y)
    xs = rng.standard_normal((333, d)) * 1.1
    assert agp.default_context(0) is not None   # the shared context exists before the environment carries the diagnostic
    monkeypatch.setenv("GPMI_PARAMS", "alloc_poison=1")
    ctx = agp.Context(devices=rank_devices(4), P=2, Q=2, nb=256)
    monkeypatch.delenv("GPMI_PARAMS")
    try:
        ctx.set_param("alloc_poison", 1)
        ctx.set_param("pool_cap_mb", POOL_MB)
        assert ctx.get_param("alloc_poison") == 1
        f = agp.GP(-0.3, 1.7 * agp.Matern32Kernel() @ agp.ScaleTransform(0.7), ctx=ctx)
        for rep in range(2):
            post = agp.posterior(f(agp.RowVecs(x[:n]), s2[:n]), y[:n])
            lp = agp.logpdf(f(agp.RowVecs(x[:n]), s2[:n]), y[:n])
            m, v = post.mean_and_var(agp.RowVecs(xs))
            p2 = agp.posterior(post(agp.RowVecs(x[n:]), s2[n:]), y[n:])
            m2, v2 = p2.mean_and_var(agp.RowVecs(xs))
            _assert_finite([post.data.alpha, post.logpdf_value, lp, m, v, p2.data.alpha, p2.logpdf_value, m2, v2])
            lp_o = float(o.logpdf(ofx, y[:n]))
            assert bc.lp_err(lp, lp_o) <= 1e-10 and bc.lp_err(post.logpdf_value, lp_o) <= 1e-10
            assert _rel(post.data.alpha, opost.alpha) <= 1e-8 and _rel(p2.data.alpha, opost2.alpha) <= 1e-8
            mo, vo = opost.mean_and_var(xs)
            np.testing.assert_allclose(m, mo, rtol=0, atol=1e-8)
            np.testing.assert_allclose(v, vo, rtol=0, atol=1e-9)
            mo2, vo2 = opost2.mean_and_var(xs)
            np.testing.assert_allclose(m2, mo2, rtol=0, atol=1e-8)
            np.testing.assert_allclose(v2, vo2, rtol=0, atol=1e-9)
            U = p2.data.C.U   # gathers the extended pieces
            _assert_finite(U)
            assert np.max(np.abs(U - opost2.U)) <= 1e-9 and not np.any(np.tril(U, -1))
            for p in (post, p2):
                p.data.C.free()
    finally:
        ctx.close()


# ---- the production scenario: alloc_poison OFF, NaN left behind by failed calls ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", [200, 1025])
def test_blocks_left_by_failed_fits_are_reused_by_good_calls(agp, n, dtype):
    """An optimiser that steps onto a non-positive-definite point and carries on: a fit that stops with a PosDefException (negative noise entry at 0.4·n) and a
    batch call with failing problems leave NaN in blocks that go back to the ctx's cache; a good fit, predictions and an update of the same sizes then take
    exactly those blocks ("pool_blocks" / "pool_cached_mb" show the reuse).  Oracle tolerances, and under "deterministic" = 1 the same bits as a fresh context."""
    f64 = dtype == np.float64
    n2 = 77
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n + n2, 3)).astype(dtype)
    y = (np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n + n2)).astype(dtype)
    s2 = (0.04 + 0.05 * rng.random(n + n2)).astype(dtype)
    bad_s2 = s2[:n].copy()
    bad_s2[int(0.4 * n)] = -10.0
    xs = rng.standard_normal((129, 3)).astype(dtype)
    of = o.GP(o.Kernel(o.MATERN52, 1.4, 0.8), 0.2)
    X64, y64, s264, xs64 = (a.astype(np.float64) for a in (X, y, s2, xs))
    ofx = o.FiniteGP(of, X64[:n], s264[:n])
    opost, opost2 = o.posterior(ofx, y64[:n]), o.posterior(o.FiniteGP(of, X64, s264), y64)
    lp_o, lp2_o = float(o.logpdf(ofx, y64[:n])), float(o.logpdf(o.FiniteGP(of, X64, s264), y64))
    small = bc.small_cases(16, seed=n, lo=40)

    def good(ctx):
        f = agp.GP(0.2, 1.4 * agp.Matern52Kernel() @ agp.ScaleTransform(0.8), ctx=ctx)
        post = agp.posterior(f(agp.RowVecs(X[:n]), s2[:n]), y[:n])
        out = {"lp": agp.logpdf(f(agp.RowVecs(X[:n]), s2[:n]), y[:n]), "post_lp": post.logpdf_value, "alpha": post.data.alpha,
               "predict": post._predict(agp.RowVecs(xs), 7), "U": post.data.C.U}
        p2 = agp.posterior(post(agp.RowVecs(X[n:]), s2[n:]), y[n:])
        out.update({"upd_lp": p2.logpdf_value, "upd_alpha": p2.data.alpha, "upd_predict": p2._predict(agp.RowVecs(xs), 7), "upd_U": p2.data.C.U})
        for p in (post, p2):
            p.data.C.free()
        return out

    def failures(ctx):
        f = agp.GP(0.2, 1.4 * agp.Matern52Kernel() @ agp.ScaleTransform(0.8), ctx=ctx)
        with pytest.raises(agp.PosDefException):
            agp.posterior(f(agp.RowVecs(X[:n]), bad_s2), y[:n])
        with pytest.raises(agp.PosDefException):
            agp.logpdf(f(agp.RowVecs(X[:n]), bad_s2), y[:n])
        bad, _ = _with_failures(_on(ctx, small), ((3, 0.4), (11, 0.9)))
        lp, al = _batch(bad, return_alpha=True, on_error="nan")
        assert sorted(np.flatnonzero(np.isnan(lp)).tolist()) == [3, 11]

    ctx, fresh = _new_ctx(False, DET, pool_mb=4096), _new_ctx(False, DET, pool_mb=4096)
    try:
        assert ctx.get_param("alloc_poison") == 0
        failures(ctx)
        blocks, cached = ctx.get_param("pool_blocks"), ctx.get_param("pool_cached_mb")
        assert blocks >= 3   # the failed calls' factor, inputs and right-hand side are in the cache now
        f = agp.GP(0.2, 1.4 * agp.Matern52Kernel() @ agp.ScaleTransform(0.8), ctx=ctx)
        post = agp.posterior(f(agp.RowVecs(X[:n]), s2[:n]), y[:n])   # a good fit of the same size: holds blocks taken from the cache
        assert ctx.get_param("pool_blocks") < blocks, "the good fit did not reuse a cached block"
        if n >= 1025:
            assert ctx.get_param("pool_cached_mb") < cached
        post.data.C.free()
        out = good(ctx)
        ref = good(fresh)
        _assert_finite(out)
        _assert_same_bits(out, ref)
        failures(ctx)          # and once more, between good calls
        _assert_same_bits(good(ctx), ref)
        if f64:
            assert bc.lp_err(out["lp"], lp_o) <= 1e-10 and bc.lp_err(out["post_lp"], lp_o) <= 1e-10 and bc.lp_err(out["upd_lp"], lp2_o) <= 1e-10
            assert _rel(out["alpha"], opost.alpha) <= 1e-8 and _rel(out["upd_alpha"], opost2.alpha) <= 1e-8
            for key, op in (("predict", opost), ("upd_predict", opost2)):
                mo, co = op.mean_and_cov(xs64)
                np.testing.assert_allclose(out[key][0], mo, rtol=0, atol=1e-8)
                np.testing.assert_allclose(out[key][1], np.diag(co), rtol=0, atol=1e-9)
                np.testing.assert_allclose(out[key][2], co, rtol=0, atol=1e-9)
            assert np.max(np.abs(out["U"] - opost.U)) <= 1e-10 and np.max(np.abs(out["upd_U"] - opost2.U)) <= 1e-10
        else:
            assert bc.lp_err(out["lp"], lp_o) <= 1e-4 and bc.lp_err(out["post_lp"], lp_o) <= 1e-4 and bc.lp_err(out["upd_lp"], lp2_o) <= 1e-4
        assert not np.any(np.tril(out["U"], -1)) and not np.any(np.tril(out["upd_U"], -1))
    finally:
        ctx.close()
        fresh.close()
