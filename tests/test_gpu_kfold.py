"""GPU: K-fold cross-validation from one factorisation — gp_kfold / gp_kfold_sum (kfold_gram_kernel, kfold_fact_kernel behind one fit and W = L⁻ᵀ)
against a plain fp64 refit per fold on the cases of tests/loo_cases.py (cond(C) ≤ 1e3, asserted in tests/test_loo_cpu.py).

Fold schemes: i mod 5 (interleaved: every fold gathers rows with gaps), contiguous blocks of 65 (one row past a 64-row tile) and a ragged scheme of
sizes 1, 64, 129, rest — cut short where n is smaller — spread by a seeded permutation (a singleton, a full tile, three tile rows with an edge).
Tolerances: the leave-one-out ones (loo_cases.L_TOL / M_TOL / V_TOL: value and per-fold lp 1e-10 relative, mean 1e-8 and var 1e-9 absolute); fp32 inputs:
the suite's fp32 logpdf tolerance, 1e-4 relative."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import loo_cases as lc

pytestmark = pytest.mark.gpu

CASES = ["n2", "n129_dense", "n257", "n300_d17", "n300_dense", "mauna_loa", "f32_n300"]
SCHEMES = ["mod5", "blocks65", "ragged"]


def _case(cid):
    if cid == "mauna_loa":
        return lc.composite_case(cid)
    return lc.single_case(cid, np.float32) if cid == "f32_n300" else lc.single_case(cid)


def _folds(n, scheme):
    if scheme == "mod5":
        return np.arange(n) % min(5, n)
    if scheme == "blocks65":
        return np.arange(n) // 65
    lab = np.repeat(np.arange(4), [1, 64, 129, max(n - 194, 0)])[:n] if n > 2 else np.arange(n)
    return lab[np.random.default_rng(40).permutation(n)]


@lru_cache(maxsize=None)
def _refit(cid, scheme):
    """(lp per fold, mean, var) by conditioning on the other folds, fold by fold, in fp64"""
    c = _case(cid)
    Cm, m = lc.covariance(c)
    y = np.asarray(c["y"], dtype=np.float64)
    folds = _folds(c["n"], scheme)
    lp, mu, var = np.zeros(folds.max() + 1), np.zeros(c["n"]), np.zeros(c["n"])
    for f in range(len(lp)):
        F, R = np.flatnonzero(folds == f), np.flatnonzero(folds != f)
        A = np.linalg.solve(Cm[np.ix_(R, R)], Cm[np.ix_(R, F)]) if len(R) else np.zeros((0, len(F)))
        mf = m[F] + A.T @ (y[R] - m[R])
        S = Cm[np.ix_(F, F)] - Cm[np.ix_(F, R)] @ A
        r = y[F] - mf
        lp[f] = -0.5 * (r @ np.linalg.solve(S, r) + np.linalg.slogdet(S)[1] + len(F) * np.log(2.0 * np.pi))
        mu[F], var[F] = mf, np.diag(S)
    return lp, mu, var


def _ratios(got, ref, f32=False):
    """error / bound of (value, lp, mean, var); fp32 inputs: everything at 1e-4 relative"""
    (val, lp, mu, var), (rlp, rmu, rvar) = got, ref
    if f32:
        out = {"value": abs(val - rlp.sum()) / (1e-4 * abs(rlp.sum())), "lp": np.max(np.abs(lp - rlp) / (1e-4 * np.maximum(np.abs(rlp), 1.0))),
               "mean": np.max(np.abs(mu - rmu) / (1e-4 * np.maximum(np.abs(rmu), 1.0))), "var": np.max(np.abs(var - rvar) / (1e-4 * rvar))}
    else:
        out = {"value": abs(val - rlp.sum()) / (lc.L_TOL * abs(rlp.sum())), "lp": np.max(np.abs(lp - rlp) / (lc.L_TOL * np.maximum(np.abs(rlp), 1.0))),
               "mean": np.max(np.abs(mu - rmu)) / lc.M_TOL, "var": np.max(np.abs(var - rvar)) / lc.V_TOL}
    print("KFOLD_RATIO", {k: f"{float(v):.3e}" for k, v in out.items()})
    return out


def _call(fx, y, folds):
    mu, var = agp.kfold_mean_and_var(fx, y, folds)
    return float(agp.kfold_logpdf(fx, y, folds)), agp.kfold_logpdf(fx, y, folds, pointwise=True), mu, var


def _assert_inside(out):
    bad = {k: float(v) for k, v in out.items() if not v <= 1.0}
    assert not bad, f"outside the tolerance (error / bound): {bad}"


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("cid", CASES)
def test_against_a_refit_per_fold(agp, cid, scheme):
    c = _case(cid)
    got = _call(c["fx"], c["y"], _folds(c["n"], scheme))
    assert got[1].dtype == got[2].dtype == got[3].dtype == (np.float32 if cid == "f32_n300" else np.float64)
    _assert_inside(_ratios(got, _refit(cid, scheme), f32=cid == "f32_n300"))


def test_singleton_folds_are_leave_one_out(agp):
    c = _case("n257")
    val, lp, mu, var = _call(c["fx"], c["y"], np.arange(c["n"]))
    lmu, lvar = agp.loo_mean_and_var(c["fx"], c["y"])
    _assert_inside(_ratios((val, lp, mu, var), (agp.loo_logpdf(c["fx"], c["y"], pointwise=True), lmu, lvar)))


def test_one_fold_of_everything_is_the_prior(agp):
    c = _case("n300_dense")
    Cm, m = lc.covariance(c)
    val, lp, mu, var = _call(c["fx"], c["y"], np.zeros(c["n"], dtype=np.int64))
    assert lp.shape == (1,) and lp[0] == val
    _assert_inside(_ratios((val, lp, mu, var), (np.array([float(agp.logpdf(c["fx"], c["y"]))]), m, np.diag(Cm))))


def test_repeatable_and_independent_of_the_labels(agp):
    """two calls return the same bytes; under a permutation of the labels every fold's lp and every point's mean and var keep their bytes"""
    c = _case("n300_d17")
    folds = _folds(c["n"], "ragged")
    perm = np.array([2, 0, 3, 1])
    a, b, p = (_call(c["fx"], c["y"], f) for f in (folds, folds, perm[folds]))
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert np.array_equal(p[1][perm], a[1]) and np.array_equal(p[2], a[2]) and np.array_equal(p[3], a[3])


def test_poisoned_blocks(agp):
    """every block handed out full of NaN: the padded entries the kernels read are written by them first"""
    c = _case("n257")
    ctx = agp.Context(0)
    try:
        ctx.set_param("alloc_poison", 1)
        f = c["fx"].f
        fx = (agp.GP(f.kernel, ctx=ctx) if f.mean_fn is None else agp.GP(f.mean_fn, f.kernel, ctx=ctx))(c["fx"].x, c["fx"].sigma2)
        got = _call(fx, c["y"], _folds(c["n"], "ragged"))
        ctx.set_param("alloc_poison", 0)
    finally:
        ctx.close()
    assert all(np.all(np.isfinite(g)) for g in got)
    _assert_inside(_ratios(got, _refit("n257", "ragged")))


@pytest.mark.parametrize("what,n,nfolds,status,reason", [
    ("label_nfolds", 8, 2, -7, "fold id out of range"),
    ("empty_fold", 8, 3, -7, "empty fold"),
    ("nfolds_0", 8, 0, -8, "nfolds must be >= 1"),
    ("fold_1025", 1025, 1, -7, "fold above GPMI355_KFOLD_MAX_FOLD"),
])
def test_argument_errors_through_the_raw_abi(agp, what, n, nfolds, status, reason):
    L, lib = agp._lib, agp._lib.load()
    x, y, out = np.linspace(0.0, 1.0, n), np.zeros(n), np.zeros(3 * n + 1)
    fold = (np.arange(n) % max(nfolds, 1)).astype(np.int32)
    if what == "label_nfolds":
        fold[3] = nfolds
    if what == "empty_fold":
        fold[fold == 1] = 0
    kk, px, nz = L.gp_kernel(0, 0, 1.5, 0, None), L.gp_points(x.ctypes.data, n, 1, 0), L.gp_noise(0, 0.1, None)
    rc = lib.gp_kfold(agp.default_context(0).handle, C.byref(kk), C.byref(px), C.byref(nz), None, y.ctypes.data, fold.ctypes.data_as(C.POINTER(C.c_int32)),
                      nfolds, out.ctypes.data, out.ctypes.data + 8, out.ctypes.data + 8 * (n + 1), out.ctypes.data + 8 * (2 * n + 1))
    assert rc == status and reason in lib.gp_last_error().decode() and not out.any()
