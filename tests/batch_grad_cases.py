"""Shared by tests/test_batch_grad_cpu.py and tests/test_gpu_batch_grad.py: the references a batched gradient is compared with and the project's fp64
gradient tolerances (tests/test_gpu_composite.py, tests/test_gpu_api.py) in one place.
  kernel and noise entries: |err| <= 1e-7·|ref| + 1e-9·g∞, g∞ the largest magnitude among that problem's kernel and noise gradient entries;
  ∂/∂y: 1e-8 in the 2-norm (relative to the reference's norm);  logpdf: 1e-10 relative to max(|ref|, 1)."""
import functools
import math

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as o
from tests import batch_cases as bc

G_RTOL, G_ATOL, DY_TOL, LP_TOL = 1e-7, 1e-9, 1e-8, 1e-10


def entries(g, keys=("variance", "scale", "noise")):
    """the kernel and noise entries of a gradient dict as one vector (a missing / None entry contributes nothing)"""
    parts = [np.atleast_1d(np.asarray(g[k], dtype=np.float64)).ravel() for k in keys if g.get(k) is not None]
    return np.concatenate(parts)


def grad_excess(got, ref, keys=("variance", "scale", "noise")):
    """(worst |err| / (1e-7·|ref| + 1e-9·g∞) over the kernel and noise entries, relative 2-norm error of ∂/∂y): within tolerance when <= 1 and <= DY_TOL.
    `mean` = −`y` is checked exactly."""
    a, r = entries(got, keys), entries(ref, keys)
    assert a.shape == r.shape, (a.shape, r.shape)
    ginf = float(np.max(np.abs(r)))
    ex = float(np.max(np.abs(a - r) / (G_RTOL * np.abs(r) + G_ATOL * ginf)))
    assert np.array_equal(np.asarray(got["mean"]), -np.asarray(got["y"]))
    return ex, bc.vec_err(got["y"], np.asarray(ref["y"], dtype=np.float64))


def within(got, ref, keys=("variance", "scale", "noise")):
    ex, ey = grad_excess(got, ref, keys)
    return ex <= 1.0 and ey <= DY_TOL


def same_bits(g, h):
    """every output of two gradient dicts bit for bit"""
    if set(g) != set(h):
        return False
    for k in g:
        a, b = g[k], h[k]
        if (a is None) != (b is None):
            return False
        if a is not None and np.asarray(a).tobytes() != np.asarray(b).tobytes():
            return False
    return True


def all_nan(g):
    return all(np.isnan(np.asarray(v, dtype=np.float64)).all() for v in g.values() if v is not None)


def oracle_grad(case):
    """(logpdf, gradient dict) of the oracle: oracle.logpdf for the value, oracle.logpdf_grad (explicit inverse, dense ∂C matrices) for the gradient"""
    return float(o.logpdf(case["ofx"], case["y"])), o.logpdf_grad(case["ofx"], case["y"])


def _dkappa(kind, r2):
    r = np.sqrt(r2)
    if kind == 0:
        return -0.5 * np.exp(-0.5 * r2)
    if kind == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, -np.exp(-r) / (2 * r), 0.0)
    if kind == 2:
        return -1.5 * np.exp(-math.sqrt(3.0) * r)
    a = math.sqrt(5.0) * r
    return -(5.0 / 6.0) * (1 + a) * np.exp(-a)


def scipy_grad(case):
    """The same gradient from SciPy's Cholesky: L⁻¹ by a triangular solve on the identity, C⁻¹ = L⁻ᵀ L⁻¹ (what the device forms), no explicit inverse of C."""
    ofx, y = case["ofx"], np.asarray(case["y"], dtype=np.float64)
    k = ofx.f.kernel
    X = o.as_points(ofx.x).astype(np.float64)
    n, d = X.shape
    m, Cm = o.mean_and_cov(ofx)
    L = sla.cholesky(Cm, lower=True)
    Li = sla.solve_triangular(L, np.eye(n), lower=True)
    Ci = Li.T @ Li
    alpha = sla.cho_solve((L, True), y - m)
    W = 0.5 * (np.outer(alpha, alpha) - Ci)
    s = k.scale_vec(d)
    U = X * s
    out = {"y": -alpha, "mean": alpha, "scale": None}
    r2 = np.zeros((n, n))
    for p in range(d):
        r2 += (U[:, None, p] - U[None, :, p]) ** 2
    out["variance"] = float(np.sum(W * o._kappa(k.kind, r2)))
    Wk = W * (k.variance * 2.0 * _dkappa(k.kind, r2))
    if k.scale is not None and np.ndim(k.scale) == 0:
        out["scale"] = float(np.sum(Wk * r2) / float(k.scale))
    elif k.scale is not None:
        out["scale"] = np.array([np.sum(Wk * (U[:, None, p] - U[None, :, p]) ** 2) / s[p] for p in range(d)])
    dn = np.diag(W).copy()
    out["noise"] = float(dn.sum()) if np.ndim(ofx.sigma2) == 0 else dn
    return out


@functools.lru_cache(maxsize=None)
def ragged_with_oracle():
    """bc.ragged_cases() and the oracle's (logpdf, gradient) of every case, computed once per process and never changed"""
    cases = bc.ragged_cases()
    return cases, [oracle_grad(c) for c in cases]


def host_grad_composite(k, x, s2, y):
    """(logpdf, {"theta", "noise", "y"}) of a composite kernel from tests/composite_ref.ref_kernelmatrix(..., grad=True) and SciPy's Cholesky"""
    from tests.composite_ref import ref_kernelmatrix

    K, dK = ref_kernelmatrix(k, x, grad=True)
    n = len(y)
    Cm = K + s2 * np.eye(n)
    lp, a = bc.host_fit(Cm, y)
    L = sla.cholesky(Cm, lower=True)
    Li = sla.solve_triangular(L, np.eye(n), lower=True)
    W = 0.5 * (np.outer(a, a) - Li.T @ Li)
    return float(lp), {"theta": np.array([np.sum(W * D) for D in dK]), "noise": float(np.trace(W)), "y": -a, "mean": a}
