"""fp64 host reference of leave-one-out cross-validation for exact GPs (Rasmussen & Williams §5.4.2), shared by tests/test_loo_cpu.py and
tests/test_gpu_loo.py: the closed form from C = K + Σy, the weight matrix G of its gradient (dL = ⟨G, dC⟩), the chain from G to the parameters the
C ABI differentiates against, a brute-force refit per left-out point, and a NumPy emulation of the way the device forms G.

  α = C⁻¹(y − m), c_i = [C⁻¹]_ii:   μ_i = y_i − α_i/c_i,  v_i = 1/c_i,  ℓ_i = −½ log 2π + ½ log c_i − ½ α_i²/c_i,  L = Σ ℓ_i
  a_i = ½(1/c_i + α_i²/c_i²), b_i = α_i/c_i, β = C⁻¹b:   G = −C⁻¹ diag(a) C⁻¹ + ½(β αᵀ + α βᵀ),  ∂L/∂y = −β

K comes from oracle.gp_oracle.kernelmatrix (single-kind kernels) or tests.composite_ref.ref_kernelmatrix (composite ones)."""
import math

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as o
from tests import composite_dx_ref as cdx
from tests import composite_ref as cr

LOG2PI = math.log(2.0 * math.pi)


def closed_form(C, delta, y):
    """{"alpha", "c", "mean", "var", "lp", "L"} of the closed form; C: (n, n) SPD, delta = y − m."""
    cf = sla.cho_factor(C, lower=True)
    Ci = sla.cho_solve(cf, np.eye(C.shape[0]))
    alpha = sla.cho_solve(cf, delta)
    c = np.diag(Ci).copy()
    lp = -0.5 * LOG2PI + 0.5 * np.log(c) - 0.5 * alpha**2 / c
    return {"alpha": alpha, "c": c, "Ci": Ci, "mean": y - alpha / c, "var": 1.0 / c, "lp": lp, "L": float(np.sum(lp))}


def weight_matrix(C, delta):
    """(G, β): dL = ⟨G, dC⟩ for symmetric dC, ∂L/∂y = −β"""
    r = closed_form(C, delta, delta)
    Ci, alpha, c = r["Ci"], r["alpha"], r["c"]
    a = 0.5 * (1.0 / c + alpha**2 / c**2)
    beta = Ci @ (alpha / c)
    G = -(Ci * a[None, :]) @ Ci + 0.5 * (np.outer(beta, alpha) + np.outer(alpha, beta))
    return 0.5 * (G + G.T), beta


def brute_force(C, m, y):
    """(μ, v, ℓ) by n refits: observation i predicted from the posterior given all the others, its own noise included (C carries Σy)."""
    n = C.shape[0]
    mu, v = np.empty(n), np.empty(n)
    for i in range(n):
        rest = np.r_[0:i, i + 1:n]
        if n == 1:
            mu[i], v[i] = m[i], C[i, i]
            continue
        cf = sla.cho_factor(C[np.ix_(rest, rest)], lower=True)
        ki = C[rest, i]
        mu[i] = m[i] + ki @ sla.cho_solve(cf, y[rest] - m[rest])
        v[i] = C[i, i] - ki @ sla.cho_solve(cf, ki)
    lp = -0.5 * LOG2PI - 0.5 * np.log(v) - 0.5 * (y - mu) ** 2 / v
    return mu, v, lp


def device_emulation(C, delta, tile=128):
    """G the way the device forms it: −C⁻¹ kept as its LOWER triangle padded to a multiple of the tile (identity on the padded diagonal, as the fit pads
    C), Z = mirror(−C⁻¹)·diag(d) with d_j = √(2a_j) and d_j = 0 for the padded j, P = −Z Zᵀ, P += β αᵀ + α βᵀ; G = ½ P on the first n rows and columns."""
    n = C.shape[0]
    npad = -(-n // tile) * tile
    Cp = np.eye(npad)
    Cp[:n, :n] = C
    cf = sla.cho_factor(Cp, lower=True)
    low = np.tril(-sla.cho_solve(cf, np.eye(npad)))             # what the SYRK leaves: the lower triangle of −C⁻¹
    alpha = np.zeros(npad)
    alpha[:n] = sla.cho_solve(cf, np.r_[delta, np.zeros(npad - n)])[:n]
    c = -np.diag(low)
    d, b = np.zeros(npad), np.zeros(npad)
    d[:n] = np.sqrt(1.0 / c[:n] + alpha[:n] ** 2 / c[:n] ** 2)
    b[:n] = alpha[:n] / c[:n]
    beta = sla.cho_solve(cf, b)
    full = low + np.tril(low, -1).T                            # the mirror pass
    Z = full * d[None, :]
    P = -(Z @ Z.T) + np.outer(beta, alpha) + np.outer(alpha, beta)
    assert np.all(P[n:, :] == 0.0) and np.all(P[:, n:] == 0.0)  # nothing leaks into or out of the padding
    return 0.5 * P[:n, :n]


def single_kind_grads(ok, X, G, noise_ndim):
    """The gradient of L against what gp_loo_grad differentiates, from the weights G (the closed forms of oracle.gp_oracle.logpdf_grad with Wt = G).
    ok: oracle Kernel; X: (n, D)."""
    n, d = X.shape
    s = ok.scale_vec(d)
    Xsc = X * s
    diff2 = (Xsc[:, None, :] - Xsc[None, :, :]) ** 2
    r2 = diff2.sum(-1)
    dk = o._dkappa_dr2(ok.kind, r2)
    g = {"variance": float(np.sum(G * o._kappa(ok.kind, r2)))}
    g["scale"] = (None if ok.scale is None else
                  (float(np.sum(G * ok.variance * dk * 2.0 * r2 / float(ok.scale))) if np.ndim(ok.scale) == 0 else
                   np.array([np.sum(G * ok.variance * dk * 2.0 * diff2[:, :, p] / s[p]) for p in range(d)])))
    Gk = G * (ok.variance * dk)
    np.fill_diagonal(Gk, 0.0)
    g["x"] = 4.0 * s[None, :] * (Gk.sum(axis=1)[:, None] * Xsc - Gk @ Xsc)
    g["noise"] = noise_grad(G, noise_ndim)
    return g


def composite_grads(k, X, G, noise_ndim):
    """The same for a composite kernel: "theta" against the flat θ of the C ABI, "x" through ∂k/∂t (both orders of the symmetric pair: 2G)."""
    _, dK = cr.ref_kernelmatrix(k, X, grad=True)
    return {"theta": np.array([np.sum(G * d) for d in dK]), "x": np.einsum("ij,ijp->ip", 2.0 * G, cdx.ref_dk_dt(k, X)), "noise": noise_grad(G, noise_ndim)}


def noise_grad(G, noise_ndim):
    """scalar σ²: tr G; diagonal Σy: G_ii; dense Σy: the full symmetric G"""
    return float(np.trace(G)) if noise_ndim == 0 else (np.diag(G).copy() if noise_ndim == 1 else G)
