"""fp64 NumPy reference of the input gradient of a composite kernel (include/gpmi355.h gp_logpdf_grad_sum_x): ∂k/∂t at the raw differences
t = x_i − x_j, built on agp.api._NormalForm like tests/composite_ref.py, and ∂logpdf/∂x from a SciPy Cholesky — what tests/test_composite_dx_cpu.py
pins to central differences and to the oracle, and what tests/test_gpu_composite_dx.py measures the device against.

    ∂logpdf/∂x_ip = Σ_j W_ij · ∂k/∂t_p (x_i − x_j),   W = α αᵀ − C⁻¹
    ∂k/∂t_p       = Σ_terms σ_t² Σ_f (Π_{g≠f} κ_g) · ∂κ_f/∂t_p

With c_p the factor's transform (1, s, v_p):  kinds 0..3 and RQ: ∂κ_f/∂t_p = ∂κ/∂d² · 2 c_p² t_p;  Periodic: −κ (π/2) sin(2π u_p)/r_p² · c_p with
u_p = c_p t_p;  White: 0.  The Matern12 derivative at d = 0 is taken as 0, like `dk` of tests/composite_ref.factor."""
import math

import numpy as np
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from tests.composite_ref import SQ3, SQ5, factor, ref_kernelmatrix, rows


def factor_dt(kind, sc, par, T):
    """∂κ_f/∂t (n, m, D) of one factor at the raw differences T (n, m, D)."""
    D = T.shape[-1]
    ns = len(sc)
    c = np.ones(D) if ns == 0 else (np.full(D, sc[0]) if ns == 1 else np.asarray(sc, dtype=np.float64))
    if kind == 6:
        return np.zeros_like(T)
    U = T * c
    if kind == 4:
        r = np.asarray(par, dtype=np.float64)
        kap = np.exp(-0.5 * np.sum((np.sin(np.pi * U) / r) ** 2, axis=-1))
        return -kap[..., None] * (np.pi / 2) * np.sin(2 * np.pi * U) / r**2 * c
    d2 = np.sum(U * U, axis=-1)
    if kind == 5:
        q = d2 / (2 * par[0])
        dk = -np.exp(-par[0] * np.log1p(q)) / (2 * (1 + q))
    else:
        d = np.sqrt(d2)
        if kind == 0:
            dk = -0.5 * np.exp(-0.5 * d2)
        elif kind == 1:
            dk = np.where(d > 0, -np.exp(-d) / (2 * np.where(d > 0, d, 1)), 0.0)
        elif kind == 2:
            dk = -1.5 * np.exp(-SQ3 * d)
        else:
            dk = -5.0 / 6.0 * (1 + SQ5 * d) * np.exp(-SQ5 * d)
    return dk[..., None] * 2 * c * c * T


def ref_dk_dt(k, X):
    """∂k/∂t_p at t = x_i − x_j for every pair: (n, n, D)."""
    X = rows(X)
    T = X[:, None, :] - X[None, :, :]
    nf = agp.api._NormalForm(k)
    p = nf.params
    out = np.zeros_like(T)
    for vi, fs in nf.terms:
        var = math.prod(p[i] for i in vi)
        kap = [factor(kind, [p[i] for i in si], [p[i] for i in pi], T)[0] for kind, si, pi in fs]
        for j, (kind, si, pi) in enumerate(fs):
            other = np.ones(T.shape[:2])
            for i, ki in enumerate(kap):
                if i != j:
                    other = other * ki
            out += var * other[..., None] * factor_dt(kind, [p[i] for i in si], [p[i] for i in pi], T)
    return out


def noise_matrix(noise, n):
    noise = np.asarray(noise, dtype=np.float64)
    return noise if noise.ndim == 2 else np.diag(np.broadcast_to(noise, (n,)))


def host_fit(k, X, y, noise, mean=0.0):
    """(logpdf, α, lower Cholesky factor) of y ~ N(mean, K + Σy) on the host; noise: scalar, vector or dense matrix."""
    X = rows(X)
    n = X.shape[0]
    L = sla.cholesky(ref_kernelmatrix(k, X) + noise_matrix(noise, n), lower=True)
    delta = np.asarray(y, dtype=np.float64) - mean
    alpha = sla.cho_solve((L, True), delta)
    lp = -0.5 * (n * math.log(2 * math.pi) + 2 * np.sum(np.log(np.diag(L))) + delta @ alpha)
    return lp, alpha, L


def ref_logpdf_grad_x(k, X, y, noise, mean=0.0):
    """∂logpdf/∂x (n, D) with the prior mean constant in x."""
    X = rows(X)
    _, alpha, L = host_fit(k, X, y, noise, mean)
    W = np.outer(alpha, alpha) - sla.cho_solve((L, True), np.eye(X.shape[0]))
    return np.einsum("ij,ijp->ip", W, ref_dk_dt(k, X))


def six_term_kernel():
    """D = 3: every kind, every transform, a two-factor product."""
    SE, M12, M32, M52 = agp.SqExponentialKernel, agp.Matern12Kernel, agp.Matern32Kernel, agp.Matern52Kernel
    return (1.3 * SE() @ agp.ARDTransform([0.5, 1.1, 0.9])
            + 0.5 * ((agp.PeriodicKernel(r=[1.0, 0.8, 1.2]) @ agp.ScaleTransform(0.7)) * (M52() @ agp.ScaleTransform(0.6)))
            + 0.2 * agp.RationalQuadraticKernel(alpha=1.5) @ agp.ARDTransform([0.9, 0.4, 1.3])
            + 0.1 * M32()
            + 0.05 * M12() @ agp.ScaleTransform(0.8)
            + 0.01 * agp.WhiteKernel())


def many_dim_kernel(d):
    """D = 8 / 16: SE∘ARD + 0.3·(Periodic(r per dim)∘ARD · Matern32∘Scale) + 0.1·RQ∘Scale."""
    return (agp.SqExponentialKernel() @ agp.ARDTransform(np.linspace(0.3, 0.6, d))
            + 0.3 * ((agp.PeriodicKernel(r=np.linspace(0.8, 1.4, d)) @ agp.ARDTransform(np.linspace(0.2, 0.5, d))) * (agp.Matern32Kernel() @ agp.ScaleTransform(0.4)))
            + 0.1 * agp.RationalQuadraticKernel(alpha=1.1) @ agp.ScaleTransform(0.5))


def six_term_data(n, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 3, size=(n, 3))
    return X, np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
