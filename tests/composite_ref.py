"""fp64 NumPy reference of the composite kernels of include/gpmi355.h gp_ksum (kinds 0..6, the normal form Σ_t σ_t² Π_f κ_f) and of their derivatives
against θ — what tests/test_composite_cpu.py pins to scikit-learn and tests/test_gpu_composite.py measures the device against.  Like the device, it takes
differences of the raw inputs and then applies each factor's transform."""
import math

import numpy as np

import abstractgps_jl_amd as agp

SQ3, SQ5 = math.sqrt(3.0), math.sqrt(5.0)


# ---- fp64 NumPy reference of the closed forms (include/gpmi355.h gp_ksum) ------------------------------------------------------------------
def rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x[:, None] if x.ndim == 1 else x


def factor(kind, sc, par, T):
    """κ and [∂κ/∂θ_q] (scale entries, then param entries) of one factor at the raw differences T (n, m, D)."""
    D = T.shape[-1]
    ns = len(sc)
    s = np.ones(D) if ns == 0 else (np.full(D, sc[0]) if ns == 1 else np.asarray(sc))
    U = T * s
    if kind == 6:
        return np.all(T == 0, axis=-1).astype(np.float64), []
    if kind == 4:
        r = np.asarray(par)
        S = np.sin(np.pi * U)
        kap = np.exp(-0.5 * np.sum((S / r) ** 2, axis=-1))
        du = -kap[..., None] * (np.pi / 2) * np.sin(2 * np.pi * U) / r**2  # ∂κ/∂u_p
        ds = [np.sum(du * T, axis=-1)] if ns == 1 else [du[..., p] * T[..., p] for p in range(ns)]
        dr = [kap * S[..., p] ** 2 / r[p] ** 3 for p in range(D)]
        return kap, ds + dr
    d2 = np.sum(U * U, axis=-1)
    extra = []
    if kind == 5:
        a = par[0]
        q = d2 / (2 * a)
        kap = np.exp(-a * np.log1p(q))
        dk = -kap / (2 * (1 + q))
        extra = [kap * (q / (1 + q) - np.log1p(q))]
    else:
        d = np.sqrt(d2)
        if kind == 0:
            kap = np.exp(-0.5 * d2)
            dk = -0.5 * kap
        elif kind == 1:
            kap = np.exp(-d)
            with np.errstate(divide="ignore", invalid="ignore"):
                dk = np.where(d > 0, -kap / (2 * np.where(d > 0, d, 1)), 0.0)
        elif kind == 2:
            kap = (1 + SQ3 * d) * np.exp(-SQ3 * d)
            dk = -1.5 * np.exp(-SQ3 * d)
        else:
            kap = (1 + SQ5 * d + 5.0 / 3.0 * d2) * np.exp(-SQ5 * d)
            dk = -5.0 / 6.0 * (1 + SQ5 * d) * np.exp(-SQ5 * d)
    if ns == 1:
        ds = [dk * 2 * sc[0] * np.sum(T * T, axis=-1)]
    else:
        ds = [dk * 2 * sc[p] * T[..., p] ** 2 for p in range(ns)]
    return kap, ds + extra


def ref_kernelmatrix(k, x, z=None, grad=False):
    """K(x, z) of the composite kernel k from raw differences (what the device does), and with grad=True also [∂K/∂θ_j] in the θ order of the
    C ABI.  x, z: vectors or (N, D) arrays."""
    X = rows(x)
    Z = X if z is None else rows(z)
    T = X[:, None, :] - Z[None, :, :]
    nf = agp.api._NormalForm(k)
    p = nf.params
    K = np.zeros(T.shape[:2])
    dK = []
    for vi, fs in nf.terms:
        var = math.prod(p[i] for i in vi)
        kd = [factor(kind, [p[i] for i in si], [p[i] for i in pi], T) for kind, si, pi in fs]
        prod = np.ones_like(K)
        for kap, _ in kd:
            prod = prod * kap
        K += var * prod
        if grad:
            dK.append(prod)
            for j, (kap, ders) in enumerate(kd):
                other = np.ones_like(K)
                for i, (ki, _) in enumerate(kd):
                    if i != j:
                        other = other * ki
                dK += [var * other * dm for dm in ders]
    return (K, dK) if grad else K


def mauna_loa_kernel():
    """examples/1-mauna-loa/script.jl:102-116 with plausible values: SE(θ₁) + Per(θ₂)·SE(θ₃) + RQ(θ₄) + (SE(θ₅) + σₙ²·White)."""
    k_smooth = 50.0**2 * agp.with_lengthscale(agp.SqExponentialKernel(), 50.0)
    k_period = 2.0**2 * agp.with_lengthscale(agp.PeriodicKernel(r=[1.0]), 1.0) * agp.with_lengthscale(agp.SqExponentialKernel(), 100.0)
    k_medium = 0.5**2 * agp.with_lengthscale(agp.RationalQuadraticKernel(alpha=1.5), 1.2)
    k_noise = 0.2**2 * agp.with_lengthscale(agp.SqExponentialKernel(), 0.1) + 0.05**2 * agp.WhiteKernel()
    return k_smooth + k_period + k_medium + k_noise


def ref_from_theta(nf, th, X):
    """K from a θ vector in the C-ABI order and the structure of nf (what the device reads)."""
    X = rows(X)
    T = X[:, None, :] - X[None, :, :]
    K, j = 0.0, 0
    for _, fs in nf.terms:
        var = th[j]
        j += 1
        prod = 1.0
        for kind, si, pi in fs:
            sc = list(th[j:j + len(si)])
            j += len(si)
            par = list(th[j:j + len(pi)])
            j += len(pi)
            prod = prod * factor(kind, sc, par, T)[0]
        K = K + var * prod
    return K


def ml_kernel():
    """The Mauna Loa form with amplitudes of order 1: the example's own amplitudes (50² for the trend) over dense inputs give K + Σy a condition
    number near 1e9, where the 1e-13·Σσ² the assembly may differ by (raw differences, then scaled) moves logpdf by more than 1e-10."""
    SE = agp.SqExponentialKernel
    return (agp.with_lengthscale(SE(), 50.0) + 0.5 * (agp.with_lengthscale(agp.PeriodicKernel(r=[1.0]), 1.0) * agp.with_lengthscale(SE(), 100.0))
            + 0.1 * agp.with_lengthscale(agp.RationalQuadraticKernel(alpha=1.5), 1.2)
            + (0.05 * agp.with_lengthscale(SE(), 0.1) + 0.01 * agp.WhiteKernel()))


def dense_data(n, seed=0):
    """n points over 65 years (years since 1958), standardised trend + seasonal + noise."""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 65.0, n)
    y = 0.02 * x**2 + 1.3 * x + 3.0 * np.sin(2 * np.pi * x) + 0.3 * rng.standard_normal(n)
    return x, (y - y.mean()) / y.std()
