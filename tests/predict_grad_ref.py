"""fp64 NumPy references of the gradients of the predictive mean and variance w.r.t. the test inputs (include/gpmi355.h gp_posterior_predict_grad /
gp_vfe_predict_grad) — what tests/test_predict_grad_cpu.py pins to central differences and what tests/test_gpu_predict_grad.py measures the device against.

For every test point j independently, the prior mean constant in x and k(x*, x*) constant:

    exact posterior (α, C = L Lᵀ, k_j = K(X, x*_j)):
        ∂mean_j/∂x*_jp =      Σ_i α_i  ∂k(x*_j, x_i)/∂x*_jp
        ∂var_j /∂x*_jp = −2 · Σ_i w_ji ∂k(x*_j, x_i)/∂x*_jp,     w_j = C⁻¹ k_j
    VFE / DTC posterior (U = chol(K_zz + jitter I).U, Λ_ε, α over the pseudo-points; A_j = U⁻ᵀ K(z, x*_j)):
        ∂mean_j/∂x*_jp =      Σ_m α_m  ∂k(x*_j, z_m)/∂x*_jp
        ∂var_j /∂x*_jp = −2 · Σ_m u_jm ∂k(x*_j, z_m)/∂x*_jp,     u_j = U⁻¹ (A_j − Λ_ε⁻¹ A_j)

∂k/∂x* = ∂k/∂t at t = x* − x: composite kernels from `factor` / `factor_dt` (raw differences, prefix × suffix over a term's factors); a single kind from
2 s_p σ² κ'(d²)(u*_p − u_p) on the scaled inputs u = s∘x.  Matern12 at d = 0 is taken as 0, White contributes 0."""
import math

import numpy as np
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests.composite_dx_ref import factor_dt, noise_matrix
from tests.composite_ref import factor, ref_kernelmatrix, rows


def composite_dk_dx(k, Xs, X):
    """∂k(x*_j, x_i)/∂x*_jp of the composite kernel k for every cross pair: (ns, n, D)."""
    T = rows(Xs)[:, None, :] - rows(X)[None, :, :]
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


def single_dk_dx(kern: o.Kernel, Xs, X):
    """The same for a single-kind oracle kernel, from the analytic form on the scaled inputs: (ns, n, D)."""
    Xs, X = rows(Xs), rows(X)
    s = kern.scale_vec(X.shape[1])
    U = Xs[:, None, :] * s - X[None, :, :] * s
    dk = o._dkappa_dr2(kern.kind, np.sum(U * U, axis=-1))
    return 2.0 * kern.variance * dk[..., None] * U * s


def _is_single(k):
    return isinstance(k, o.Kernel)


def kmat(k, X, Z=None):
    return o.kernelmatrix(k, rows(X), None if Z is None else rows(Z)) if _is_single(k) else ref_kernelmatrix(k, X, Z)


def prior_var(k, ns):
    return np.full(ns, k.variance if _is_single(k) else agp.api._prior_variance(k))


def dk_dx(k, Xs, X):
    return single_dk_dx(k, Xs, X) if _is_single(k) else composite_dk_dx(k, Xs, X)


class HostPosterior:
    """Exact posterior on the host: α and the lower factor of K + Σy (noise: scalar, vector or dense matrix); k: an oracle Kernel or a composite kernel."""

    def __init__(self, k, X, y, noise, mean=0.0):
        self.k, self.X, self.mean0 = k, rows(X), mean
        n = self.X.shape[0]
        self.L = sla.cholesky(kmat(k, self.X) + noise_matrix(noise, n), lower=True)
        self.alpha = sla.cho_solve((self.L, True), np.asarray(y, dtype=np.float64) - mean)

    def mean_and_var(self, Xs):
        Ks = kmat(self.k, Xs, self.X)
        V = sla.solve_triangular(self.L, Ks.T, lower=True)
        return self.mean0 + Ks @ self.alpha, prior_var(self.k, Ks.shape[0]) - np.sum(V * V, axis=0)

    def grads(self, Xs):
        """(∂mean/∂x*, ∂var/∂x*), both (ns, D)."""
        Ks = kmat(self.k, Xs, self.X)
        W = sla.cho_solve((self.L, True), Ks.T).T
        dk = dk_dx(self.k, Xs, self.X)
        return np.einsum("i,jip->jp", self.alpha, dk), -2.0 * np.einsum("ji,jip->jp", W, dk)

    def diag_ratio(self):
        d = np.abs(np.diag(self.L))
        return float(d.max() / d.min())


def sparse_grads(post: o.ApproxPosteriorGP, Xs):
    """(∂mean/∂x*, ∂var/∂x*) of an oracle VFE / DTC posterior (single-kind kernel), from its cached U, Λ_ε.U and α: both (ns, D)."""
    k = post.prior.kernel
    A = o.Ut_solve(post.U, o.gp_cov(post.prior, post.z, rows(Xs)))       # (M, ns)
    u = o.U_solve(post.U, A - o.chol_solve(post.Lam_U, A))               # (M, ns)
    dk = single_dk_dx(k, Xs, post.z)
    return np.einsum("m,jmp->jp", post.alpha, dk), -2.0 * np.einsum("mj,jmp->jp", u, dk)


def central_differences(mean_and_var, Xs, h=1e-5):
    """Central differences of a mean_and_var callable: every test point depends on its own coordinates only, so one pair of calls per dimension."""
    Xs = rows(Xs)
    gm, gv = np.zeros_like(Xs), np.zeros_like(Xs)
    for p in range(Xs.shape[1]):
        Xp, Xm = Xs.copy(), Xs.copy()
        Xp[:, p] += h
        Xm[:, p] -= h
        (mp, vp), (mm, vm) = mean_and_var(Xp), mean_and_var(Xm)
        gm[:, p], gv[:, p] = (mp - mm) / (2 * h), (vp - vm) / (2 * h)
    return gm, gv
