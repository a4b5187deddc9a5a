"""Seeded cases shared by tests/test_cols_cpu.py and tests/test_gpu_cols.py: S independent GPs that share x, kernel, Σy and the prior mean and differ in y
(the columns of Y), each built as a FiniteGP of the mirror, and the fp64 reference column by column — oracle/gp_oracle.py for the single-kind kernels with a
scalar / diagonal Σy, tests/composite_ref.py and tests/composite_dx_ref.py (NumPy + SciPy's Cholesky) for composite kernels and for a dense Σy, which the
oracle does not take.  Σy is at least 1e-2 of the prior variance, so every reference is far inside the tolerances it is used with.

The shapes are a pairwise selection over n ∈ {1, 63, 64, 65, 129, 300}, ns ∈ {1, 63, 65, 200}, S ∈ {1, 2, 15, 16, 17, 128}, D ∈ {1, 3, 16, 17}, the four
kinds × none / Scale / ARD, the three input containers, scalar / diagonal / dense Σy, zero / const / custom mean: the smallest that reach every edge of the
kernels — S around one 16-column MFMA block and at the cap, n around the 32-point strip, the 64-point test tile and the 128-row tile, n = 300 (10 strips)
where the training range of kmul is split, D = 17 where a single-kind kernel takes the per-column kvec launches."""
import math
from functools import lru_cache

import numpy as np
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_cases as bc
from tests import composite_dx_ref as cdx
from tests import composite_ref as cr

LP_TOL, A_TOL, M_TOL, V_TOL, G_RTOL, G_ATOL = 1e-10, 1e-8, 1e-8, 1e-9, 1e-7, 1e-9
# fp32 fits against the fp64 reference, as tests/test_gpu_parity.py (logpdf rel 1e-4), tests/test_gpu_api.py (mean / var / cov atol 1e-3, gradients 2e-2 of
# the largest entry) and tests/test_gpu_units_f32.py (fits: up to 5e-3) hold them
LP_TOL32, A_TOL32, M_TOL32, V_TOL32, G_TOL32 = 1e-4, 5e-3, 1e-3, 1e-3, 2e-2

# (id, n, ns, S, kind, transform, D, container, noise, mean)
SINGLE = [
    ("n1", 1, 1, 1, 0, "none", 1, "vector", "scalar", "zero"),
    ("n63", 63, 63, 2, 1, "scale", 3, "colvecs", "vector", "const"),
    ("n64", 64, 65, 15, 2, "ard", 16, "rowvecs", "scalar", "custom"),
    ("n65", 65, 200, 16, 3, "none", 3, "rowvecs", "vector", "zero"),
    ("n129", 129, 1, 17, 0, "ard", 3, "colvecs", "scalar", "const"),
    ("n300_cap", 300, 63, 128, 2, "scale", 1, "vector", "vector", "zero"),
    ("n300_d17", 300, 200, 2, 1, "none", 17, "rowvecs", "scalar", "custom"),
    ("n129_d17", 129, 65, 16, 3, "ard", 17, "colvecs", "vector", "zero"),
    ("n65_dense", 65, 63, 15, 0, "scale", 3, "rowvecs", "dense", "const"),
    ("n300_dense", 300, 65, 17, 3, "ard", 3, "colvecs", "dense", "zero"),
]
COMPOSITE = [("mauna_loa", 300, 200, 16), ("persewhite_d2", 129, 65, 17)]
F32 = [("f32_n300", 300, 65, 17, 3, "scale", 3, "rowvecs", "scalar", "const"), ("f32_cap", 65, 200, 128, 0, "ard", 3, "colvecs", "scalar", "zero")]


def per_se_rq_white():
    """Periodic · SE + RQ + White in D = 2."""
    return (0.8 * ((agp.PeriodicKernel(r=[1.0, 0.7]) @ agp.ScaleTransform(0.6)) * (agp.SqExponentialKernel() @ agp.ARDTransform([0.5, 0.9])))
            + 0.3 * agp.RationalQuadraticKernel(alpha=1.4) @ agp.ScaleTransform(0.8) + 0.02 * agp.WhiteKernel())


def _columns(rng, n, S, dtype):
    """S different columns: smooth parts of different phase plus noise (so that no two columns are multiples of each other)"""
    t = np.linspace(0.0, 3.0, n)[:, None]
    return (np.sin(t * (1.0 + 0.37 * np.arange(S)[None, :]) + np.arange(S)[None, :]) + 0.3 * rng.standard_normal((n, S))).astype(dtype)


def _dense_noise(rng, n, var, dtype):
    B = rng.standard_normal((n, 3))
    return (var * (2e-2 * np.eye(n) + 1e-2 * (B @ B.T) / 3.0)).astype(dtype)


def _test_points(rng, X, ns, dtype):
    """ns test points: some training points exactly (White, Matern12 at distance 0), the others random"""
    n, d = X.shape
    Xs = (rng.uniform(0.0, 4.0, size=(ns, d)) / math.sqrt(d)).astype(dtype)
    Xs[::5] = X[rng.integers(0, n, size=len(Xs[::5]))]
    return Xs


def _container(X, container):
    return X[:, 0].copy() if container == "vector" else (agp.ColVecs(np.ascontiguousarray(X.T)) if container == "colvecs" else agp.RowVecs(X))


@lru_cache(maxsize=None)
def single_case(cid, dtype=np.float64):
    (_, n, ns, S, kind, tr, d, container, noise, mean), = [c for c in SINGLE + F32 if c[0] == cid]
    seed = 1000 + [c[0] for c in SINGLE + F32].index(cid)
    c = bc.make_case(n, kind, tr, d, container, "scalar" if noise == "dense" else noise, mean, seed, dtype)
    rng = np.random.default_rng(seed + 1)
    if dtype == np.float32:  # fp32-sized noise, as the fp32 fits of tests/test_gpu_api.py
        c["s2"] = np.float32(0.1)
        c["fx"] = c["fx"].f(c["fx"].x, c["s2"])
        c["ofx"] = o.FiniteGP(c["ofx"].f, np.asarray(c["ofx"].x, dtype=np.float64), 0.1)
    if noise == "dense":
        c["s2"] = _dense_noise(rng, n, 1.3, dtype)
        c["fx"] = c["fx"].f(c["fx"].x, c["s2"])
        c["ofx"] = None
    c.update(id=cid, S=S, ns=ns, Y=_columns(rng, n, S, dtype), okernel=c.get("ofx") and c["ofx"].f.kernel, composite=False)
    c["Xs"] = _test_points(rng, c["X"], ns, dtype)
    c["xs"] = _container(c["Xs"], c["container"])
    c["mean_fn"] = {"zero": None, "const": 0.4, "custom": bc.custom_mean}[mean]
    c["scale"] = {"none": None, "scale": 0.7, "ard": np.linspace(0.5, 0.9, c["d"])}[tr]
    return c


@lru_cache(maxsize=None)
def composite_case(cid):
    (_, n, ns, S), = [c for c in COMPOSITE if c[0] == cid]
    rng = np.random.default_rng(77 + n)
    if cid == "mauna_loa":
        k = cr.ml_kernel()
        x, _ = cr.dense_data(n)
        X = x[:, None]
        s2, mean_fn, container = 0.05, None, "vector"
    else:
        k = per_se_rq_white()
        X = rng.uniform(0.0, 3.0, size=(n, 2))
        s2, mean_fn, container = 0.03 * rng.uniform(1.0, 2.0, size=n), 0.4, "rowvecs"
    f = agp.GP(k) if mean_fn is None else agp.GP(mean_fn, k)
    Xs = rng.uniform(X.min(), X.max(), size=(ns, X.shape[1]))
    Xs[::5] = X[rng.integers(0, n, size=len(Xs[::5]))]
    return {"id": cid, "n": n, "ns": ns, "S": S, "d": X.shape[1], "fx": f(_container(X, container), s2), "ofx": None, "X": X, "s2": s2, "kernel": k,
            "Y": _columns(rng, n, S, np.float64), "Xs": Xs, "xs": _container(Xs, container), "mean_fn": mean_fn, "container": container, "composite": True,
            "noise": "scalar" if np.ndim(s2) == 0 else "vector"}


def _okernel(c):
    return o.Kernel(c["kind"], 1.3, c["scale"])


def gram(c, A, B=None):
    """K(A, B) of the case's kernel in fp64"""
    A = np.asarray(A, dtype=np.float64)
    B = None if B is None else np.asarray(B, dtype=np.float64)
    if c["composite"]:
        return cr.ref_kernelmatrix(c["kernel"], A, B)
    return o.kernelmatrix(_okernel(c), A, B)


def mean_at(c, X):
    return o.mean_vector(c["mean_fn"], np.asarray(X, dtype=np.float64) if c["d"] > 1 else np.asarray(X, dtype=np.float64)[:, 0])


@lru_cache(maxsize=None)
def _reference(kind_of_case, cid, dtype):
    c = composite_case(cid) if kind_of_case == "composite" else single_case(cid, dtype)
    n, S = c["n"], c["S"]
    X = np.asarray(c["X"], dtype=np.float64)
    Y = np.asarray(c["Y"], dtype=np.float64)
    Xs = np.asarray(c["Xs"], dtype=np.float64)
    ref = {}
    if c["ofx"] is not None:  # the oracle, column by column
        fits = [o.logpdf_and_posterior(c["ofx"], Y[:, s]) for s in range(S)]
        ref["lp"] = np.array([float(lp) for lp, _ in fits])
        ref["alpha"] = np.stack([np.asarray(p.alpha) for _, p in fits], axis=1)
        ref["mean"] = np.stack([p.mean(Xs if c["d"] > 1 else Xs[:, 0]) for _, p in fits], axis=1)
        p0 = fits[0][1]
        ref["var"], ref["cov"] = p0.var(Xs if c["d"] > 1 else Xs[:, 0]), p0.cov(Xs if c["d"] > 1 else Xs[:, 0])
        gs = [o.logpdf_grad(c["ofx"], Y[:, s]) for s in range(S)]
        ref["grad"] = {"variance": sum(g["variance"] for g in gs), "scale": None if gs[0]["scale"] is None else sum(np.asarray(g["scale"]) for g in gs),
                       "noise": sum(np.asarray(g["noise"]) for g in gs), "x": sum(g["x"] for g in gs)}
        return ref
    # composite kernels / dense Σy: NumPy with SciPy's Cholesky, column by column
    m = mean_at(c, X)
    Cm = gram(c, X) + cdx.noise_matrix(np.asarray(c["s2"], dtype=np.float64), n)
    L = sla.cholesky(Cm, lower=True)
    D = Y - m[:, None]
    A = np.stack([sla.cho_solve((L, True), D[:, s]) for s in range(S)], axis=1)
    ref["alpha"] = A
    ref["lp"] = np.array([-0.5 * (n * math.log(2 * math.pi) + 2 * np.sum(np.log(np.diag(L))) + D[:, s] @ A[:, s]) for s in range(S)])
    Ks = gram(c, Xs, X)
    ref["mean"] = mean_at(c, Xs)[:, None] + np.stack([Ks @ A[:, s] for s in range(S)], axis=1)
    V = sla.solve_triangular(L, Ks.T, lower=True)
    ref["cov"] = gram(c, Xs) - V.T @ V
    ref["var"] = np.diag(ref["cov"]).copy()
    Ci = sla.cho_solve((L, True), np.eye(n))
    W = sum(np.outer(A[:, s], A[:, s]) - Ci for s in range(S))  # Σ_s (α_s α_sᵀ − C⁻¹)
    g = {"noise": 0.5 * W if np.ndim(c["s2"]) == 2 else (0.5 * np.diag(W).copy() if np.ndim(c["s2"]) == 1 else 0.5 * np.trace(W))}
    if c["composite"]:
        _, dK = cr.ref_kernelmatrix(c["kernel"], X, grad=True)
        g["theta"] = np.array([0.5 * np.sum(W * d) for d in dK])
        g["x"] = np.einsum("ij,ijp->ip", W, cdx.ref_dk_dt(c["kernel"], X))
    else:  # single kind with a dense Σy: the oracle's closed forms with Σ_s over the weights
        ok = _okernel(c)
        s = ok.scale_vec(c["d"])
        Xsc = X * s
        diff2 = (Xsc[:, None, :] - Xsc[None, :, :]) ** 2
        r2 = diff2.sum(-1)
        dk = o._dkappa_dr2(ok.kind, r2)
        Wt = 0.5 * W
        g["variance"] = float(np.sum(Wt * o._kappa(ok.kind, r2)))
        g["scale"] = (None if ok.scale is None else
                      (float(np.sum(Wt * ok.variance * dk * 2.0 * r2 / float(ok.scale))) if np.ndim(ok.scale) == 0 else
                       np.array([np.sum(Wt * ok.variance * dk * 2.0 * diff2[:, :, p] / s[p]) for p in range(c["d"])])))
        G = Wt * (ok.variance * dk)
        np.fill_diagonal(G, 0.0)
        g["x"] = 4.0 * s[None, :] * (G.sum(axis=1)[:, None] * Xsc - G @ Xsc)
    ref["grad"] = g
    return ref


def reference(c, dtype=np.float64):
    """{"lp" (S,), "alpha" (n, S), "mean" (ns, S), "var" (ns,), "cov" (ns, ns), "grad": gradient of Σ_s logpdf}: computed once per case, shared, not modified"""
    return _reference("composite" if c["composite"] else "single", c["id"], dtype)


def grad_x_shaped(c, gx):
    """the reference's (n, D) input gradient in the shape logpdf_and_grad returns it for the case's container"""
    gx = np.asarray(gx)
    if c["container"] == "vector":
        return gx[:, 0] if gx.ndim == 2 else gx
    return gx.T if c["container"] == "colvecs" else gx


def rel(a, ref):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))
