"""Seeded cases shared by tests/test_vfe_cols_cpu.py and tests/test_gpu_vfe_cols.py: S sparse (VFE / DTC) GPs that share x, z, kernel, jitter, Σy and the
prior mean and differ in y (the columns of Y), each built as a FiniteGP of the mirror, and the fp64 reference: oracle/gp_oracle.py column by column
(vfe_posterior, elbo, dtc_log_evidence, vfe_update_obs, vfe_update_z, and elbo_grad summed over the columns).

Inputs are drawn as tests/test_gpu_random_vfe.py and tests/cols_cases.py draw theirs: Σy is at least 1e-2 of the prior variance, the jitter 1e-6 … 1e-4,
the columns smooth parts of different phase plus noise, so the oracle stays as far inside the tolerances as it does in those files.

The shapes are a pairwise selection, the smallest that reach every edge: M ∈ {1, 63, 128, 129, 200} around the 128-row tile and the padding of the M×M
side, S ∈ {1, 2, 15, 16, 17, 128} around one 16-column MFMA block and at the cap, n ∈ {1, 65, 300} as one chunk and n = 4 500 as three chunks of 2 048
(the last ragged) on a private Context, D ∈ {1, 3, 17} (D > 16 takes vgrad_kernel and the per-column kvec means), the four kinds × none / Scale / ARD,
the three containers, scalar and diagonal Σy, zero / const / custom mean.  The gradient reference (2.6 s per column at n = 4 500) runs with S = 2 there."""
from functools import lru_cache

import numpy as np

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_cases as bc

OBJ_RTOL, M_ATOL, V_ATOL, A_RTOL = 1e-8, 1e-7, 1e-8, 1e-8
OBJ_RTOL32, P_ATOL32, G_RTOL32 = 1e-4, 1e-3, 5e-3
VAR = 1.3
NS = 9

# (id, M, S, n, D, kind, transform, container, noise, mean, jitter, chunk)
CASES = [
    ("m1_s1", 1, 1, 1, 1, 0, "none", "vector", "scalar", "zero", 1e-4, 0),
    ("m63_s2", 63, 2, 65, 1, 0, "scale", "vector", "vector", "const", 1e-4, 0),
    ("m128_s15", 128, 15, 300, 17, 2, "ard", "rowvecs", "scalar", "custom", 1e-5, 0),
    ("m129_s16", 129, 16, 300, 3, 3, "none", "rowvecs", "vector", "zero", 1e-4, 0),
    ("m200_s17", 200, 17, 300, 3, 1, "ard", "colvecs", "scalar", "const", 1e-6, 0),
    ("m63_s128", 63, 128, 300, 3, 2, "scale", "colvecs", "vector", "zero", 1e-4, 0),
    ("m129_s2_n4500", 129, 2, 4500, 3, 1, "none", "rowvecs", "scalar", "custom", 1e-4, 2048),
    ("m200_s16_n65", 200, 16, 65, 17, 3, "scale", "colvecs", "vector", "zero", 1e-5, 0),
    ("m1_s17", 1, 17, 65, 3, 3, "ard", "rowvecs", "scalar", "const", 1e-4, 0),
    ("m128_s128_n1", 128, 128, 1, 1, 1, "scale", "vector", "vector", "custom", 1e-4, 0),
]
IDS = [c[0] for c in CASES]
# the gradient reference costs 0.14 s per column at n = 300: the cap case (128 columns) is left to the fit / prediction tests
GRAD_IDS = [i for i in IDS if i not in ("m63_s128", "m128_s128_n1")]
# updates need observations to stream again and room for a second batch
UPDATE_IDS = ["m63_s2", "m129_s16", "m200_s17", "m129_s2_n4500"]
# fp32 handles: (id of the shape, S)
F32 = [("m129_s16", 17), ("m63_s128", 128)]
N2, M2 = 77, 10


def container(X, kind):
    return X[:, 0].copy() if kind == "vector" else (agp.ColVecs(np.ascontiguousarray(X.T)) if kind == "colvecs" else agp.RowVecs(X))


def opoints(X, kind):
    return X[:, 0] if kind == "vector" else X


def columns(rng, X, S, dtype=np.float64):
    """S different columns: smooth parts of different phase plus noise"""
    t = X.sum(1)[:, None]
    s = np.arange(S)[None, :]
    return (np.sin(t * (1.0 + 0.37 * s) + s) + 0.1 * rng.standard_normal((X.shape[0], S))).astype(dtype)


@lru_cache(maxsize=None)
def case(cid, dtype=np.float64, S_override=None):
    (_, M, S, n, d, kind, tr, cont, noise, mean, jitter, chunk), = [c for c in CASES if c[0] == cid]
    S = S_override or S
    rng = np.random.default_rng(7000 + IDS.index(cid))
    X = rng.uniform(-2.0, 2.0, size=(n + N2, d)).astype(dtype)
    Z = rng.uniform(-2.0, 2.0, size=(M + M2, d))
    if M <= n // 2:  # pseudo-points near observations, as tests/test_gpu_random_vfe.py
        Z[:M] = X[rng.permutation(n)[:M]] + 0.01 * rng.standard_normal((M, d))
    Z = Z.astype(dtype)
    scale = {"none": None, "scale": 0.7, "ard": np.linspace(0.5, 0.9, d)}[tr]
    k = VAR * agp.Kernel(kind)
    if tr == "scale":
        k = k @ agp.ScaleTransform(0.7)
    elif tr == "ard":
        k = k @ agp.ARDTransform(scale)
    if dtype == np.float32:  # fp32-sized noise, as the fp32 fits of tests/test_gpu_api.py
        s2_all = np.float32(0.1) if noise == "scalar" else rng.uniform(0.1, 0.3, size=n + N2).astype(dtype)
    else:
        s2_all = float(rng.uniform(0.02, 0.3)) if noise == "scalar" else rng.uniform(0.02, 0.3, size=n + N2)
    mfn = {"zero": None, "const": 0.4, "custom": bc.custom_mean}[mean]
    Y = columns(rng, X, S, dtype)
    Xs = rng.uniform(-2.0, 2.0, size=(NS, d)).astype(dtype)
    s2 = lambda a, b: s2_all if np.ndim(s2_all) == 0 else s2_all[a:b]
    return {"id": cid, "M": M, "S": S, "n": n, "d": d, "kind": kind, "tr": tr, "container": cont, "noise": noise, "mean": mean, "jitter": jitter, "chunk": chunk,
            "kernel": k, "okernel": o.Kernel(kind, VAR, scale), "mean_fn": mfn, "X": X, "Z": Z, "Y": Y, "Xs": Xs, "s2_1": s2(0, n), "s2_2": s2(n, n + N2),
            "s2_all": s2_all, "dtype": dtype}


def mirror(c, ctx=None):
    """(f, fz, fx, fx2, fz2, xs) of the mirror for the case; ctx: a private Context for the chunked case"""
    f = agp.GP(c["kernel"], ctx=ctx) if c["mean_fn"] is None else agp.GP(c["mean_fn"], c["kernel"], ctx=ctx)
    n, M, cont = c["n"], c["M"], c["container"]
    return (f, f(container(c["Z"][:M], cont), c["jitter"]), f(container(c["X"][:n], cont), c["s2_1"]), f(container(c["X"][n:], cont), c["s2_2"]),
            f(container(c["Z"][M:], cont), c["jitter"]), container(c["Xs"], cont))


def oracle_parts(c):
    """(of, z, ofx, ofx2, z2, xs, ofx_all) of the oracle, fp64 — one prior object per case (the oracle asserts `post.prior is fx.f`)"""
    return _oracle_parts(c["id"], c["dtype"], c["S"])


@lru_cache(maxsize=None)
def _oracle_parts(cid, dtype, S):
    c = case(cid, dtype, S)
    n, M, cont = c["n"], c["M"], c["container"]
    X, Z = np.asarray(c["X"], dtype=np.float64), np.asarray(c["Z"], dtype=np.float64)
    of = o.GP(c["okernel"], c["mean_fn"])
    f64 = lambda v: float(v) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)
    return (of, opoints(Z[:M], cont), o.FiniteGP(of, opoints(X[:n], cont), f64(c["s2_1"])), o.FiniteGP(of, opoints(X[n:], cont), f64(c["s2_2"])),
            opoints(Z[M:], cont), opoints(np.asarray(c["Xs"], dtype=np.float64), cont), o.FiniteGP(of, opoints(X, cont), f64(c["s2_all"])))


@lru_cache(maxsize=None)
def reference(cid, dtype=np.float64, S_override=None):
    """Column by column from the oracle, computed once per case, shared, not modified:
    {"elbo", "dtc" (S,), "alpha", "m_eps" (M, S), "U", "Lam_U" (M, M), "b_y" (n, S), "mean" (ns, S), "var" (ns,), "cov" (ns, ns), "posts": the S oracle posteriors}"""
    c = case(cid, dtype, S_override)
    of, z, ofx, _, _, xs, _ = oracle_parts(c)
    Y = np.asarray(c["Y"], dtype=np.float64)[:c["n"]]
    posts = [o.vfe_posterior(of, z, c["jitter"], ofx, Y[:, s]) for s in range(c["S"])]
    p0 = posts[0]
    return {"elbo": np.array([o.elbo(of, z, c["jitter"], ofx, Y[:, s]) for s in range(c["S"])]),
            "dtc": np.array([o.dtc_log_evidence(of, z, c["jitter"], ofx, Y[:, s]) for s in range(c["S"])]),
            "alpha": np.stack([p.alpha for p in posts], axis=1), "m_eps": np.stack([p.m_eps for p in posts], axis=1), "U": p0.U, "Lam_U": p0.Lam_U,
            "b_y": np.stack([p.b_y for p in posts], axis=1), "mean": np.stack([p.mean(xs) for p in posts], axis=1), "var": p0.var(xs), "cov": p0.cov(xs),
            "posts": posts}


def sum_grads(gs):
    """Σ_s of the oracle's elbo_grad dicts; "y" / "mean" stacked as (n, S)"""
    g0 = gs[0]
    return {"variance": sum(g["variance"] for g in gs), "scale": None if g0["scale"] is None else sum(np.asarray(g["scale"]) for g in gs),
            "noise": sum(np.asarray(g["noise"]) for g in gs), "y": np.stack([g["y"] for g in gs], axis=1), "mean": np.stack([g["mean"] for g in gs], axis=1),
            "z": sum(g["z"] for g in gs), "x": sum(g["x"] for g in gs)}


@lru_cache(maxsize=None)
def grad_reference(cid, vfe=True):
    """Σ_s elbo_grad of the fresh fit"""
    c = case(cid)
    of, z, ofx, _, _, _, _ = oracle_parts(c)
    Y = np.asarray(c["Y"], dtype=np.float64)[:c["n"]]
    return sum_grads([o.elbo_grad(of, z, c["jitter"], ofx, Y[:, s], vfe=vfe) for s in range(c["S"])])


def rel(a, ref):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))
