"""Seeded cases shared by tests/test_loo_cpu.py and tests/test_gpu_loo.py, each built as a FiniteGP of the mirror, and their fp64 reference
(tests/loo_ref.py), computed once per case and not modified.

Shapes: n ∈ {1, 2, 127, 128, 129, 257, 300} — one point, the smallest problem with a neighbour, the edges of one 128-row tile, three tile rows with a
ragged edge (257: the mirror kernel sees off-diagonal tiles) and 300; D ∈ {1, 3, 16, 17} (17 leaves the scratch-free gradient kernels); the four kinds ×
none / Scale / ARD, each once; the three input containers; scalar, diagonal and dense Σy (a C-ordered array goes out as noise kind 3, a Fortran-ordered
one as kind 2: either triangle); zero / const / custom mean.

Conditioning: the leave-one-out terms divide by [C⁻¹]_ii and the gradient multiplies by C⁻¹ twice, so the forward tolerances of the GPU tests mean
something only for a well-conditioned C.  The noise level of every case is λ_max(K) / 500 (times 1 … 2 for a diagonal Σy, plus a low-rank part for a
dense one), which bounds cond(C) by about 600; tests/test_loo_cpu.py asserts cond(C) ≤ 1e3 for every case."""
from functools import lru_cache

import numpy as np

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_cases as bc
from tests import composite_dx_ref as cdx
from tests import composite_ref as cr
from tests import loo_ref as lr

L_TOL, M_TOL, V_TOL, G_RTOL, G_ATOL, GX_ATOL = 1e-10, 1e-8, 1e-9, 1e-7, 1e-9, 1e-8

# (id, n, kind, transform, D, container, noise, mean)
SINGLE = [
    ("n1", 1, 0, "none", 1, "vector", "scalar", "zero"),
    ("n2", 2, 1, "scale", 3, "colvecs", "vector", "const"),
    ("n127", 127, 2, "ard", 16, "rowvecs", "scalar", "custom"),
    ("n128", 128, 3, "none", 3, "rowvecs", "vector", "zero"),
    ("n129_dense", 129, 0, "ard", 3, "colvecs", "dense_c", "const"),
    ("n257", 257, 1, "none", 1, "vector", "vector", "zero"),
    ("n300_d17", 300, 2, "none", 17, "rowvecs", "scalar", "custom"),
    ("n257_dense", 257, 3, "ard", 3, "colvecs", "dense_f", "zero"),
    ("n300", 300, 0, "scale", 3, "rowvecs", "scalar", "const"),
    ("n129_d17", 129, 1, "ard", 17, "colvecs", "vector", "zero"),
    ("n300_dense", 300, 2, "scale", 1, "vector", "dense_c", "custom"),
    ("n257_d16", 257, 3, "scale", 16, "rowvecs", "scalar", "const"),
]
COMPOSITE = [("mauna_loa", 200), ("six_term", 150)]
F32 = ("f32_n300", 300, 3, "scale", 3, "rowvecs", "scalar", "const")
CPU_IDS = ["n1", "n2", "n129_dense", "n300"]  # (the brute-force sizes of tests/test_loo_cpu.py are its own)


def noise_for(rng, K, form, dtype=np.float64):
    """Σy of the given form at the level λ_max(K) / 500"""
    n = K.shape[0]
    s2 = float(np.linalg.eigvalsh(K)[-1]) / 500.0
    if form == "scalar":
        return dtype(s2)
    if form == "vector":
        return (s2 * rng.uniform(1.0, 2.0, size=n)).astype(dtype)
    B = rng.standard_normal((n, 3))
    S = (s2 * (np.eye(n) + 0.5 * (B @ B.T) / 3.0)).astype(dtype)
    return np.asfortranarray(S) if form == "dense_f" else np.ascontiguousarray(S)


def okernel(c):
    return o.Kernel(c["kind"], 1.3, {"none": None, "scale": 0.7, "ard": np.linspace(0.5, 0.9, c["d"])}[c["tr"]])


@lru_cache(maxsize=None)
def single_case(cid, dtype=np.float64):
    (_, n, kind, tr, d, container, noise, mean), = [c for c in SINGLE + [F32] if c[0] == cid]
    seed = 2800 + [c[0] for c in SINGLE + [F32]].index(cid)
    c = bc.make_case(n, kind, tr, d, container, "scalar", mean, seed, dtype)
    c["K"] = o.kernelmatrix(okernel(c), np.asarray(c["X"], dtype=np.float64))
    c["s2"] = noise_for(np.random.default_rng(seed + 1), c["K"], noise, dtype)
    c["fx"] = c["fx"].f(c["fx"].x, c["s2"])
    c.update(id=cid, noise=noise, composite=False, mean_fn={"zero": None, "const": 0.4, "custom": bc.custom_mean}[mean])
    return c


@lru_cache(maxsize=None)
def composite_case(cid):
    (_, n), = [c for c in COMPOSITE if c[0] == cid]
    rng = np.random.default_rng(2877 + n)
    if cid == "mauna_loa":
        k = cr.ml_kernel()
        x, y = cr.dense_data(n)
        X, container, mean_fn, form = x[:, None], "vector", None, "scalar"
        xin = x
    else:
        k = cdx.six_term_kernel()
        X, y = cdx.six_term_data(n, seed=5)
        container, mean_fn, form = "rowvecs", 0.4, "vector"
        xin = agp.RowVecs(X)
    K = cr.ref_kernelmatrix(k, X)
    s2 = noise_for(rng, K, form)
    f = agp.GP(k) if mean_fn is None else agp.GP(mean_fn, k)
    return {"id": cid, "n": n, "d": X.shape[1], "fx": f(xin, s2), "X": X, "y": y, "s2": s2, "K": K, "kernel": k, "container": container, "noise": form,
            "mean_fn": mean_fn, "composite": True}


def covariance(c):
    """(C, m) in fp64"""
    X = np.asarray(c["X"], dtype=np.float64)
    s2 = np.asarray(c["s2"], dtype=np.float64)
    if s2.ndim == 2:  # the mirror reads the upper triangle of the array it is given
        s2 = np.triu(s2) + np.triu(s2, 1).T
    m = o.mean_vector(c["mean_fn"], X if c["d"] > 1 else X[:, 0])
    return c["K"] + cdx.noise_matrix(s2, c["n"]), m


@lru_cache(maxsize=None)
def _reference(composite, cid, dtype):
    c = composite_case(cid) if composite else single_case(cid, dtype)
    C, m = covariance(c)
    y = np.asarray(c["y"], dtype=np.float64)
    ref = lr.closed_form(C, y - m, y)
    G, beta = lr.weight_matrix(C, y - m)
    nd = min(np.ndim(c["s2"]), 2)
    X = np.asarray(c["X"], dtype=np.float64)
    ref["grad"] = lr.composite_grads(c["kernel"], X, G, nd) if composite else lr.single_kind_grads(okernel(c), X, G, nd)
    ref["grad"]["y"] = -beta
    ref["G"] = G
    return ref


def reference(c, dtype=np.float64):
    """{"L", "lp", "mean", "var", "alpha", "c", "G", "grad": {"variance", "scale" | "theta", "noise", "y", "x"}}"""
    return _reference(c["composite"], c["id"], dtype)


def grad_x_shaped(c, gx):
    """the reference's (n, D) input gradient in the shape loo_logpdf_and_grad returns it for the case's container"""
    gx = np.asarray(gx)
    if c["container"] == "vector":
        return gx[:, 0] if gx.ndim == 2 else gx
    return gx.T if c["container"] == "colvecs" else gx


def grad_ratio(got, ref, rtol=G_RTOL, atol=G_ATOL):
    """worst |got − ref| / (rtol·|ref| + atol·max|ref|) over the entries of one gradient group (θ and noise gradients: 1e-7·|ref| + 1e-9·g∞)"""
    got, ref = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    err, den = np.abs(got - ref), rtol * np.abs(ref) + atol * np.max(np.abs(ref))
    with np.errstate(divide="ignore", invalid="ignore"):  # a group that is identically zero (∂/∂scale of a one-point problem) must come back as zeros
        return float(np.max(np.where(err == 0.0, 0.0, err / den)))


def gradx_ratio(got, ref):
    """worst |got − ref| / (1e-7·|ref| + 1e-8·max(1, max|ref|)) over the entries of ∂/∂x"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / (G_RTOL * np.abs(ref) + GX_ATOL * max(1.0, float(np.max(np.abs(ref)))))))
