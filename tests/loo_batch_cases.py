"""Seeded ragged cases shared by tests/test_loo_batch_cpu.py and tests/test_gpu_loo_batch.py (gp_loo_batch / gp_loo_grad_batch and their *_sum forms), each
built as a FiniteGP of the mirror, and their fp64 reference (tests/loo_ref.py), computed once per case and not modified.

Shapes — the smallest at which the batch kernels can go wrong: n ∈ {1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 320}: the edges of the
64-column block, of the 128-row tile of the strips (batch_inv_kernel, batch_loo_kernel, batch_loo_beta_kernel), a last strip tile of 64 rows (191, 192:
np = 192) and three to five k-tiles in the product behind Z; D ∈ {1, 3, 16}; the four kinds × none / Scale / ARD, each at least once; the three input
containers; scalar and diagonal Σy; zero / const / custom mean.  Composite kernels: the Mauna Loa form (tests/composite_ref.ml_kernel) and a kernel with
29 θ entries (two GRAD_NP passes of batch_grad_kernel).  Three more batches share one x object (nx = 1), one y object (ny = 1), and both.

Conditioning as in tests/loo_cases.py: the noise level of every case is λ_max(K) / 500 (times 1 … 2 for a diagonal Σy), which bounds cond(C) by about
600; tests/test_loo_batch_cpu.py asserts cond(C) ≤ 1e3 for every case."""
from functools import lru_cache

import numpy as np

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_cases as bc
from tests import composite_ref as cr
from tests import loo_cases as lc
from tests import loo_ref as lr

# (id, n, kind, transform, D, container, noise, mean)
SINGLE = [
    ("b_n1", 1, 0, "scale", 3, "rowvecs", "scalar", "const"),
    ("b_n2", 2, 1, "ard", 3, "colvecs", "vector", "zero"),
    ("b_n63", 63, 2, "none", 1, "vector", "scalar", "custom"),
    ("b_n64", 64, 3, "scale", 16, "rowvecs", "vector", "zero"),
    ("b_n65", 65, 0, "ard", 16, "colvecs", "scalar", "const"),
    ("b_n127", 127, 1, "none", 3, "rowvecs", "vector", "custom"),
    ("b_n128", 128, 2, "scale", 1, "vector", "scalar", "zero"),
    ("b_n129", 129, 3, "ard", 3, "colvecs", "vector", "const"),
    ("b_n191", 191, 0, "none", 16, "rowvecs", "scalar", "custom"),
    ("b_n192", 192, 1, "scale", 3, "colvecs", "vector", "zero"),
    ("b_n193", 193, 2, "ard", 3, "rowvecs", "scalar", "const"),
    ("b_n257", 257, 3, "none", 3, "colvecs", "vector", "custom"),
    ("b_n320", 320, 0, "scale", 1, "vector", "scalar", "zero"),
    ("b_n320_ard16", 320, 1, "ard", 16, "rowvecs", "vector", "const"),
    ("b_n257_m32", 257, 2, "scale", 3, "rowvecs", "scalar", "zero"),
    ("b_n65_m52", 65, 3, "none", 1, "vector", "scalar", "const"),
]
SINGLE_IDS = [c[0] for c in SINGLE]
COMPOSITE = [("b_ml_193", 193, "scalar"), ("b_ml_128", 128, "vector"), ("b_theta29_130", 130, "vector"), ("b_theta29_65", 65, "scalar")]
COMPOSITE_IDS = [c[0] for c in COMPOSITE]
SHARED = ["shared_x", "shared_y", "shared_xy"]


def theta29_kernel():
    """29 θ entries (more than one pass of 16 in batch_grad_kernel) and a variance shared by two terms; D = 4"""
    SE, M32 = agp.SqExponentialKernel, agp.Matern32Kernel
    return (0.9 * (SE() @ agp.ARDTransform([0.6, 0.7, 0.8, 0.9]) + M32() @ agp.ARDTransform([0.5, 0.4, 0.3, 0.6]))
            * (agp.PeriodicKernel(r=[1.0, 1.1, 1.2, 1.3]) @ agp.ARDTransform([0.3, 0.2, 0.25, 0.35]))
            + 0.2 * agp.RationalQuadraticKernel(alpha=0.8) @ agp.ScaleTransform(0.9))


def _single(spec, seed, dtype=np.float64):
    cid, n, kind, tr, d, container, noise, mean = spec
    c = bc.make_case(n, kind, tr, d, container, "scalar", mean, seed, dtype)
    c["K"] = o.kernelmatrix(lc.okernel(c), np.asarray(c["X"], dtype=np.float64))
    c["s2"] = lc.noise_for(np.random.default_rng(seed + 1), c["K"], noise, dtype)
    c["fx"] = c["fx"].f(c["fx"].x, c["s2"])
    c.update(id=cid, noise=noise, composite=False, mean_fn={"zero": None, "const": 0.4, "custom": bc.custom_mean}[mean])
    return c


@lru_cache(maxsize=None)
def single_case(cid):
    i = SINGLE_IDS.index(cid)
    return _single(SINGLE[i], 3200 + 2 * i)


def _composite(cid, k, xin, X, y, form, mean_fn, seed):
    K = cr.ref_kernelmatrix(k, X)
    s2 = lc.noise_for(np.random.default_rng(seed), K, form)
    f = agp.GP(k) if mean_fn is None else agp.GP(mean_fn, k)
    return {"id": cid, "n": X.shape[0], "d": X.shape[1], "fx": f(xin, s2), "X": X, "y": y, "s2": s2, "K": K, "kernel": k,
            "container": "vector" if X.shape[1] == 1 else "rowvecs", "noise": form, "mean_fn": mean_fn, "composite": True}


@lru_cache(maxsize=None)
def composite_case(cid):
    (_, n, form), = [c for c in COMPOSITE if c[0] == cid]
    seed = 3300 + COMPOSITE_IDS.index(cid)
    if cid.startswith("b_ml"):
        x, y = cr.dense_data(n)
        return _composite(cid, cr.ml_kernel(), x, x[:, None], y, form, None, seed)
    rng = np.random.default_rng(seed + 50)
    X = rng.uniform(0, 3, size=(n, 4))
    y = np.cos(X[:, 0]) + 0.1 * rng.standard_normal(n)
    return _composite(cid, theta29_kernel(), agp.RowVecs(X), X, y, form, 0.4, seed)


def case(cid):
    return composite_case(cid) if cid in COMPOSITE_IDS else single_case(cid)


def ragged_batch():
    """the single-kind cases in an order that mixes the sizes (the kernels sort a wave by size themselves)"""
    order = [5, 12, 0, 9, 3, 14, 1, 11, 7, 2, 13, 4, 10, 6, 15, 8]
    return [single_case(SINGLE_IDS[i]) for i in order]


def composite_batch():
    return [composite_case(cid) for cid in COMPOSITE_IDS]


@lru_cache(maxsize=None)
def shared_batch(which):
    """four problems that share ONE x object ("shared_x"), ONE y object ("shared_y": four x of one size) or both; kernels, noise forms and means differ.
    n = 129 (two strip tiles, the second one ragged), D = 3."""
    n, d = 129, 3
    specs = [(0, "ard", "scalar", "zero"), (1, "none", "vector", "const"), (2, "scale", "scalar", "custom"), (3, "ard", "vector", "zero")]
    base = [_single((f"{which}_{b}", n, kind, tr, d, "rowvecs", noise, mean), 3400 + 10 * SHARED.index(which) + (0 if which != "shared_y" else b))
            for b, (kind, tr, noise, mean) in enumerate(specs)]
    # (one seed for all where x is shared: the same X; the noise level follows each problem's own K)
    out = []
    x0, y0 = base[0]["fx"].x, base[0]["y"]
    for b, c in enumerate(base):
        c = dict(c)
        if which != "shared_y":
            assert np.array_equal(c["X"], base[0]["X"])
            c["fx"] = c["fx"].f(x0, c["s2"])
        if which == "shared_x":
            c["y"] = np.random.default_rng(3490 + b).standard_normal(n)
        else:
            c["y"] = y0
        out.append(c)
    return out


def all_cases():
    return ragged_batch() + composite_batch() + [c for w in SHARED for c in shared_batch(w)]


_REFS = {}


def reference(c):
    """{"L", "lp", "mean", "var", "alpha", "c", "G", "grad": {"variance", "scale" | "theta", "noise", "y"}} — the recipe of tests/loo_cases.reference;
    keyed by the case's id and the identity of its y (the shared batches reuse ids of one recipe with different observations)"""
    key = (c["id"], id(c["y"]))
    if key not in _REFS:
        C, m = lc.covariance(c)
        y = np.asarray(c["y"], dtype=np.float64)
        ref = lr.closed_form(C, y - m, y)
        G, beta = lr.weight_matrix(C, y - m)
        nd = min(np.ndim(c["s2"]), 2)
        X = np.asarray(c["X"], dtype=np.float64)
        ref["grad"] = lr.composite_grads(c["kernel"], X, G, nd) if c["composite"] else lr.single_kind_grads(lc.okernel(c), X, G, nd)
        ref["grad"]["y"] = -beta
        ref["G"] = G
        ref["keep"] = c["y"]  # the id stays taken
        _REFS[key] = ref
    return _REFS[key]


def ratios(c, ref, L=None, lp=None, mean=None, var=None, g=None):
    """{group: error / bound} of whatever is given against the reference, at the tolerances of tests/loo_cases.py (as tests/test_gpu_loo.py applies them)"""
    out = {}
    if L is not None:
        out["L"] = abs(float(L) - ref["L"]) / (lc.L_TOL * abs(ref["L"]))
    if lp is not None:
        out["lp"] = float(np.max(np.abs(lp - ref["lp"]))) / (lc.L_TOL * max(1.0, float(np.max(np.abs(ref["lp"])))))
    if mean is not None:
        out["mean"] = float(np.max(np.abs(mean - ref["mean"]))) / lc.M_TOL
    if var is not None:
        out["var"] = float(np.max(np.abs(var - ref["var"]))) / lc.V_TOL
    if g is not None:
        rg = ref["grad"]
        if c["composite"]:
            out["theta"] = lc.grad_ratio(g["theta"], rg["theta"])
        else:
            out["variance"] = lc.grad_ratio(g["variance"], rg["variance"])
            if rg["scale"] is None:
                assert g["scale"] is None
            else:
                out["scale"] = lc.grad_ratio(g["scale"], rg["scale"])
        out["noise"] = lc.grad_ratio(g["noise"], rg["noise"])
        out["y"] = lc.grad_ratio(g["y"], rg["y"])
    return out


GOLDEN_BATCH_GRAD = "bits/batch_grad_bits_r32.npz"  # under tests/golden/ (a directory of its own: tests/test_oracle.py reads every .npz beside the oracle's)


def batch_grad_outputs():
    """{name: array} of every output of agp.logpdf_and_grad_batch (gp_logpdf_grad_batch / _sum, whose tile kernel this round generalised) on a fixed batch:
    twelve single-kind problems of 40 … 300 points with every kind, transform and noise form, and two Mauna Loa kernels at n = 150 — what
    tests/golden/bits/batch_grad_bits_r32.npz holds, recorded with the library of the commit before the generalisation."""
    singles = bc.small_cases(12, seed=32, lo=40)
    x, y = bc.mauna_loa_data(150)
    kernels = bc.perturbed_kernels(cr.mauna_loa_kernel(), 2)
    out = {}
    lp, grads = agp.logpdf_and_grad_batch([c["fx"] for c in singles], [c["y"] for c in singles])
    lpc, gradsc = agp.logpdf_and_grad_batch([agp.GP(k)(x, 1e-2 * agp.api._prior_variance(k)) for k in kernels], y)
    for tag, lps, gs in (("s", lp, grads), ("c", lpc, gradsc)):
        out[f"{tag}_logpdf"] = np.asarray(lps)
        for b, g in enumerate(gs):
            for k, v in g.items():
                if v is not None:
                    out[f"{tag}{b}_{k}"] = np.atleast_1d(np.asarray(v))
    return out


def grad_bytes(g):
    """every entry of a gradient dict as bytes, for bit comparisons"""
    return {k: (None if v is None else np.asarray(v).tobytes()) for k, v in g.items()}
