"""Seeded problems shared by tests/test_gpu_batch.py and tests/test_batch_cpu.py: each case is built twice, as a FiniteGP of the mirror and as one of the
oracle, from the same arrays.  Σy is at least 1e-2 of the prior variance, so that K + Σy is well conditioned and the oracle itself is far inside the
tolerances the GPU tests use (tests/test_batch_cpu.py checks that against SciPy)."""
import math

import numpy as np

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o

FIXED_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 545, 1000]
TRANSFORMS = ["none", "scale", "ard"]
CONTAINERS = ["vector", "colvecs", "rowvecs"]
NOISES = ["scalar", "vector"]
MEANS = ["zero", "const", "custom"]


def custom_mean(v):
    return 0.3 * float(np.sum(v)) + 0.1


def make_case(n, kind, tr, d, container, noise, mean, seed, dtype=np.float64):
    """One problem: dict with the mirror's FiniteGP ("fx"), the oracle's ("ofx"), y and the spec."""
    rng = np.random.default_rng(seed)
    if container == "vector":
        d = 1
    X = (rng.uniform(0.0, 4.0, size=(n, d)) / math.sqrt(d)).astype(dtype)
    y = rng.standard_normal(n).astype(dtype)
    var = 1.3
    scale = {"none": None, "scale": 0.7, "ard": np.linspace(0.5, 0.9, d)}[tr]
    base = [agp.SqExponentialKernel, agp.Matern12Kernel, agp.Matern32Kernel, agp.Matern52Kernel][kind]()
    k = var * base
    if tr == "scale":
        k = k @ agp.ScaleTransform(0.7)
    elif tr == "ard":
        k = k @ agp.ARDTransform(scale)
    s2 = 1.3e-2 if noise == "scalar" else (var * rng.uniform(1e-2, 5e-2, size=n)).astype(dtype)
    mfn = {"zero": None, "const": 0.4, "custom": custom_mean}[mean]
    xin = X[:, 0].copy() if container == "vector" else (agp.ColVecs(np.ascontiguousarray(X.T)) if container == "colvecs" else agp.RowVecs(X))
    f = agp.GP(k) if mfn is None else agp.GP(mfn, k)
    ofx = o.FiniteGP(o.GP(o.Kernel(kind, var, scale), mfn), X[:, 0] if container == "vector" else X, s2)
    return {"fx": f(xin, s2), "ofx": ofx, "y": y, "n": n, "kind": kind, "tr": tr, "d": d, "container": container, "noise": noise, "mean": mean,
            "X": X, "s2": s2}


def ragged_cases(nrandom=26, seed=2024, max_random=900):
    """The fixed sizes and `nrandom` random ones; kinds, transforms, D, containers, noise forms and means cycle with co-prime periods and are then
    shuffled against the sizes, so that every value of every category occurs."""
    rng = np.random.default_rng(seed)
    sizes = FIXED_SIZES + [int(v) for v in rng.integers(3, max_random, size=nrandom)]
    cases = []
    for b, n in enumerate(sizes):
        cont = CONTAINERS[b % 3]
        d = 1 if cont == "vector" else [1, 3, 8][(b // 3) % 3]
        cases.append(make_case(n, b % 4, TRANSFORMS[(b // 4) % 3], d, cont, NOISES[(b // 2) % 2], MEANS[(b // 5) % 3], seed=1000 + b))
    return cases


def small_cases(nb, seed, lo=1, hi=300):
    """nb quick problems of random sizes in [lo, hi] (neighbours, failure batches)."""
    rng = np.random.default_rng(seed)
    return [make_case(int(rng.integers(lo, hi + 1)), b % 4, TRANSFORMS[b % 3], [1, 3, 8][b % 3], CONTAINERS[1 + b % 2], NOISES[b % 2], MEANS[b % 3],
                      seed=seed * 7919 + b) for b in range(nb)]


def host_fit(C, delta):
    """logpdf and α of N(0, C) at delta by SciPy's Cholesky (LAPACK dpotrf / dpotrs)."""
    import scipy.linalg as sla

    cf = sla.cho_factor(C, lower=True)
    alpha = sla.cho_solve(cf, delta)
    lp = -0.5 * (len(delta) * math.log(2 * math.pi) + 2.0 * np.sum(np.log(np.diag(cf[0]))) + delta @ alpha)
    return lp, alpha


def oracle_fit(case):
    lp, post = o.logpdf_and_posterior(case["ofx"], case["y"])
    return float(lp), np.asarray(post.alpha)


def lp_err(lp, ref):
    """error of a logpdf relative to max(|reference|, 1): a one-point problem's logpdf can be near zero"""
    return abs(float(lp) - float(ref)) / max(abs(float(ref)), 1.0)


def vec_err(a, ref):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def mauna_loa_data(n=545, seed=0):
    """Seeded monthly series, x in years: trend + seasonal + noise (the shape of examples/1-mauna-loa)."""
    rng = np.random.default_rng(seed)
    x = np.arange(n) / 12.0
    y = 0.02 * x**2 + 1.3 * x + 3.0 * np.sin(2 * np.pi * x) + 0.8 * np.cos(4 * np.pi * x) + 0.3 * rng.standard_normal(n)
    return x, y - y.mean()


def perturbed_kernels(k, nb, seed=5, width=0.05):
    """nb copies of the composite kernel k with every parameter moved by up to ± width (relative)."""
    rng = np.random.default_rng(seed)
    th = agp.api.params(k)
    return [agp.api.with_params(k, th * (1.0 + width * rng.uniform(-1, 1, size=th.shape))) for _ in range(nb)]
