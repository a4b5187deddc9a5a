"""Seeded problems shared by tests/test_gpu_batch_joint.py and tests/test_batch_joint_cpu.py: the problems of tests/batch_cases.py (Σy at least 1e-2 of the
prior variance) with test points, a Σy* over them, held-out observations and standard normals — each built for the mirror and for the oracle from the same
arrays.  Test points are drawn like the training inputs; in every third problem half of them ARE training points.  Σy* alternates between the scalar 1.3e-2
and a vector in [1e-2, 5e-2] · variance, so that C* + Σy* is well conditioned and the oracle itself is far inside the tolerances the GPU tests use
(tests/test_batch_joint_cpu.py checks that against SciPy).

The sizes are the smallest at which the kernels of gp_joint_batch can still go wrong: n around the 64-column block of the fit and one of three blocks; ns on
both sides of a 32-row wave tile (31, 32, 33), of a 64×64 covariance tile (63, 64, 65), of a predict strip of 128 test points (127, 128, 129: a covariance
tile that spans two strips, a last strip with one valid row), three strips with a half-filled last one (193) and 300."""
import functools

import numpy as np

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_cases as bc

N_SIZES = [1, 63, 64, 65, 129, 300]
NS_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 300]
NSAMP = 3
VAR = 1.3  # the prior variance of bc.make_case


def as_container(case, XS):
    if case["container"] == "vector":
        return XS[:, 0].copy()
    return agp.ColVecs(np.ascontiguousarray(XS.T)) if case["container"] == "colvecs" else agp.RowVecs(XS)


def with_joint(case, ns, seed, coincide=False, vector_noise=False, nsamp=NSAMP):
    """The case with ns test points ("xs" for the mirror, "oxs" for the oracle), Σy* ("nz"), held-out observations ("ys") and standard normals ("xi", ns × nsamp)."""
    rng = np.random.default_rng(seed)
    n, d = case["X"].shape
    XS = (rng.uniform(0.0, 4.0, size=(ns, d)) / np.sqrt(d)).astype(case["X"].dtype)
    if coincide:
        k = ns // 2
        XS[:k] = case["X"][rng.integers(0, n, size=k)]
    nz = (VAR * rng.uniform(1e-2, 5e-2, size=ns)) if vector_noise else 1.3e-2
    return dict(case, xs=as_container(case, XS), oxs=(XS[:, 0] if case["container"] == "vector" else XS), XS=XS, ns=ns, nz=nz,
                ys=rng.standard_normal(ns), xi=rng.standard_normal((ns, nsamp)))


@functools.lru_cache(maxsize=None)
def joint_cases():
    """Every ns twice against the training sizes cycling with another period; kinds, transforms, D, containers, noise forms and means cycle as in
    bc.ragged_cases."""
    cases = []
    for b, ns in enumerate(NS_SIZES + NS_SIZES):
        n = N_SIZES[(b + 3 * (b // len(NS_SIZES))) % len(N_SIZES)]
        cont = bc.CONTAINERS[b % 3]
        d = 1 if cont == "vector" else [1, 3, 8][(b // 3) % 3]
        c = bc.make_case(n, b % 4, bc.TRANSFORMS[(b // 4) % 3], d, cont, bc.NOISES[(b // 2) % 2], bc.MEANS[(b // 5) % 3], seed=5000 + b)
        cases.append(with_joint(c, ns, seed=6000 + b, coincide=b % 3 == 0, vector_noise=b % 2 == 1))
    return cases


def oracle_joint(case):
    """dict: the training logpdf, mean, latent covariance, held-out logpdf and samples of one case by the oracle"""
    post = o.posterior(case["ofx"], case["y"])
    m, C = post.mean_and_cov(case["oxs"])
    fxs = o.FiniteGP(post, case["oxs"], case["nz"])
    return {"lp": float(o.logpdf(case["ofx"], case["y"])), "mean": np.asarray(m), "cov": np.asarray(C), "hl": float(o.logpdf(fxs, case["ys"])),
            "samples": np.asarray(o.rand_from(fxs, case["xi"]))}


@functools.lru_cache(maxsize=None)
def joint_refs():
    """the oracle's answers to joint_cases(), computed once and shared"""
    return [oracle_joint(c) for c in joint_cases()]


def call(cases, **kw):
    """agp.joint_batch on the cases with everything they carry"""
    kw.setdefault("what", 29)
    return agp.joint_batch([c["fx"] for c in cases], [c["y"] for c in cases], [c["xs"] for c in cases], noise=[c["nz"] for c in cases],
                           ys_heldout=[c["ys"] for c in cases], xi=[c["xi"] for c in cases], **kw)


def errs(quad, lp, ref):
    """(mean, cov, training logpdf, held-out logpdf, samples): absolute maxima; the logpdfs relative to max(|reference|, 1)"""
    amax = lambda a, r: float(np.max(np.abs(np.asarray(a) - r))) if np.size(r) else 0.0
    return (amax(quad[0], ref["mean"]), amax(quad[1], ref["cov"]), bc.lp_err(lp, ref["lp"]), bc.lp_err(quad[2], ref["hl"]), amax(quad[3], ref["samples"]))
