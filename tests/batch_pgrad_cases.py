"""Seeded problems with test points shared by tests/test_gpu_batch_predict_grad.py and tests/test_batch_predict_grad_cpu.py, and their fp64 host
references (tests/predict_grad_ref.HostPosterior).  The problems are those of tests/batch_cases.make_case; the test points are drawn as
tests/test_gpu_batch_predict.py draws them: from the box of the training inputs, the first three on training points."""
import functools

import numpy as np
import scipy.linalg as sla

from tests import batch_cases as bc
from tests.predict_grad_ref import HostPosterior, dk_dx, kmat
from tests.test_gpu_batch_predict import oracle_predict, with_points

SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 545, 768]
NS = [0, 1, 31, 32, 33, 127, 128, 129, 200]
G_RTOL, G_ATOL = 1e-7, 1e-8  # the project's input-gradient tolerance for fp64: rtol, atol · max(1, max|g_ref|)


def mean_vector(case, X):
    """m(X) of a bc.make_case problem on the host"""
    if case["mean"] == "zero":
        return np.zeros(len(X))
    if case["mean"] == "const":
        return np.full(len(X), 0.4)
    return np.asarray([bc.custom_mean(r) for r in X], dtype=np.float64)


def mean_grad_of(case):
    """the derivative of the case's mean function at its test points, (ns × d): what mean_grads takes for a CustomMean (None otherwise)"""
    if case["mean"] != "custom":
        return None
    return lambda xs: np.full((case["ns"], case["d"]), 0.3)


def host(case, kernel=None):
    """HostPosterior of a case (α from y − m(X)); kernel: the oracle kernel of a single-kind case (default) or a composite kernel"""
    X = np.asarray(case["X"], dtype=np.float64)
    return HostPosterior(kernel if kernel is not None else single_kernel(case), X, np.asarray(case["y"], dtype=np.float64) - mean_vector(case, X),
                         np.asarray(case["s2"], dtype=np.float64))


def single_kernel(case):
    scale = {"none": None, "scale": 0.7, "ard": np.linspace(0.5, 0.9, case["d"])}[case["tr"]]
    return bc.o.Kernel(case["kind"], 1.3, scale)


def xs_rows(case):
    return np.asarray(case["oxs"], dtype=np.float64).reshape(case["ns"], case["d"])


def host_grads(case, kernel=None):
    """(∂mean/∂x*, ∂var/∂x*) of a case on the host, (ns, d) each; the prior mean counts as constant"""
    return host(case, kernel).grads(xs_rows(case))


def grads_through_S(hp, Xs):
    """The same gradients in the device's form: S = L⁻ᵀ explicitly, V = K* S, W = V Sᵀ."""
    n = hp.L.shape[0]
    S = sla.solve_triangular(hp.L, np.eye(n), lower=True).T
    Ks = kmat(hp.k, Xs, hp.X)
    W = (Ks @ S) @ S.T
    dk = dk_dx(hp.k, Xs, hp.X)
    return np.einsum("i,jip->jp", hp.alpha, dk), -2.0 * np.einsum("ji,jip->jp", W, dk)


def g_bound(g_ref):
    """elementwise bound of the gradient tolerance"""
    return G_ATOL * max(1.0, float(np.abs(g_ref).max()) if g_ref.size else 0.0) + G_RTOL * np.abs(g_ref)


@functools.lru_cache(maxsize=None)
def ragged_cases():
    """Every size twice, the numbers of test points cycling against them, the categories cycling as in bc.ragged_cases, plus one D = 16 problem."""
    cases = []
    for b, n in enumerate(SIZES + SIZES):
        cont = bc.CONTAINERS[b % 3]
        d = 1 if cont == "vector" else [1, 3, 8][(b // 3) % 3]
        c = bc.make_case(n, b % 4, bc.TRANSFORMS[(b // 4) % 3], d, cont, bc.NOISES[(b // 2) % 2], bc.MEANS[(b // 5) % 3], seed=5000 + b)
        cases.append(with_points(c, NS[b % len(NS)], seed=6000 + b))
    cases.append(with_points(bc.make_case(300, 3, "ard", 16, "colvecs", "vector", "const", seed=5100), 70, seed=6100))
    return tuple(cases)


def limit_cases():
    """the kernels' own limit: n = 1 100 (ARD, vector noise) and n = 2 048, 65 test points each"""
    return [with_points(bc.make_case(1100, 2, "ard", 3, "rowvecs", "vector", "custom", seed=97), 65, seed=197),
            with_points(bc.make_case(2048, 3, "scale", 3, "colvecs", "scalar", "const", seed=99), 65, seed=199)]


@functools.lru_cache(maxsize=None)
def ragged_refs():
    """(oracle logpdf / mean / var, host gradients) of the ragged cases, computed once"""
    return tuple((oracle_predict(c), host_grads(c) if c["ns"] else (np.zeros((0, c["d"])), np.zeros((0, c["d"])))) for c in ragged_cases())
