"""Shared by tests/test_batch_gradx_cpu.py and tests/test_gpu_batch_gradx.py: the references the batched input gradient (gp_logpdf_grad_batch_x /
gp_logpdf_grad_batch_sum_x, agp.logpdf_and_grad_batch(..., wrt_x=True)) is compared with, and the project's input-gradient tolerance in one place
(tests/test_gpu_api.py::test_logpdf_grad_wrt_inputs, tests/test_gpu_composite_dx.py::_assert_gx):
    fp64: |err| <= 1e-7·|ref| + 1e-8·max(1, max|g_ref|)        fp32: 2e-2 for both.
The other outputs keep the tolerances of tests/batch_grad_cases.py."""
import functools

import numpy as np
import scipy.linalg as sla

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_cases as bc
from tests import batch_grad_cases as gc

BOUNDARY_SIZES = [1, 2, 63, 64, 65, 128, 129, 130, 193]
DIMS = [1, 3, 8, 16]


def tolerances(dtype):
    return (2e-2, 2e-2) if np.dtype(dtype) == np.float32 else (1e-7, 1e-8)


def rows_of(gx, case):
    """a problem's "x" entry as the oracle has it: (n,) for a vector input, else (n, d) — the mirror returns (d, n) for ColVecs"""
    gx = np.asarray(gx)
    return gx.T if case["container"] == "colvecs" else gx


def x_shape(case):
    """the shape of the input container's array, which "x" must have"""
    n, d = case["n"], case["d"]
    return {"vector": (n,), "colvecs": (d, n), "rowvecs": (n, d)}[case["container"]]


def dx_excess(g, g_ref, dtype=np.float64):
    """worst |g − g_ref| / (rtol·|g_ref| + atol·max(1, max|g_ref|)) over the entries: within tolerance when <= 1"""
    rtol, atol = tolerances(dtype)
    g, g_ref = np.asarray(g, dtype=np.float64), np.asarray(g_ref, dtype=np.float64)
    assert g.shape == g_ref.shape, (g.shape, g_ref.shape)
    if g.size == 0:
        return 0.0
    if not np.all(np.isfinite(g)):
        return float("inf")
    return float(np.max(np.abs(g - g_ref) / (rtol * np.abs(g_ref) + atol * max(1.0, float(np.abs(g_ref).max())))))


def report_x(tag, case, gx, ref_x):
    """prints the figure, then returns whether "x" has the container's shape and dtype and lies within the tolerance of the reference (n, d) / (n,)"""
    gx = np.asarray(gx)
    ex = dx_excess(rows_of(gx, case), ref_x, gx.dtype)
    print(f"{tag} n={case['n']} kind={case.get('kind')} {case.get('tr')} D={case['d']} {case['container']} {case.get('noise')} {case.get('mean')}: "
          f"dx {ex:.2e} of the tolerance, max|g_ref| = {float(np.abs(ref_x).max()) if np.size(ref_x) else 0.0:.2e}")
    return gx.shape == x_shape(case) and ex <= 1.0


def boundary_cases():
    """The boundary sizes of the 64×64 tiles and of the 128-row S tiles, each with D = 1, 3, 8, 16 in turn; kinds, transforms, noise forms, means and
    containers cycle with co-prime periods the way batch_cases.ragged_cases does it (a vector container is D = 1 by construction)."""
    cases = []
    for b, n in enumerate(BOUNDARY_SIZES * 2):
        d = DIMS[(b + b // len(BOUNDARY_SIZES)) % 4]
        cont = "vector" if d == 1 and b % 2 == 0 else bc.CONTAINERS[1 + b % 2]
        cases.append(bc.make_case(n, b % 4, bc.TRANSFORMS[(b // 4) % 3], d, cont, bc.NOISES[(b // 2) % 2], bc.MEANS[(b // 5) % 3], seed=4000 + b))
    return cases


@functools.lru_cache(maxsize=None)
def boundary_with_oracle():
    cases = boundary_cases()
    return cases, [gc.oracle_grad(c) for c in cases]


def scipy_grad_x(case):
    """∂logpdf/∂x from SciPy's Cholesky, independent of the oracle's explicit inverse: L⁻¹ by a triangular solve on the identity, C⁻¹ = L⁻ᵀ L⁻¹ (what the
    device forms, as batch_grad_cases.scipy_grad does for θ), W = α αᵀ − C⁻¹ with a zero diagonal, and per dimension
    Σ_j W_ij · 2 σ² s_p κ'(r²_ij) (u_ip − u_jp), u = s ∘ x."""
    ofx, y = case["ofx"], np.asarray(case["y"], dtype=np.float64)
    k = ofx.f.kernel
    X = o.as_points(ofx.x).astype(np.float64)
    n, d = X.shape
    m, Cm = o.mean_and_cov(ofx)
    L = sla.cholesky(Cm, lower=True)
    Li = sla.solve_triangular(L, np.eye(n), lower=True)
    alpha = sla.cho_solve((L, True), y - m)
    W = np.outer(alpha, alpha) - Li.T @ Li
    np.fill_diagonal(W, 0.0)
    s = k.scale_vec(d)
    U = X * s
    r2 = np.zeros((n, n))
    for p in range(d):
        r2 += (U[:, None, p] - U[None, :, p]) ** 2
    G = W * (2.0 * k.variance * gc._dkappa(k.kind, r2))
    gx = np.stack([s[p] * np.sum(G * (U[:, None, p] - U[None, :, p]), axis=1) for p in range(d)], axis=1)
    return gx[:, 0] if np.asarray(ofx.x).ndim == 1 else gx


def duplicate_case(kind, seed, n=150):
    """inputs with coincident distinct points — inside one tile, across tiles, and a triple — and noise of 0.2 of the prior variance: K + Σy stays positive
    definite though K itself is singular"""
    c = bc.make_case(n, kind, "ard", 3, "rowvecs", "scalar", "const", seed=seed)
    X = c["X"].copy()
    X[11] = X[10]
    X[140] = X[40]
    X[70] = X[71] = X[5]
    s2 = 0.26
    k = 1.3 * [agp.SqExponentialKernel, agp.Matern12Kernel][kind]() @ agp.ARDTransform(np.linspace(0.5, 0.9, 3))
    ofx = o.FiniteGP(o.GP(o.Kernel(kind, 1.3, np.linspace(0.5, 0.9, 3)), 0.4), X, s2)
    return dict(c, fx=agp.GP(0.4, k)(agp.RowVecs(X), s2), ofx=ofx, X=X, s2=s2)
