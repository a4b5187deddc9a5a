"""CPU: the fp64 reference of the composite input gradient (tests/composite_dx_ref.py) against central differences of the host logpdf and against the
oracle's single-kind ∂/∂x, and the two entry points that carry it through the C ABI (gp_logpdf_grad_sum_x, gp_logpdf_terms_sum): declared, bound, exported."""
import numpy as np
import pytest

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests.composite_dx_ref import host_fit, ref_logpdf_grad_x, six_term_data, six_term_kernel


def test_reference_gradient_against_central_differences_of_the_host_logpdf():
    """n = 150, D = 3, σ² = 0.05, h = 1e-5, every 7th point.  The truncation error of the central difference is h²/6·|∂³logpdf/∂x³| ≈ 2e-11·|g'''| and its
    rounding error ε·|logpdf|/h ≈ 1e-16·1e2/1e-5 = 1e-9: the bound of 1e-7·max|g| leaves two orders over both (a prototype of this check measured 1.6e-9)."""
    X, y = six_term_data(150, seed=3)
    k = six_term_kernel()
    g = ref_logpdf_grad_x(k, X, y, 0.05)
    h, worst = 1e-5, 0.0
    for i in range(0, 150, 7):
        for p in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[i, p] += h
            Xm[i, p] -= h
            fd = (host_fit(k, Xp, y, 0.05)[0] - host_fit(k, Xm, y, 0.05)[0]) / (2 * h)
            worst = max(worst, abs(fd - g[i, p]))
    print(f"max |fd - g| / max|g| = {worst / np.abs(g).max():.2e}")
    assert worst <= 1e-7 * np.abs(g).max()


@pytest.mark.parametrize("kind,okind", [(0, o.SE), (1, o.MATERN12), (2, o.MATERN32), (3, o.MATERN52)])
def test_one_term_composites_against_the_oracle(kind, okind):
    rng = np.random.default_rng(20 + kind)
    X = rng.standard_normal((120, 3))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(120)
    v = np.array([0.5, 1.1, 0.9])
    k = agp.KernelSum((1.4 * agp.Kernel(kind) @ agp.ARDTransform(v),))
    go = o.logpdf_grad(o.FiniteGP(o.GP(o.Kernel(okind, 1.4, v)), X, 0.05), y)["x"]
    g = ref_logpdf_grad_x(k, X, y, 0.05)
    err = np.max(np.abs(g - go) / np.maximum(1.0, np.abs(go)))
    print(f"kind {kind}: max |g - oracle| / max(1, |g|) = {err:.2e}")
    assert err <= 1e-11


def test_the_new_entry_points_are_declared_bound_and_exported(agp):
    lib = agp._lib.load()
    declared = agp._lib.header_functions()
    for name in ("gp_logpdf_grad_sum_x", "gp_logpdf_terms_sum"):
        assert name in declared, name
        assert name in agp._lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert len(agp._lib.PROTOTYPES["gp_logpdf_grad_sum_x"][1]) == len(agp._lib.PROTOTYPES["gp_logpdf_grad_sum"][1]) + 1
    assert agp._lib.PROTOTYPES["gp_logpdf_terms_sum"][1][2:] == agp._lib.PROTOTYPES["gp_logpdf_terms"][1][2:]
    assert lib.gp_abi_version() == 4
