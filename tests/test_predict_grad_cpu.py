"""CPU: the fp64 references of the predictive-mean / predictive-variance input gradients (tests/predict_grad_ref.py) against central differences of the
host posteriors, the composite form against the single-kind analytic form, and the two entry points that carry the gradients through the C ABI
(gp_posterior_predict_grad, gp_vfe_predict_grad): declared, bound, exported.

Bound and error model of the central-difference checks are those of tests/test_composite_dx_cpu.py: h = 1e-5, truncation h²/6·|f'''| ≈ 2e-11·|f'''|,
rounding ε·|f|/h ≈ 1e-16·1/1e-5 = 1e-11 for values of order 1; 1e-7·max|g| leaves orders over both (measured: 2.1e-9 at worst)."""
import numpy as np
import pytest

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests.composite_dx_ref import many_dim_kernel, six_term_data, six_term_kernel
from tests.predict_grad_ref import HostPosterior, central_differences, composite_dk_dx, single_dk_dx, sparse_grads


def _check_fd(what, g, fd):
    for name, a, b in (("mean", g[0], fd[0]), ("var", g[1], fd[1])):
        worst = float(np.abs(a - b).max())
        print(f"{what} d{name}: max |fd - g| / max|g| = {worst / np.abs(a).max():.2e}")
        assert worst <= 1e-7 * np.abs(a).max()


def test_exact_reference_against_central_differences_six_term_kernel():
    X, y = six_term_data(150, seed=3)
    Xs = np.random.default_rng(4).uniform(0, 3, size=(40, 3))
    post = HostPosterior(six_term_kernel(), X, y, 0.05)
    _check_fd("six-term", post.grads(Xs), central_differences(post.mean_and_var, Xs))


def test_exact_reference_against_central_differences_sixteen_dimensions():
    rng = np.random.default_rng(216)
    X = rng.uniform(0, 2, size=(150, 16))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(150)
    Xs = rng.uniform(0, 2, size=(40, 16))
    post = HostPosterior(many_dim_kernel(16), X, y, 0.05)
    _check_fd("many-dim D=16", post.grads(Xs), central_differences(post.mean_and_var, Xs))


@pytest.mark.parametrize("okind", [o.SE, o.MATERN32, o.MATERN52])
def test_sparse_reference_against_central_differences_of_the_oracle(okind):
    """VFE, N = 400, M = 37, jitter 1e-6, behind an ARD transform: differences of oracle.gp_oracle.ApproxPosteriorGP.mean_and_var."""
    rng = np.random.default_rng(30 + okind)
    X = rng.uniform(-2, 2, size=(400, 3))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(400)
    z = rng.uniform(-2, 2, size=(37, 3))
    Xs = rng.uniform(-2, 2, size=(40, 3))
    f = o.GP(o.Kernel(okind, 1.3, np.array([0.5, 1.1, 0.9])))
    post = o.vfe_posterior(f, z, 1e-6, o.FiniteGP(f, X, 0.05), y)
    _check_fd(f"vfe kind {okind}", sparse_grads(post, Xs), central_differences(post.mean_and_var, Xs))


@pytest.mark.parametrize("kind,okind", [(0, o.SE), (1, o.MATERN12), (2, o.MATERN32), (3, o.MATERN52)])
def test_one_term_composites_against_the_single_kind_form(kind, okind):
    rng = np.random.default_rng(20 + kind)
    X = rng.standard_normal((120, 3))
    Xs = np.concatenate([rng.standard_normal((30, 3)), X[:3]])  # three test points ON training points (Matern12 convention)
    v = np.array([0.5, 1.1, 0.9])
    g = composite_dk_dx(agp.KernelSum((1.4 * agp.Kernel(kind) @ agp.ARDTransform(v),)), Xs, X)
    gs = single_dk_dx(o.Kernel(okind, 1.4, v), Xs, X)
    err = np.max(np.abs(g - gs) / np.maximum(1.0, np.abs(gs)))
    print(f"kind {kind}: max |composite - single| / max(1, |single|) = {err:.2e}")
    assert err <= 1e-11


def test_the_new_entry_points_are_declared_bound_and_exported(agp):
    lib = agp._lib.load()
    declared = agp._lib.header_functions()
    for name, sibling in (("gp_posterior_predict_grad", "gp_posterior_predict"), ("gp_vfe_predict_grad", "gp_vfe_predict")):
        assert name in declared, name
        assert name in agp._lib.PROTOTYPES, name
        assert hasattr(lib, name), name
        assert len(agp._lib.PROTOTYPES[name][1]) == len(agp._lib.PROTOTYPES[sibling][1]) + 1
        assert agp._lib.PROTOTYPES[name][1][:4] == agp._lib.PROTOTYPES[sibling][1][:4]
    assert lib.gp_abi_version() == 4
