"""CPU: the fp64 reference of leave-one-out cross-validation (tests/loo_ref.py) — the closed form against brute-force refits, its gradient against
central differences of the brute-force objective, the NumPy emulation of the device's formulation of G against G, the conditioning of every case of
tests/loo_cases.py, the four entry points (declared, bound, exported) and the mirror's refusals.

Central differences: bound and error model are those at the top of tests/test_predict_grad_cpu.py (from tests/test_composite_dx_cpu.py): h = 1e-5,
truncation h²/6·|L'''| ≈ 2e-11·|L'''|, rounding ε·|L|/h ≈ 1e-16·1e2/1e-5 = 1e-9 for |L| of order 1e2; the groups' largest entries are of order 1e1 … 1e3,
so 1e-7·max|g| leaves orders over both."""
import numpy as np
import pytest

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import composite_dx_ref as cdx
from tests import composite_ref as cr
from tests import loo_cases as lc
from tests import loo_ref as lr


def _problem(n, d, noise, with_mean, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 4.0, size=(n, d)) / np.sqrt(d)
    ok = o.Kernel(o.SE if d == 1 else o.MATERN52, 1.3, None if d == 1 else np.linspace(0.5, 0.9, d))
    K = o.kernelmatrix(ok, X)
    S = cdx.noise_matrix(np.asarray(lc.noise_for(rng, K, noise)), n)
    m = 0.3 * X.sum(1) + 0.1 if with_mean else np.zeros(n)
    y = np.sin(2.0 * X.sum(1)) + 0.3 * rng.standard_normal(n)
    return ok, X, K + S, m, y


@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("noise", ["scalar", "vector", "dense_c"])
@pytest.mark.parametrize("n,d", [(1, 1), (2, 3), (40, 1), (130, 3)])
def test_closed_form_against_brute_force_refits(n, d, noise, with_mean):
    _, _, C, m, y = _problem(n, d, noise, with_mean, seed=100 * n + d)
    assert np.linalg.cond(C) <= 1e3
    ref = lr.closed_form(C, y - m, y)
    mu, v, lp = lr.brute_force(C, m, y)
    e_mu, e_v = float(np.max(np.abs(ref["mean"] - mu))), float(np.max(np.abs(ref["var"] - v) / v))
    e_L = abs(ref["L"] - lp.sum()) / abs(lp.sum())
    print(f"n={n} d={d} {noise} mean={with_mean}: mean abs {e_mu:.1e}, var rel {e_v:.1e}, lp abs {np.max(np.abs(ref['lp'] - lp)):.1e}, L rel {e_L:.1e}")
    assert e_mu <= 1e-11 and e_v <= 1e-11 and e_L <= 1e-11 and np.max(np.abs(ref["lp"] - lp)) <= 1e-11
    if n == 1:  # the prior prediction
        assert mu[0] == m[0] and abs(ref["mean"][0] - m[0]) <= 1e-15 and abs(ref["var"][0] - C[0, 0]) <= 1e-15 * C[0, 0]


def _fd(f, h=1e-5):
    return (f(h) - f(-h)) / (2.0 * h)


def _check(what, g, fd):
    g, fd = np.atleast_1d(np.asarray(g, dtype=np.float64)), np.atleast_1d(np.asarray(fd, dtype=np.float64))
    worst = float(np.max(np.abs(g - fd)))
    print(f"{what}: max |fd - g| / max|g| = {worst / np.abs(g).max():.2e}  (max|g| = {np.abs(g).max():.3g})")
    assert worst <= 1e-7 * np.abs(g).max()


def test_single_kind_gradient_against_central_differences_of_the_brute_force_objective():
    """Matern52 ∘ ARD, n = 40, D = 3, diagonal Σy, a mean: every parameter group gp_loo_grad differentiates against"""
    n, d = 40, 3
    ok, X, C, m, y = _problem(n, d, "vector", True, seed=7)
    s2 = np.diag(C - o.kernelmatrix(ok, X)).copy()

    def L(ok_=ok, X_=X, s2_=s2, m_=m, y_=y):
        return float(lr.brute_force(o.kernelmatrix(ok_, X_) + np.diag(s2_), m_, y_)[2].sum())

    G, beta = lr.weight_matrix(C, y - m)
    g = lr.single_kind_grads(ok, X, G, 1)
    _check("variance", g["variance"], _fd(lambda h: L(ok_=o.Kernel(ok.kind, ok.variance + h, ok.scale))))
    e = np.eye(d)
    _check("scale", g["scale"], [_fd(lambda h: L(ok_=o.Kernel(ok.kind, ok.variance, ok.scale + h * e[p]))) for p in range(d)])
    idx = list(range(0, n, 7))
    en = np.eye(n)
    _check("noise", g["noise"][idx], [_fd(lambda h: L(s2_=s2 + h * en[i])) for i in idx])
    _check("y", -beta[idx], [_fd(lambda h: L(y_=y + h * en[i])) for i in idx])
    _check("mean", beta[idx], [_fd(lambda h: L(m_=m + h * en[i])) for i in idx])

    def moved(i, p, h):
        Xh = X.copy()
        Xh[i, p] += h
        return Xh

    _check("x", g["x"][idx], [[_fd(lambda h: L(X_=moved(i, p, h))) for p in range(d)] for i in idx])


def test_composite_gradient_and_dense_noise_against_central_differences():
    """six-term kernel, n = 60, D = 3, dense Σy: ∂/∂θ, ∂/∂x and ⟨G, dΣy⟩ along a symmetric direction"""
    n = 60
    X, y = cdx.six_term_data(n, seed=9)
    k = cdx.six_term_kernel()
    rng = np.random.default_rng(11)
    K = cr.ref_kernelmatrix(k, X)
    S = np.asarray(lc.noise_for(rng, K, "dense_c"))
    m = np.zeros(n)
    assert np.linalg.cond(K + S) <= 1e3
    G, _ = lr.weight_matrix(K + S, y - m)
    g = lr.composite_grads(k, X, G, 2)
    th = agp.api._NormalForm(k).theta()
    nf = agp.api._NormalForm(k)

    def L(K_=K, S_=S):
        return float(lr.brute_force(K_ + S_, m, y)[2].sum())

    e = np.eye(len(th))
    _check("theta", g["theta"], [_fd(lambda h: L(K_=cr.ref_from_theta(nf, np.asarray(th) + h * e[j], X))) for j in range(len(th))])
    D = rng.standard_normal((n, n))
    D = D + D.T
    _check("dense noise", np.sum(g["noise"] * D), _fd(lambda h: L(S_=S + h * 1e-2 * D)) / 1e-2)

    def moved(i, p, h):
        Xh = X.copy()
        Xh[i, p] += h
        return Xh

    idx = list(range(0, n, 11))
    _check("x", g["x"][idx], [[_fd(lambda h: L(K_=cr.ref_kernelmatrix(k, moved(i, p, h)))) for p in range(3)] for i in idx])


@pytest.mark.parametrize("n,d,noise", [(1, 1, "scalar"), (127, 3, "vector"), (129, 3, "dense_c"), (300, 1, "scalar")])
def test_device_formulation_in_numpy_equals_G(n, d, noise):
    """mirror from the lower triangle with padding to 128, Z Zᵀ, rank-2 fold: the weights the device hands to the gradient kernels"""
    _, _, C, m, y = _problem(n, d, noise, True, seed=300 + n)
    G, _ = lr.weight_matrix(C, y - m)
    Gd = lr.device_emulation(C, y - m)
    err = float(np.max(np.abs(Gd - G)) / np.max(np.abs(G)))
    print(f"n={n}: max |G_device - G| / max|G| = {err:.1e}")
    assert err <= 1e-12


@pytest.mark.parametrize("cid", [c[0] for c in lc.SINGLE] + [lc.F32[0]] + [c[0] for c in lc.COMPOSITE])
def test_every_case_is_well_conditioned(cid):
    """the GPU tolerances are forward comparisons: they mean nothing beyond cond(C) ≈ 1e3"""
    c = lc.composite_case(cid) if cid in [k[0] for k in lc.COMPOSITE] else lc.single_case(cid)
    C, _ = lc.covariance(c)
    cond = float(np.linalg.cond(C))
    print(f"{cid}: cond(C) = {cond:.3g}")
    assert cond <= 1e3
    nz = agp.api._Marshal(np.float64).noise(c["s2"], c["n"])
    assert nz.kind == {"scalar": 0, "vector": 1, "dense_c": 3, "dense_f": 2}[c["noise"]]


def test_the_reference_of_a_case_matches_its_brute_force():
    c = lc.single_case("n129_dense")
    ref = lc.reference(c)
    C, m = lc.covariance(c)
    mu, v, lp = lr.brute_force(C, m, np.asarray(c["y"], dtype=np.float64))
    assert np.max(np.abs(ref["mean"] - mu)) <= 1e-11 and np.max(np.abs(ref["var"] - v) / v) <= 1e-11 and abs(ref["L"] - lp.sum()) <= 1e-11 * abs(lp.sum())


def test_the_four_entry_points_are_declared_bound_and_exported(agp):
    lib = agp._lib.load()
    declared = agp._lib.header_functions()
    for name in ("gp_loo", "gp_loo_sum", "gp_loo_grad", "gp_loo_grad_sum"):
        assert name in declared, name
        assert name in agp._lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    P = agp._lib.PROTOTYPES
    assert [type(a) for a in P["gp_loo_grad"][1]] == [type(a) for a in P["gp_logpdf_grad"][1]] and len(P["gp_loo_grad"][1]) == len(P["gp_logpdf_grad"][1])
    assert len(P["gp_loo_grad_sum"][1]) == len(P["gp_logpdf_grad_sum_x"][1])
    assert P["gp_loo_sum"][1][2:] == P["gp_loo"][1][2:] and len(P["gp_loo"][1]) == 10
    assert lib.gp_abi_version() == 4
    for name in ("loo_mean_and_var", "loo_logpdf", "loo_logpdf_and_grad"):
        assert callable(getattr(agp, name)), name
    shim = (agp._lib.HEADER.parent.parent / "abstractgps.jl_amd" / "julia" / "HipGPs.jl").read_text()
    for name in ("gp_loo", "gp_loo_sum", "gp_loo_grad", "gp_loo_grad_sum"):
        assert f"(:{name}, libgpmi355)" in shim, name


def test_refusals_of_the_mirror():
    """a matrix of observations and a PosteriorGP prior raise TypeError before anything reaches the device"""
    f = agp.GP(agp.SqExponentialKernel())
    x = np.linspace(0.0, 1.0, 5)
    fx = f(x, 0.1)
    for fn in (agp.loo_mean_and_var, agp.loo_logpdf, agp.loo_logpdf_and_grad):
        with pytest.raises(TypeError):
            fn(fx, np.zeros((5, 2)))
        with pytest.raises(ValueError):
            fn(fx, np.zeros(4))
    post = agp.PosteriorGP.__new__(agp.PosteriorGP)  # (no device: the type alone decides)
    pfx = agp.FiniteGP.__new__(agp.FiniteGP)
    pfx.f, pfx.x, pfx.sigma2 = post, x, 0.1
    for fn in (agp.loo_mean_and_var, agp.loo_logpdf, agp.loo_logpdf_and_grad):
        with pytest.raises(TypeError):
            fn(pfx, np.zeros(5))
