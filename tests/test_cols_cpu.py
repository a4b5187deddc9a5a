"""CPU: the context-free half of the column calls (posterior_columns / logpdf_and_grad_columns: marshalling of Y, the shared mean, dtype promotion, the
refusals), the declared / exported / bound symbols and their guard, GPMI355_COLS_MAX, the split rule's documented threshold — and, in NumPy, the identity the
device's gradient relies on: the gradient of Σ_s logpdf(fx, Y[:, s]) is the contraction of ∂C/∂θ with ½(A Aᵀ − S·C⁻¹)."""
import re
from pathlib import Path

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import cols_cases as cc
from tests import test_abi_guard_static as gs
from tests import test_shim_static as ss

ROOT = Path(__file__).resolve().parent.parent
NEW = ("gp_posterior_fit_cols", "gp_posterior_fit_cols_sum", "gp_posterior_ncols", "gp_posterior_predict_cols", "gp_logpdf_grad_cols", "gp_logpdf_grad_cols_sum")


def _fx(n=10, dtype=np.float64, mean=None, kernel=None):
    x = np.linspace(0.0, 1.0, n).astype(dtype)
    k = kernel or 1.3 * agp.SqExponentialKernel()
    return (agp.GP(k) if mean is None else agp.GP(mean, k))(x, 0.1)


def test_the_symbols_are_declared_exported_bound_and_the_abi_version_stays(agp):
    lib = agp._lib.load()
    assert all(hasattr(lib, s) for s in NEW) and set(NEW) <= set(agp._lib.header_functions()) and set(NEW) <= set(agp._lib.PROTOTYPES)
    assert lib.gp_abi_version() == 4
    protos = ss.header_prototypes()
    fit, fit1 = protos["gp_posterior_fit_cols"], protos["gp_posterior_fit"]
    assert fit[1] == fit1[1][:6] + ["i64", "i32"] + fit1[1][6:] and protos["gp_posterior_fit_cols_sum"] == fit
    assert protos["gp_posterior_predict_cols"] == protos["gp_posterior_predict"]
    g, g1 = protos["gp_logpdf_grad_cols"], protos["gp_logpdf_grad"]
    assert g[1] == g1[1][:6] + ["i64", "i32"] + g1[1][6:]
    gsx = protos["gp_logpdf_grad_sum_x"]
    assert protos["gp_logpdf_grad_cols_sum"][1] == gsx[1][:6] + ["i64", "i32"] + gsx[1][6:]
    for name in ("posterior_columns", "logpdf_and_grad_columns", "ColumnsPosteriorGP"):
        assert getattr(agp, name) is getattr(agp.api, name)


def test_the_cap_is_one_block_of_right_hand_side_rows_and_the_mirror_reads_it(agp):
    txt = (ROOT / "include" / "gpmi355.h").read_text()
    (v,) = re.findall(r"^#define GPMI355_COLS_MAX (\d+)$", txt, flags=re.M)
    assert int(v) == 128 == agp._lib.cols_max()
    src = (gs.CSRC / "gpmi355.hip").read_text()
    assert "GPMI355_COLS_MAX" in src
    for name in ("cols_kernel_calls", "cols_kernel_splits"):  # read-only: documented, served, and not among the settable defaults
        assert f'"{name}"' in txt and f'"{name}"' in src
        assert name not in re.search(r"#define GPMI355_PARAM_DEFAULTS(.*?)\nint32_t gp_ctx_set_param", txt, flags=re.S).group(1)


def test_every_new_entry_point_starts_with_the_guard():
    src = gs.strip_comments((gs.CSRC / "gpmi355.hip").read_text())
    defs = gs.definitions(src)
    want = gs.header_handle_functions(gs.HEADER.read_text())
    for name in NEW:
        assert want[name] == ("gp_post" if name in ("gp_posterior_ncols", "gp_posterior_predict_cols") else "gp_ctx")
        assert gs.guard_problem(name, want[name], defs) is None, name


def test_the_new_kernels_use_no_atomics():
    src = gs.strip_comments((gs.CSRC / "kernels.hpp").read_text())
    a, b = src.index("constexpr int KMUL_TM"), src.index("void cols_weight_kernel")
    end = src.index("\n}\n", b)
    assert "atomic" not in src[a:end]
    for k in ("kmul_kernel", "kmul_sum_kernel", "kmul_reduce_kernel", "cols_weight_kernel"):
        assert k in src[a:end]


def test_marshalling_of_Y_the_shared_mean_and_dtype_promotion():
    rng = np.random.default_rng(0)
    fx = _fx(10, mean=0.4)
    Yc = rng.standard_normal((10, 3))                      # C order: copied once into column-major
    a = agp.api._cols_marshal(fx, Yc, "t")
    assert a.Y.flags.f_contiguous and a.ldy == 10 and a.ncols == 3 and np.array_equal(a.Y, Yc) and a.dt is np.float64
    assert a.mean.shape == (10,) and np.all(a.mean == 0.4) and a.sfx == "" and a.nf is None  # ONE mean vector for all columns
    Yf = np.asfortranarray(Yc)                             # column-major: goes as it lies
    a = agp.api._cols_marshal(fx, Yf, "t")
    assert a.Y is Yf and a.ldy == 10
    tall = np.asfortranarray(rng.standard_normal((14, 3)))  # the leading rows of a taller column-major array: zero-copy, ldy = its column stride
    a = agp.api._cols_marshal(fx, tall[:10], "t")
    assert a.ldy == 14 and a.Y.ctypes.data == tall.ctypes.data and a.ncols == 3
    a = agp.api._cols_marshal(fx, Yc[:, :1], "t")          # one column is a matrix too
    assert a.ncols == 1 and a.ldy == 10
    a = agp.api._cols_marshal(fx, Yc.astype(np.float32), "t")  # fp64 inputs promote fp32 observations
    assert a.dt is np.float64 and a.Y.dtype == np.float64
    a = agp.api._cols_marshal(_fx(10, np.float32), Yc.astype(np.float32), "t")
    assert a.dt is np.float32 and a.Y.dtype == np.float32 and a.kk.dtype == 1
    a = agp.api._cols_marshal(_fx(10, np.float32), Yc, "t")    # fp32 inputs with fp64 observations: fp64
    assert a.dt is np.float64
    a = agp.api._cols_marshal(_fx(10, kernel=agp.SqExponentialKernel() + 0.1 * agp.WhiteKernel()), Yc, "t")
    assert a.sfx == "_sum" and a.nf is not None


def test_refusals_of_the_mirror():
    fx = _fx(10)
    Y = np.zeros((10, 3))
    for fn in (agp.posterior_columns, agp.logpdf_and_grad_columns):
        with pytest.raises(TypeError):
            fn(fx, Y[:, 0])                                  # a vector goes to posterior / logpdf_and_grad
        with pytest.raises(ValueError):
            fn(fx, np.zeros((9, 3)))                         # DimensionMismatch
        with pytest.raises(ValueError):
            fn(fx, np.zeros((10, 129)))                      # more than GPMI355_COLS_MAX columns
        with pytest.raises(ValueError):
            fn(fx, np.zeros((10, 0)))
        post = object.__new__(agp.PosteriorGP)               # a PosteriorGP prior: sequential conditioning of columns is not offered
        with pytest.raises(TypeError):
            fn(agp.FiniteGP(post, fx.x, 0.1), Y)


def test_the_split_rule_documented_in_the_header_is_the_one_in_the_source():
    src = (gs.CSRC / "gpmi355.hip").read_text()
    body = src[src.index("static inline void kmul_split("):]
    body = body[:body.index("\n}\n")]
    assert "(512 + tiles - 1) / tiles" in body and "nstrips / 4" in body
    ksrc = (gs.CSRC / "kernels.hpp").read_text()
    assert "KMUL_TM = 64, KMUL_KS = 32" in ksrc

    def nsplit(n, ns):  # the rule, in Python
        tiles, nstrips = -(-ns // 64), -(-n // 32)
        s = min(-(-512 // tiles), max(1, nstrips // 4))
        sps = -(-nstrips // s)
        return -(-nstrips // sps)

    assert nsplit(224, 1) == 1 and nsplit(225, 1) == 2 and nsplit(300, 63) == 2 and nsplit(129, 1) == 1 and nsplit(300, 64 * 512) == 1
    assert "the smallest n that splits is 225" in (ROOT / "include" / "gpmi355.h").read_text()


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("tr", ["none", "scale", "ard"])
def test_gradient_of_the_summed_logpdf_is_one_contraction_with_the_summed_weights(kind, tr):
    """Σ_s ∇logpdf(fx, Y[:, s]) (the oracle, column by column) = ⟨∂C/∂θ, ½(A Aᵀ − S·C⁻¹)⟩ with A = C⁻¹(Y − m): what cols_weight_kernel hands the gradient
    kernels.  ∂C/∂θ by the oracle's own closed forms."""
    n, S, d = 40, 5, 3
    rng = np.random.default_rng(10 * kind + len(tr))
    X = rng.uniform(0, 4, size=(n, d)) / np.sqrt(d)
    Y = rng.standard_normal((n, S))
    scale = {"none": None, "scale": 0.7, "ard": np.linspace(0.5, 0.9, d)}[tr]
    k = o.Kernel(kind, 1.3, scale)
    s2 = 1.3 * rng.uniform(1e-2, 5e-2, size=n)
    fx = o.FiniteGP(o.GP(k, 0.4), X, s2)
    gs_ = [o.logpdf_grad(fx, Y[:, s]) for s in range(S)]
    m, Cm = o.mean_and_cov(fx)
    Ci = np.linalg.inv(Cm)
    A = Ci @ (Y - m[:, None])
    W = 0.5 * (A @ A.T - S * Ci)
    sv = k.scale_vec(d)
    Xs = X * sv
    diff2 = (Xs[:, None, :] - Xs[None, :, :]) ** 2
    r2 = diff2.sum(-1)
    dk = o._dkappa_dr2(kind, r2)

    def close(got, want):
        want = np.asarray(want, dtype=np.float64)
        assert np.linalg.norm(np.asarray(got) - want) <= 1e-10 * max(np.linalg.norm(want), 1e-300)

    close(np.sum(W * o._kappa(kind, r2)), sum(g["variance"] for g in gs_))
    close(np.diag(W), sum(g["noise"] for g in gs_))
    close(-A, np.stack([g["y"] for g in gs_], axis=1))
    if tr == "scale":
        close(np.sum(W * 1.3 * dk * 2.0 * r2 / 0.7), sum(g["scale"] for g in gs_))
    elif tr == "ard":
        close([np.sum(W * 1.3 * dk * 2.0 * diff2[:, :, p] / sv[p]) for p in range(d)], sum(g["scale"] for g in gs_))
    G = W * (1.3 * dk)
    np.fill_diagonal(G, 0.0)
    close(4.0 * sv[None, :] * (G.sum(axis=1)[:, None] * Xs - G @ Xs), sum(g["x"] for g in gs_))


def test_the_shared_reference_agrees_with_the_oracle_where_both_exist():
    """tests/cols_cases.py: the NumPy / SciPy branch (composite kernels, dense Σy) against the oracle branch on a case both can form"""
    c = cc.single_case("n63")
    ref = cc.reference(c)
    assert ref["alpha"].shape == (63, 2) and ref["mean"].shape == (63, 2) and ref["lp"].shape == (2,)
    lp = o.logpdf(c["ofx"], c["Y"])                       # the oracle's own matrix form
    np.testing.assert_allclose(ref["lp"], lp, rtol=1e-12)
    d = cc.single_case("n65_dense")
    rd = cc.reference(d)
    assert rd["grad"]["noise"].shape == (65, 65) and rd["alpha"].shape == (65, 15) and np.all(np.isfinite(rd["grad"]["x"]))
