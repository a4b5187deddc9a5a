"""No GPU: the host side of the dense observation-noise covariance Σy (include/gpmi355.h gp_noise kinds 2 / 3) — how the Python mirror marshals an (n, n)
array, what FiniteGP.noise_vector() returns for it, and that the header and the Julia shim say what the library does."""
import re
from pathlib import Path

import numpy as np
import pytest

import abstractgps_jl_amd as agp

ROOT = Path(__file__).resolve().parent.parent


def _sym(n, seed=0):
    A = np.random.default_rng(seed).standard_normal((n, n))
    return A @ A.T + n * np.eye(n)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_marshal_layouts_of_a_dense_noise(dtype):
    """The mirror always means the UPPER triangle of the array it is given (Symmetric(Σy)): a C-ordered array is the column-major array of its transpose —
    kind 3 (lower triangle) with the array's own pointer; a Fortran-ordered array is column-major as it lies — kind 2 with its own pointer; anything else is
    copied ONCE into C order (kind 3)."""
    n = 7
    S = _sym(n).astype(dtype)
    m = agp.api._Marshal(dtype)
    Sc = np.ascontiguousarray(S)
    nz = m.noise(Sc, n)
    assert (nz.kind, nz.diag) == (3, Sc.ctypes.data)
    Sf = np.asfortranarray(S)
    assert not Sf.flags.c_contiguous
    nz = m.noise(Sf, n)
    assert (nz.kind, nz.diag) == (2, Sf.ctypes.data)
    # strided view: neither order -> one C-ordered copy, kept alive by the marshaller
    big = np.zeros((2 * n, 2 * n), dtype=dtype)
    big[::2, ::2] = S
    view = big[::2, ::2]
    assert not view.flags.c_contiguous and not view.flags.f_contiguous
    nz = m.noise(view, n)
    assert nz.kind == 3 and nz.diag != view.ctypes.data
    copy = next(a for a in m.keep if isinstance(a, np.ndarray) and a.ctypes.data == nz.diag)
    assert copy.flags.c_contiguous and copy.dtype == dtype and np.array_equal(copy, S)
    # another dtype: converted once
    other = np.float32 if dtype == np.float64 else np.float64
    So = np.ascontiguousarray(S.astype(other))
    nz = m.noise(So, n)
    assert nz.kind == 3 and nz.diag != So.ctypes.data
    copy = next(a for a in m.keep if isinstance(a, np.ndarray) and a.ctypes.data == nz.diag)
    assert copy.dtype == dtype
    # a list of lists is an array like any other
    assert m.noise(S.tolist(), n).kind == 3


def test_scalar_and_vector_noise_are_marshalled_as_before():
    m = agp.api._Marshal(np.float64)
    nz = m.noise(0.25, 5)
    assert (nz.kind, nz.s, nz.diag) == (0, 0.25, None)
    v = np.linspace(0.1, 0.5, 5)
    nz = m.noise(v, 5)
    assert (nz.kind, nz.diag) == (1, v.ctypes.data)


@pytest.mark.parametrize("shape", [(4, 5), (5, 4), (4, 4), (6, 6), (5, 5, 1)])
def test_dimension_mismatch_of_a_dense_noise(shape):
    m = agp.api._Marshal(np.float64)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        m.noise(np.ones(shape), 5)


def test_noise_vector_and_cov_of_a_dense_noise():
    """var / mean_and_var / marginals add diag(Σy) (src/finite_gp_projection.jl:115-116, 156-157); cov adds the matrix, read as Symmetric(Σy)."""
    n = 6
    S = _sym(n, 3)
    f = agp.GP(agp.SqExponentialKernel())
    fx = f(np.linspace(0, 1, n), S)
    nv = fx.noise_vector()
    assert nv.shape == (n,) and np.array_equal(nv, np.diag(S))
    assert np.array_equal(f(np.linspace(0, 1, n), 0.5).noise_vector(), np.full(n, 0.5))
    assert np.array_equal(agp.var(fx), 1.0 + np.diag(S))
    mean, v = agp.mean_and_var(fx)
    assert np.array_equal(v, 1.0 + np.diag(S)) and np.array_equal(mean, np.zeros(n))
    assert np.array_equal(agp.marginals(fx)[1], np.sqrt(1.0 + np.diag(S)))
    Sl = S.copy()
    Sl[np.tril_indices(n, -1)] = np.nan  # only the upper triangle counts
    M = f(np.linspace(0, 1, n), Sl).noise_matrix_or_none()
    assert np.array_equal(M, S)
    assert f(np.linspace(0, 1, n), 0.5).noise_matrix_or_none() is None


def test_vfe_with_a_dense_noise_is_refused_before_the_library_is_called():
    n = 20
    x = np.linspace(0, 1, n)
    f = agp.GP(agp.SqExponentialKernel())
    vfe = agp.VFE(f(x[::4], 1e-6))
    with pytest.raises(NotImplementedError, match="dense Σy"):
        agp.posterior(vfe, f(x, _sym(n)), np.zeros(n))
    with pytest.raises(NotImplementedError, match="dense Σy"):
        agp.elbo(vfe, f(x, _sym(n)), np.zeros(n))
    with pytest.raises(NotImplementedError, match="dense Σy"):
        agp.approx_log_evidence(agp.DTC(f(x[::4], 1e-6)), f(x, _sym(n)), np.zeros(n))


def test_header_documents_the_dense_kinds_and_the_gradient():
    hdr = (ROOT / "include" / "gpmi355.h").read_text()
    assert "#define GPMI355_ABI_VERSION 4" in hdr
    sec = hdr[hdr.index("/* Observation noise"):hdr.index("} gp_noise;")]
    assert "not accelerated" not in sec
    for needle in ("kind 2", "kind 3", "COLUMN-MAJOR", "UPPER triangle", "LOWER triangle", "gp_vfe_fit", "gp_posterior_update", "dense_stage_mb"):
        assert needle in sec, needle
    grad = hdr[hdr.index("Value and gradient of logpdf"):hdr.index("int32_t gp_logpdf_grad(")]
    assert "G = ½(α αᵀ − C⁻¹)" in grad and "⟨G, dΣy⟩" in grad and "SYMMETRIC" in grad and "n×n" in grad
    assert "dense_stage_mb=64" in re.sub(r'"\s*\\\s*\n\s*"', "", hdr)
    # the struct itself is unchanged
    assert re.search(r"typedef struct \{\s*int32_t kind;\s*double s;\s*const void\* diag;\s*\} gp_noise;", hdr)


def test_julia_shim_has_a_noise_method_for_matrices():
    jl = (ROOT / "abstractgps.jl_amd" / "julia" / "HipGPs.jl").read_text()
    assert re.search(r"function noise\(Σ::AbstractMatrix", jl)
    assert re.search(r"function noise\(Σ::Symmetric", jl) and "Σ.uplo == 'U' ? 2 : 3" in jl
    assert "noise_tangent(Σ::Matrix, dn)" in jl
    assert "dense Σy: not accelerated" not in jl
    # the sparse fits keep the stock path for a dense Σy
    body = jl[jl.index("function vfe_call"):jl.index("function AbstractGPs.posterior(approx::Union{VFE,DTC}")]
    assert "is_dense(a.cn) && return nothing" in body
