"""GPU: the FLOAT instantiation of each HIP kernel family against a plain fp64 reference of the same operation, through the fp32 device-level entry points
(gpd_*_f32).  These instantiations — a different BK, four k-values per 16-byte chunk, Tr<float>::crow — run every fp32 fit and the fp32 VFE headline, and the
fits' tolerances (1e-4 … 5e-3 against the fp64 oracle) are set by the conditioning of a GP fit, not by the kernels.  Here the references are formed in fp64 from the
exact fp32 inputs and every bound is a componentwise rounding bound with u = 2⁻²⁴, γ_m = m·u / (1 − m·u) (Higham, Accuracy and Stability of Numerical Algorithms:
Theorem 10.3 for Cholesky, 8.5 for substitution, §3.5 for products), or exact equality where the data make every partial sum an integer.  Each bounded test prints
`RATIO <case> <max error / bound>`; a ratio above 1 is a finding about the kernel, not a tolerance to widen."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import unit_helpers as uh  # noqa: E402
from tests.unit_helpers import P, gamma, ratio_of, report  # noqa: E402

F32 = torch.float32


@pytest.fixture(scope="module")
def lib(agp):
    return agp._lib.load()


@pytest.fixture(scope="module")
def h(ctx):
    return ctx.handle


@pytest.fixture(scope="module")
def pad_h(agp):
    with uh.padded_context(agp) as hh:
        yield hh


@pytest.fixture(params=list(uh.GEMM_CONFIGS))
def gemm_h(request, lib, h, pad_h):
    """the handle to launch on, under one of the GEMM launch variants (unit_helpers.GEMM_CONFIGS)"""
    with uh.gemm_variant(lib, h, pad_h, request.param) as hh:
        yield hh


def test_mfma_f32_lane_maps(lib, h):
    """D = A·B for one 16×16×4 tile through Tr<float> with ASYMMETRIC small-integer operands: exact, and any permutation of lanes or rows shows"""
    rng = np.random.default_rng(0)
    A = rng.integers(-8, 9, (16, 4)).astype(np.float32)
    B = rng.integers(-8, 9, (4, 16)).astype(np.float32)
    D = np.full((16, 16), np.nan, dtype=np.float32)
    assert lib.gp_probe_mfma_f32(h, A.ctypes.data, B.ctypes.data, D.ctypes.data) == 0
    assert np.array_equal(D.astype(np.float64), A.astype(np.float64) @ B.astype(np.float64))
    assert not np.array_equal(A @ B, (A @ B).T)


@pytest.mark.parametrize("m,n", uh.GEMM_RECT)
def test_gemm_nt_exact_rect(lib, gemm_h, m, n):
    uh.gemm_exact(lib, gemm_h, F32, m, n)


@pytest.mark.parametrize("m,n,off,coff", uh.GEMM_LOWER)
def test_gemm_nt_exact_lower(lib, gemm_h, m, n, off, coff):
    uh.gemm_exact(lib, gemm_h, F32, m, n, lower=(off, coff))


@pytest.mark.parametrize("sk", [1, 0])
@pytest.mark.parametrize("m,n,k,lower", [(128, 128, 32, None), (256, 128, 64, None), (192, 64, 128, None), (320, 448, 288, None), (1024, 1024, 1024, None),
                                         (2176, 2304, 64, None), (4224, 1152, 32, None), (1024, 1024, 20000, None), (128, 128, 20000, None),
                                         (320, 192, 64, (64, 64)), (2432, 2176, 64, (384, 128)), (2304, 2304, 4096, (0, 0))])
def test_gemm_nt_rounding(lib, h, m, n, k, lower, sk):
    """standard-normal operands: |Ĉ − C| <= γ_{k + 2·num_cus} (|C₀| + |A||B|ᵀ) componentwise — k products and k adds per element in whatever order, plus one add per
    share when launch_gemm cuts a tile along k (at most 2·num_cus shares).  k = 20 000: the reduction length of the fits' trailing updates."""
    from abstractgps_jl_amd._lib import check, gp_grid

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device="cuda").manual_seed(m + 3 * n + k)
    lda, ldc = k + 32, n + 32
    A = torch.randn(m + 128, lda, dtype=F32, device="cuda", generator=g)
    B = torch.randn(n + 128, lda, dtype=F32, device="cuda", generator=g)
    C0 = torch.randn(m + 128, ldc, dtype=F32, device="cuda", generator=g)
    win = uh.gemm_window(m, n, m + 128, ldc, lower)
    Cm = C0.clone()
    grid = None if lower is None else C.byref(gp_grid(1, 0, 1, 0, 1, 1))
    row0, col0 = (0, 0) if lower is None else lower
    with uh.params(lib, h, gemm_streamk=sk):
        torch.cuda.synchronize()
        check(lib.gpd_gemm_nt_f32(h, P(Cm), ldc, P(A), lda, P(B), lda, m, n, k, grid, row0, col0))
        uh.sync(lib, h)
    ref = C0.double()
    ref[:m, :n] -= A[:m, :k].double() @ B[:n, :k].double().T
    bound = C0.double().abs()
    bound[:m, :n] += A[:m, :k].double().abs() @ B[:n, :k].double().abs().T
    bound *= gamma(k + 2 * ncu)
    ratio = ratio_of((Cm.double() - ref).abs()[win], bound[win])
    report(f"gemm_rounding[{m}x{n}x{k},lower={lower},streamk={sk}]", ratio)
    assert ratio <= 1.0, ratio
    assert torch.equal(uh.bits(Cm)[~win], uh.bits(C0)[~win])


def _spd_f32(n, g):
    """S = G Gᵀ/n + I formed in fp32 and symmetrised (cond₂ <= 5.1 for n = 64 … 2048)"""
    G = torch.randn(n, n, dtype=F32, device="cuda", generator=g)
    S = G @ G.T / n + torch.eye(n, dtype=F32, device="cuda")
    return (S + S.T) / 2


def _potrf_f32_case(lib, h, n, extra, tag):
    from abstractgps_jl_amd._lib import check

    g = torch.Generator(device="cuda").manual_seed(n + extra)
    m, ld = n + extra, n + 32
    S = _spd_f32(n, g)
    X = torch.randn(extra, n, dtype=F32, device="cuda", generator=g)
    nan = float("nan")
    inside = torch.zeros(m + 128, ld, dtype=torch.bool, device="cuda")  # the lower triangle and the rows below it: all the call may read or write
    inside[:n, :n] = torch.tril(torch.ones(n, n, dtype=torch.bool, device="cuda"))
    inside[n:m, :n] = True
    A = torch.full((m + 128, ld), nan, dtype=F32, device="cuda")
    A[:n, :n] = S
    A[n:m, :n] = X
    A[~inside] = nan
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    logdet = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    check(lib.gpd_potrf_f32(h, P(A), ld, m, n, P(info), 0, n, P(logdet)))
    uh.sync(lib, h)
    assert info.item() == 0
    isn = torch.isnan(A)
    assert not isn[inside].any().item(), "NaN inside the factor: something outside the lower triangle was read"
    assert isn[~inside].all().item(), "the strictly upper part or the padding was written"
    S64 = S.double()
    L = torch.tril(torch.nan_to_num(A[:n, :n].double()))
    tri = inside[:n, :n]
    r1 = ratio_of((S64 - L @ L.T).abs()[tri], (gamma(n + 1) * (L.abs() @ L.abs().T))[tri])
    report(f"potrf_factor[{tag}]", r1)
    assert r1 <= 1.0, r1
    if extra:
        Xh = A[n:m, :n].double()
        r2 = ratio_of((Xh @ L.T - X.double()).abs(), gamma(n) * (Xh.abs() @ L.abs().T))
        report(f"potrf_rows_below[{tag}]", r2)
        assert r2 <= 1.0, r2
    ev = torch.linalg.eigvalsh(S64)
    cond = (ev[-1] / ev[0]).item()
    ref = torch.log(torch.diagonal(torch.linalg.cholesky(S64))).sum().item()
    r3 = abs(logdet.item() - ref) / (n * cond * gamma(n + 1))
    report(f"potrf_logdet[{tag}]", r3)
    assert r3 <= 1.0, (r3, cond)


@pytest.mark.parametrize("group", [64, 128, 256, 512])
@pytest.mark.parametrize("n,extra", [(64, 0), (64, 192), (128, 64), (192, 128), (256, 0), (1024, 256),
                                      (64, 128 * 700), (128, 128 * 300 + 64)])  # > 256 workgroups: late starters
def test_potrf_with_rows_below(lib, h, n, extra, group):
    """panel64_kernel<float> (the only fp32 leaf), its left-looking kpre tiles (leaf_group / 64 − 1 of them), and the fp32 trailing GEMMs: the backward errors of
    the factor (Theorem 10.3: |S − L̂L̂ᵀ| <= γ_{n+1} |L̂||L̂|ᵀ) and of the rows below it (8.5: |X̂L̂ᵀ − X| <= γ_n |X̂||L̂|ᵀ), Σ log L̂_ii within n·cond₂(S)·γ_{n+1}, and a
    NaN-filled strictly-upper triangle and padding that stay out of it.  The theorems assume correctly rounded √ and substitution; fast_rsqrt<float> and the leaf's
    explicit inverse tiles add a few·cond·u per element on these matrices (cond <= 5.1): LAPACK fp32 sits at 0.005–0.10 of the same bounds."""
    with uh.params(lib, h, leaf_group=group):
        _potrf_f32_case(lib, h, n, extra, f"n={n},extra={extra},leaf_group={group}")


def test_potrf_reports_first_bad_pivot(lib, h):
    from abstractgps_jl_amd._lib import check

    n, ld = 256, 288
    A = torch.zeros(n + 128, ld, dtype=F32, device="cuda")
    A[:n, :n] = torch.eye(n, dtype=F32, device="cuda")
    A[130, 130] = -2.0
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    check(lib.gpd_potrf_f32(h, P(A), ld, n, n, P(info), 0, n, None))
    uh.sync(lib, h)
    assert info.item() == 131  # LAPACK-style 1-based leading-minor order


def _chol_f32(n, g):
    """a lower factor with fp32 entries (the fp64 Cholesky of G Gᵀ/n + I, rounded)"""
    G = torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g)
    return torch.linalg.cholesky(G @ G.T / n + torch.eye(n, dtype=torch.float64, device="cuda")).to(F32)


@pytest.mark.parametrize("m,n", [(64, 64), (192, 256), (384, 1088)])
def test_trsm_rec(lib, h, m, n):
    """X ← X L⁻ᵀ (trsm64_mfma_kernel<float> leaves + fp32 GEMMs): |X̂Lᵀ − X| <= γ_n |X̂||L|ᵀ; nothing outside the m × n block is touched"""
    from abstractgps_jl_amd._lib import check

    g = torch.Generator(device="cuda").manual_seed(m + n)
    L = _chol_f32(n, g)
    ld = n + 32
    Lp = torch.zeros(n + 128, ld, dtype=F32, device="cuda")
    Lp[:n, :n] = L
    X0 = torch.randn(m + 128, ld, dtype=F32, device="cuda", generator=g)
    X = X0.clone()
    torch.cuda.synchronize()
    check(lib.gpd_trsm_f32(h, P(X), ld, m, P(Lp), ld, n))
    uh.sync(lib, h)
    Xh, L64 = X[:m, :n].double(), L.double()
    ratio = ratio_of((Xh @ L64.T - X0[:m, :n].double()).abs(), gamma(n) * (Xh.abs() @ L64.abs().T))
    report(f"trsm[{m}x{n}]", ratio)
    assert ratio <= 1.0, ratio
    assert torch.equal(uh.bits(X)[m:], uh.bits(X0)[m:]) and torch.equal(uh.bits(X)[:m, n:], uh.bits(X0)[:m, n:])


@pytest.mark.parametrize("nbv", [128, 256, 512, 1024])
@pytest.mark.parametrize("np_,nrhs", [(128, 1), (1024, 2), (1152, 2), (2432, 1), (4096, 3)])
def test_trsv_forward_backward(lib, h, np_, nrhs, nbv):
    """the vector solves (trtri_64_kernel<float> + trsv_diag / trsv_diag2 / trsv_upd_*<float>) at every diagonal block size: |L x̂ − r| <= γ_np |L||x̂| forward, the same
    with Lᵀ backward; the strictly upper triangle is NaN and must never be read"""
    from abstractgps_jl_amd._lib import check

    g = torch.Generator(device="cuda").manual_seed(np_)
    L = _chol_f32(np_, g)
    ld = np_ + 32
    nan = float("nan")
    Lp = torch.full((np_, ld), nan, dtype=F32, device="cuda")
    Lp[:, :np_] = torch.tril(L) + torch.triu(torch.full_like(L, nan), 1)
    R = torch.randn(nrhs, np_, dtype=F32, device="cuda", generator=g)
    L64 = torch.tril(L).double()
    with uh.params(lib, h, trsv_nb=nbv):
        for fwd in (1, 0):
            W = R.clone()
            torch.cuda.synchronize()
            check(lib.gpd_trsv_f32(h, P(Lp), ld, np_, P(W), np_, nrhs, fwd))
            uh.sync(lib, h)
            assert torch.isfinite(W).all().item(), (np_, fwd)
            T = L64 if fwd else L64.T
            x = W.double().T
            ratio = ratio_of((T @ x - R.double().T).abs(), gamma(np_) * (T.abs() @ x.abs()))
            report(f"trsv[np={np_},nrhs={nrhs},trsv_nb={nbv},{'forward' if fwd else 'backward'}]", ratio)
            assert ratio <= 1.0, (ratio, fwd)


def test_gemv_t_exact(lib, h):
    uh.gemv_t_exact(lib, h, F32)


def test_rowsumsq_exact(lib, h):
    uh.rowsumsq_exact(lib, h, F32)


def test_fp32_contracts_are_refused_with_a_reason(lib, h):
    """what the float kernels cannot take — k not a multiple of 32, rows that are not whole 16-byte pieces, a misaligned base — is refused with a status and a text;
    gpd_assemble_f32 wants an 8-byte aligned a_loc and an even lda >= n_loc"""
    Z = torch.zeros(256 + 128, 288, dtype=F32, device="cuda")
    v = torch.zeros(256, dtype=F32, device="cuda")
    off = C.c_void_p(Z.data_ptr() + 4)
    assert lib.gpd_gemm_nt_f32(h, P(Z), 288, P(Z), 288, P(Z), 288, 128, 128, 16, None, 0, 0) == -8 and b"multiple of 32" in lib.gp_last_error()
    assert lib.gpd_gemm_nt_f32(h, P(Z), 288, P(Z), 286, P(Z), 288, 128, 128, 32, None, 0, 0) == -4
    assert lib.gpd_gemm_nt_f32(h, P(Z), 288, P(Z), 288, off, 288, 128, 128, 32, None, 0, 0) == -6 and b"16-byte" in lib.gp_last_error()
    assert lib.gpd_potrf_f32(h, off, 288, 256, 256, None, 0, 256, None) == -2
    assert lib.gpd_potrf_f32(h, P(Z), 286, 256, 256, None, 0, 256, None) == -3 and b"multiple of 4" in lib.gp_last_error()
    assert lib.gpd_potrf_f32(h, P(Z), 288, 250, 250, None, 0, 250, None) == -4
    assert lib.gpd_trsm_f32(h, P(Z), 286, 128, P(Z), 288, 128) == -2
    assert lib.gpd_trsm_f32(h, P(Z), 288, 128, off, 288, 128) == -5
    assert lib.gpd_trsv_f32(h, P(Z), 286, 256, P(v), 256, 1, 1) == -2
    assert lib.gpd_trsv_f32(h, P(Z), 288, 200, P(v), 256, 1, 1) == -4
    # gpd_assemble_f32: the Gram kernel stores two columns (8 bytes) per lane
    from abstractgps_jl_amd._lib import gp_grid, gp_kernel

    kern, grid = gp_kernel(0, 1, 1.5, 0, None), gp_grid(1, 0, 1, 0, 1, 0)
    x = torch.zeros(3, 256, dtype=F32, device="cuda")
    asm = lambda a, lda: lib.gpd_assemble_f32(h, C.byref(kern), P(x), 200, 256, 3, P(v), C.byref(grid), a, lda, 256, 256)
    assert asm(off, 288) == -9 and b"8-byte" in lib.gp_last_error()
    assert asm(P(Z), 287) == -10 and b"even" in lib.gp_last_error()
    assert asm(P(Z), 254) == -10
    assert asm(P(Z), 288) == 0
    uh.sync(lib, h)
