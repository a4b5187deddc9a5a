"""GPU: the Strassen form of the large off-diagonal products (ctx parameter "strassen_min_rows"; csrc/gpmi355.hip gemm_nt_strassen / syrk_lower_split,
csrc/kernels.hpp strassen_sums_kernel and the dual-target epilogue of gemm_nt_dma_kernel).

Shapes are the smallest at which a wrong quadrant, sign, target offset or k half shows: quadrants of one or two 128×128 tiles, unequal M / N, an uneven SYRK split,
leading dimensions that differ from the extents and operands that do not start at the head of their allocation.  With small-integer operands every partial sum of
either form is an integer far below 2^53, so the two forms must agree to the BIT; with Gaussian operands the Strassen error is bounded against the classical error on
the same inputs.  Every test runs on a context of its own: the shared default context never leaves its defaults."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import gp_oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off * t.element_size())


@pytest.fixture
def dev(agp):
    """(lib, ctx) — a private context with time_kernels on: gpd_gemm_time's launch count tells which form a call took (the seven products are 4 launches, against 1)"""
    ctx = agp.Context(0)
    ctx.set_param("time_kernels", 1)
    try:
        yield agp._lib.load(), ctx
    finally:
        ctx.close()


def _launches(lib, ctx):
    from abstractgps_jl_amd._lib import check

    ms, n = C.c_double(), C.c_int64()
    check(lib.gpd_gemm_time(ctx.handle, C.byref(ms), C.byref(n)))  # synchronises the stream and clears the records
    return n.value


def _gemm(lib, ctx, Cbuf, coff, ldc, A, aoff, lda, B, boff, ldb, m, n, k, grid=None, row0=0):
    from abstractgps_jl_amd._lib import check

    out = Cbuf.clone()
    torch.cuda.synchronize()
    check(lib.gpd_gemm_nt(ctx.handle, _p(out, coff), ldc, _p(A, aoff), lda, _p(B, boff), ldb, m, n, k, grid, row0, row0))
    return out, _launches(lib, ctx)


def _bits(t):
    """the bit patterns, with −0 folded onto +0 (the classical kernel forms −(−C + Σ), the Strassen epilogue C − Σ: an exact zero may carry either sign)"""
    return (t + 0.0).view(torch.int64)


def _view(buf, off, rows, ld, cols):
    return buf[off:off + rows * ld].view(rows, ld)[:, :cols]


# (m, n, k, offset of A in elements, GEMM launches expected with the parameter on: 4 = the seven products)
#   (768, 512, 96): unequal quadrants; k/2 = 48 is three whole fp64 k-steps of 16, so the Strassen form takes it (K a multiple of 32 is the rule)
#   (512, 512, 48): k is no multiple of 32 -> one classical launch;  A offset 7: rows not 16-byte aligned -> one classical launch
INT_CASES = [(512, 512, 64, 6, 4), (768, 512, 96, 6, 4), (1024, 512, 256, 6, 4), (512, 512, 48, 6, 1), (512, 512, 64, 7, 1)]


@pytest.mark.parametrize("m,n,k,aoff,products", INT_CASES)
def test_integer_product_is_bit_equal_to_the_host_product_and_to_the_classical_form(dev, m, n, k, aoff, products):
    lib, ctx = dev
    g = torch.Generator(device="cuda").manual_seed(m + 3 * n + 7 * k + aoff)
    lda, ldb, ldc, boff, coff = k + 40, k + 24, n + 24, 10, 3
    A = torch.randint(-8, 9, (aoff + (m + 128) * lda,), device="cuda", generator=g).double()
    B = torch.randint(-8, 9, (boff + (n + 128) * ldb,), device="cuda", generator=g).double()
    C0 = torch.randint(-64, 65, (coff + (m + 1) * ldc,), device="cuda", generator=g).double()
    ref = C0.clone()
    _view(ref, coff, m, ldc, n).sub_(_view(A, aoff, m, lda, k) @ _view(B, boff, n, ldb, k).T)  # integers below 2^53: exact in any order
    ctx.set_param("strassen_min_rows", 0)
    classical, n0 = _gemm(lib, ctx, C0, coff, ldc, A, aoff, lda, B, boff, ldb, m, n, k)
    ctx.set_param("strassen_min_rows", 256)
    strassen, n1 = _gemm(lib, ctx, C0, coff, ldc, A, aoff, lda, B, boff, ldb, m, n, k)
    assert (n0, n1) == (1, products)
    assert torch.equal(_bits(classical), _bits(ref))
    assert torch.equal(_bits(strassen), _bits(ref))  # the window AND everything around it (ld padding, offsets)


@pytest.mark.parametrize("m,n,k", [(512, 512, 256), (1024, 1024, 512)])
def test_gaussian_product_error_is_within_four_times_the_classical_error(dev, m, n, k):
    """max |C − ref| / max |ref| against a host long-double product: one level of Strassen errs 1.0–2.3 × the classical product in a NumPy model (sizes 512…1 024,
    K 256…2 048); the bound of 4 × leaves room for the MFMA summation order.  Both figures are printed."""
    lib, ctx = dev
    g = torch.Generator(device="cuda").manual_seed(m + k)
    A = torch.randn((m + 128) * k, dtype=torch.float64, device="cuda", generator=g)
    B = torch.randn((n + 128) * k, dtype=torch.float64, device="cuda", generator=g)
    C0 = torch.randn(m * n, dtype=torch.float64, device="cuda", generator=g)
    Ah, Bh = A[:m * k].view(m, k).cpu().numpy().astype(np.longdouble), B[:n * k].view(n, k).cpu().numpy().astype(np.longdouble)
    ref = C0.view(m, n).cpu().numpy().astype(np.longdouble)
    for j in range(0, k, 64):  # rank-64 updates keep the long-double temporaries small
        ref -= Ah[:, j:j + 64] @ Bh[:, j:j + 64].T
    scale = np.max(np.abs(ref))
    err = {}
    for v, launches in ((0, 1), (256, 4)):
        ctx.set_param("strassen_min_rows", v)
        out, nl = _gemm(lib, ctx, C0, 0, n, A, 0, k, B, 0, k, m, n, k)
        assert nl == launches
        err[v] = float(np.max(np.abs(out.view(m, n).cpu().numpy().astype(np.longdouble) - ref)) / scale)
    print(f"STRASSEN {m}x{n}x{k}: classical {err[0]:.3e} strassen {err[256]:.3e} ratio {err[256] / err[0]:.2f}", flush=True)
    assert err[256] <= 4 * err[0], err


@pytest.mark.parametrize("m", [1024, 1280])
def test_lower_syrk_split_is_bit_equal_to_the_single_launch(dev, m):
    """a == b, lower, 128 carried rows below the square.  m = 1 024 splits at 512 | 512; m = 1 280 at 512 | 768 (the split is rounded down to 256), whose 768-row half
    splits again at 256 | 512; every 512-row diagonal block splits once more at 256 | 256 (quadrants of one tile).  Lower triangle and carried rows: the host integer product; the 64×64 sub-tiles strictly above the diagonal: untouched."""
    from abstractgps_jl_amd._lib import gp_grid

    lib, ctx = dev
    k, extra, row0 = 256, 128, 384
    g = torch.Generator(device="cuda").manual_seed(m)
    ldp, ldc = k + 32, m + 40
    Pm = torch.randint(-8, 9, ((m + extra + 128) * ldp,), device="cuda", generator=g).double()
    C0 = torch.randint(-64, 65, ((m + extra) * ldc,), device="cuda", generator=g).double()
    Pv = _view(Pm, 0, m + extra, ldp, k)
    r = torch.arange(m + extra, device="cuda")[:, None]
    c = torch.arange(ldc, device="cuda")[None, :]
    win = ((c // 64) <= (r // 64)) & (c < m)  # what a lower launch updates: 64×64 sub-tiles on and below the diagonal, every column of the carried rows
    ref = C0.view(m + extra, ldc).clone()
    ref[:, :m] -= Pv @ Pv[:m].T
    ref = torch.where(win, ref, C0.view(m + extra, ldc))
    grid = C.byref(gp_grid(1, 0, 1, 0, 1, 1))
    ctx.set_param("strassen_min_rows", 0)
    classical, n0 = _gemm(lib, ctx, C0, 0, ldc, Pm, 0, ldp, Pm, 0, ldp, m + extra, m, k, grid, row0)
    ctx.set_param("strassen_min_rows", 256)
    split, n1 = _gemm(lib, ctx, C0, 0, ldc, Pm, 0, ldp, Pm, 0, ldp, m + extra, m, k, grid, row0)
    # launches: side 256 -> 1, side 512 -> 1 + 4 + 1 = 6;  1 024: 6 + 4 + 6 + carried rows = 17;  1 280: 6 + 4 + (1 + 4 + 6) + carried rows = 22
    assert (n0, n1) == (1, 17 if m == 1024 else 22)
    assert torch.equal(_bits(classical.view(m + extra, ldc)), _bits(ref))
    assert torch.equal(_bits(split.view(m + extra, ldc)), _bits(ref))


# ---- fits through the public API --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fits():
    """inputs and oracle results of the two fits (N = 2 048: whole panels; N = 1 920: padded to 2 048), computed once"""
    out = {}
    for n in (2048, 1920):
        x, y = o.synth_inputs(n, 3, 100 + n)
        Y = np.stack([y, np.cos(y), y * y - 1.0], axis=1)
        ofx = o.FiniteGP(o.GP(o.Kernel(o.SE)), x, 0.01)
        lp, post = o.logpdf_and_posterior(ofx, y)
        out[n] = dict(x=x, y=y, Y=Y, lp=lp, alpha=post.alpha, U=post.U, lpY=o.logpdf(ofx, Y))
    return out


def _ctx(agp, **kw):
    ctx = agp.Context(0)
    for k, v in {**dict(nb=256, strassen_min_rows=256), **kw}.items():  # 256-column panels: bulk updates of side 1 536, 1 280, ..., 512 run split, the last ones whole
        ctx.set_param(k, v)
    return ctx


def _fit(agp, ctx, d):
    f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
    post = agp.posterior(f(agp.RowVecs(d["x"]), 0.01), d["y"])
    res = (np.float64(post.logpdf_value), np.array(post.data.alpha), np.array(post.data.C.U))
    post.data.C.free()
    return res


@pytest.mark.parametrize("n", [2048, 1920])
def test_fit_with_the_strassen_form_meets_the_oracle(agp, fits, n):
    d = fits[n]
    ctx = _ctx(agp, time_kernels=1)
    try:
        lp, alpha, U = _fit(agp, ctx, d)
        tm = ctx.timings()
        f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
        lpY = agp.logpdf(f(agp.RowVecs(d["x"]), 0.01), d["Y"])  # three columns: carried rows below every bulk update
    finally:
        ctx.close()
    assert tm["gemm_launches"] > 60  # 7 panels × (U1 + 1 bulk launch) without the split; every split adds 5 or more
    assert lp == pytest.approx(d["lp"], rel=1e-10)
    assert np.linalg.norm(alpha - d["alpha"]) / np.linalg.norm(d["alpha"]) <= 1e-8
    assert np.max(np.abs(U - d["U"])) <= 1e-10
    np.testing.assert_allclose(lpY, d["lpY"], rtol=1e-10)


def test_deterministic_fits_with_the_strassen_form_are_bit_identical(agp, fits):
    d = fits[1920]
    ctx = _ctx(agp, deterministic=1)
    try:
        a, b = _fit(agp, ctx, d), _fit(agp, ctx, d)
    finally:
        ctx.close()
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert a[0] == pytest.approx(d["lp"], rel=1e-10)


def test_poisoned_blocks_do_not_change_a_strassen_fit(agp, fits):
    """alloc_poison = 1 fills every block (the sum panels included) with NaN bytes before use: every panel element a product reads was written by the sums first"""
    d = fits[1920]
    res = []
    for poison in (0, 1):
        ctx = _ctx(agp, deterministic=1, alloc_poison=poison)
        try:
            res.append(_fit(agp, ctx, d))
        finally:
            ctx.close()
    for u, v in zip(*res):
        assert np.array_equal(u, v)


def test_not_positive_definite_input_reports_the_same_minor(agp):
    """σ² = 0 with a duplicated point: the leading minor that fails does not depend on the form of the trailing updates before it"""
    x, y = o.synth_inputs(2048, 3, 5)
    x[1700] = x[900]
    info = []
    for v in (0, 256):
        ctx = _ctx(agp, strassen_min_rows=v, deterministic=1)
        try:
            f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
            with pytest.raises(agp.PosDefException) as e:
                agp.logpdf(f(agp.RowVecs(x), 0.0), y)
            info.append(e.value.info)
        finally:
            ctx.close()
    print(f"STRASSEN not-PD info: classical {info[0]} strassen {info[1]}", flush=True)
    assert info[0] == info[1] and 1 <= info[0] <= 2048
