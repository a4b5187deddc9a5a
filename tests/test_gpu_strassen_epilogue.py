"""GPU: the dual-target epilogue of the Strassen products (csrc/kernels.hpp gemm_nt_tile): every product is accumulated from zero and then subtracted from one or
two target quadrants.  The read-modify-writes of a tile are issued in batches — the loads of a 16-row group of both targets, the FMAs, the stores — where they
used to go element by element; a tile writes each target element exactly once, so the result must be bit for bit what it was.

Exact cases: integer operands with |a| <= 8 and K <= 96 (every sum, product and partial sum an integer far below 2^53), C pre-filled with DISTINCT integers and
embedded in a buffer of sentinels — guard rows above and below and the leading-dimension padding — so that a dropped, doubled or mis-targeted read-modify-write
shows as a wrong bit, in the window or around it.  Shapes from one tile per product and one k step per half, (256, 256, 32): the smallest case in which all seven
products and both targets exist, to quadrants three tiles wide.  Every shape with "ldpad" (the pad of the sum panels' row stride) 0 and 48; per block (gpd_gemm_nt
on a rectangle: the launches with nbatch = 2 and c2stride, through gemm_nt_dma_kernel) and grouped (the lower SYRK at m = 512 and 1 024 through gemm_nt_grp_kernel).

Gaussian cases: the bound of tests/test_gpu_strassen.py for one level — the error against a host long-double product at most four times the classical kernel's on
the same operands — per block on the rectangle and grouped on the SYRK that holds the same rectangle as its Strassen block; under "deterministic" two calls give
the same bits.  One fit at N = 2 048 on the two-stream schedule against the oracle at the project's tolerances.  Last, the size-dependent threshold
"strassen_min_rows_large": where it applies and that an explicit "strassen_min_rows" overrides it."""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import gp_oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 3          # sentinel rows above and below C
SENTINEL = -7.0e9  # sentinels are SENTINEL − index: distinct, and far from every value the window can take


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off * t.element_size())


def _bits(t):
    """the bit patterns, with −0 folded onto +0 (as in tests/test_gpu_strassen.py)"""
    return (t + 0.0).view(torch.int64)


@pytest.fixture
def dev(agp):
    ctx = agp.Context(0)
    for k, v in dict(time_kernels=1, strassen_min_rows=256, strassen_group_min_rows=256).items():
        ctx.set_param(k, v)
    try:
        yield agp._lib.load(), ctx
    finally:
        ctx.close()


def _launches(lib, ctx):
    from abstractgps_jl_amd._lib import check

    ms, n = C.c_double(), C.c_int64()
    check(lib.gpd_gemm_time(ctx.handle, C.byref(ms), C.byref(n)))  # synchronises the stream and clears the records
    return n.value


def _guarded(rows, cols, ldc, gen):
    """(buffer, offset of C in it, mask of the rows × cols window): GUARD sentinel rows, rows × ldc, GUARD sentinel rows; the window holds a permutation of
    distinct integers, everything else distinct sentinels"""
    total = (rows + 2 * GUARD) * ldc
    buf = SENTINEL - torch.arange(total, device="cuda", dtype=torch.float64)
    view = buf.view(rows + 2 * GUARD, ldc)
    vals = (torch.randperm(rows * cols, device="cuda", generator=gen) - (rows * cols) // 2).double()
    view[GUARD:GUARD + rows, :cols] = vals.view(rows, cols)
    mask = torch.zeros(rows + 2 * GUARD, ldc, dtype=torch.bool, device="cuda")
    mask[GUARD:GUARD + rows, :cols] = True
    return buf, GUARD * ldc, mask


# ---- exact integer products, per block ---------------------------------------------------------------------------------------------------------------------------
RECTS = [(256, 256, 32), (512, 256, 64), (256, 768, 96), (768, 768, 64)]


@pytest.mark.parametrize("ldpad", [0, 48])
@pytest.mark.parametrize("m,n,k", RECTS)
def test_integer_rectangle_per_block_is_bit_equal_to_the_host_product_and_leaves_the_sentinels(dev, m, n, k, ldpad):
    from abstractgps_jl_amd._lib import check

    lib, ctx = dev
    ctx.set_param("ldpad", ldpad)
    ctx.set_param("strassen_group", 0)
    g = torch.Generator(device="cuda").manual_seed(m + 3 * n + 7 * k + ldpad)
    lda, ldb, ldc = k + 40, k + 24, n + 24
    A = torch.randint(-8, 9, ((m + 128) * lda,), device="cuda", generator=g).double()
    B = torch.randint(-8, 9, ((n + 128) * ldb,), device="cuda", generator=g).double()
    C0, coff, mask = _guarded(m, n, ldc, g)
    Ah = A[:m * lda].view(m, lda)[:, :k].cpu().numpy().astype(np.int64)
    Bh = B[:n * ldb].view(n, ldb)[:, :k].cpu().numpy().astype(np.int64)
    ref = C0.clone()
    ref.view(-1, ldc)[GUARD:GUARD + m, :n] -= torch.from_numpy((Ah @ Bh.T).astype(np.float64)).cuda()  # the host int64 product
    out = C0.clone()
    torch.cuda.synchronize()
    check(lib.gpd_gemm_nt(ctx.handle, _p(out, coff), ldc, _p(A), lda, _p(B), ldb, m, n, k, None, 0, 0))
    assert _launches(lib, ctx) == 4  # the seven products: M1 alone, then three launches of two products (nbatch = 2, c2stride)
    assert torch.equal(out.view(-1, ldc)[~mask], C0.view(-1, ldc)[~mask])  # guard rows and ld padding: not a bit changed
    assert torch.equal(_bits(out), _bits(ref))
    assert not torch.equal(out.view(-1, ldc)[mask], C0.view(-1, ldc)[mask])


# ---- exact integer products, grouped -----------------------------------------------------------------------------------------------------------------------------
EXTRA, ROW0 = 128, 384


def _syrk(lib, ctx, C0, coff, Pm, m, ldc, ldp, k, group):
    from abstractgps_jl_amd._lib import check, gp_grid

    ctx.set_param("strassen_group", group)
    out = C0.clone()
    torch.cuda.synchronize()
    grid = C.byref(gp_grid(1, 0, 1, 0, 1, 1))
    check(lib.gpd_gemm_nt(ctx.handle, _p(out, coff), ldc, _p(Pm), ldp, _p(Pm), ldp, m + EXTRA, m, k, grid, ROW0, ROW0))
    return out, _launches(lib, ctx)


@pytest.mark.parametrize("ldpad", [0, 48])
@pytest.mark.parametrize("k", [32, 64, 96])
@pytest.mark.parametrize("m", [512, 1024])
def test_integer_grouped_syrk_is_bit_equal_to_the_host_product_and_to_the_per_block_form(dev, m, k, ldpad):
    """m = 512: one Strassen block of 256 × 256 (one tile per product; k = 32: one k step per half); m = 1 024: a 512 × 512 block and two 256 × 256 ones.
    128 carried rows below the square.  Lower window and carried rows: the host int64 product; everything else — the sub-tiles above the diagonal, the ld
    padding, the guard rows — untouched."""
    lib, ctx = dev
    ctx.set_param("ldpad", ldpad)
    g = torch.Generator(device="cuda").manual_seed(m + 7 * k + ldpad)
    rows, ldp, ldc = m + EXTRA, k + 32, m + 40
    Pm = torch.randint(-8, 9, ((rows + 128) * ldp,), device="cuda", generator=g).double()
    C0, coff, mask = _guarded(rows, m, ldc, g)
    Ph = Pm[:rows * ldp].view(rows, ldp)[:, :k].cpu().numpy().astype(np.int64)
    r = torch.arange(rows, device="cuda")[:, None]
    c = torch.arange(ldc, device="cuda")[None, :]
    win = ((c // 64) <= (r // 64)) & (c < m)  # what a lower launch updates: 64×64 sub-tiles on and below the diagonal, every column of the carried rows
    ref = C0.clone()
    body = ref.view(-1, ldc)[GUARD:GUARD + rows]
    upd = body.clone()
    upd[:, :m] -= torch.from_numpy((Ph @ Ph[:m].T).astype(np.float64)).cuda()
    body.copy_(torch.where(win, upd, body))
    per_block, n0 = _syrk(lib, ctx, C0, coff, Pm, m, ldc, ldp, k, 0)
    grouped, n1 = _syrk(lib, ctx, C0, coff, Pm, m, ldc, ldp, k, 1)
    assert n1 == 4 and n0 > 4
    for out in (grouped, per_block):
        assert torch.equal(out.view(-1, ldc)[~mask], C0.view(-1, ldc)[~mask])
        assert torch.equal(_bits(out), _bits(ref))
    assert torch.equal(_bits(grouped), _bits(per_block))


# ---- Gaussian operands -------------------------------------------------------------------------------------------------------------------------------------------
GAUSS = [(512, 512, 64), (1024, 768, 2048)]


@functools.lru_cache(maxsize=None)
def _gauss_case(m, n, k):
    """operands of the SYRK of side n + m whose Strassen block — rows [n, n + m) × columns [0, n) — is the m × n × k rectangle (the split of side n + m falls at n
    for both cases), C0, and the host long-double result of that rectangle; computed once, never changed"""
    side = n + m
    assert (side // 2) // 256 * 256 == n and m % 256 == 0
    g = torch.Generator(device="cuda").manual_seed(m + n + k)
    ldp = k + 32
    Pm = torch.randn((side + 128) * ldp, dtype=torch.float64, device="cuda", generator=g)
    C0 = torch.randn(side * side, dtype=torch.float64, device="cuda", generator=g)
    Pv = Pm[:side * ldp].view(side, ldp)[:, :k].cpu().numpy()
    Ch, Bh = C0.view(side, side)[n:, :n].cpu().numpy(), Pv[:n].astype(np.longdouble)

    def rows(i):  # 64 rows of the long-double result (NumPy's long-double product is a plain loop that releases the GIL: eight at a time)
        return Ch[i:i + 64].astype(np.longdouble) - Pv[n + i:n + i + 64].astype(np.longdouble) @ Bh.T

    with ThreadPoolExecutor(8) as ex:
        ref = np.concatenate(list(ex.map(rows, range(0, m, 64))))
    return Pm, C0, ldp, ref, float(np.max(np.abs(ref)))


def _block_err(out, side, m, n, ref, scale):
    return float(np.max(np.abs(out.view(side, side)[n:, :n].cpu().numpy().astype(np.longdouble) - ref)) / scale)


@pytest.mark.parametrize("m,n,k", GAUSS)
def test_gaussian_per_block_error_is_within_four_times_the_classical_error_and_repeats_to_the_bit(dev, m, n, k):
    from abstractgps_jl_amd._lib import check

    lib, ctx = dev
    ctx.set_param("deterministic", 1)
    ctx.set_param("strassen_group", 0)
    Pm, C0, ldp, ref, scale = _gauss_case(m, n, k)
    side = n + m
    res, err = {}, {}
    for name, v, launches in (("classical", 0, 1), ("strassen", 256, 4), ("again", 256, 4)):
        ctx.set_param("strassen_min_rows", v)
        out = C0.clone()
        torch.cuda.synchronize()
        check(lib.gpd_gemm_nt(ctx.handle, _p(out, n * side), side, _p(Pm, n * ldp), ldp, _p(Pm), ldp, m, n, k, None, 0, 0))
        assert _launches(lib, ctx) == launches
        res[name], err[name] = out, _block_err(out, side, m, n, ref, scale)
    print(f"EPILOGUE per-block {m}x{n}x{k}: classical {err['classical']:.3e} strassen {err['strassen']:.3e} ratio {err['strassen'] / err['classical']:.2f}", flush=True)
    assert err["strassen"] <= 4 * err["classical"], err
    assert torch.equal(res["strassen"].view(torch.int64), res["again"].view(torch.int64))


@pytest.mark.parametrize("m,n,k", GAUSS)
def test_gaussian_grouped_error_is_within_four_times_the_classical_error_and_repeats_to_the_bit(dev, m, n, k):
    """the lower SYRK of side n + m: grouped, its m × n Strassen block is checked against the same long-double rectangle; the classical figure is the one-launch SYRK's"""
    from abstractgps_jl_amd._lib import check, gp_grid

    lib, ctx = dev
    ctx.set_param("deterministic", 1)
    ctx.set_param("strassen_group", 1)
    Pm, C0, ldp, ref, scale = _gauss_case(m, n, k)
    side = n + m
    grid = C.byref(gp_grid(1, 0, 1, 0, 1, 1))
    res, err = {}, {}
    for name, v, launches in (("classical", 0, 1), ("grouped", 256, 4), ("again", 256, 4)):
        ctx.set_param("strassen_min_rows", v)
        out = C0.clone()
        torch.cuda.synchronize()
        check(lib.gpd_gemm_nt(ctx.handle, _p(out), side, _p(Pm), ldp, _p(Pm), ldp, side, side, k, grid, 0, 0))
        assert _launches(lib, ctx) == launches
        res[name], err[name] = out, _block_err(out, side, m, n, ref, scale)
    print(f"EPILOGUE grouped {m}x{n}x{k}: classical {err['classical']:.3e} grouped {err['grouped']:.3e} ratio {err['grouped'] / err['classical']:.2f}", flush=True)
    assert err["grouped"] <= 4 * err["classical"], err
    assert torch.equal(res["grouped"].view(torch.int64), res["again"].view(torch.int64))


# ---- one fit -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_fit_on_the_two_stream_schedule_with_grouped_strassen_updates_meets_the_oracle(agp):
    """N = 2 048, nb = 256, both Strassen floors at 256, the look-ahead forced on: logpdf rel 1e-10, ‖α − α_ref‖ / ‖α_ref‖ <= 1e-8, max|U − U_ref| <= 1e-10"""
    n = 2048
    x, y = o.synth_inputs(n, 3, 100 + n)
    lp_o, post_o = o.logpdf_and_posterior(o.FiniteGP(o.GP(o.Kernel(o.SE)), x, 0.01), y)
    ctx = agp.Context(0)
    try:
        for k, v in dict(nb=256, strassen_min_rows=256, strassen_group=1, strassen_group_min_rows=256, lookahead=1, lookahead_min_n=0, time_kernels=1).items():
            ctx.set_param(k, v)
        f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
        post = agp.posterior(f(agp.RowVecs(x), 0.01), y)
        lp, alpha, U = np.float64(post.logpdf_value), np.array(post.data.alpha), np.array(post.data.C.U)
        tm = ctx.timings()
        post.data.C.free()
    finally:
        ctx.close()
    e_a = float(np.linalg.norm(alpha - post_o.alpha) / np.linalg.norm(post_o.alpha))
    e_u = float(np.max(np.abs(U - post_o.U)))
    print(f"EPILOGUE fit N={n}: logpdf rel {abs(lp - lp_o) / abs(lp_o):.2e} alpha rel {e_a:.2e} max|U-Uref| {e_u:.2e} gemm launches {tm['gemm_launches']}", flush=True)
    assert lp == pytest.approx(lp_o, rel=1e-10)
    assert e_a <= 1e-8 and e_u <= 1e-10


# ---- "strassen_min_rows_large": the threshold of the fits that take the look-ahead schedule ------------------------------------------------------------------------
def _small_fit(agp, **kw):
    """N = 2 048 at nb = 256 with the grouping floor at 256, deterministic; returns (logpdf, α, GEMM launches, the two thresholds as read back before the fit)"""
    x, y = o.synth_inputs(2048, 3, 100 + 2048)
    ctx = agp.Context(0)
    try:
        before = (ctx.get_param("strassen_min_rows"), ctx.get_param("strassen_min_rows_large"))
        for k, v in {**dict(nb=256, strassen_group_min_rows=256, deterministic=1, time_kernels=1), **kw}.items():
            ctx.set_param(k, v)
        f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
        post = agp.posterior(f(agp.RowVecs(x), 0.01), y)
        res = (np.float64(post.logpdf_value), np.array(post.data.alpha), ctx.timings()["gemm_launches"], before)
        post.data.C.free()
    finally:
        ctx.close()
    return res


def test_strassen_min_rows_large_applies_from_lookahead_min_n_on_and_only_until_strassen_min_rows_is_set(agp):
    """defaults 8 192 and 4 096.  With strassen_min_rows_large = 256 and lookahead_min_n = 0 the fit is the fit with an explicit strassen_min_rows = 256 (launches
    and, deterministic, bits); below lookahead_min_n (its default, far above N) and with strassen_min_rows set by the caller — even to its default — it is the
    classical fit."""
    explicit = _small_fit(agp, strassen_min_rows=256, lookahead_min_n=0)
    classical = _small_fit(agp, strassen_min_rows=0, lookahead_min_n=0)
    large = _small_fit(agp, strassen_min_rows_large=256, lookahead_min_n=0)
    below = _small_fit(agp, strassen_min_rows_large=256)
    pinned = _small_fit(agp, strassen_min_rows_large=256, strassen_min_rows=8192, lookahead_min_n=0)
    assert large[3] == (8192, 4096)
    print(f"EPILOGUE threshold: launches explicit {explicit[2]} large {large[2]} classical {classical[2]} below {below[2]} pinned {pinned[2]}", flush=True)
    assert explicit[2] > classical[2]
    assert large[2] == explicit[2] and large[0] == explicit[0] and np.array_equal(large[1], explicit[1])
    assert pinned[2] == classical[2] and pinned[0] == classical[0] and np.array_equal(pinned[1], classical[1])
    assert below[2] == classical[2]  # below lookahead_min_n the default threshold of 8 192 holds: no update of this fit is split
