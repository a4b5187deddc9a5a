"""GPU: the grouped form of a bulk update (ctx parameters "strassen_group" / "strassen_group_min_rows"; csrc/bulk_plan.hpp, csrc/kernels.hpp gemm_nt_grp_kernel,
csrc/gpmi355.hip run_grouped): the sums of every Strassen block, then FOUR launches over the tiles of all pieces of the update.

The grouped form changes no tile's arithmetic and no quadrant's order of products, so under "deterministic" it must equal the per-block launch sequence to the BIT —
on integers in any mode.  Shapes as in tests/test_gpu_strassen.py: quadrants of one or two tiles, an uneven split three levels deep, a 128-row remainder strip,
carried rows, leading dimensions that differ from the extents.  The plan itself (targets, order, coverage, workspace) is checked without a GPU in
tests/test_bulk_plan_cpu.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import gp_oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu

K, EXTRA, ROW0 = 256, 128, 384
# 1 024: 512 | 512, then 256 | 256;  1 280: 512 | 768, three levels deep;  1 408: 512 | 896 with a 128-row remainder strip below the 768-row Strassen block
SIDES = [1024, 1280, 1408]


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture
def dev(agp):
    ctx = agp.Context(0)
    for k, v in dict(time_kernels=1, strassen_min_rows=256, strassen_group_min_rows=256).items():
        ctx.set_param(k, v)
    try:
        yield agp._lib.load(), ctx
    finally:
        ctx.close()


def _syrk(lib, ctx, C0, Pm, m, ldc, ldp, group):
    """C0 (a clone) −= P·P[0:m]ᵀ through gpd_gemm_nt in lower mode; returns the buffer and the number of GEMM launches"""
    from abstractgps_jl_amd._lib import check, gp_grid

    ctx.set_param("strassen_group", group)
    out = C0.clone()
    torch.cuda.synchronize()
    grid = C.byref(gp_grid(1, 0, 1, 0, 1, 1))
    check(lib.gpd_gemm_nt(ctx.handle, _p(out), ldc, _p(Pm), ldp, _p(Pm), ldp, m + EXTRA, m, K, grid, ROW0, ROW0))
    ms, n = C.c_double(), C.c_int64()
    check(lib.gpd_gemm_time(ctx.handle, C.byref(ms), C.byref(n)))  # synchronises the stream and clears the records
    return out, n.value


def _bits(t):
    return (t + 0.0).view(torch.int64)  # −0 folded onto +0, as in tests/test_gpu_strassen.py


@pytest.mark.parametrize("m", SIDES)
def test_grouped_integer_syrk_is_bit_equal_to_the_host_product_and_to_the_ungrouped_form_in_four_launches(dev, m):
    lib, ctx = dev
    g = torch.Generator(device="cuda").manual_seed(m)
    ldp, ldc = K + 32, m + 40
    Pm = torch.randint(-8, 9, ((m + EXTRA + 128) * ldp,), device="cuda", generator=g).double()
    C0 = torch.randint(-64, 65, ((m + EXTRA) * ldc,), device="cuda", generator=g).double()
    Pv = Pm[:(m + EXTRA) * ldp].view(m + EXTRA, ldp)[:, :K]
    r = torch.arange(m + EXTRA, device="cuda")[:, None]
    c = torch.arange(ldc, device="cuda")[None, :]
    win = ((c // 64) <= (r // 64)) & (c < m)  # the lower window in 64×64 sub-tiles and every column of the carried rows
    ref = C0.view(m + EXTRA, ldc).clone()
    ref[:, :m] -= Pv @ Pv[:m].T  # integers far below 2^53: exact in any order
    ref = torch.where(win, ref, C0.view(m + EXTRA, ldc))
    ungrouped, n0 = _syrk(lib, ctx, C0, Pm, m, ldc, ldp, 0)
    grouped, n1 = _syrk(lib, ctx, C0, Pm, m, ldc, ldp, 1)
    print(f"GROUPED m={m}: launches ungrouped {n0} grouped {n1}", flush=True)
    assert n1 == 4 and n0 > 4
    assert torch.equal(_bits(grouped.view(m + EXTRA, ldc)), _bits(ref))  # the window, the carried rows, AND the ld padding / the sub-tiles above the diagonal untouched
    assert torch.equal(_bits(grouped), _bits(ungrouped))                 # the whole buffer


@pytest.mark.parametrize("m", SIDES)
def test_grouped_gaussian_syrk_is_bit_equal_to_the_ungrouped_form(dev, m):
    """same per-tile arithmetic, same order of products per quadrant; deterministic = 1 keeps the stream-K tails (atomics) out of the ungrouped classical pieces"""
    lib, ctx = dev
    ctx.set_param("deterministic", 1)
    g = torch.Generator(device="cuda").manual_seed(7 * m)
    ldp, ldc = K + 32, m + 40
    Pm = torch.randn((m + EXTRA + 128) * ldp, dtype=torch.float64, device="cuda", generator=g)
    C0 = torch.randn((m + EXTRA) * ldc, dtype=torch.float64, device="cuda", generator=g)
    ungrouped, n0 = _syrk(lib, ctx, C0, Pm, m, ldc, ldp, 0)
    grouped, n1 = _syrk(lib, ctx, C0, Pm, m, ldc, ldp, 1)
    assert n1 == 4 and n0 > 4
    assert torch.equal(grouped.view(torch.int64), ungrouped.view(torch.int64))
    assert not torch.equal(grouped, C0)


# ---- fits through the public API (the recipe of tests/test_gpu_strassen.py's `fits`) -------------------------------------------------------------------------------
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
    # 256-column panels: the bulk updates of side 1 536 … 512 are split, and with the floor at 256 every one of them runs grouped
    for k, v in {**dict(nb=256, strassen_min_rows=256, strassen_group=1, strassen_group_min_rows=256), **kw}.items():
        ctx.set_param(k, v)
    return ctx


def _fit(agp, ctx, d):
    f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
    post = agp.posterior(f(agp.RowVecs(d["x"]), 0.01), d["y"])
    res = (np.float64(post.logpdf_value), np.array(post.data.alpha), np.array(post.data.C.U))
    post.data.C.free()
    return res


@pytest.mark.parametrize("n", [2048, 1920])
def test_grouped_fit_meets_the_oracle_and_counts_the_flops_of_the_ungrouped_fit(agp, fits, n):
    d = fits[n]
    tm = {}
    for group in (1, 0):
        ctx = _ctx(agp, time_kernels=1, strassen_group=group)
        try:
            lp, alpha, U = _fit(agp, ctx, d)
            tm[group] = ctx.timings()
            if group:
                f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
                lpY = agp.logpdf(f(agp.RowVecs(d["x"]), 0.01), d["Y"])  # three columns: carried rows below every bulk update
                res = (lp, alpha, U)
        finally:
            ctx.close()
    lp, alpha, U = res
    print(f"GROUPED fit N={n}: launches grouped {tm[1]['gemm_launches']} ungrouped {tm[0]['gemm_launches']} gemm_flops {tm[1]['gemm_flops']:.6e} / {tm[0]['gemm_flops']:.6e}",
          flush=True)
    assert tm[1]["gemm_launches"] < tm[0]["gemm_launches"]  # five split updates: 4 launches each instead of 6 … 27
    assert tm[1]["gemm_flops"] == tm[0]["gemm_flops"]
    assert lp == pytest.approx(d["lp"], rel=1e-10)
    assert np.linalg.norm(alpha - d["alpha"]) / np.linalg.norm(d["alpha"]) <= 1e-8
    assert np.max(np.abs(U - d["U"])) <= 1e-10
    np.testing.assert_allclose(lpY, d["lpY"], rtol=1e-10)


@pytest.mark.parametrize("n", [2048, 1920])
def test_deterministic_grouped_fits_are_bit_identical_to_each_other_and_to_the_ungrouped_fit(agp, fits, n):
    """two grouped fits on contexts of their own and the ungrouped fit: the same bits"""
    d = fits[n]
    res = []
    for group in (1, 1, 0):
        ctx = _ctx(agp, deterministic=1, strassen_group=group)
        try:
            res.append(_fit(agp, ctx, d))
        finally:
            ctx.close()
    for other in res[1:]:
        for u, v in zip(res[0], other):
            assert np.array_equal(u, v)
    assert res[0][0] == pytest.approx(d["lp"], rel=1e-10)


@pytest.mark.parametrize("n", [2048, 1920])
def test_two_deterministic_grouped_fits_on_one_context_are_bit_identical(agp, fits, n):
    """the second fit reuses the page-locked table staging, the workspace block and the table block of the first"""
    d = fits[n]
    ctx = _ctx(agp, deterministic=1)
    try:
        a, b = _fit(agp, ctx, d), _fit(agp, ctx, d)
    finally:
        ctx.close()
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("n", [2048, 1920])
def test_poisoned_blocks_do_not_change_a_grouped_fit(agp, fits, n):
    """alloc_poison = 1 fills every block — the problem tables and every block's sum panels included — with 0xFF bytes before use: all of it is written before it is read"""
    d = fits[n]
    res = []
    for poison in (0, 1):
        ctx = _ctx(agp, deterministic=1, alloc_poison=poison)
        try:
            res.append(_fit(agp, ctx, d))
        finally:
            ctx.close()
    for u, v in zip(*res):
        assert np.array_equal(u, v)


def test_not_positive_definite_input_reports_the_same_minor_with_grouping(agp):
    """σ² = 0 with a duplicated point (the case of tests/test_gpu_strassen.py): the failing leading minor does not depend on the form of the updates before it"""
    x, y = o.synth_inputs(2048, 3, 5)
    x[1700] = x[900]
    info = []
    for kw in (dict(strassen_min_rows=0), dict(strassen_group=0), dict(strassen_group=1)):
        ctx = _ctx(agp, deterministic=1, **kw)
        try:
            f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
            with pytest.raises(agp.PosDefException) as e:
                agp.logpdf(f(agp.RowVecs(x), 0.0), y)
            info.append(e.value.info)
        finally:
            ctx.close()
    print(f"GROUPED not-PD info: classical {info[0]} ungrouped {info[1]} grouped {info[2]}", flush=True)
    assert info[0] == info[1] == info[2] and 1 <= info[0] <= 2048
