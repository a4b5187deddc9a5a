"""GPU: the two N-long reductions of the sparse fit's streamed pass — ystats_kernel<T> and ystats_cols_kernel<T, 1|2> — through their device-level entry points
(gpd_ystats, gpd_ystats_cols and the _f32 twins; include/gpmi355.h), on integers: every partial sum is an integer below 2⁵³, so the result equals the fp64 reference
EXACTLY whatever the order — a dropped tail column, a doubled block of data points, a row written to the wrong place is a whole-number error.  The API tests reach these
kernels only behind a fit, at rel 1e-8 (fp64) / 1e-4 (fp32).

Small integers ([−3, 3]) are exact in fp32 arithmetic too, so they cannot tell an fp64 accumulator from a float one; the `wide` cases multiply them by 4097 = 2¹² + 1:
a square or product then needs 25 to 28 bits — exact in the fp64 fused multiply-adds the kernels promise, not in float.

What the contract says is not read holds NaN (columns beyond ncols of Y, b and By; rows of Y outside the launch); rows of cacc / rowss outside the launch and the Cacc rows
of By's zero rows hold a sentinel and must come back bit-identical."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import unit_helpers as uh  # noqa: E402
from tests.unit_helpers import P, SENTINEL, bits, entry  # noqa: E402

DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]
WIDE = 4097  # 2**12 + 1


@pytest.fixture(scope="module")
def lib(agp):
    return agp._lib.load()


@pytest.fixture(scope="module")
def h(ctx):
    return ctx.handle


def ints(g, lo, hi, shape, dtype, mult=1):
    return (torch.randint(lo, hi + 1, shape, device="cuda", generator=g) * mult).to(dtype)


def ystats_exact(lib, h, dtype, ncols, row_lo, mult):
    """rowss[r] += Σ_c Y[r][c]², cacc[r] −= Σ_c Y[r][c]·b[c] for the rows [row_lo, row_lo + 5) of a Y with 3 more rows behind them"""
    from abstractgps_jl_amd._lib import check

    e = 16 // torch.empty(0, dtype=dtype).element_size()
    nrows, total = 5, row_lo + 5 + 3
    ldy = (ncols + e - 1) // e * e + e  # 16-byte rows, at least one column of padding
    g = torch.Generator(device="cuda").manual_seed(1000 * ncols + row_lo + mult)
    Y = ints(g, -3, 3, (total, ldy), dtype, mult)
    b = ints(g, -3, 3, (ldy,), dtype, mult)
    Y[:, ncols:] = float("nan")
    b[ncols:] = float("nan")
    Y[:row_lo] = float("nan")
    Y[row_lo + nrows:] = float("nan")
    cacc0 = ints(g, -64, 64, (total,), torch.float64)
    rowss0 = ints(g, -64, 64, (total,), torch.float64)
    live = torch.zeros(total, dtype=torch.bool, device="cuda")
    live[row_lo:row_lo + nrows] = True
    cacc0[~live] = SENTINEL
    rowss0[~live] = SENTINEL
    cacc, rowss = cacc0.clone(), rowss0.clone()
    torch.cuda.synchronize()
    check(entry(lib, "gpd_ystats", dtype)(h, P(Y), ldy, ncols, P(b), row_lo, nrows, P(cacc), P(rowss)))
    uh.sync(lib, h)
    Yd, bd = Y[live, :ncols].double(), b[:ncols].double()
    assert torch.equal(rowss[live], rowss0[live] + (Yd * Yd).sum(1)), ("ystats_kernel rowss", ncols, row_lo, mult)
    assert torch.equal(cacc[live], cacc0[live] - Yd @ bd), ("ystats_kernel cacc", ncols, row_lo, mult)
    assert torch.equal(bits(rowss)[~live], bits(rowss0)[~live]) and torch.equal(bits(cacc)[~live], bits(cacc0)[~live]), ("ystats_kernel: a row outside the launch changed", ncols)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ncols", [1, 3, 4, 5, 1023, 1024, 1027, 2051])
def test_ystats_exact(lib, h, dtype, ncols):
    """the nc4 vector body (4 columns per thread and pass), its scalar tail, and more than one 1024-column pass; row_lo 0 and 7"""
    for row_lo in (0, 7):
        ystats_exact(lib, h, dtype, ncols, row_lo, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ncols", [5, 1027, 2051])
def test_ystats_exact_on_integers_float_cannot_hold(lib, h, dtype, ncols):
    """multiples of 4097: Y² and Y·b need more than 24 bits, the sums stay below 9·4097²·2051 < 2³⁹ — exact in fp64 accumulators only"""
    ystats_exact(lib, h, dtype, ncols, 7, WIDE)


def ystats_cols_exact(lib, h, dtype, ncols, rows, sb, row_lo, mult):
    """rowss[r] += Σ_c Y[r][c]², Cacc[s][r] −= Σ_c Y[r][c]·By[s][c] for r in [row_lo, row_lo + rows), s < 16·sb; By's rows beyond S = 16·sb − 5 are zero.  Then the
    same call with one column of By changed: the other columns keep their bits."""
    from abstractgps_jl_amd._lib import check

    e = 16 // torch.empty(0, dtype=dtype).element_size()
    total, S, ldc = row_lo + rows + 4, 16 * sb - 5, row_lo + rows + 8  # ldc > rows
    ldy = ldb = ncols + e
    g = torch.Generator(device="cuda").manual_seed(ncols + 100 * rows + 10 * sb + row_lo + mult)
    Y = ints(g, -3, 3, (total, ldy), dtype, mult)
    By = ints(g, -3, 3, (16 * sb, ldb), dtype, mult)
    By[S:] = 0
    Y[:, ncols:] = float("nan")
    By[:, ncols:] = float("nan")
    Y[:row_lo] = float("nan")
    Y[row_lo + rows:] = float("nan")
    live = torch.zeros(ldc, dtype=torch.bool, device="cuda")
    live[row_lo:row_lo + rows] = True
    C0 = ints(g, -64, 64, (16 * sb, ldc), torch.float64)
    C0[:, ~live] = SENTINEL
    C0[S:] = SENTINEL  # −= 0 leaves the value as it is
    rowss0 = ints(g, -64, 64, (ldc,), torch.float64)
    rowss0[~live] = SENTINEL
    fn = entry(lib, "gpd_ystats_cols", dtype)
    form = f"ystats_cols_kernel<RT={2 if rows % 32 == 0 else 1}>"

    def run(Bm):
        Cm, rs = C0.clone(), rowss0.clone()
        torch.cuda.synchronize()
        check(fn(h, P(Y), ldy, ncols, P(Bm), ldb, sb, row_lo, rows, P(Cm), ldc, P(rs)))
        uh.sync(lib, h)
        return Cm, rs

    Cm, rs = run(By)
    Yd = Y[row_lo:row_lo + rows, :ncols].double()
    want = C0.clone()
    want[:S, live] -= By[:S, :ncols].double() @ Yd.T
    tag = (form, ncols, rows, sb, row_lo, mult)
    assert torch.equal(rs[live], rowss0[live] + (Yd * Yd).sum(1)), (tag, "rowss")
    assert torch.equal(Cm[:S][:, live], want[:S][:, live]), (tag, "Cacc")
    assert torch.equal(bits(rs)[~live], bits(rowss0)[~live]), (tag, "a rowss entry outside the launch changed")
    assert torch.equal(bits(Cm)[:, ~live], bits(C0)[:, ~live]), (tag, "a Cacc row outside the launch changed")
    assert torch.equal(bits(Cm)[S:], bits(C0)[S:]), (tag, "a zero row of By changed its Cacc row")
    s0 = S // 2
    By2 = By.clone()
    By2[s0, :ncols] = ints(g, -3, 3, (ncols,), dtype, mult)
    Cm2, rs2 = run(By2)
    others = torch.arange(16 * sb, device="cuda") != s0
    assert torch.equal(bits(Cm2)[others], bits(Cm)[others]) and torch.equal(bits(rs2), bits(rs)), (tag, "another column's bits depend on By's column", s0)
    assert torch.equal(Cm2[s0, live], C0[s0, live] - Yd @ By2[s0, :ncols].double()), (tag, "the changed column")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows", [16, 32, 48])
@pytest.mark.parametrize("sb", [1, 2, 8])
def test_ystats_cols_exact(lib, h, dtype, rows, sb):
    """rows = 16 and 48 are accepted by the 16-row form only (RT = 1), 32 runs the 32-row form the fit launches (RT = 2); ncols = one MFMA pass of the four waves
    (16·VEC), 128, and 2048 + 128 (several passes per wave)"""
    e = 16 // torch.empty(0, dtype=dtype).element_size()
    for ncols in (16 * e, 128, 2048 + 128):
        for row_lo in (0, 32):
            ystats_cols_exact(lib, h, dtype, ncols, rows, sb, row_lo, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows", [32, 48])
def test_ystats_cols_exact_on_integers_float_cannot_hold(lib, h, dtype, rows):
    ystats_cols_exact(lib, h, dtype, 2048 + 128, rows, 2, 32, WIDE)
