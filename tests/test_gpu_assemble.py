"""GPU: gpd_assemble / gpd_assemble_f32 — the tiles of K + Σy filled through the block-cyclic GridMap — against the oracle's kernel matrix on the same values.
It is the only direct handle on the index arithmetic the multi-device driver relies on (local tile -> global tile, noise on the GLOBAL diagonal only, identity
padding, tiles above the global diagonal skipped), and on kmat_kernel<T, DR> in both element types and all four instances (D <= 4 / 8 / 16 row forms, the
accumulate form; "kmat_rows" = 0 forces the last).  Bounds: tests/unit_helpers.py assemble_bound.  Each call prints `RATIO <case> <max error / bound>`."""
import functools

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import unit_helpers as uh  # noqa: E402

DTYPES = {"f64": torch.float64, "f32": torch.float32}


@pytest.fixture(scope="module")
def lib(agp):
    return agp._lib.load()


@pytest.fixture(scope="module")
def h(ctx):
    return ctx.handle


@functools.lru_cache(maxsize=4)
def _problem(dt, kind, d, n_valid, n_pad):
    return uh.assemble_problem(DTYPES[dt], kind, d, n_valid, n_pad)


@pytest.mark.parametrize("d", uh.ASSEMBLE_D)
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_assemble_values(lib, h, dt, kind, d):
    """every kernel kind at the instance boundaries of launch_kmat, row form and accumulate form, full and lower: interior tiles, the diagonal tiles with the noise
    vector, a partly padded tile (n_valid = 475 is not a multiple of 128) and a wholly padded one"""
    n_valid, n_pad = 475, 640
    prob = _problem(dt, kind, d, n_valid, n_pad)
    for rows in (1, 0):
        with uh.params(lib, h, kmat_rows=rows):  # process-wide: put back whatever happens
            for lower in (0, 1):
                uh.assemble_check(lib, h, DTYPES[dt], kind, d, prob, n_valid, n_pad, 1, 1, 0, 0, 1, lower,
                                  f"assemble[{dt},kind={kind},D={d},kmat_rows={rows},lower={lower}]")


@pytest.mark.parametrize("lower", [0, 1])
@pytest.mark.parametrize("tb", [1, 2])
@pytest.mark.parametrize("Pg,Qg", [(1, 1), (2, 2), (2, 3)])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_assemble_block_cyclic_grid(lib, h, dt, Pg, Qg, tb, lower):
    """every rank (p, q) of the process grid assembles its local tiles of ONE global matrix (12 × 12 tiles of 128, n_valid = 1371): local tile (t_r, t_c) must hold
    the global tile the header's formula names, the noise must land on global-diagonal elements only (a local diagonal tile of an off-diagonal rank is not one),
    padding rows are identity rows, and with `lower` the tiles strictly above the global diagonal keep their sentinel"""
    kind, d, n_valid, n_pad = 3, 3, 1371, 1536
    prob = _problem(dt, kind, d, n_valid, n_pad)
    for p in range(Pg):
        for q in range(Qg):
            uh.assemble_check(lib, h, DTYPES[dt], kind, d, prob, n_valid, n_pad, Pg, Qg, p, q, tb, lower,
                              f"assemble_grid[{dt},P={Pg},Q={Qg},p={p},q={q},tb={tb},lower={lower}]")
