"""CPU: gp_vfe_joint_batch is declared, exported and bound; the argument errors of its test side are reported before the handle is looked at."""
import ctypes

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests.test_vfe_batch_cpu import _problem


def test_symbol_is_declared_exported_and_bound():
    assert "gp_vfe_joint_batch" in agp._lib.header_functions() and "gp_vfe_joint_batch" in agp._lib.PROTOTYPES
    assert hasattr(agp._lib.load(), "gp_vfe_joint_batch") and agp._lib.load().gp_abi_version() == 4
    assert len(agp._lib.PROTOTYPES["gp_vfe_joint_batch"][1]) == 28
    lim = agp._lib.vfe_joint_batch_limits()
    assert lim["MAX_N"] > 0 and 0 < lim["MAX_NS"] <= 2048
    for name in ("approx_joint_batch", "approx_mean_and_cov_batch", "approx_logpdf_heldout_batch", "approx_rand_batch"):
        assert getattr(agp, name) is getattr(agp.api, name)


# (nxs, xs given, what, nsamp, which of mean / cov / ys / hlogpdf / xi / samples are given) -> the argument the library names; nb = 2 and no handle.  The last
# two rows have a valid test side (the arrays of a bit not asked for are not read, nsamp = 0 draws nothing) and get as far as the handle.
@pytest.mark.parametrize("nxs,xs,what,nsamp,given,arg", [
    (3, True, 29, 1, "mcyhxs", 14), (1, False, 29, 1, "mcyhxs", 15), (2, True, 0, 1, "mcyhxs", 18), (2, True, 2, 1, "mcyhxs", 18), (2, True, 32, 1, "mcyhxs", 18),
    (1, True, 29, 1, "cyhxs", 19), (1, True, 29, 1, "myhxs", 20), (2, True, 29, 1, "mchxs", 21), (2, True, 29, 1, "mcyxs", 22), (2, True, 29, -1, "mcyhxs", 23),
    (2, True, 29, 1, "mcyhs", 24), (2, True, 29, 1, "mcyhx", 25), (2, True, 8, 1, "yh", 1), (1, True, 21, 0, "mc", 1)])
def test_test_side_errors_need_no_device(nxs, xs, what, nsamp, given, arg):
    pts, arr, hl = (agp._lib.gp_points * 2)(), (ctypes.c_void_p * 2)(), (ctypes.c_double * 2)()
    g = lambda c, v: v if c in given else None
    rc = agp._lib.load().gp_vfe_joint_batch(None, 2, None, 2, None, 2, None, None, None, None, 2, None, None, nxs, pts if xs else None, None, None, what,
                                            g("m", arr), g("c", arr), g("y", arr), g("h", ctypes.addressof(hl)), nsamp, g("x", arr), g("s", arr), None, None, None)
    assert rc == -arg and f"argument {arg}" in agp._lib.load().gp_last_error().decode()


def test_python_checks_come_before_any_device_work():
    a, fx, y = _problem()
    a2, fx2, y2 = _problem(seed=1)
    xs = np.linspace(0, 3, 5)
    for what in (0, 2, 32):
        with pytest.raises(ValueError, match="what"):
            agp.approx_joint_batch([a, a2], [fx, fx2], [y, y2], xs, what=what)
    with pytest.raises(ValueError, match="ys_heldout"):
        agp.approx_joint_batch([a, a2], [fx, fx2], [y, y2], xs, what=8)
    with pytest.raises(ValueError, match="xi"):
        agp.approx_joint_batch([a, a2], [fx, fx2], [y, y2], xs, what=16)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.approx_joint_batch([a, a2], [fx, fx2], [y, y2], [xs, xs, xs])
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.approx_logpdf_heldout_batch([a, a2], [fx, fx2], [y, y2], xs, [np.zeros(5), np.zeros(4)])
    with pytest.raises(ValueError):
        agp.approx_joint_batch([a], [fx], [y], xs, on_error="ignore")
    assert agp.approx_joint_batch([], [], [], []) == []
    quads, obj = agp.approx_joint_batch([], [], [], [], return_objective=True)
    assert quads == [] and obj.shape == (0,)
