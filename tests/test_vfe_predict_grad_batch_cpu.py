"""CPU: gp_vfe_predict_grad_batch is declared, exported and bound; the argument errors of its test side are reported before the handle is looked at."""
import ctypes

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests.test_vfe_batch_cpu import _problem


def test_symbol_is_declared_exported_and_bound():
    assert "gp_vfe_predict_grad_batch" in agp._lib.header_functions() and "gp_vfe_predict_grad_batch" in agp._lib.PROTOTYPES
    assert hasattr(agp._lib.load(), "gp_vfe_predict_grad_batch") and agp._lib.load().gp_abi_version() == 4
    assert len(agp._lib.PROTOTYPES["gp_vfe_predict_grad_batch"][1]) == 23
    assert agp._lib.vfe_predict_grad_batch_max_n() > 0
    assert agp.approx_mean_and_var_grad_batch is agp.api.approx_mean_and_var_grad_batch


# (nxs, xs given, what, which of mean / var / dmean / dvar are given) -> the argument the library names; nb = 2 and no handle.  The last two rows have a valid
# test side (one array of a side is enough, those of a side not asked for are not read) and get as far as the handle.
@pytest.mark.parametrize("nxs,xs,what,given,arg", [(3, True, 3, "mvMV", 14), (1, False, 3, "mvMV", 15), (2, True, 0, "mvMV", 17), (2, True, 4, "mvMV", 17),
                                                   (1, True, 1, "vV", 18), (1, True, 3, "mM", 19), (2, True, 3, "MV", 1), (2, True, 2, "v", 1)])
def test_test_side_errors_need_no_device(nxs, xs, what, given, arg):
    pts, outs = (agp._lib.gp_points * 2)(), (ctypes.c_void_p * 2)()
    rc = agp._lib.load().gp_vfe_predict_grad_batch(None, 2, None, 2, None, 2, None, None, None, None, 2, None, None, nxs, pts if xs else None, None, what,
                                                   *[outs if c in given else None for c in "mvMV"], None, None)
    assert rc == -arg and f"argument {arg}" in agp._lib.load().gp_last_error().decode()


def test_python_checks_come_before_any_device_work():
    a, fx, y = _problem()
    a2, fx2, y2 = _problem(seed=1)
    xs = np.linspace(0, 3, 5)
    for what in (0, 4):
        with pytest.raises(ValueError, match="what"):
            agp.approx_mean_and_var_grad_batch([a, a2], [fx, fx2], [y, y2], xs, what=what)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.approx_mean_and_var_grad_batch([a, a2], [fx, fx2], [y, y2], [xs, xs, xs])
    with pytest.raises(ValueError, match="mean_grads"):
        agp.approx_mean_and_var_grad_batch([a, a2], [fx, fx2], [y, y2], xs, mean_grads=[None])
    with pytest.raises(ValueError):
        agp.approx_mean_and_var_grad_batch([a], [fx], [y], xs, on_error="ignore")
    assert agp.approx_mean_and_var_grad_batch([], [], [], []) == []
    quads, obj = agp.approx_mean_and_var_grad_batch([], [], [], [], return_objective=True)
    assert quads == [] and obj.shape == (0,)
