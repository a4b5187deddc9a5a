"""CPU: gp_vfe_grad_batch is declared, exported and bound; the argument checks of elbo_and_grad_batch come before any device work."""
import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests.test_vfe_batch_cpu import _problem


def test_symbol_is_declared_exported_and_bound():
    assert "gp_vfe_grad_batch" in agp._lib.header_functions() and "gp_vfe_grad_batch" in agp._lib.PROTOTYPES
    assert hasattr(agp._lib.load(), "gp_vfe_grad_batch") and agp._lib.load().gp_abi_version() == 4
    assert len(agp._lib.PROTOTYPES["gp_vfe_grad_batch"][1]) == 21
    assert "#define GPMI355_VFE_GRAD_BATCH_MAX_N " in agp._lib.HEADER.read_text()
    assert agp.elbo_and_grad_batch is agp.api.elbo_and_grad_batch


def test_argument_errors_come_before_any_device_work():
    a, fx, y = _problem()
    a2, fx2, y2 = _problem(seed=1)
    for fxs, ys in (([fx, fx2, fx], [y, y2]), ([fx, fx2], [y, y2, y]), ([fx, fx2], [y, y2[:-1]])):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            agp.elbo_and_grad_batch([a, a2], fxs, ys)
    comp = _problem(kernel=agp.SqExponentialKernel() + agp.Matern32Kernel())
    dense = _problem(sigma2=0.1 * np.eye(12))
    for extra in (comp, dense):
        with pytest.raises(NotImplementedError):
            agp.elbo_and_grad_batch([a, extra[0]], [fx, extra[1]], [y, extra[2]])
    with pytest.raises(ValueError):
        agp.elbo_and_grad_batch([a], [fx], [y], on_error="ignore")
    with pytest.raises(TypeError):
        agp.elbo_and_grad_batch([a], [fx], [y], wrt_x=1)
    obj, grads = agp.elbo_and_grad_batch([], [], [])
    assert obj.shape == (0,) and grads == []
