"""CPU: gp_vfe_batch is declared, exported and bound; the context-free half of elbo_batch (checks, grouping, shared-input detection, marshalling)."""
import numpy as np
import pytest

import abstractgps_jl_amd as agp


def _problem(n=12, m=4, seed=0, kernel=None, sigma2=0.1, x=None):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 3, n) if x is None else x
    f = agp.GP(kernel or 1.3 * agp.SqExponentialKernel())
    return agp.VFE(f(x[:m] + 0.01, 1e-4)), f(x, sigma2), np.sin(x)


def test_symbol_is_declared_exported_and_bound():
    assert "gp_vfe_batch" in agp._lib.header_functions() and "gp_vfe_batch" in agp._lib.PROTOTYPES
    assert hasattr(agp._lib.load(), "gp_vfe_batch") and agp._lib.load().gp_abi_version() == 4
    assert len(agp._lib.PROTOTYPES["gp_vfe_batch"][1]) == 17
    lim = agp._lib.vfe_batch_limits()
    assert lim["MAX_M"] == 128 and lim["SEG"] % 64 == 0
    assert agp.elbo_batch is agp.api.elbo_batch and agp.approx_log_evidence_batch is agp.api.approx_log_evidence_batch


def test_argument_errors_come_before_any_device_work():
    a, fx, y = _problem()
    a2, fx2, y2 = _problem(seed=1)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.elbo_batch([a, a2], [fx, fx2, fx], [y, y2])
    with pytest.raises(ValueError, match="DimensionMismatch"):
        agp.elbo_batch([a, a2], [fx, fx2], [y, y2, y])
    with pytest.raises(ValueError, match="DimensionMismatch"):  # wrong len(y)
        agp.elbo_batch([a, a2], [fx, fx2], [y, y2[:-1]])
    with pytest.raises(AssertionError):  # vfe.fz.f === fx.f
        agp.elbo_batch([a, a], [fx, fx2], [y, y2])
    comp = _problem(kernel=agp.SqExponentialKernel() + agp.Matern32Kernel())
    with pytest.raises(NotImplementedError):
        agp.elbo_batch([a, comp[0]], [fx, comp[1]], [y, comp[2]])
    dense = _problem(sigma2=0.1 * np.eye(12))
    with pytest.raises(NotImplementedError):
        agp.elbo_batch([dense[0]], [dense[1]], [dense[2]])
    with pytest.raises(ValueError):
        agp.elbo_batch([a], [fx], [y], on_error="ignore")
    assert agp.elbo_batch([], [], []).shape == (0,)
    obj, alphas, m_eps = agp.elbo_batch([], [], [], return_alpha=True, return_m_eps=True)
    assert obj.shape == (0,) and alphas == [] and m_eps == []


def test_shared_inputs_are_sent_once_and_the_arguments_line_up():
    x = np.linspace(0, 3, 12)
    y = np.cos(x)
    z = x[::3].copy()
    fs = [agp.GP(v * agp.Matern52Kernel() @ agp.ScaleTransform(0.5 + 0.1 * i)) for i, v in enumerate([1.0, 1.5, 2.0])]
    approxs = [(agp.DTC if i == 1 else agp.VFE)(f(z, 1e-4 * (i + 1))) for i, f in enumerate(fs)]
    (g,) = agp.api._vfe_batch_groups(approxs, [f(x, 0.1) for f in fs], [y])  # one y for all
    call = agp.api._vfe_batch_marshal(g, True, False)
    assert (call.nb, call.nx, call.nz, call.ny) == (3, 1, 1, 1)
    nb, karr, nx, pts, nz, zs, narr, jit, marr, ny, yarr, kinds, out, info, aarr, earr = call.args
    assert (len(pts), len(zs), len(yarr), len(karr), len(narr)) == (1, 1, 1, 3, 3) and zs[0].n == 4 and pts[0].n == 12
    assert list(jit) == pytest.approx([1e-4, 2e-4, 3e-4]) and list(kinds) == [0, 1, 0] and marr is None and earr is None
    assert [v.shape for v in call.alphas] == [(4,)] * 3 and call.m_eps is None
    # equal values in distinct objects are NOT shared
    (g2,) = agp.api._vfe_batch_groups([agp.VFE(f(z.copy(), 1e-4)) for f in fs], [f(x.copy(), 0.1) for f in fs], [y.copy() for _ in fs])
    assert (g2.nx, g2.nxs, g2.ny) == (3, 3, 3)

