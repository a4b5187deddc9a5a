"""CPU: the context-free half of logpdf_batch (grouping, shared-input detection, marshalling, merging), the exported batch symbols, and the check that the
oracle is itself far inside the tolerances tests/test_gpu_batch.py uses."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import abstractgps_jl_amd as agp
from tests import batch_cases as bc

ROOT = Path(__file__).resolve().parent.parent


def _fx(n, seed, dtype=np.float64, kernel=None, x=None):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 3, size=n).astype(dtype) if x is None else x
    return agp.GP(kernel or 1.3 * agp.SqExponentialKernel())(x, 0.02), rng.standard_normal(n).astype(dtype)


def test_groups_keep_the_callers_order_and_split_by_dtype_and_kernel_form():
    comp = agp.SqExponentialKernel() + 0.5 * agp.Matern32Kernel()
    specs = [(5, np.float64, None), (7, np.float32, None), (4, np.float64, comp), (9, np.float64, None), (3, np.float32, None), (6, np.float64, comp)]
    pairs = [_fx(n, i, dt, k) for i, (n, dt, k) in enumerate(specs)]
    groups = agp.api._batch_groups([p[0] for p in pairs], [p[1] for p in pairs])
    assert [(g.dtype, g.composite, g.index) for g in groups] == [(np.float64, False, [0, 3]), (np.float32, False, [1, 4]), (np.float64, True, [2, 5])]
    assert all(g.nx == len(g.index) and g.ny == len(g.index) for g in groups)
    assert sorted(i for g in groups for i in g.index) == list(range(6))


def test_shared_inputs_are_detected_by_identity_and_marshalled_once():
    x = np.linspace(0, 3, 11)
    y = np.sin(x)
    ks = [v * agp.Matern52Kernel() @ agp.ScaleTransform(0.5 + 0.1 * i) for i, v in enumerate([1.0, 1.5, 2.0, 2.5])]
    fxs = [agp.GP(k)(x, 0.1) for k in ks]
    (g,) = agp.api._batch_groups(fxs, y)  # ONE vector for all
    assert (g.nx, g.ny, g.index) == (1, 1, [0, 1, 2, 3])
    call = agp.api._batch_marshal(g, return_alpha=True)
    assert (call.entry, call.nb, call.nx, call.ny) == ("gp_logpdf_batch", 4, 1, 1)
    nb, karr, nx, pts, narr, marr, ny, yarr, out, info, aarr = call.args
    assert (nb, nx, ny, len(pts), len(yarr), len(karr), len(narr), len(aarr)) == (4, 1, 1, 1, 1, 4, 4, 4)
    assert marr is None and pts[0].n == 11 and pts[0].layout == 0
    assert [karr[i].variance for i in range(4)] == [1.0, 1.5, 2.0, 2.5] and karr[2].scale[0] == pytest.approx(0.7)
    assert [a.shape for a in call.alphas] == [(11,)] * 4
    # equal values in distinct objects are NOT shared
    (g2,) = agp.api._batch_groups([agp.GP(k)(x.copy(), 0.1) for k in ks], [y.copy() for _ in ks])
    assert (g2.nx, g2.ny) == (4, 4)
    c2 = agp.api._batch_marshal(g2, return_alpha=False)
    assert len(c2.args[3]) == 4 and len(c2.args[7]) == 4 and c2.args[10] is None and c2.alphas is None


def test_marshal_packs_means_noise_forms_and_composite_descriptors():
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 2, size=(6, 3))
    comp = agp.SqExponentialKernel() @ agp.ARDTransform([0.5, 0.6, 0.7]) + 0.2 * agp.WhiteKernel()
    fxs = [agp.GP(0.4, comp)(agp.RowVecs(X), 0.1), agp.GP(comp)(agp.ColVecs(X.T.copy()), np.full(6, 0.2))]
    ys = [rng.standard_normal(6), rng.standard_normal(6)]
    (g,) = agp.api._batch_groups(fxs, ys)
    call = agp.api._batch_marshal(g, return_alpha=False)
    nb, karr, nx, pts, narr, marr, ny, yarr, out, info, aarr = call.args
    assert call.entry == "gp_logpdf_batch_sum" and (nb, nx, ny) == (2, 2, 2)
    assert karr[0].nterms == 2 and [pts[i].d for i in range(2)] == [3, 3] and [pts[i].n for i in range(2)] == [6, 6]
    assert [narr[i].kind for i in range(2)] == [0, 1] and narr[0].s == pytest.approx(0.1)
    assert marr[0] is not None and marr[1] is None
    m0 = np.ctypeslib.as_array(C.cast(marr[0], C.POINTER(C.c_double)), shape=(6,))
    assert np.array_equal(m0, np.full(6, 0.4))


def test_merge_restores_the_order_and_raises_with_the_index_of_the_first_failure():
    parts = [([0, 3], np.array([1.0, 4.0]), np.array([0, 0], dtype=np.int32), [np.array([1.0]), np.array([4.0, 4.0])]),
             ([1, 2, 4], np.array([2.0, np.nan, np.nan], dtype=np.float32), np.array([0, 7, 2], dtype=np.int32), [np.array([2.0]), np.array([np.nan]), np.array([np.nan])])]
    lp, al = agp.api._batch_merge(5, parts, True, "nan")
    assert lp.dtype == np.float64 and np.array_equal(lp[[0, 1, 3]], [1.0, 2.0, 4.0]) and np.isnan(lp[[2, 4]]).all()
    assert [a.shape[0] for a in al] == [1, 1, 1, 2, 1]
    with pytest.raises(agp.PosDefException) as e:
        agp.api._batch_merge(5, parts, False, "raise")
    assert (e.value.info, e.value.index) == (7, 2)
    only32 = agp.api._batch_merge(1, [([0], np.array([3.0], dtype=np.float32), np.array([0], dtype=np.int32), None)], False, "raise")
    assert only32.dtype == np.float32


def test_argument_checks_of_the_mirror_need_no_device():
    fx, y = _fx(5, 0)
    assert agp.logpdf_batch([], []).shape == (0,)
    lp, al = agp.logpdf_batch([], [], return_alpha=True)
    assert lp.shape == (0,) and al == []
    with pytest.raises(ValueError):
        agp.api._batch_groups([fx, fx], [y])
    with pytest.raises(ValueError):
        agp.api._batch_groups([fx], [y[:4]])
    with pytest.raises(TypeError):
        agp.api._batch_groups([object()], [y])
    with pytest.raises(ValueError):
        agp.logpdf_batch([fx], [y], on_error="ignore")


def test_both_batch_symbols_are_exported_and_the_constant_is_a_multiple_of_128(agp):
    lib = agp._lib.load()
    assert hasattr(lib, "gp_logpdf_batch") and hasattr(lib, "gp_logpdf_batch_sum")
    assert {"gp_logpdf_batch", "gp_logpdf_batch_sum"} <= set(agp._lib.header_functions())
    m = re.search(r"#define GPMI355_BATCH_MAX_N (\d+)", (ROOT / "include" / "gpmi355.h").read_text())
    assert m and int(m.group(1)) % 128 == 0 and int(m.group(1)) == agp._lib.batch_max_n()
    assert agp._lib.load().gp_abi_version() == 4


def test_the_oracle_is_far_inside_the_gpu_tolerances_on_the_ragged_cases():
    """What the GPU tests compare against: oracle.logpdf / posterior against SciPy's dpotrf on the same matrices, every case of the ragged batch.  The
    GPU bounds are 1e-10 (logpdf) and 1e-8 (α): the reference's own error has to be orders below them."""
    worst_lp = worst_a = worst_cond = 0.0
    for case in bc.ragged_cases():
        ofx = case["ofx"]
        m, Cm = bc.o.mean_and_cov(ofx)
        lp_h, a_h = bc.host_fit(Cm, case["y"] - m)
        lp_o, a_o = bc.oracle_fit(case)
        worst_lp = max(worst_lp, bc.lp_err(lp_o, lp_h))
        worst_a = max(worst_a, bc.vec_err(a_o, a_h))
        if case["n"] <= 600:
            worst_cond = max(worst_cond, float(np.linalg.cond(Cm)))
    print(f"oracle vs SciPy: logpdf {worst_lp:.1e}, alpha {worst_a:.1e}, cond <= {worst_cond:.1e}")
    assert worst_lp <= 1e-12 and worst_a <= 1e-11 and worst_cond <= 1e5
    cats = {key: {c[key] for c in bc.ragged_cases()} for key in ("kind", "tr", "d", "container", "noise", "mean")}
    assert cats == {"kind": {0, 1, 2, 3}, "tr": set(bc.TRANSFORMS), "d": {1, 3, 8}, "container": set(bc.CONTAINERS), "noise": set(bc.NOISES),
                    "mean": set(bc.MEANS)}
    assert set(bc.FIXED_SIZES) <= {c["n"] for c in bc.ragged_cases()} and len(bc.ragged_cases()) >= 32
