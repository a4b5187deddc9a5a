"""GPU: U1 — the update of the next panel's columns — with its rectangle below the panel's square as one Strassen block in four grouped launches (ctx parameter
"strassen_u1_min_rows", "strassen_u1_min_k"; csrc/bulk_plan.hpp u1_plan_build, csrc/gpmi355.hip potrf_full_la), and the third tier of the automatic panel width ("nb_huge",
"nb_huge_min_n").

SE, D = 3, σ² = 0.01 on o.synth_inputs, the sizes of tests/test_gpu_schedule_matrix.py at nb = 512 with the two U1 floors and both Strassen floors at 256:
    N = 2 048   rectangles of 1 024 and 512 rows: whole quadrants
    N = 1 920   rectangles of 896 and 384 rows: a 128-row remainder strip below the block; the last panel 384 columns wide
    N = 1 801   the same panels with 119 identity-padded rows
The third panel step has no rectangle (the next panel is the last) and keeps the single launch.  Every fit takes milliseconds, deterministic = 1 throughout.

(d) compares the factors of the two forms through the reference tests/test_gpu_strassen.py uses for one product — a host long-double product, max-abs error over
max-abs reference, the Strassen form allowed four times the classical error.  A long-double Cholesky of these sizes would take half a minute, so the product is
the one a factor has to reproduce: rows of UᵀU against the same rows of K + σ²I formed in long double from the inputs, on 48 fixed rows of the lower half — the
rows every Strassen block of U1 wrote.

Every context here is the test's own and is closed in `finally`; the default context is never touched."""
import functools

import numpy as np
import pytest

from oracle import gp_oracle as o

pytestmark = pytest.mark.gpu

NB = 512
BASE = dict(nb=NB, strassen_min_rows=256, strassen_group=1, strassen_group_min_rows=256, strassen_u1_min_rows=256, strassen_u1_min_k=256, deterministic=1, time_kernels=1)
CLASSICAL_U1 = dict(strassen_u1_min_rows=0)
TWO = dict(lookahead=1, lookahead_min_n=0)
SIZES = [2048, 1920, 1801]
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def _case(n):
    """inputs of one size and the oracle's fit on the host; read-only, shared by every test"""
    x, y = o.synth_inputs(n, 3, 100 + n)
    lp, post = o.logpdf_and_posterior(o.FiniteGP(o.GP(o.Kernel(o.SE)), x, 0.01), y)
    d = dict(n=n, x=x, y=y, lp=lp, alpha=post.alpha)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _open(agp, **kw):
    ctx = agp.Context(0)
    try:
        for k, v in {**BASE, **kw}.items():
            ctx.set_param(k, v)
            assert ctx.get_param(k) == v, (k, v, ctx.get_param(k))
    except BaseException:
        ctx.close()
        raise
    return ctx


def _fit(agp, ctx, d):
    post = agp.posterior(agp.GP(agp.SqExponentialKernel(), ctx=ctx)(agp.RowVecs(d["x"]), 0.01), d["y"])
    r = dict(lp=np.float64(post.logpdf_value), alpha=np.array(post.data.alpha), U=np.array(post.data.C.U), tm=ctx.timings())
    post.data.C.free()
    return r


_memo = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_shared_results():
    yield
    _memo.clear()
    _case.cache_clear()


def _run(agp, n, **kw):
    """the fit of size n on a FRESH context with BASE + kw, once per module (its results are compared, never changed)"""
    key = (n, tuple(sorted(kw.items())))
    if key not in _memo:
        ctx = _open(agp, **kw)
        try:
            _memo[key] = _fit(agp, ctx, _case(n))
        finally:
            ctx.close()
    return _memo[key]


def _same(a, b, what):
    bad = [k for k in ("lp", "alpha", "U") if not np.array_equal(a[k], b[k])]
    for k in bad:
        print(f"U1 {what}: {k} differs, max abs {np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k]))):.3e}", flush=True)
    assert not bad, f"{what}: not the same bits in {bad}"


def _steps_in_the_form(n):
    """panel steps whose rectangle has the shape, by the rule written out again: whole 256-row quadrants of the rows below the next panel, at least the floor (256),
    a next panel of whole 256-column quadrants, K a multiple of 32"""
    np_, steps = -(-n // 128) * 128, 0
    for k in range(0, np_, NB):
        k1 = k + min(NB, np_ - k)
        if k1 >= np_:
            break
        k2 = k1 + min(NB, np_ - k1)
        bs = (np_ - k2) // 256 * 256
        steps += int(bs >= 256 and (k2 - k1) % 256 == 0 and (k1 - k) % 32 == 0)
    return steps


# ---- (a) the form ran ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_the_form_adds_three_launches_per_step_with_the_shape_and_removes_flops(agp, n):
    form, classical = _run(agp, n)["tm"], _run(agp, n, **CLASSICAL_U1)["tm"]
    steps = _steps_in_the_form(n)
    print(f"U1 N={n}: steps in the form {steps}; launches {classical['gemm_launches']} -> {form['gemm_launches']}; flops {classical['gemm_flops']:.6e} -> {form['gemm_flops']:.6e}", flush=True)
    assert steps == 2
    assert form["gemm_launches"] == classical["gemm_launches"] + 3 * steps  # four grouped launches for one
    assert form["gemm_flops"] < classical["gemm_flops"]                    # seven half-size products for eight


# ---- (b) against the oracle ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", ["one", "two"])
@pytest.mark.parametrize("n", SIZES)
def test_logpdf_and_alpha_against_the_oracle(agp, n, sched):
    d, r = _case(n), _run(agp, n, **(TWO if sched == "two" else {}))
    e_lp = abs(r["lp"] - d["lp"]) / abs(d["lp"])
    e_a = float(np.linalg.norm(r["alpha"] - d["alpha"]) / np.linalg.norm(d["alpha"]))
    print(f"U1 N={n} {sched}-stream: logpdf rel {e_lp:.2e} alpha rel {e_a:.2e}", flush=True)
    assert np.all(np.isfinite(r["alpha"])) and np.all(np.isfinite(r["U"]))
    assert e_lp <= 1e-10 and e_a <= 1e-8


# ---- (c) the same bits -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_same_bits_on_one_stream_and_on_two(agp, n):
    _same(_run(agp, n), _run(agp, n, **TWO), f"N={n}: one stream vs two")


@pytest.mark.parametrize("n", SIZES)
def test_same_bits_with_poisoned_blocks(agp, n):
    """alloc_poison = 1 fills the workspace of sum panels and the table block with 0xFF bytes before the fit writes them"""
    _same(_run(agp, n, **TWO), _run(agp, n, alloc_poison=1, **TWO), f"N={n}: alloc_poison 0 vs 1")


@pytest.mark.parametrize("n", SIZES)
def test_same_bits_on_repetition(agp, n):
    """two more fits on one context: the second reuses the workspace, the table block and the page-locked staging"""
    ctx = _open(agp, **TWO)
    try:
        got = [_fit(agp, ctx, _case(n)) for _ in range(2)]
    finally:
        ctx.close()
    for i, r in enumerate(got):
        _same(r, _run(agp, n, **TWO), f"N={n}: fit {i} on a reused context vs a fresh one")


# ---- (d) the factor against the U1-classical fit ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows_ref(n):
    """48 fixed rows of the lower half of K + σ²I in long double from the inputs: (rows, list of row vectors [0 .. i])"""
    x = _case(n)["x"].astype(LD)
    rows = np.linspace(n // 2, n - 1, 48).astype(int)
    ref = []
    for i in rows:
        d2 = ((x[i][None, :] - x[:i + 1]) ** 2).sum(axis=1)
        a = np.exp(-LD(0.5) * d2)
        a[i] += LD(0.01)  # the double the device adds
        ref.append(a)
    return rows, ref


def _factor_err(n, U):
    """max |(UᵀU)[i, :i+1] − (K + σ²I)[i, :i+1]| over the sampled rows, over the largest reference entry: U is upper, so row i of UᵀU is U[:i+1, i]ᵀ U[:i+1, :i+1]"""
    rows, ref = _rows_ref(n)
    err, scale, Ul = LD(0), LD(0), np.triu(U).astype(LD)
    for i, a in zip(rows, ref):
        err = max(err, np.max(np.abs(Ul[:i + 1, i] @ Ul[:i + 1, :i + 1] - a)))
        scale = max(scale, np.max(np.abs(a)))
    return float(err / scale)


@pytest.mark.parametrize("n", SIZES)
def test_factor_error_is_within_four_times_the_classical_u1_fits(agp, n):
    """the bound of tests/test_gpu_strassen.py::test_gaussian_product_error_is_within_four_times_the_classical_error for one level of Strassen, on the product a
    factor has to reproduce.  Both figures are printed."""
    e_form, e_cl = _factor_err(n, _run(agp, n)["U"][:n, :n]), _factor_err(n, _run(agp, n, **CLASSICAL_U1)["U"][:n, :n])
    print(f"U1 N={n}: max|UtU - A| / max|A| on 48 rows: classical U1 {e_cl:.3e} Strassen U1 {e_form:.3e} ratio {e_form / e_cl:.2f}", flush=True)
    assert e_form <= 4 * e_cl, (e_form, e_cl)
    assert not np.array_equal(_run(agp, n)["U"], _run(agp, n, **CLASSICAL_U1)["U"])  # the two forms are different computations


# ---- (e) the third tier of the automatic width --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_nb_huge_applies_from_its_floor_on_and_not_below_it(agp, n):
    """nb = −1, nb_huge = 512: with the floor below N the bits of the explicit nb = 512 fit; with the floor above N the bits of today's automatic fit (nb_small on one
    stream at these sizes), which another width makes another computation"""
    today = _run(agp, n, nb=-1)
    _same(_run(agp, n, nb=-1, nb_huge=NB, nb_huge_min_n=1024), _run(agp, n), f"N={n}: tier floor below N vs nb = {NB}")
    _same(_run(agp, n, nb=-1, nb_huge=NB, nb_huge_min_n=4096), today, f"N={n}: tier floor above N vs today's automatic fit")
    assert today["tm"]["gemm_launches"] != _run(agp, n)["tm"]["gemm_launches"]
