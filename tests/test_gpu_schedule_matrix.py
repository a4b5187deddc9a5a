"""GPU: the schedule of the headline fit (C4: N = 65 536) in miniature — the two-stream look-ahead of potrf_full_la TOGETHER with the Strassen form of the bulk
trailing updates, grouped into four gemm_nt_grp_kernel launches from tables uploaded before the first panel (csrc/gpmi355.hip potrf_full_la, PlanTables,
run_grouped, syrk_lower_split; csrc/bulk_plan.hpp), with carried right-hand-side rows below every update.

SE, D = 3, σ² = 0.01 on o.synth_inputs; nb = 256 and both Strassen floors at 256, so the bulk updates have side 1 536 … 512 (the shapes of
tests/test_gpu_strassen.py) and every fit takes milliseconds:
    N = 2 048   whole panels
    N = 1 920   the last panel 128 columns wide
    N = 1 801   n_valid inside a tile: 119 identity-padded rows
Forms of a bulk update: classical (strassen_min_rows = 0), per-block (strassen_group = 0), grouped.  Schedules: one stream ("lookahead_min_n" at its
default, far above these sizes) and two streams (lookahead = 1, lookahead_min_n = 0: every panel on the panel stream beside the update on the main stream).

References: oracle/gp_oracle.py, tests/composite_dx_ref.py host_fit and the host Cholesky of tests/test_gpu_dense_noise.py, each computed once.  Tolerances are
the project's: logpdf rel 1e-10, ‖α − α_ref‖ / ‖α_ref‖ <= 1e-8, max|U − U_ref| <= 1e-10; gradients as tests/test_gpu_parity.py::test_logpdf_grad_vs_oracle.

Under "deterministic" = 1 a tile's arithmetic does not depend on the stream its launch went to, every quadrant receives its products in one order, and the
leaves' Σ log L_ii additions are totally ordered: the forms and schedules are compared bit for bit.

Nothing the C ABI reports says which stream a launch ran on (gp_timings has no per-stream field; the per-launch record carries the stream but only the
GPMI_DUMP_GEMM print shows it), so that the panel stream was used is established by the parameters reading back as set and by `la` in potrf_full_la being a
function of exactly those parameters — not by a counter.  The Strassen and grouped paths do show: gemm_launches and gemm_flops under time_kernels = 1.

Every context here is the test's own and is closed in `finally`; the default context is never touched."""
import functools

import numpy as np
import pytest

from oracle import gp_oracle as o

pytestmark = pytest.mark.gpu

BASE = dict(nb=256, strassen_min_rows=256, strassen_group=1, strassen_group_min_rows=256)
FORMS = {"classical": dict(strassen_min_rows=0), "per-block": dict(strassen_group=0), "grouped": {}}
ONE, TWO = {}, dict(lookahead=1, lookahead_min_n=0)
SIZES = [2048, 1920, 1801]


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


@functools.lru_cache(maxsize=None)
def _case(n):
    """inputs of one size and (for the sizes that are compared with it) the oracle's fit; read-only, shared by every test"""
    x, y = o.synth_inputs(n, 3, 100 + n)
    Y = np.stack([y, np.cos(y), y * y - 1.0], axis=1)
    d = dict(n=n, x=x, y=y, Y=Y)
    if n in SIZES:
        ofx = o.FiniteGP(o.GP(o.Kernel(o.SE)), x, 0.01)
        lp, post = o.logpdf_and_posterior(ofx, y)
        d.update(lp=lp, alpha=post.alpha, U=post.U, lpY=o.logpdf(ofx, Y))
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _open(agp, **kw):
    """a context of the test's own with BASE and kw set — and read back: a parameter the library dropped or rounded would make the test prove nothing"""
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
    """posterior fit (logpdf, α, the whole factor U), the launch counters of that fit, and the three-column logpdf (carried rows below every update)"""
    f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
    post = agp.posterior(f(agp.RowVecs(d["x"]), 0.01), d["y"])
    r = dict(lp=np.float64(post.logpdf_value), alpha=np.array(post.data.alpha), U=np.array(post.data.C.U), tm=ctx.timings())
    post.data.C.free()
    r["lpY"] = np.array(agp.logpdf(f(agp.RowVecs(d["x"]), 0.01), d["Y"]))
    return r


_memo = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_shared_results():
    yield
    _memo.clear()
    _case.cache_clear()
    _dense_case.cache_clear()


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
    bad = [k for k in ("lp", "alpha", "U", "lpY") if not np.array_equal(a[k], b[k])]
    for k in bad:
        print(f"SCHED {what}: {k} differs, max abs {np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k]))):.3e}", flush=True)
    assert not bad, f"{what}: not the same bits in {bad}"


def _meets_oracle(r, d, what):
    e_lp = abs(r["lp"] - d["lp"]) / abs(d["lp"])
    e_a = _rel(r["alpha"], d["alpha"])
    e_u = float(np.max(np.abs(r["U"] - d["U"])))
    e_y = float(np.max(np.abs(r["lpY"] - d["lpY"]) / np.abs(d["lpY"])))
    print(f"SCHED {what} N={d['n']}: logpdf rel {e_lp:.2e} alpha rel {e_a:.2e} max|U-Uref| {e_u:.2e} logpdf(3 cols) rel {e_y:.2e}", flush=True)
    assert np.all(np.isfinite(r["alpha"])) and np.all(np.isfinite(r["U"]))
    assert e_lp <= 1e-10 and e_a <= 1e-8 and e_u <= 1e-10 and e_y <= 1e-10


# ---- 1. forms × schedules under "deterministic" -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_every_form_gives_the_same_bits_on_one_stream_and_on_two_and_grouped_equals_per_block(agp, n):
    """3 forms × 2 schedules, deterministic = 1, time_kernels = 1.  logpdf, α, the whole U and the three-column logpdf: each form the same bits on one stream and
    on two; grouped == per-block on two streams; every cell within the oracle tolerances.  That the forms ran: per-block has more GEMM launches than classical,
    grouped fewer than per-block, per-block and grouped count the same flops."""
    d = _case(n)
    cell = {(f, s): _run(agp, n, deterministic=1, time_kernels=1, **fk, **sk) for f, fk in FORMS.items() for s, sk in (("one", ONE), ("two", TWO))}
    for (f, s), r in cell.items():
        _meets_oracle(r, d, f"{f}/{s}-stream")
    for f in FORMS:
        _same(cell[f, "one"], cell[f, "two"], f"N={n} {f}: one stream vs two")
    _same(cell["grouped", "two"], cell["per-block", "two"], f"N={n} two streams: grouped vs per-block")
    for s in ("one", "two"):
        c, p, g = (cell[f, s]["tm"] for f in ("classical", "per-block", "grouped"))
        print(f"SCHED N={n} {s}-stream launches classical {c['gemm_launches']} per-block {p['gemm_launches']} grouped {g['gemm_launches']}; "
              f"flops {c['gemm_flops']:.6e} {p['gemm_flops']:.6e} {g['gemm_flops']:.6e}", flush=True)
        assert c["gemm_launches"] < g["gemm_launches"] < p["gemm_launches"]
        assert g["gemm_flops"] == p["gemm_flops"] < c["gemm_flops"]  # seven half-size products for eight
    for f in FORMS:  # the schedule moves launches between streams: it adds and removes none
        assert cell[f, "one"]["tm"]["gemm_launches"] == cell[f, "two"]["tm"]["gemm_launches"]
        assert cell[f, "one"]["tm"]["gemm_flops"] == cell[f, "two"]["tm"]["gemm_flops"]


# ---- 2. the automatic panel width ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2048, 1801])
def test_automatic_width_picks_nb_large_on_two_streams_and_nb_small_on_one(agp, n):
    """nb = −1 with nb_large = 256, nb_small = 512: at lookahead_min_n = 0 the fit is the explicit nb = 256 two-stream fit, at the default threshold the explicit
    nb = 512 one-stream fit — to the bit (deterministic), grouped updates in all four"""
    auto = dict(nb=-1, nb_large=256, nb_small=512, deterministic=1)
    _same(_run(agp, n, **auto, **TWO), _run(agp, n, deterministic=1, time_kernels=1, **TWO), f"N={n} automatic width, two streams vs nb = 256")
    wide = _run(agp, n, nb=512, deterministic=1)
    _same(_run(agp, n, **auto), wide, f"N={n} automatic width, one stream vs nb = 512")
    _meets_oracle(wide, _case(n), "nb=512 grouped/one-stream")
    assert not np.array_equal(wide["U"], _run(agp, n, deterministic=1, time_kernels=1, **TWO)["U"])  # the two widths are different computations


# ---- 3. "ldpad": the pad of every leading dimension and of the sum panels' row stride --------------------------------------------------------------------------------
@pytest.mark.parametrize("ldpad", [0, 48])
@pytest.mark.parametrize("n", [2048, 1801])
def test_ldpad_zero_and_48_on_the_grouped_two_stream_schedule(agp, n, ldpad):
    """default 32; 0 gives A and the sum panels power-of-two row strides at N = 2 048 (2 048 and 128 elements), 48 strides that are no multiple of 32.
    Each against the oracle and, under deterministic, bit-equal to its own per-block form."""
    g = _run(agp, n, ldpad=ldpad, deterministic=1, **TWO)
    _meets_oracle(g, _case(n), f"ldpad={ldpad} grouped/two-stream")
    _same(g, _run(agp, n, ldpad=ldpad, deterministic=1, strassen_group=0, **TWO), f"N={n} ldpad={ldpad}: grouped vs per-block")


# ---- 4. default mode: stream-K tails and atomics on ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sk", [{}, dict(sk_max_tiles=0)], ids=["stream-k", "sk_max_tiles0"])
@pytest.mark.parametrize("n", [2048, 1801])
def test_default_mode_grouped_two_stream_fits_twice_on_one_context(agp, n, sk):
    """deterministic = 0: stream-K tails on both streams (U1 and the in-panel updates; the grouped launches never take them); sk_max_tiles = 0 sends every
    launch to the tile kernel.  Two fits on one context — the second reuses the workspace, the table block and the page-locked staging — both within tolerance."""
    d = _case(n)
    ctx = _open(agp, deterministic=0, gemm_streamk=1, **sk, **TWO)
    try:
        for i in range(2):
            _meets_oracle(_fit(agp, ctx, d), d, f"default mode {sk} fit {i}")
    finally:
        ctx.close()


# ---- 5. one context, several sizes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [0, 1])
def test_context_reuse_across_sizes_gives_the_bits_of_a_fresh_context(agp, poison):
    """N = 1 024, 2 048, 1 024, 1 920 on one grouped two-stream deterministic context: the 2 048 fit has larger tables (the page-locked staging is reallocated),
    the others take workspace and table blocks of other sizes from the pool.  alloc_poison = 1 fills every block with 0xFF bytes first."""
    kw = dict(deterministic=1, **TWO)
    ctx = _open(agp, alloc_poison=poison, **kw)
    try:
        got = [(n, _fit(agp, ctx, _case(n))) for n in (1024, 2048, 1024, 1920)]
    finally:
        ctx.close()
    for i, (n, r) in enumerate(got):
        _same(r, _run(agp, n, **kw), f"fit {i} (N={n}) on the reused context vs a fresh one")
    _meets_oracle(got[3][1], _case(1920), "reused context, fourth fit")


# ---- 6. a failed fit, then a good one ---------------------------------------------------------------------------------------------------------------------------------
def test_not_positive_definite_fit_then_a_good_fit_on_the_same_context(agp):
    """σ² = 0 with a duplicated point (tests/test_gpu_strassen.py::test_not_positive_definite_input_reports_the_same_minor): the grouped two-stream fit reports the
    minor the classical one-stream fit reports, and the error path leaves the context as good as new — both streams drained, the call's blocks back in the pool"""
    x, y = o.synth_inputs(2048, 3, 5)
    x[1700] = x[900]
    info, after = {}, None
    for name, kw in (("classical/one", dict(strassen_min_rows=0)), ("grouped/two", TWO)):
        ctx = _open(agp, deterministic=1, **kw)
        try:
            f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
            with pytest.raises(agp.PosDefException) as e:
                agp.logpdf(f(agp.RowVecs(x), 0.0), y)
            info[name] = e.value.info
            if kw is TWO:
                after = _fit(agp, ctx, _case(2048))
        finally:
            ctx.close()
    print(f"SCHED not-PD info: {info}", flush=True)
    assert info["classical/one"] == info["grouped/two"] and 1 <= info["grouped/two"] <= 2048
    _same(after, _run(agp, 2048, deterministic=1, **TWO), "the fit after a failed fit vs a fresh context")


# ---- 7. the other fits through fit_impl, default mode ------------------------------------------------------------------------------------------------------------------
def test_composite_kernel_fit_on_the_grouped_two_stream_schedule(agp):
    from tests.composite_dx_ref import host_fit, six_term_data, six_term_kernel

    n = 1920
    X, y = six_term_data(n, seed=n)
    k = six_term_kernel()
    lp_h, a_h, _ = host_fit(k, X, y, 0.05)
    ctx = _open(agp, **TWO)
    try:
        fx = agp.GP(k, ctx=ctx)(agp.RowVecs(X), 0.05)
        lp = agp.logpdf(fx, y)
        post = agp.posterior(fx, y)
        alpha = np.array(post.data.alpha)
        post.data.C.free()
    finally:
        ctx.close()
    print(f"SCHED composite N={n}: logpdf rel {abs(lp - lp_h) / abs(lp_h):.2e} alpha rel {_rel(alpha, a_h):.2e}", flush=True)
    assert lp == pytest.approx(lp_h, rel=1e-10) and post.logpdf_value == pytest.approx(lp_h, rel=1e-10)
    assert _rel(alpha, a_h) <= 1e-8


@functools.lru_cache(maxsize=1)
def _dense_case(n):
    from tests.test_gpu_dense_noise import OK, _data, _host_fit, _sigma

    X, y = _data(n, n)
    S, _ = _sigma(n, n)
    lp, alpha, _ = _host_fit(o.kernelmatrix(OK, X, threads=8), S, y)
    return X, y, S, lp, alpha


@pytest.mark.parametrize("order", ["C", "F"])
def test_dense_noise_fit_on_the_grouped_two_stream_schedule(agp, order):
    from tests.test_gpu_dense_noise import _kernel, _ordered

    n = 1920
    X, y, S, lp_h, a_h = _dense_case(n)
    ctx = _open(agp, **TWO)
    try:
        fx = agp.GP(_kernel(), ctx=ctx)(agp.RowVecs(X), _ordered(S, order))
        lp = agp.logpdf(fx, y)
        post = agp.posterior(fx, y)
        alpha = np.array(post.data.alpha)
        post.data.C.free()
    finally:
        ctx.close()
    print(f"SCHED dense {order} N={n}: logpdf rel {abs(lp - lp_h) / abs(lp_h):.2e} alpha rel {_rel(alpha, a_h):.2e}", flush=True)
    assert lp == pytest.approx(lp_h, rel=1e-10) and post.logpdf_value == pytest.approx(lp_h, rel=1e-10)
    assert _rel(alpha, a_h) <= 1e-8


def test_value_and_gradient_of_a_matern52_ard_fit_on_the_grouped_two_stream_schedule(agp):
    """tolerances of tests/test_gpu_parity.py::test_logpdf_grad_vs_oracle (its ARD row: prior mean 0.2, vector noise)"""
    rng = np.random.default_rng(43)
    n = 1801
    X = rng.standard_normal((n, 3))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
    scale, sig = np.array([0.5, 1.1, 0.9]), rng.uniform(0.03, 0.1, n)
    ofx = o.FiniteGP(o.GP(o.Kernel(o.MATERN52, 1.4, scale), 0.2), X, sig)
    go, lp_o = o.logpdf_grad(ofx, y), float(o.logpdf(ofx, y))
    ctx = _open(agp, **TWO)
    try:
        f = agp.GP(0.2, 1.4 * agp.Matern52Kernel() @ agp.ARDTransform(scale), ctx=ctx)
        lp, g = agp.logpdf_and_grad(f(agp.RowVecs(X), sig), y)
    finally:
        ctx.close()
    print(f"SCHED grad N={n}: logpdf rel {abs(lp - lp_o) / abs(lp_o):.2e} variance rel {abs(g['variance'] - go['variance']) / abs(go['variance']):.2e} "
          f"scale {np.max(np.abs(g['scale'] - go['scale'])):.2e} noise {np.max(np.abs(g['noise'] - go['noise'])):.2e} y {np.max(np.abs(g['y'] - go['y'])):.2e}", flush=True)
    assert float(lp) == pytest.approx(lp_o, rel=1e-10)
    assert g["variance"] == pytest.approx(go["variance"], rel=1e-8, abs=1e-8 * max(1.0, abs(go["variance"])))
    np.testing.assert_allclose(g["scale"], go["scale"], rtol=1e-8, atol=1e-8 * max(1.0, np.abs(go["scale"]).max()))
    np.testing.assert_allclose(g["noise"], go["noise"], rtol=1e-7, atol=1e-7 * max(1.0, np.abs(go["noise"]).max()))
    np.testing.assert_allclose(g["y"], go["y"], rtol=0, atol=1e-8 * np.abs(go["y"]).max())


# ---- 8. "xcd_swizzle" keeps the per-block sequence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2048, 1801])
def test_xcd_swizzle_with_strassen_group_runs_the_per_block_sequence(agp, n):
    """the grouped kernel has no super-tile order, so xcd_swizzle = 1 turns grouping off whatever strassen_group says: the launch count of strassen_group = 0,
    and (deterministic) its bits"""
    per_block = _run(agp, n, deterministic=1, time_kernels=1, strassen_group=0, **TWO)
    swz = _run(agp, n, deterministic=1, time_kernels=1, xcd_swizzle=1, **TWO)
    assert swz["tm"]["gemm_launches"] == per_block["tm"]["gemm_launches"] and swz["tm"]["gemm_flops"] == per_block["tm"]["gemm_flops"]
    _same(swz, per_block, f"N={n} xcd_swizzle = 1 vs strassen_group = 0")
