"""Shared bodies of the device-level unit tests (test_gpu_units.py: fp64, test_gpu_units_f32.py: fp32, test_gpu_assemble.py: both): one implementation per check,
the element type a parameter.  Imported by GPU test modules only, after their importorskip("torch")."""
import contextlib
import ctypes as C

import numpy as np
import torch

U32 = 2.0 ** -24  # unit roundoff of fp32
SENTINEL = -7.25  # finite, non-zero, never produced by the integer-valued cases


def gamma(m, u=U32):
    """γ_m = m·u / (1 − m·u) (Higham, Accuracy and Stability of Numerical Algorithms, §3.1)"""
    assert m * u < 1
    return m * u / (1.0 - m * u)


def P(t):
    return C.c_void_p(t.data_ptr())


def entry(lib, name, dtype):
    """the fp64 entry point or its fp32 twin"""
    return getattr(lib, name + ("_f32" if dtype == torch.float32 else ""))


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def sync(lib, h):
    from abstractgps_jl_amd._lib import check

    check(lib.gpd_sync(h))


def report(name, ratio):
    """one line per bounded check: the largest error / bound over all components (run pytest with -s to collect them)"""
    print(f"RATIO {name} {ratio:.4g}", flush=True)


def ratio_of(err, bound):
    """max over components of err / bound; a component with bound 0 must have err 0 (it counts as inf otherwise)"""
    tiny = torch.finfo(torch.float64).tiny
    return (err / bound.clamp_min(tiny)).max().item() if err.numel() else 0.0


@contextlib.contextmanager
def params(lib, h, **kw):
    """ctx parameters set for the body and put back to what they were, whatever happens"""
    from abstractgps_jl_amd._lib import check

    old = {}
    for k in kw:
        v = C.c_int64()
        check(lib.gp_ctx_get_param(h, k.encode(), C.byref(v)))
        old[k] = v.value
    try:
        for k, v in kw.items():
            check(lib.gp_ctx_set_param(h, k.encode(), v))
        yield
    finally:
        for k, v in old.items():
            check(lib.gp_ctx_set_param(h, k.encode(), v))


# The GEMM launch variants every exact case runs under: name -> (on the padded context?, ctx parameters).  launch_gemm takes the persistent stream-K kernel
# (gemm_nt_sk_kernel, no dynamic LDS) whenever gemm_streamk is on, the launch is not deterministic and the map is not the XCD order; only otherwise does it launch
# gemm_nt_dma_kernel, the one kernel that gets the gemm_pad_lds request.  So "pad" and "pipe0" alone stay on the stream-K kernel, and the *_streamk0 variants are what
# reaches gemm_nt_dma_kernel<T, T, 1 / 0> with and without the 20 KiB of dynamic LDS (one workgroup per CU).
GEMM_CONFIGS = {"default": (False, {}), "streamk0": (False, {"gemm_streamk": 0}), "deterministic": (False, {"deterministic": 1}), "pipe0": (False, {"gemm_pipe": 0}),
                "pad": (True, {}), "xcd": (False, {"xcd_swizzle": 1, "xcd_min_tiles": 1}),
                "pipe0_streamk0": (False, {"gemm_pipe": 0, "gemm_streamk": 0}),
                "pad_streamk0": (True, {"gemm_streamk": 0}), "pad_pipe0_streamk0": (True, {"gemm_pipe": 0, "gemm_streamk": 0})}


@contextlib.contextmanager
def padded_context(agp):
    """a context of its own with gemm_pad_lds = 20 480: once set, the parameter cannot be returned to 'not set'"""
    c = agp.Context(0)
    try:
        c.set_param("gemm_pad_lds", 20480)
        yield c.handle
    finally:
        c.close()


@contextlib.contextmanager
def gemm_variant(lib, h, pad_h, name):
    """the handle to launch on under the GEMM launch variant `name`, its parameters put back afterwards"""
    padded, kw = GEMM_CONFIGS[name]
    hh = pad_h if padded else h
    with params(lib, hh, **kw):
        yield hh


GEMM_RECT = [(128, 128), (256, 128), (64, 64), (192, 64), (320, 448), (1024, 1024), (2176, 2304), (4224, 1152),  # (m, n) of test_gemm_nt_rect
             (2944, 2944)]  # 23 × 23 = 529 tiles > 2·256 workgroups: the stream-K kernel's whole rounds (no atomics) AND its tail cut along k
GEMM_LOWER = [(256, 256, 0, 0), (320, 192, 64, 64), (512, 128, 128, 128), (2304, 2304, 0, 0), (2432, 2176, 384, 128), (3200, 2560, 1152, 0),
              (2048, 2048, 64, 64)]  # (m, n, row0, col0) of test_gemm_nt_lower_skips_upper


def gemm_window(m, n, rows, ldc, lower):
    """mask of the elements of the rows × ldc buffer a launch must update: the m × n window, in lower mode without the 64×64 sub-tiles strictly above the diagonal"""
    win = torch.zeros(rows, ldc, dtype=torch.bool, device="cuda")
    if lower is None:
        win[:m, :n] = True
    else:
        r = torch.arange(m, device="cuda")[:, None] + lower[0]
        c = torch.arange(n, device="cuda")[None, :] + lower[1]
        win[:m, :n] = (c // 64) <= (r // 64)
    return win


def gemm_exact(lib, h, dtype, m, n, lower=None):
    """C −= A·Bᵀ with integer operands in [−3, 3] and C₀ in [−64, 64], k = BK, 2·BK, 3·BK, 1024, 4096: every partial sum is an integer below 2²⁴ (|result| <= 64 + 9·4096),
    so the result equals the fp64 reference EXACTLY in any summation order (stream-K atomics included) — one dropped or doubled k-step, one row written to the wrong
    place, is a whole-number error.  Everything outside the updated window holds a sentinel and must come back bit-identical."""
    from abstractgps_jl_amd._lib import check, gp_grid

    bk = 128 // torch.empty(0, dtype=dtype).element_size()  # 16 (f64) / 32 (f32)
    ks = (bk, 2 * bk, 3 * bk, 1024, 4096)
    g = torch.Generator(device="cuda").manual_seed(m * 7 + n * 3 + (0 if lower is None else 1 + lower[0] + lower[1]))
    lda, ldc = max(ks) + 32, n + 32
    A = torch.randint(-3, 4, (m + 128, lda), device="cuda", generator=g).to(dtype)  # 128 slack rows: the operand over-read contract
    B = torch.randint(-3, 4, (n + 128, lda), device="cuda", generator=g).to(dtype)
    C0 = torch.randint(-64, 65, (m + 128, ldc), device="cuda", generator=g).to(dtype)
    win = gemm_window(m, n, m + 128, ldc, lower)
    C0[~win] = SENTINEL
    grid = None if lower is None else C.byref(gp_grid(1, 0, 1, 0, 1, 1))
    row0, col0 = (0, 0) if lower is None else lower
    fn = entry(lib, "gpd_gemm_nt", dtype)
    for k in ks:
        ref = C0.to(torch.float64, copy=True)  # a copy for fp64 too: .double() would alias C0
        ref[:m, :n] -= A[:m, :k].double() @ B[:n, :k].double().T
        Cm = C0.clone()
        torch.cuda.synchronize()
        check(fn(h, P(Cm), ldc, P(A), lda, P(B), lda, m, n, k, grid, row0, col0))
        sync(lib, h)
        wrong = (Cm.double() != ref) & win
        assert not wrong.any().item(), (k, int(wrong.sum().item()), (Cm.double() - ref)[wrong].abs().max().item())
        assert torch.equal(bits(Cm)[~win], bits(C0)[~win]), (k, "an element outside the updated window changed")


def gemv_t_exact(lib, h, dtype):
    """r[j] −= Σ_i L[i][j]·a[i] on integers (exact in either dtype), ragged nrows / ncols (not multiples of 64 / 256); r beyond ncols untouched"""
    from abstractgps_jl_amd._lib import check

    g = torch.Generator(device="cuda").manual_seed(5)
    fn = entry(lib, "gpd_gemv_t", dtype)
    for nrows, ncols in ((200, 777), (64, 256), (1, 1), (333, 1000)):
        ldl = ncols + 24
        L = torch.randint(-3, 4, (nrows, ldl), device="cuda", generator=g).to(dtype)
        a = torch.randint(-3, 4, (nrows + 8,), device="cuda", generator=g).to(dtype)
        r0 = torch.randint(-64, 65, (ldl,), device="cuda", generator=g).to(dtype)
        r0[ncols:] = SENTINEL
        r = r0.clone()
        torch.cuda.synchronize()
        check(fn(h, P(L), ldl, nrows, ncols, P(a), P(r)))
        sync(lib, h)
        ref = r0[:ncols].double() - L[:, :ncols].double().T @ a[:nrows].double()
        assert torch.equal(r[:ncols].double(), ref), (nrows, ncols)
        assert torch.equal(bits(r)[ncols:], bits(r0)[ncols:]), (nrows, ncols)


def rowsumsq_exact(lib, h, dtype):
    """out[i] = Σ_c x[i][c]² on integers, ragged ncols; out beyond nrows untouched (the sums are fp64 whatever the element type)"""
    from abstractgps_jl_amd._lib import check

    g = torch.Generator(device="cuda").manual_seed(6)
    fn = entry(lib, "gpd_rowsumsq", dtype)
    for nrows, ncols, ldx in ((5, 777, 1000), (3, 1, 8), (130, 256, 256), (2, 1023, 1024)):
        X = torch.randint(-3, 4, (nrows, ldx), device="cuda", generator=g).to(dtype)
        out = torch.full((nrows + 4,), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        check(fn(h, P(X), ldx, nrows, ncols, P(out)))
        sync(lib, h)
        assert torch.equal(out[:nrows], (X[:, :ncols].double() ** 2).sum(1)), (nrows, ncols)
        assert (out[nrows:] == SENTINEL).all().item()


# ---- gpd_assemble ---------------------------------------------------------------------------------------------------------------------------------------------
ASSEMBLE_D = (1, 3, 4, 5, 8, 9, 16, 17, 33)  # the instance boundaries of launch_kmat (D <= 4 / 8 / 16 row forms, the accumulate form beyond)
VARIANCE = 1.5


def assemble_problem(dtype, kind, d, n_valid, n_pad):
    """Inputs (dimension-major [d][n_pad], zero beyond n_valid), a noise vector, and the fp64 matrix K + Σy of the oracle on exactly those values, padded with identity.
    The inputs are uniform on [0, s]^D with s = √(6/D): E d² = 1, so κ sits mid-range for every kind and every D (uniform [0, 4]^D makes K vanish at D = 33)."""
    from oracle import gp_oracle as o

    npdt = np.float32 if dtype == torch.float32 else np.float64
    rng = np.random.default_rng(1000 * kind + d)
    x = (rng.random((n_valid, d)) * np.sqrt(6.0 / d)).astype(npdt)
    noise = (0.25 + 0.5 * rng.random(n_pad)).astype(npdt)
    K = o.kernelmatrix(o.Kernel(kind, VARIANCE), x.astype(np.float64))
    off = K[~np.eye(n_valid, dtype=bool)] / VARIANCE
    assert 0.2 <= np.median(off) <= 0.8, np.median(off)  # the case really exercises κ
    Kg = np.eye(n_pad)
    Kg[:n_valid, :n_valid] = K
    Kg[np.arange(n_valid), np.arange(n_valid)] += noise[:n_valid].astype(np.float64)
    xd = np.zeros((d, n_pad), dtype=npdt)
    xd[:, :n_valid] = x.T
    return xd, noise, Kg


def assemble_bound(dtype, d):
    """fp64: the project's own |ΔK| <= 1e-14·σ².  fp32: (D + 16)·u·σ² — the relative error of d² is <= (D + 1)u (D differences, D fused adds), |d²·κ′(d²)| <= 1 for every kind,
    and √, the polynomial and exp add a few u."""
    return 1e-14 * VARIANCE if dtype == torch.float64 else (d + 16) * U32 * VARIANCE


def assemble_check(lib, h, dtype, kind, d, problem, n_valid, n_pad, Pg, Qg, p, q, tb, lower, tag):
    """one gpd_assemble call on rank (p, q) of a Pg × Qg grid against the global matrix: local tile (t_r, t_c) holds global tile (((t / tb)·P + p)·tb + t % tb, same with Q, q)
    — the header's formula — which covers the noise (global diagonal only), the identity padding and, with lower, the sentinel left in tiles strictly above the global diagonal"""
    from abstractgps_jl_amd._lib import check, gp_grid, gp_kernel

    xd, noise, Kg = problem
    nt = n_pad // 128
    assert nt % (tb * Pg) == 0 and nt % (tb * Qg) == 0
    tr, tc = nt // Pg, nt // Qg
    m_loc, n_loc, lda = 128 * tr, 128 * tc, 128 * tc + 32
    gtile = lambda t, Pn, pn: ((t // tb) * Pn + pn) * tb + t % tb
    want = np.full((m_loc, lda), SENTINEL)
    for a in range(tr):
        for b in range(tc):
            ga, gb = gtile(a, Pg, p), gtile(b, Qg, q)
            if lower and gb > ga:
                continue
            want[128 * a:128 * (a + 1), 128 * b:128 * (b + 1)] = Kg[128 * ga:128 * (ga + 1), 128 * gb:128 * (gb + 1)]
    x_dev, nz_dev = torch.from_numpy(xd).cuda(), torch.from_numpy(noise).cuda()
    out = torch.full((m_loc, lda), SENTINEL, dtype=dtype, device="cuda")
    kern = gp_kernel(kind, 0 if dtype == torch.float64 else 1, VARIANCE, 0, None)
    grid = gp_grid(Pg, p, Qg, q, tb, lower)
    torch.cuda.synchronize()
    check(entry(lib, "gpd_assemble", dtype)(h, C.byref(kern), P(x_dev), n_valid, n_pad, d, P(nz_dev), C.byref(grid), P(out), lda, m_loc, n_loc))
    sync(lib, h)
    got = out.double().cpu().numpy()
    kept = want == SENTINEL
    assert np.array_equal(got[kept], want[kept]), (tag, "an element outside the assembled tiles changed")
    pad_rows = np.zeros_like(kept)
    for a in range(tr):
        lo = 128 * gtile(a, Pg, p)
        pad_rows[128 * a:128 * (a + 1)] = (lo + np.arange(128) >= n_valid)[:, None]
    exact = pad_rows & ~kept
    assert np.array_equal(got[exact], want[exact]), (tag, "padding rows are not rows of the identity")
    ratio = float(np.max(np.abs(got - want)[~kept]) / assemble_bound(dtype, d))
    report(tag, ratio)
    assert ratio <= 1.0, (tag, ratio)
