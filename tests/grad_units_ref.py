"""The longdouble reference and the rounding bounds of the gradient-contraction unit tests (test_gpu_units_grad.py; held against mpmath by
test_grad_units_ref_cpu.py).  NumPy only: importable without a GPU and without torch.

What the device entry points compute (include/gpmi355.h gpd_grad_contract / gpd_vgrad; formulas as csrc/kfun.hpp and csrc/kernels.hpp document them), with
u = the pre-scaled inputs, t_p = u_ip − u_jp, d² = Σ_p t_p², κ = κ_kind(d²), κ' = dκ/dd²:

    SE  κ = e^{−d²/2}, κ' = −κ/2        Matern12  κ = e^{−r}, κ' = −κ/(2r), taken as 0 at r = 0
    Matern32  κ = (1 + a) e^{−a}, κ' = −(3/2) e^{−a}, a = √3 r          Matern52  κ = (1 + a + (5/3) d²) e^{−a}, κ' = −(5/6)(1 + a) e^{−a}, a = √5 r

    g[0]     = Σ W κ                                  ∂/∂variance
    g[2 + p] = Σ W σ² κ' · 2 d² / s   (one scale)  |  Σ W σ² κ' · 2 t_p² / s_p   (ARD)
    row sums   gx[p][i] = Σ_j W σ² κ' · 2 s_p t_p,      column sums   gz[p][j] = −zfac Σ_i W σ² κ' · 2 s_p t_p

Everything is evaluated in np.longdouble (x87 extended: u = 5.4e-20) from exactly the T-rounded values the device gets, widened — so the reference's own error is
three orders below the fp64 bounds (test_grad_units_ref_cpu.py asserts that against 40-digit mpmath).

THE BOUND of an output q (form of unit_helpers.assemble_bound and of test_gpu_backward_error.py):

    |Δ_q| <= Σ_ij Wabs_ij · e_q(i, j)  +  (c_w·u64 + γ_m(u64)) · Σ_ij Wabs_ij |F_q(i, j)|                                   u64 = 2⁻⁵³

  Wabs   the weight's magnitude before cancellation: (|a_i a_j| + |c_ij|)·(½ on the diagonal) for the exact contraction, |c_ij| for explicit weights,
         |rs_i| (2 |c_ij| + |b_i ν_j|) for the streamed form.  The weight is formed in fp64 from T values: c_w = 2 roundings (product, sum; the ½ is exact), 0 for explicit
         weights, 3 for rs_i (−2 c_ij + b_i ν_j).
  e_q    the per-element error of the kernel function or derivative evaluated in T (u = 2⁻⁵³ / 2⁻²⁴):
         κ:  the project's own bound, 1e-14·σ² in fp64 and (D + 16)·u32·σ² in fp32 (unit_helpers.assemble_bound).
         κ'·q with q = d², t_p² or t_p:  the device forms t_p = fl(u_ip − u_jp) (relative error u) and d² by D fused multiply-adds, so the computed d² is d²(1 + ε),
         |ε| <= ε_d = γ_{D+2}(u) (2u from the squared difference, at most D roundings of the chain).  κ' evaluated at the perturbed argument moves by
         |d² κ''(d²)| ε_d (SE d²κ/4 · Matern12 (1 + r) e^{−r}/(4r) · Matern32 (3a/4) e^{−a} · Matern52 (5/12) a² e^{−a}), and its evaluation in T adds a relative
         (3a + 16)u, a the magnitude of the exponential's argument: 3a·u from the argument (√, the rounded constant, their product), 16u for exp itself (<= 3 ulp),
         the polynomial factor, the rounded constants and Matern12's division — the "few u" the κ bound also carries as its 16.  q itself carries ε_q = ε_d (d²),
         3u (t_p²: two roundings of t, one of the square in the D > 16 form) or u (t_p).  Hence
             e(κ' q) = |q| · ( e_κ' (1 + ε_q) + |κ'| ε_q ),   e_κ' = |d²κ''| ε_d + |κ'| (3a + 16) u / (1 − (3a + 16) u).
         The fixed factors (2, σ², s_p, 1/s_p) are applied in fp64: their roundings are counted in m.
  m      the longest chain of fp64 operations an output passes through, counted from the kernels:
         hyper-parameter sums   64 terms per thread (32 rows × 2 columns) + 6 wave shuffles + 3 LDS adds + one atomic per tile + 8 (the products w·σ²·κ'·2·t·t, the
                                final division by the scale and the add onto the caller's value)
         row sums (gx, rowq, rowp)   2 terms per lane + 6 shuffles + one atomic per column tile + 8
         column sums (gz)            32 terms per thread + 3 LDS adds + one atomic per row tile + 8
         dn[i] = ½(a_i² + c_ii): 2 fp64 roundings, then the rounding to T;  g[1] = Σ_i dn[i]: 6 shuffles + 3 LDS adds + one atomic per 256 rows + 2.
  A bound of 0 (an output no weight reaches) demands an error of 0."""
import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
U32 = 2.0 ** -24
SQ3 = np.sqrt(LD(3))
SQ5 = np.sqrt(LD(5))


def unit(npdt):
    return U32 if np.dtype(npdt) == np.float32 else U64


def gamma(m, u):
    assert m * u < 1
    return m * u / (1.0 - m * u)


def kappa_dk(kind, d2):
    """κ and dκ/dd² of kinds 0..3 at d2 (longdouble array)"""
    d2 = np.asarray(d2, dtype=LD)
    if kind == 0:
        k = np.exp(-d2 / 2)
        return k, -k / 2
    r = np.sqrt(d2)
    if kind == 1:
        k = np.exp(-r)
        with np.errstate(divide="ignore", invalid="ignore"):
            dk = np.where(r > 0, -k / (2 * r), LD(0))
        return k, dk
    if kind == 2:
        a = SQ3 * r
        e = np.exp(-a)
        return (1 + a) * e, -LD(3) / 2 * e
    a = SQ5 * r
    e = np.exp(-a)
    return (1 + a + LD(5) / 3 * d2) * e, -LD(5) / 6 * (1 + a) * e


def elem_errors(kind, d2, D, npdt):
    """(e_κ, e_κ', ε_d): the absolute per-element errors of κ and κ' evaluated in T at a d² accumulated in T, per unit variance (module docstring)"""
    u = unit(npdt)
    eps_d = gamma(D + 2, u)
    d2 = np.asarray(d2, dtype=LD)
    r = np.sqrt(d2)
    _, dk = kappa_dk(kind, d2)
    if kind == 0:
        a = d2 / 2
        d2k2 = d2 * np.exp(-a) / 4
    elif kind == 1:
        a = r
        with np.errstate(divide="ignore", invalid="ignore"):
            d2k2 = np.where(r > 0, (1 + r) * np.exp(-r) / (4 * r), LD(0))
    elif kind == 2:
        a = SQ3 * r
        d2k2 = 3 * a / 4 * np.exp(-a)
    else:
        a = SQ5 * r
        d2k2 = LD(5) / 12 * a * a * np.exp(-a)
    ev = (3 * a + 16) * u
    e_dk = d2k2 * eps_d + np.abs(dk) * ev / (1 - ev)
    e_k = np.full(d2.shape, 1e-14 if u == U64 else (D + 16) * U32, dtype=LD)
    return e_k, e_dk, eps_d


def _wide(a):
    return np.asarray(a).astype(LD)


def _d2(xr, xc):
    d2 = np.zeros((xr.shape[1], xc.shape[1]), dtype=LD)
    for p in range(xr.shape[0]):
        t = xr[p][:, None] - xc[p][None, :]
        d2 += t * t
    return d2


class Out:
    """one output (or array of outputs): the reference value, the sum of absolute terms, the bound from zeroed outputs, and the number of atomic adds onto the caller's
    value (each costs u64·|initial value| more when the output does not start from zero)"""

    def __init__(self, val, absum, bound, natom):
        self.val, self.abs, self.bound, self.natom = val, absum, bound, natom

    def bound_from(self, init):
        return self.bound + self.natom * U64 * np.abs(_wide(init))


def _sums(kind, variance, nscale, scale, xr, xc, W, Wabs, c_w, npdt, ntiles, ncoltiles, nrowtiles, want_rows, want_cols, zfac):
    """the sums every contraction shares, over the weight matrix W (rows: xr's points, columns: xc's): dict of Out"""
    D = xr.shape[0]
    u = unit(npdt)
    var = LD(variance)
    d2 = _d2(xr, xc)
    kap, dk = kappa_dk(kind, d2)
    e_k, e_dk, eps_d = elem_errors(kind, d2, D, npdt)
    m_h, m_r, m_c = 64 + 6 + 3 + ntiles + 8, 2 + 6 + ncoltiles + 8, 32 + 3 + nrowtiles + 8

    def out(terms, aterms, eterms, m, natom, axis=None):
        a = aterms.sum(axis)
        return Out(terms.sum(axis), a, eterms.sum(axis) + (c_w * U64 + gamma(m, U64)) * a, natom)

    def deriv_err(q, eps_q):
        return np.abs(q) * (e_dk * (1 + eps_q) + np.abs(dk) * eps_q)

    res = {"g0": out(W * kap, Wabs * np.abs(kap), Wabs * e_k, m_h, ntiles)}
    sc = [LD(s) for s in scale] if nscale else []
    gs = []
    if nscale == 1:
        gs.append(out(W * var * dk * 2 * d2 / sc[0], Wabs * var * np.abs(dk) * 2 * d2 / sc[0], Wabs * var * 2 * deriv_err(d2, eps_d) / sc[0], m_h, ntiles))
    rows, cols = [], []
    for p in range(D):
        t = xr[p][:, None] - xc[p][None, :]
        if nscale > 1:
            gs.append(out(W * var * dk * 2 * t * t / sc[p], Wabs * var * np.abs(dk) * 2 * t * t / sc[p], Wabs * var * 2 * deriv_err(t * t, 3 * u) / sc[p], m_h, ntiles))
        sp = LD(1) if nscale == 0 else (sc[0] if nscale == 1 else sc[p])
        F, Fa, Fe = W * var * dk * 2 * sp * t, Wabs * var * np.abs(dk) * 2 * sp * np.abs(t), Wabs * var * 2 * sp * deriv_err(t, u)
        if want_rows:
            rows.append(out(F, Fa, Fe, m_r, ncoltiles, axis=1))
        if want_cols:
            cols.append(out(-zfac * F, abs(zfac) * Fa, abs(zfac) * Fe, m_c, nrowtiles, axis=0))
    stack = lambda L: Out(np.stack([o.val for o in L]), np.stack([o.abs for o in L]), np.stack([o.bound for o in L]), L[0].natom)  # noqa: E731
    if gs:
        res["gs"] = stack(gs)
    if rows:
        res["rows"] = stack(rows)
    if cols:
        res["cols"] = stack(cols)
    res["_kap"], res["_ek"] = kap, e_k
    return res


def contract_reference(kind, variance, nscale, scale, x, ci, alpha, n, np_pad, want_gx):
    """gpd_grad_contract on the T-valued arrays x ([d][>= n]), ci ([>= n][>= n], lower used) and alpha: dict of Out — g0, gs ([nscale]), g1, dn ([n]) and, with want_gx,
    gx ([d][n]).  np_pad: the padded size the launch covers (tile counts of m)."""
    npdt = np.asarray(x).dtype
    xw, a = _wide(x)[:, :n], _wide(alpha)[:n]
    c = np.tril(_wide(ci)[:n, :n])
    half = np.where(np.eye(n, dtype=bool), LD(0.5), LD(1))
    aa = np.outer(a, a)
    low = np.tril(np.ones((n, n), dtype=bool))
    W = np.where(low, (aa + c) * half, LD(0))
    Wabs = np.where(low, (np.abs(aa) + np.abs(c)) * half, LD(0))
    T = np_pad // 128
    res = _sums(kind, variance, nscale, scale, xw, xw, W, Wabs, 2, npdt, T * (T + 1) // 2, T, T, False, False, 0.0)
    res.pop("_kap"), res.pop("_ek")
    v = (a * a + np.diag(c)) / 2
    va = (a * a + np.abs(np.diag(c))) / 2
    res["dn"] = Out(v, va, 2 * U64 * va + (unit(npdt) * np.abs(v) if unit(npdt) != U64 else 0), 0)
    nblk = (n + 255) // 256
    res["g1"] = Out(v.sum(), va.sum(), (2 * U64 + gamma(6 + 3 + nblk + 2, U64)) * va.sum(), nblk)
    if want_gx:
        cs = c + np.tril(c, -1).T
        off = ~np.eye(n, dtype=bool)
        Wf = np.where(off, aa + cs, LD(0))
        Wfa = np.where(off, np.abs(aa) + np.abs(cs), LD(0))
        res["gx"] = _sums(kind, variance, nscale, scale, xw, xw, Wf, Wfa, 2, npdt, 1, T, T, True, False, 0.0)["rows"]
    return res


def rect_reference(kind, variance, nscale, scale, xr, xc, cm, explicit_w, rs, bv, nu, nr, nc, zfac, want_gx):
    """gpd_vgrad on the T-valued arrays: dict of Out — g0, gs, gz ([d][nc]), gx ([d][nr], with want_gx) and, for explicit_w = 0, rowq / rowp ([nr])"""
    npdt = np.asarray(xr).dtype
    xrw, xcw = _wide(xr)[:, :nr], _wide(xc)[:, :nc]
    c = _wide(cm)[:nr, :nc]
    if explicit_w:
        W, Wabs, c_w = c, np.abs(c), 0
    else:
        r, b, v = _wide(rs)[:nr, None], _wide(bv)[:nr, None], _wide(nu)[None, :nc]
        W, Wabs, c_w = r * (-2 * c + b * v), np.abs(r) * (2 * np.abs(c) + np.abs(b * v)), 3
    tr, tc = (nr + 127) // 128, (nc + 127) // 128
    res = _sums(kind, variance, nscale, scale, xrw, xcw, W, Wabs, c_w, npdt, tr * tc, tc, tr, want_gx, True, zfac)
    kap, e_k = res.pop("_kap"), res.pop("_ek")
    res["gz"] = res.pop("cols")
    if want_gx:
        res["gx"] = res.pop("rows")
    if not explicit_w:
        var = LD(variance)
        m_r = 2 + 6 + tc + 8
        for name, wq in (("rowq", -c), ("rowp", np.broadcast_to(_wide(nu)[None, :nc], c.shape))):
            a = (var * np.abs(kap) * np.abs(wq)).sum(1)
            res[name] = Out((var * kap * wq).sum(1), a, (var * e_k * np.abs(wq)).sum(1) + gamma(m_r, U64) * a, tc)
    return res


# ---- the composite form (gpd_grad_contract_sum) ------------------------------------------------------------------------------------------------------------
PI = LD("3.14159265358979323846264338327950288")


def composite_reference(s1, r, s, a, s2, x, ci, alpha, n, np_pad):
    """gpd_grad_contract_sum for k = σ₁²·Periodic(r)·RQ(α)∘Scale(s) + σ₂²·White on RAW inputs x ([d][>= n], T-valued; every θ value must be exactly representable in T: the
    device casts θ to T where it evaluates a factor).  θ order as pack_ksum lays it out: [σ₁², r_0 … r_{D−1}, s, α, σ₂²].  dict of Out: theta ([D + 4]), gx ([d][n]), dn, g1.

    Formulas (csrc/kfun.hpp), t = x_i − x_j, r² = Σ t_p², d² = s² r², q = d²/(2α):
        κ_P = exp(−½ Σ_p (sinpi t_p / r_p)²),   κ_R = exp(−α log1p q),   White = [t == 0]
        ∂/∂σ₁² : κ_P κ_R      ∂/∂σ₂² : [t == 0]      ∂/∂r_p : σ₁² κ_R κ_P sinpi(t_p)² / r_p³
        ∂/∂s   : σ₁² κ_P · (−κ_R / (2(1 + q))) · 2 s r²        ∂/∂α : σ₁² κ_P κ_R (q/(1 + q) − log1p q)
        gx[p][j] = −Σ_{i≠j} W_ij σ₁² [ −κ_R κ_P (π/2) sinpi(2 t_p) / r_p²  +  κ_P · 2 (−κ_R / (2(1 + q))) s² t_p ],   t = x_i − x_j,  W_ij = α_i α_j + c_{max,min}
    Per-element errors, u = the unit roundoff of T, every "few u" constant counted: sinpi 4u (2 ulp), log1p 4u, exp 6u (3 ulp).
        t_p carries u; sinpi(t_p(1 + δ)) moves by π|t_p|u, so |Δ sinpi| <= π|t_p|u + 4u|sinpi|;  v_p = sinpi/r_p: |Δv_p| <= |Δ sinpi|/r_p + u|v_p|;
        acc = Σ v_p²: |Δacc| <= Σ 2|v_p||Δv_p| + γ_{D+2}(u) acc;   δ_P = |Δκ_P|/κ_P <= ½|Δacc| + 6u.
        r² carries ε_d = γ_{D+2}(u), d² = s·s·r² carries ε_d2 = ε_d + 2u, q in T one more u;  δ_R = |Δκ_R|/κ_R <= α q (ε_d2 + u)/(1 + q) + 5u·α log1p q + 6u
        (the perturbed argument of log1p, its evaluation and the product with α, then exp).
        The derivative factors are formed in fp64 from the T values: 1/(1 + q) moves by q ε_d2/(1 + q) relative, h(q) = q/(1 + q) − log1p q by q² ε_d2/(1 + q)² (h' = −q/(1 + q)²)
        plus 4 u64 (q/(1 + q) + log1p q) for its own cancellation; sinpi(t_p)² by 2|sinpi||Δ sinpi|; sinpi(2 t_p) by 2π|t_p|u + 4u|sinpi 2t_p|.
    m: θ sums 64 elements per thread + 6 shuffles + 3 LDS adds + one atomic per tile + 16 (the prefix / suffix products and factors of a term);
       gx 64 rows × 2 adds per thread + 1 LDS add + one atomic per row tile + 16."""
    npdt = np.asarray(x).dtype
    u = unit(npdt)
    D = x.shape[0]
    xw, av = _wide(x)[:, :n], _wide(alpha)[:n]
    c = np.tril(_wide(ci)[:n, :n])
    aa = np.outer(av, av)
    half = np.where(np.eye(n, dtype=bool), LD(0.5), LD(1))
    low = np.tril(np.ones((n, n), dtype=bool))
    W = np.where(low, (aa + c) * half, LD(0))
    Wabs = np.where(low, (np.abs(aa) + np.abs(c)) * half, LD(0))
    cs = c + np.tril(c, -1).T
    off = ~np.eye(n, dtype=bool)
    Wf, Wfa = np.where(off, aa + cs, LD(0)), np.where(off, np.abs(aa) + np.abs(cs), LD(0))
    s1, s, a, s2 = LD(s1), LD(s), LD(a), LD(s2)
    rr = [LD(v) for v in r]
    T = np_pad // 128
    eps_d = gamma(D + 2, u)
    eps_d2 = eps_d + 2 * u
    t = [xw[p][:, None] - xw[p][None, :] for p in range(D)]
    sn = [np.sin(PI * tp) for tp in t]
    dsn = [PI * np.abs(tp) * u + 4 * u * np.abs(sp) for tp, sp in zip(t, sn)]
    v = [sp / rp for sp, rp in zip(sn, rr)]
    dv = [dp / rp + u * np.abs(vp) for dp, rp, vp in zip(dsn, rr, v)]
    acc = sum(vp * vp for vp in v)
    dacc = sum(2 * np.abs(vp) * dvp for vp, dvp in zip(v, dv)) + eps_d * acc
    kP = np.exp(-acc / 2)
    dP = dacc / 2 + 6 * u
    r2 = sum(tp * tp for tp in t)
    eq = r2 == 0
    q = s * s * r2 / (2 * a)
    L = np.log1p(q)
    kR = np.exp(-a * L)
    dR = a * q * (eps_d2 + u) / (1 + q) + 5 * u * a * L + 6 * u
    dPR = dP + dR
    dk = -kR / (2 * (1 + q))
    h = q / (1 + q) - L
    m_h, m_x = 64 + 6 + 3 + T * (T + 1) // 2 + 16, 128 + 1 + T + 16

    def out(F, E, Wv, Wa, m, natom, axis=None):
        ab = (Wa * np.abs(F)).sum(axis)
        return Out((Wv * F).sum(axis), ab, (Wa * E).sum(axis) + (2 * U64 + gamma(m, U64)) * ab, natom)

    nt = T * (T + 1) // 2
    th = [out(kP * kR, kP * kR * dPR, W, Wabs, m_h, nt)]
    for p in range(D):
        F = s1 * kR * kP * sn[p] ** 2 / rr[p] ** 3
        th.append(out(F, np.abs(F) * dPR + s1 * kR * kP / rr[p] ** 3 * 2 * np.abs(sn[p]) * dsn[p], W, Wabs, m_h, nt))
    F = s1 * kP * dk * 2 * s * r2
    th.append(out(F, np.abs(F) * (dPR + q * eps_d2 / (1 + q) + eps_d), W, Wabs, m_h, nt))
    F = s1 * kP * kR * h
    th.append(out(F, s1 * kP * kR * (np.abs(h) * dPR + q * q * eps_d2 / (1 + q) ** 2 + 4 * U64 * (q / (1 + q) + L)), W, Wabs, m_h, nt))
    th.append(out(eq.astype(LD), np.zeros_like(r2), W, Wabs, m_h, nt))
    res = {"theta": Out(np.stack([o.val for o in th]), np.stack([o.abs for o in th]), np.stack([o.bound for o in th]), nt)}
    gx = []
    for p in range(D):  # row j of gx sums over i: with t = x_j − x_i here (rows = j), the sign flips twice — ∂k/∂t is odd — so gx[p][j] = Σ_i W_ji ∂k/∂t_p(x_j − x_i)
        s2p = np.sin(2 * PI * t[p])
        A = -s1 * kR * kP * (PI / 2) * s2p / rr[p] ** 2
        B = s1 * kP * 2 * dk * s * s * t[p]
        EA = np.abs(A) * dPR + s1 * kR * kP * (PI / 2) / rr[p] ** 2 * (2 * PI * np.abs(t[p]) * u + 4 * u * np.abs(s2p))
        EB = np.abs(B) * (dPR + q * eps_d2 / (1 + q) + u)
        ab = (Wfa * (np.abs(A) + np.abs(B))).sum(1)
        gx.append(Out((Wf * (A + B)).sum(1), ab, (Wfa * (EA + EB)).sum(1) + (2 * U64 + gamma(m_x, U64)) * ab, T))
    res["gx"] = Out(np.stack([o.val for o in gx]), np.stack([o.abs for o in gx]), np.stack([o.bound for o in gx]), T)
    vv, va = (av * av + np.diag(c)) / 2, (av * av + np.abs(np.diag(c))) / 2
    res["dn"] = Out(vv, va, 2 * U64 * va + (u * np.abs(vv) if u != U64 else 0), 0)
    nblk = (n + 255) // 256
    res["g1"] = Out(vv.sum(), va.sum(), (2 * U64 + gamma(6 + 3 + nblk + 2, U64)) * va.sum(), nblk)
    return res


def ratio(err, bound):
    """max over components of |err| / bound in longdouble (the NumPy sibling of unit_helpers.ratio_of: torch has no longdouble); a component with bound 0 must have
    err 0, and a non-finite error counts as inf whatever its bound"""
    err, bound = np.abs(np.asarray(err, dtype=LD)).ravel(), np.asarray(bound, dtype=LD).ravel()
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, LD(0), LD(np.inf)))
    q = np.where(np.isfinite(err), q, LD(np.inf))
    return float(q.max())
