"""The longdouble reference and the rounding bounds of the prediction-kernel unit tests (test_gpu_units_predict.py; held against mpmath by
test_predict_units_ref_cpu.py).  NumPy only: importable without a GPU and without torch.

What the device entry points compute (include/gpmi355.h gpd_kvec / gpd_kmul / gpd_kpgrad; csrc/kernels.hpp), with F(i, j) = k(xs_j, x_i):

    kvec     out[j]    = Σ_{i<n} F(i, j) α_i
    kmul     out[c][j] = Σ_{i<n} F(i, j) α_ci
    kpgrad   gm[p][j]  = Σ_i α_i ∂F/∂xs_jp,   gv[p][j] = −2 Σ_i w_ji ∂F/∂xs_jp,   ∂F/∂xs_p = 2 s_p σ² κ'(d²)(u*_p − u_p)  (single kind)  |  ∂k/∂t_p  (composite)

κ, κ', their per-element errors, γ and the composite closed forms (σ₁²·Periodic·RQ∘Scale + σ₂²·White) are those of tests/grad_units_ref.py — imported, not restated.
Everything is evaluated in np.longdouble from exactly the T-rounded values the device gets, widened.

THE BOUND of an output, componentwise (u = the unit roundoff of T, u64 = 2⁻⁵³):

    |Δ| <= Σ_i |w_i| e(i, j)  +  γ_m(·) Σ_i |w_i| (|F(i, j)| + e(i, j))          (+ the final rounding to T where there is one)

  e    the per-element error of the kernel value evaluated in T: σ²·(1e-14 | (D + 16)·u32) for a single kind (unit_helpers.assemble_bound — it covers the product
       variance·κ), the composite forms' δ_P + δ_R (+ γ_3(u): the two products σ₁²·κ_P·κ_R and the sum of the terms, ksum_eval) for the composite kernel; for kpgrad
       the error of κ'·t_p from grad_units_ref.elem_errors: |t_p| (e_κ'(1 + u) + |κ'| u), the difference t_p = fl(u*_p − u_p) carrying one u.
  m    counted from the kernels:
       kvec    the product (variance·κ)·α_i is formed in T: ONE rounding u on top of e (the product variance·κ is inside e).  The sum is fp64: a per-thread chain of
               ceil(n/256) adds, 6 wave shuffles, 3 LDS adds  →  m64 = ceil(n/256) + 9, γ_m64(u64).  Then one rounding to T: u·|computed sum|.
               bound = E + u·(|S| + E),  E = Σ|α|e + (u + γ_m64(u64)(1 + u)) Σ|α|(|F| + e).
       kmul    the A fragment is variance·κ in T (inside e); the MFMA accumulates products and sums in T over the strips of the workgroup's share — 32·sps terms,
               the masked ones exact zeros — and kmul_reduce_kernel adds the nsplit slices in T: m = 32·sps + (nsplit − 1), γ_m(u) (the dot-product bound, whatever
               the order inside an MFMA).  A single kind with D > 16 takes kvec, and its bound.
       kpgrad  everything after κ' is fp64: cm = α_i·κ' (1), cm·t_p (1), the chain ceil(n/256), 6 shuffles, 3 LDS adds, sm·s_p·v (2)  →  m64 = ceil(n/256) + 13.
               Composite: ksum_gradx forms ∂k/∂t_p in fp64 from the T-valued factors (16 operations, as grad_units_ref counts them for kgradx_sum_kernel), then
               cm·g_p (1), the same chain and reduction, the final scale (2)  →  m64 = ceil(n/256) + 28.
  A bound of 0 (no weight reaches the output, or every term is exact) demands an error of 0.  One-hot weights: every other term is an exact zero, sums with zeros are
  exact, so the bound is e alone (+ the final rounding for kvec).

kmul_split restates the host rule (csrc/gpmi355.hip kmul_split) from its inputs n and ns — the tests assert the ctx counter "cols_kernel_splits" against it."""
import numpy as np

from tests.grad_units_ref import LD, U32, U64, Out, _wide, composite_dt, composite_parts, elem_errors, gamma, kappa_dk, ratio, unit  # noqa: F401

KMUL_TM, KMUL_KS = 64, 32


def kmul_split(n, ns):
    """(nsplit, strips per split) of a kmul launch: strips of 32 training points dealt out until about 512 workgroups exist, never fewer than 4 strips each"""
    tiles, nstrips = (ns + KMUL_TM - 1) // KMUL_TM, (n + KMUL_KS - 1) // KMUL_KS
    nsplit = min((512 + tiles - 1) // tiles, max(1, nstrips // 4))
    sps = (nstrips + nsplit - 1) // nsplit
    return (nstrips + sps - 1) // sps, sps


def _diffs(xs, x):
    """t_p[j, i] = xs[p][j] − x[p][i] (rows: test points), longdouble"""
    xs, x = _wide(xs), _wide(x)
    return [xs[p][:, None] - x[p][None, :] for p in range(xs.shape[0])]


class Elements:
    """F[j, i] = k(xs_j, x_i) with its per-element error e, and (lazily, per dimension) dF[p][j, i] = ∂F/∂xs_jp with its error de[p]"""

    def __init__(self, F, e, dF):
        self.F, self.e, self._dF = F, e, dF

    def dF(self, p):
        return self._dF(p)


def kind_elements(kind, variance, nscale, scale, xs, x):
    """a single kind on pre-scaled T-valued inputs xs [d][ns], x [d][n]"""
    npdt = np.asarray(x).dtype
    u, D, var = unit(npdt), x.shape[0], LD(variance)
    t = _diffs(xs, x)
    d2 = sum(tp * tp for tp in t)
    kap, dk = kappa_dk(kind, d2)
    e_k, e_dk, _ = elem_errors(kind, d2, D, npdt)

    def dF(p):
        sp = LD(1) if nscale == 0 else LD(scale[0] if nscale == 1 else scale[p])
        return 2 * sp * var * dk * t[p], 2 * sp * var * np.abs(t[p]) * (e_dk * (1 + u) + np.abs(dk) * u)

    return Elements(var * kap, var * e_k, dF)


def composite_elements(s1, r, s, a, s2, xs, x):
    """k = σ₁²·Periodic(r)·RQ(α)∘Scale(s) + σ₂²·White on RAW T-valued inputs (θ values exactly representable in T)"""
    npdt = np.asarray(x).dtype
    u = unit(npdt)
    s1, s, a, s2 = LD(s1), LD(s), LD(a), LD(s2)
    rr = [LD(v) for v in r]
    t = _diffs(xs, x)
    c_ = composite_parts(rr, s, a, t, u)
    main = s1 * c_["kP"] * c_["kR"]
    F = main + s2 * c_["eq"].astype(LD)
    rel = (1 + c_["dPR"]) * (1 + gamma(3, u)) - 1
    e = main * rel + u * (F + main * rel)

    def dF(p):
        A, B, EA, EB = composite_dt(c_, s1, rr, s, t, p, u)
        return A + B, EA + EB

    return Elements(F, e, dF)


def kvec_reference(el, alpha, npdt):
    """out[j] = Σ_i F[j, i] α_i: Out with val / abs / bound of shape [ns]"""
    u = unit(npdt)
    a = _wide(alpha)[None, :]
    n = a.shape[1]
    S = (el.F * a).sum(1)
    mag = (np.abs(a) * (np.abs(el.F) + el.e)).sum(1)
    m64 = -(-n // 256) + 9
    E = (np.abs(a) * el.e).sum(1) + (u + gamma(m64, U64) * (1 + u)) * mag
    if np.count_nonzero(_wide(alpha)) <= 1:  # a single weight: one product rounding, every sum is with exact zeros
        E = (np.abs(a) * el.e).sum(1) + u * mag
    return Out(S, mag, E + u * (np.abs(S) + E), 0)


def kmul_reference(el, alpha, n, ns, npdt):
    """out[c][j] = Σ_i F[j, i] α_ci for alpha [S][n]: Out of shape [S][ns].  m from kmul_split(n, ns)."""
    u = unit(npdt)
    A = _wide(alpha)
    nsplit, sps = kmul_split(n, ns)
    g = gamma(32 * sps + nsplit - 1, u)
    val = A @ el.F.T
    mag = np.abs(A) @ (np.abs(el.F) + el.e).T
    onehot = np.count_nonzero(A, axis=1) <= 1  # a column with a single weight: its other terms are exact zeros — e (and the product's rounding) alone
    bound = np.abs(A) @ el.e.T + np.where(onehot[:, None], u, g) * mag
    return Out(val, mag, bound, 0)


def kpgrad_reference(el, d, alpha, W, n, composite=False):
    """gm [d][ns] from alpha [n] (or None), gv [d][ns] from W [ns][n] (or None): (Out | None, Out | None)"""
    m64 = -(-n // 256) + (28 if composite else 13)
    g = gamma(m64, U64)
    gm, gv = [], []
    for p in range(d):
        dF, de = el.dF(p)
        if alpha is not None:
            a = _wide(alpha)[None, :]
            mag = (np.abs(a) * (np.abs(dF) + de)).sum(1)
            gm.append(Out((a * dF).sum(1), mag, (np.abs(a) * de).sum(1) + g * mag, 0))
        if W is not None:
            w = _wide(W)
            mag = 2 * (np.abs(w) * (np.abs(dF) + de)).sum(1)
            gv.append(Out(-2 * (w * dF).sum(1), mag, 2 * (np.abs(w) * de).sum(1) + g * mag, 0))
    stack = lambda L: Out(np.stack([o.val for o in L]), np.stack([o.abs for o in L]), np.stack([o.bound for o in L]), 0) if L else None  # noqa: E731
    return stack(gm), stack(gv)
