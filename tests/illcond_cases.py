"""Ill-conditioned SPD inputs and componentwise backward-error measures for the factorisation and solve tests (tests/test_illcond_cpu.py on the host,
tests/test_gpu_backward_error.py on the device).  numpy / scipy only: no torch, no device.

Two seeded families, each cast to the dtype under test FIRST; every reference product below is then formed in np.longdouble from the cast values.

  gp    x = sort(default_rng(0).uniform(0, 1, n)), A = exp(−½ (x_i − x_j)² / 0.3²) + σ² I.  Graded: the factor's diagonal falls from 1 to about σ.
        fp64 σ² = 1e-4 / 1e-8 / 1e-10 (cond ≈ 2e6 / 2e10 / 2e12 at n = 320, diagonal ratio of the factor 95 / 9.3e3 / 9.2e4: the last just under the 1e5 guard of the
        explicit-inverse paths), fp32 σ² = 1e-1 / 1e-2 / 1e-3 (diagonal ratio 3 / 10 / 30, under the fp32 guard of 300).
  spec  A = Q diag(λ) Qᵀ symmetrised, Q from the QR of a seeded Gaussian, λ geometric from 1 down to 1 / cond; cond = 1e4 / 1e8 / 1e10 (fp64), 1e2 / 1e3 (fp32).
        Not graded: the diagonal blocks are ill-conditioned in a different way.

Measures (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.; u = 2⁻⁵³ or 2⁻²⁴, γ_m = m·u / (1 − m·u)); each returns max error / bound over components:

  F  |A − L̂L̂ᵀ| <= γ_{n+1} |L̂||L̂|ᵀ on the lower triangle                 (Theorem 10.3)
  R  |X̂L̂ᵀ − X| <= γ_n |X̂||L̂|ᵀ                                          (Theorem 8.5, row form)
  V  |L̂x̂ − b| <= γ_n |L̂||x̂|, and the same with L̂ᵀ                        (Theorem 8.5)
  A  |Cα̂ − δ| <= γ_{3n+1} |L̂||L̂ᵀ||α̂|                                   (Theorem 10.4)
  D  |d̂ − Σ log L̂_ii| <= γ_{n+2} Σ|log L̂_ii| (both sides times 2 for logdet): n − 1 additions and a log correct to a few u
  Q  |q̂ − zᵀz| <= 2 γ_n |z|ᵀ|L̂⁻¹||L̂||z| + γ_n zᵀz, z = L̂⁻¹δ in longdouble: first order, the solve's backward error (V) carried to z, then the sum of squares

D and Q are conditional on the factor they are given, so they test the reduction and the solve, not cond(C).

A longdouble product runs at about 0.2 Gflop/s, so above n = 576 F and R are evaluated on a fixed sample of rows (row i of L̂L̂ᵀ needs L̂[i, :]·L̂[:i+1, :]ᵀ only): every
row of the last 64-row tile, the first row of every 64-row tile and 32 seeded rows."""
import functools

import numpy as np
import scipy.linalg as sla

LD = np.longdouble
assert np.finfo(LD).eps < 1.2e-19, "np.longdouble is not the 64-bit-mantissa extended type here: the references would be no better than the results under test"

U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
NPDT = {"f64": np.float64, "f32": np.float32}
GP_LEVELS = {"f64": (1e-4, 1e-8, 1e-10), "f32": (1e-1, 1e-2, 1e-3)}
SPEC_CONDS = {"f64": (1e4, 1e8, 1e10), "f32": (1e2, 1e3)}
GP_ELL = 0.3
FULL_MAX_N = 576


def cases(prec):
    """(family, level) of every case of a precision"""
    return [("gp", s2) for s2 in GP_LEVELS[prec]] + [("spec", c) for c in SPEC_CONDS[prec]]


def case_id(c):
    return f"{c[0]}-{c[1]:g}"


def gamma(m, u):
    assert m * u < 1
    return m * u / (1.0 - m * u)


@functools.lru_cache(maxsize=None)
def gp_x(n):
    return np.sort(np.random.default_rng(0).uniform(0.0, 1.0, n))


def gp_inputs(n, prec):
    """the GP family's points as the API-level tests pass them: divided by the length scale (a kernel without a transform then gives the family's matrix) and cast"""
    return (gp_x(n) / GP_ELL).astype(NPDT[prec])


def gp_kernel_ld(xa, xb):
    """exp(−½ (a_i − b_j)²) in longdouble from the given (already cast) inputs"""
    d = xa.astype(LD)[:, None] - xb.astype(LD)[None, :]
    return np.exp(-d * d / 2)


@functools.lru_cache(maxsize=None)
def matrix(family, n, level, prec):
    """the n × n input in the working precision (read-only: shared among tests)"""
    if family == "gp":
        x = gp_x(n)
        d = x[:, None] - x[None, :]
        A = np.exp(-0.5 * d * d / GP_ELL ** 2) + level * np.eye(n)
    else:
        Q, _ = np.linalg.qr(np.random.default_rng(n).standard_normal((n, n)))
        lam = float(level) ** (-np.arange(n) / max(n - 1, 1))
        A = (Q * lam) @ Q.T
        A = (A + A.T) / 2
    A = A.astype(NPDT[prec])
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def lapack_factor(family, n, level, prec):
    """LAPACK's lower factor in the working precision; a failure on any of these inputs is an error (info is asserted)"""
    L, info = sla.lapack.get_lapack_funcs("potrf", (matrix(family, n, level, prec),))(matrix(family, n, level, prec), lower=1, clean=1)
    assert info == 0, (family, n, level, prec, info)
    assert L.dtype == NPDT[prec]
    L.setflags(write=False)
    return L


def rhs(shape, seed, prec):
    return np.random.default_rng(seed).standard_normal(shape).astype(NPDT[prec])


def sample_rows(n, ncols=None):
    """the rows (of an n-row matrix with ncols columns, ncols = n by default) F and R are evaluated on: all of them up to ncols = FULL_MAX_N, beyond it the fixed sample
    of the module docstring above"""
    if (n if ncols is None else ncols) <= FULL_MAX_N:
        return np.arange(n)
    fixed = np.concatenate([np.arange((n - 1) // 64 * 64, n), np.arange(0, n, 64)])
    return np.unique(np.concatenate([fixed, np.random.default_rng(n).integers(0, n, 32)]))


def _max_ratio(err, bound):
    """max over components of err / bound; a component with bound 0 must have err 0 (it counts as inf otherwise)"""
    if err.size == 0:
        return 0.0
    tiny = LD(np.finfo(np.float64).tiny)
    return float(np.max(err / np.maximum(bound, tiny)))


def times_Lt(X, Ll, bs=64):
    """X · Lᵀ for a lower-triangular L in longdouble, column block by column block, so that the zero half of L costs nothing"""
    n = Ll.shape[0]
    out = np.empty((X.shape[0], n), dtype=LD)
    for j0 in range(0, n, bs):
        j1 = min(j0 + bs, n)
        out[:, j0:j1] = X[:, :j1] @ Ll[j0:j1, :j1].T
    return out


def _diag_blocks(n, w, segments):
    """(j0, j1) of the w-wide diagonal blocks, aligned from the start of each segment of columns"""
    edges = list(segments) + [n]
    return [(j0, min(j0 + w, e1)) for e0, e1 in zip(edges[:-1], edges[1:]) for j0 in range(e0, e1, w)]


def inverse_kernel(T):
    """|T⁻ᵀ||Tᵀ| of a lower-triangular block (fp64 inverse: it enters bounds only)"""
    Ti = sla.solve_triangular(np.tril(T).astype(np.float64), np.eye(T.shape[0]), lower=True)
    return np.abs(Ti).T.astype(LD) @ np.abs(np.tril(T)).T.astype(LD)


def measure_F(A, L, u, tol=0.0, inverse=(), segments=(0,)):
    """A: the matrix that was factored (lower triangle read; any dtype, longdouble included), L: the computed lower factor.  Returns (ratio, ratio_subst):
    ratio_subst is F as it stands (+ tol, the tolerance of A's own entries, in the bound); ratio adds to the bound, for every (w, span) in `inverse`, the term of
    the explicit inverses of the w × w diagonal blocks T = L̂[J, J] (blocks aligned from the start of each of `segments`): the block X̂ = L̂[i, J] of a row i below
    the block (and inside the same span-aligned block, if span) is computed as S·Ŵᵀ, S the updated block and Ŵ ≈ T⁻¹ with the right residual |TŴ − I| <= γ_w |T||Ŵ|
    of an inverse formed by substitution (Higham §14.2, Method 1).  Then X̂Tᵀ − S = S (TŴ − I)ᵀ + ΔTᵀ with |Δ| <= γ_w |S||Ŵᵀ| (§3.5), so
    |X̂Tᵀ − S| <= 2γ_w |S||T⁻ᵀ||Tᵀ| to first order, with S = X̂Tᵀ (§14.1: solving with an inverse is stable only up to cond(T))."""
    n = A.shape[0]
    Ll = np.tril(L).astype(LD)
    La = np.abs(Ll)
    rows = sample_rows(n)
    if len(rows) == n:
        prod, base = times_Lt(Ll, Ll), times_Lt(La, La)
    else:
        prod, base = np.zeros((len(rows), n), dtype=LD), np.zeros((len(rows), n), dtype=LD)
        for k, i in enumerate(rows):
            prod[k, :i + 1] = Ll[:i + 1, :i + 1] @ Ll[i, :i + 1]
            base[k, :i + 1] = La[:i + 1, :i + 1] @ La[i, :i + 1]
    mask = np.arange(n)[None, :] <= rows[:, None]
    err = np.abs(np.asarray(A)[rows].astype(LD) - prod)
    base = gamma(n + 1, u) * base + LD(tol)
    extra = np.zeros_like(base)
    for w, span in inverse:
        for j0, j1 in _diag_blocks(n, w, segments):
            end = n if not span else min(n, (j0 // span + 1) * span)
            sel = (rows >= j1) & (rows < end)
            if sel.any():
                T = Ll[j0:j1, j0:j1]
                extra[sel, j0:j1] += 2 * gamma(w, u) * (np.abs(Ll[rows[sel], j0:j1] @ T.T) @ inverse_kernel(T))
    return _max_ratio(err[mask], (base + extra)[mask]), _max_ratio(err[mask], base[mask])


def measure_R(X0, Xh, L, u):
    """Xh: the computed X0 · L⁻ᵀ (rows below a factor, or a triangular solve from the right)"""
    n = L.shape[0]
    rows = sample_rows(X0.shape[0], n)
    Ll = np.tril(L).astype(LD)
    Xl = Xh[rows].astype(LD)
    return _max_ratio(np.abs(times_Lt(Xl, Ll) - X0[rows].astype(LD)), gamma(n, u) * times_Lt(np.abs(Xl), np.abs(Ll)))


def measure_V(L, x, b, u, forward):
    """x: the computed solution of L x = b (forward) or Lᵀ x = b; x and b are n × nrhs"""
    n = L.shape[0]
    T = np.tril(L).astype(LD)
    T = T if forward else T.T
    xl = x.astype(LD)
    return _max_ratio(np.abs(T @ xl - b.astype(LD)), gamma(n, u) * (np.abs(T) @ np.abs(xl)))


def measure_V_tiles(L, x, b, u, forward, w=64):
    """V for a solve whose w-wide steps multiply by the explicit inverse Ŵ ≈ T⁻¹ of the diagonal tile T (formed column by column by substitution: right residual
    |TŴ − I| <= γ_{w+1} |T||Ŵ|, the + 1 for the reciprocal of the diagonal).  Forward, x_J = Ŵ r: T x̂ − r = (TŴ − I) r + T Δ, |Δ| <= γ_w |Ŵ||r|, so
    |T x̂ − r| <= 2γ_{w+1} |T||T⁻¹||r|.  Backward, x_J = Ŵᵀ r: Tᵀx̂ − r = (ŴT − I)ᵀ r + TᵀΔ, and such an inverse has no small LEFT residual of its own:
    ŴT − I = T⁻¹ (TŴ − I) T, so (ŴT − I)ᵀ r = Tᵀ (TŴ − I)ᵀ (T⁻ᵀ r) with T⁻ᵀ r the solution itself: |Tᵀx̂ − r| <= γ_{w+1} |Tᵀ||T⁻ᵀ||Tᵀ||x̂| + γ_w |Tᵀ||T⁻ᵀ||r|.  Both to first
    order with r = T x̂ (Tᵀ x̂); the term is added to V's bound on the rows of the tile.  Returns (ratio, ratio_subst)."""
    n = L.shape[0]
    T = np.tril(L).astype(LD)
    T = T if forward else T.T
    xl = x.astype(LD)
    err = np.abs(T @ xl - b.astype(LD))
    base = gamma(n, u) * (np.abs(T) @ np.abs(xl))
    extra = np.zeros_like(base)
    for j0 in range(0, n, w):
        J = slice(j0, min(j0 + w, n))
        Tj = np.tril(L[J, J]).astype(np.float64)
        Ti, Ta = np.abs(sla.solve_triangular(Tj, np.eye(Tj.shape[0]), lower=True)).astype(LD), np.abs(Tj).astype(LD)
        if forward:
            extra[J] = 2 * gamma(w + 1, u) * (Ta @ (Ti @ np.abs(Tj.astype(LD) @ xl[J])))
        else:
            extra[J] = gamma(w + 1, u) * (Ta.T @ (Ti.T @ (Ta.T @ np.abs(xl[J])))) + gamma(w, u) * (Ta.T @ (Ti.T @ np.abs(Tj.T.astype(LD) @ xl[J])))
    return _max_ratio(err, base + extra), _max_ratio(err, base)


def _tile_terms(L, v, u, w):
    """(e_f, e_b) of measure_V_tiles' bounds for the w-wide tiles of L at the solution v (n × k): the forward term with r = T v_J, the backward one with r = Tᵀ v_J"""
    n = L.shape[0]
    ef, eb = np.zeros(v.shape, dtype=LD), np.zeros(v.shape, dtype=LD)
    for j0 in range(0, n, w):
        J = slice(j0, min(j0 + w, n))
        Tj = np.tril(L[J, J]).astype(np.float64)
        Ti, Ta = np.abs(sla.solve_triangular(Tj, np.eye(Tj.shape[0]), lower=True)).astype(LD), np.abs(Tj).astype(LD)
        ef[J] = 2 * gamma(w + 1, u) * (Ta @ (Ti @ np.abs(Tj.astype(LD) @ v[J])))
        eb[J] = gamma(w + 1, u) * (Ta.T @ (Ti.T @ (Ta.T @ np.abs(v[J])))) + gamma(w, u) * (Ta.T @ (Ti.T @ np.abs(Tj.T.astype(LD) @ v[J])))
    return ef, eb


def measure_A(C, L, alpha, delta, u, tol=0.0, inverse=(), segments=(0,), tiles=0):
    """alpha: the computed C⁻¹δ (n or n × k); C symmetric and complete (any dtype); L: the factor of Theorem 10.4's bound; tol: the tolerance of C's own entries,
    + tol·‖α̂‖₁ in the bound.  Returns (ratio, ratio_subst): ratio_subst is Theorem 10.4 as it stands.  ratio is for a fit whose factor carries the explicit-inverse terms
    E of measure_F (`inverse`, `segments`) and whose two sweeps run through w = `tiles`-wide inverse tiles (measure_V_tiles): with C = L̂L̂ᵀ + ΔC, L̂ẑ = δ + f, L̂ᵀα̂ = ẑ + b,
    Cα̂ − δ = ΔCα̂ + L̂b + f, so beside Theorem 10.4's γ_{3n+1} |L̂||L̂ᵀ||α̂| the bound gets E|α̂| + |L̂| e_b(α̂) + e_f(ẑ), ẑ = L̂ᵀα̂ to first order."""
    n = C.shape[0]
    Ll = np.tril(L).astype(LD)
    La = np.abs(Ll)
    al = alpha.astype(LD).reshape(n, -1)
    err = np.abs(np.asarray(C).astype(LD) @ al - delta.astype(LD).reshape(n, -1))
    base = gamma(3 * n + 1, u) * (La @ (La.T @ np.abs(al))) + LD(tol) * np.abs(al).sum(0)
    extra = np.zeros_like(base)
    if inverse:
        E = np.zeros((n, n), dtype=LD)
        for w, span in inverse:
            for j0, j1 in _diag_blocks(n, w, segments):
                end = n if not span else min(n, (j0 // span + 1) * span)
                if j1 < end:
                    T = Ll[j0:j1, j0:j1]
                    E[j1:end, j0:j1] += 2 * gamma(w, u) * (np.abs(Ll[j1:end, j0:j1] @ T.T) @ inverse_kernel(T))
        extra += (E + E.T) @ np.abs(al)
    if tiles:
        ef, _ = _tile_terms(L, Ll.T @ al, u, tiles)
        _, eb = _tile_terms(L, al, u, tiles)
        extra += La @ eb + ef
    return _max_ratio(err, base + extra), _max_ratio(err, base)


def measure_D(L, got, u, logdet=False):
    """got: the returned Σ log L_ii (or logdet = twice that) against the same sum in longdouble from the returned factor"""
    n = L.shape[0]
    lg = np.log(np.diagonal(L).astype(LD))
    k = 2 if logdet else 1
    return float(abs(LD(got) - k * lg.sum()) / max(k * gamma(n + 2, u) * np.abs(lg).sum(), LD(np.finfo(np.float64).tiny)))


def measure_Q(L, got, delta, u):
    """got[j]: the returned ‖L⁻¹δ_j‖² against the longdouble value from the returned factor (delta n × k)"""
    n = L.shape[0]
    Ll = np.tril(L).astype(LD)
    z = solve_lower_ld(Ll, delta.astype(LD))
    Linv = np.abs(sla.solve_triangular(np.tril(L).astype(np.float64), np.eye(n), lower=True)).astype(LD)
    za = np.abs(z)
    bound = 2 * gamma(n, u) * np.einsum("ij,ij->j", za, Linv @ (np.abs(Ll) @ za)) + gamma(n, u) * (z * z).sum(0)
    return _max_ratio(np.abs(np.asarray(got).astype(LD) - (z * z).sum(0)), bound)


def solve_lower_ld(Ll, B):
    """L⁻¹B by forward substitution in longdouble (B n × k)"""
    n = Ll.shape[0]
    Z = np.array(B, dtype=LD, copy=True)
    for i in range(n):
        Z[i] = (Z[i] - Ll[i, :i] @ Z[:i]) / Ll[i, i]
    return Z


def cholesky_ld(C):
    """the lower factor in longdouble (the reference factor of the calls that return none)"""
    n = C.shape[0]
    L = np.zeros((n, n), dtype=LD)
    A = C.astype(LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0, (j, d)
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


# ---- host emulations of the two explicit-inverse designs (fp64 NumPy, the same order of operations block by block) ------------------------------------------
def _inverse_by_columns(T):
    """inv(T) column by column by forward substitution on the identity: what trtri_64_kernel and the leaves' rank-1 chain compute (right residual small)"""
    return sla.solve_triangular(T, np.eye(T.shape[0]), lower=True)


def _inverse_by_rows(T):
    """inv(T) row by row by substitution on Tᵀ (left residual small): the variant that was tried for the backward sweep"""
    return sla.solve_triangular(T.T, np.eye(T.shape[0]), lower=False).T


def emulate_leaf_cholesky(A, w=16):
    """blocked Cholesky as every leaf does it: the w × w diagonal block by plain Cholesky, the blocks below it as (updated block)·inv(T)ᵀ"""
    n = A.shape[0]
    A = np.tril(np.asarray(A, dtype=np.float64))
    L = np.zeros_like(A)
    for j in range(0, n, w):
        J = slice(j, min(j + w, n))
        D = A[J, J] - L[J, :j] @ L[J, :j].T
        L[J, J] = np.linalg.cholesky(np.tril(D) + np.tril(D, -1).T)
        if J.stop < n:
            L[J.stop:, J] = (A[J.stop:, J] - L[J.stop:, :j] @ L[J, :j].T) @ _inverse_by_columns(L[J, J]).T
    return L


def emulate_tile_solve(L, b, forward, w=64, by_rows=False):
    """the vector solves as trsv does them: each w-wide step a product with inv(T) of the diagonal tile, the rest of the vector updated behind it"""
    n = L.shape[0]
    x = np.array(b, dtype=np.float64, copy=True)
    tiles = [(j, min(j + w, n)) for j in range(0, n, w)]
    for j0, j1 in (tiles if forward else tiles[::-1]):
        T = L[j0:j1, j0:j1]
        W = _inverse_by_rows(T) if (by_rows and not forward) else _inverse_by_columns(T)
        x[j0:j1] = (W if forward else W.T) @ x[j0:j1]
        if forward:
            x[j1:] -= L[j1:, j0:j1] @ x[j0:j1]
        else:
            x[:j0] -= L[j0:j1, :j0].T @ x[j0:j1]
    return x

