"""CPU: the longdouble reference of the gradient-contraction unit tests (tests/grad_units_ref.py) against a 40-digit mpmath restatement of the same sums, in the
style of oracle/mp_check.py: a small case of every kind and transform, input values drawn in fp64 and in fp32 (widened exactly).  The reference has to agree within
1e-3 of the fp64 bound it hands to the GPU tests — so what those tests measure is the kernel, not the reference."""
import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from tests import grad_units_ref as R  # noqa: E402

mp.mp.dps = 40
VARIANCE = 1.5
N, NR, NC, D = 10, 9, 7, 3


def M(v):
    return mp.mpf(float(v))  # a float64 (or widened float32) value, exactly


def kd_mp(kind, d2):
    if kind == 0:
        k = mp.e ** (-d2 / 2)
        return k, -k / 2
    r = mp.sqrt(d2)
    if kind == 1:
        k = mp.e ** (-r)
        return k, (-k / (2 * r) if r > 0 else mp.mpf(0))
    if kind == 2:
        a = mp.sqrt(3) * r
        e = mp.e ** (-a)
        return (1 + a) * e, -mp.mpf(3) / 2 * e
    a = mp.sqrt(5) * r
    e = mp.e ** (-a)
    return (1 + a + mp.mpf(5) / 3 * d2) * e, -mp.mpf(5) / 6 * (1 + a) * e


def mp_sums(kind, nscale, scale, xr, xc, weight, nr, nc, zfac):
    """g0, gs, rows [d][nr], cols [d][nc], rowk(w2) helpers over every (i, j) with weight(i, j) != None"""
    d = xr.shape[0]
    var = mp.mpf(VARIANCE)
    g0, gs = mp.mpf(0), [mp.mpf(0) for _ in range(nscale)]
    rows = [[mp.mpf(0)] * nr for _ in range(d)]
    cols = [[mp.mpf(0)] * nc for _ in range(d)]
    kap = [[None] * nc for _ in range(nr)]
    for i in range(nr):
        for j in range(nc):
            t = [M(xr[p, i]) - M(xc[p, j]) for p in range(d)]
            d2 = sum(tp * tp for tp in t)
            k, dk = kd_mp(kind, d2)
            kap[i][j] = k
            w = weight(i, j)
            if w is None:
                continue
            g0 += w * k
            if nscale == 1:
                gs[0] += w * var * dk * 2 * d2 / M(scale[0])
            for p in range(d):
                if nscale > 1:
                    gs[p] += w * var * dk * 2 * t[p] * t[p] / M(scale[p])
                sp = mp.mpf(1) if nscale == 0 else M(scale[0] if nscale == 1 else scale[p])
                f = w * var * dk * 2 * sp * t[p]
                rows[p][i] += f
                cols[p][j] -= zfac * f
    return g0, gs, rows, cols, kap


def close(name, got, want, bound):
    got, bound = np.asarray(got, dtype=R.LD).ravel(), np.asarray(bound, dtype=R.LD).ravel()
    want = np.asarray(want, dtype=object).ravel()
    for g, w, b in zip(got, want, bound):
        hi = float(g)
        err = abs(mp.mpf(hi) + mp.mpf(float(g - R.LD(hi))) - w)  # a longdouble as the exact sum of two doubles
        assert err <= mp.mpf(1e-3) * mp.mpf(float(b)), (name, float(err), float(b))


def problem(npdt, kind, nscale, seed):
    rng = np.random.default_rng(seed)
    scale = (0.5 + rng.random(nscale)).tolist()
    draw = lambda *s: rng.standard_normal(s).astype(npdt).astype(np.float64)  # noqa: E731  (T values, widened: the bound is the fp64 one)
    pts = lambda n: (rng.random((D, n)) * np.sqrt(6.0 / D)).astype(npdt).astype(np.float64)  # noqa: E731
    return rng, scale, draw, pts


CASES = [(kind, nscale, npdt) for kind in range(4) for nscale in (0, 1, D) for npdt in (np.float64, np.float32)]


@pytest.mark.parametrize("kind,nscale,npdt", CASES, ids=[f"kind{k}-ns{s}-{np.dtype(t).name}" for k, s, t in CASES])
def test_contract_reference_against_mpmath(kind, nscale, npdt):
    rng, scale, draw, pts = problem(npdt, kind, nscale, 100 * kind + nscale)
    x, ci, alpha = pts(N), draw(N, N), draw(N)
    x[:, 3] = x[:, 7]  # a coincident pair: Matern12's κ' = 0 branch
    ref = R.contract_reference(kind, VARIANCE, nscale, scale, x, ci, alpha, N, 128, True)

    def w_low(i, j):
        return None if j > i else (M(alpha[i]) * M(alpha[j]) + M(ci[i, j])) * (mp.mpf(0.5) if i == j else 1)

    def w_full(i, j):
        return None if i == j else M(alpha[i]) * M(alpha[j]) + M(ci[max(i, j), min(i, j)])

    g0, gs, _, _, _ = mp_sums(kind, nscale, scale, x, x, w_low, N, N, 0)
    _, _, rows, _, _ = mp_sums(kind, nscale, scale, x, x, w_full, N, N, 0)
    close("g0", ref["g0"].val, g0, ref["g0"].bound)
    if nscale:
        close("gs", ref["gs"].val, gs, ref["gs"].bound)
    close("gx", ref["gx"].val, rows, ref["gx"].bound)
    dn = [(M(alpha[i]) ** 2 + M(ci[i, i])) / 2 for i in range(N)]
    close("dn", ref["dn"].val, dn, ref["dn"].bound)
    close("g1", ref["g1"].val, sum(dn), ref["g1"].bound)
    assert all(float(b) > 0 for b in np.asarray(ref["gx"].bound).ravel())


@pytest.mark.parametrize("kind,nscale,npdt", CASES, ids=[f"kind{k}-ns{s}-{np.dtype(t).name}" for k, s, t in CASES])
@pytest.mark.parametrize("explicit_w", [0, 1])
def test_rect_reference_against_mpmath(kind, nscale, npdt, explicit_w):
    rng, scale, draw, pts = problem(npdt, kind, nscale, 1000 + 100 * kind + nscale + 7 * explicit_w)
    xr, xc, cm, rs, bv, nu = pts(NR), pts(NC), draw(NR, NC), draw(NR), draw(NR), rng.standard_normal(NC)
    xc[:, 2] = xr[:, 5]
    zfac = 2.0 if explicit_w else 1.0
    ref = R.rect_reference(kind, VARIANCE, nscale, scale, xr, xc, cm, explicit_w, rs, bv, nu, NR, NC, zfac, True)

    def w(i, j):
        return M(cm[i, j]) if explicit_w else M(rs[i]) * (-2 * M(cm[i, j]) + M(bv[i]) * M(nu[j]))

    g0, gs, rows, cols, kap = mp_sums(kind, nscale, scale, xr, xc, w, NR, NC, mp.mpf(zfac))
    close("g0", ref["g0"].val, g0, ref["g0"].bound)
    if nscale:
        close("gs", ref["gs"].val, gs, ref["gs"].bound)
    close("gx", ref["gx"].val, rows, ref["gx"].bound)
    close("gz", ref["gz"].val, cols, ref["gz"].bound)
    if not explicit_w:
        var = mp.mpf(VARIANCE)
        close("rowq", ref["rowq"].val, [sum(-var * kap[i][j] * M(cm[i, j]) for j in range(NC)) for i in range(NR)], ref["rowq"].bound)
        close("rowp", ref["rowp"].val, [sum(var * kap[i][j] * M(nu[j]) for j in range(NC)) for i in range(NR)], ref["rowp"].bound)
    else:
        assert "rowq" not in ref


def test_per_element_error_of_the_derivative_matches_a_direct_perturbation():
    """e_κ' of grad_units_ref.elem_errors is |d²κ''|·ε_d + (evaluation): its first part must cover κ'(d²(1 ± ε_d)) − κ'(d²) computed directly in mpmath — the
    closed forms of d²κ'' in the docstring are what this pins (a wrong one would make every GPU bound wrong in the same direction)."""
    for kind in range(4):
        for d2 in (1e-3, 0.3, 1.0, 2.5, 6.0):
            for npdt, Dn in ((np.float64, 3), (np.float32, 33)):
                _, e_dk, eps = R.elem_errors(kind, np.array([d2], dtype=R.LD), Dn, npdt)
                _, dk0 = kd_mp(kind, mp.mpf(d2))
                ev = (3 * {0: d2 / 2, 1: d2 ** 0.5, 2: (3 * d2) ** 0.5, 3: (5 * d2) ** 0.5}[kind] + 16) * R.unit(npdt)
                first = mp.mpf(float(e_dk[0])) - abs(dk0) * ev / (1 - ev)
                for sgn in (-1, 1):
                    _, dk1 = kd_mp(kind, mp.mpf(d2) * (1 + sgn * mp.mpf(eps)))
                    moved = abs(dk1 - dk0)
                    assert moved <= first * (1 + 1e-3) + mp.mpf(1e-25), (kind, d2, float(moved), float(first))
                    assert moved >= first * mp.mpf(0.5), (kind, d2, float(moved), float(first))  # and is no gross over-estimate


@pytest.mark.parametrize("npdt", [np.float64, np.float32], ids=["float64", "float32"])
def test_composite_reference_against_mpmath(npdt):
    """grad_units_ref.composite_reference (σ₁² Periodic · RQ∘Scale + σ₂² White) against the same sums in mpmath; θ values exact in fp32; one coincident pair (White)"""
    n, d = 8, D
    rng = np.random.default_rng(77)
    s1, r, s, a, s2 = 1.5, [0.75, 1.25, 0.875], 1.25, 2.5, 0.25
    x = (rng.random((d, n)) * np.sqrt(6.0 / d)).astype(npdt).astype(np.float64)
    x[:, 2] = x[:, 6]
    ci, alpha = rng.standard_normal((n, n)).astype(npdt).astype(np.float64), rng.standard_normal(n).astype(npdt).astype(np.float64)
    ref = R.composite_reference(s1, r, s, a, s2, x, ci, alpha, n, 128)
    th = [mp.mpf(0)] * (d + 4)
    gx = [[mp.mpf(0)] * n for _ in range(d)]
    for i in range(n):
        for j in range(n):
            t = [M(x[p, i]) - M(x[p, j]) for p in range(d)]
            sn = [mp.sinpi(tp) for tp in t]
            kP = mp.e ** (-sum((sp / M(rp)) ** 2 for sp, rp in zip(sn, r)) / 2)
            r2 = sum(tp * tp for tp in t)
            q = M(s) ** 2 * r2 / (2 * M(a))
            kR = mp.e ** (-M(a) * mp.log1p(q))
            dk = -kR / (2 * (1 + q))
            if j <= i:
                w = (M(alpha[i]) * M(alpha[j]) + M(ci[i, j])) * (mp.mpf(0.5) if i == j else 1)
                th[0] += w * kP * kR
                for p in range(d):
                    th[1 + p] += w * M(s1) * kR * kP * sn[p] ** 2 / M(r[p]) ** 3
                th[1 + d] += w * M(s1) * kP * dk * 2 * M(s) * r2
                th[2 + d] += w * M(s1) * kP * kR * (q / (1 + q) - mp.log1p(q))
                th[3 + d] += w * (1 if r2 == 0 else 0)
            if i != j:
                w = M(alpha[i]) * M(alpha[j]) + M(ci[max(i, j), min(i, j)])
                for p in range(d):
                    gx[p][i] += w * M(s1) * (-kR * kP * mp.pi / 2 * mp.sinpi(2 * t[p]) / M(r[p]) ** 2 + kP * 2 * dk * M(s) ** 2 * t[p])
    close("theta", ref["theta"].val, th, ref["theta"].bound)
    close("gx", ref["gx"].val, gx, ref["gx"].bound)
    assert float(ref["theta"].val[-1]) != float(ref["theta"].val[0]) and all(float(b) > 0 for b in np.asarray(ref["theta"].bound)[:-1])
