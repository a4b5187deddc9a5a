// kfun.hpp — the covariance functions as __device__ code, shared by every translation unit that evaluates a kernel on the device
// (kernels.hpp: kmat / kvec / kgrad and their composite forms; batch.hip: the batched small-problem kernels), and the derivatives the gradient kernels of both share.
#pragma once
#include "engine.hpp"
#include "kcommon.hpp"

namespace gpmi {

// ------------------------------------------------------------------------------------------------
// e^x for x <= 0 (every κ below evaluates exp at a non-positive argument).  fp64: Cody–Waite reduction x = n·ln2 + r with two fma, the
// degree-13 Taylor polynomial of e^r on |r| <= ln2/2 (truncation 4e-18 relative), v_ldexp_f64 — 19 instructions against the ≈ 35 of the
// library exp with its overflow / special-case handling (underflow falls out of ldexp; NaN propagates).  kmat_kernel is VALU-bound, not
// store-bound: the same tile stores with 32 dependent fma per element in front run at 5.7 TB/s, with 48 at 4.4 TB/s, the kernel itself at
// 4.6 TB/s (tools/kmat_probe.hip, round 5).  Agreement with the library exp: <= 2 ulp (tests: |ΔK| <= 1e-14·σ² against the oracle).
template <typename T> __device__ __forceinline__ T exp_nonpos(T x) { return exp(x); }
template <> __device__ __forceinline__ double exp_nonpos<double>(double x) {
    x = (x < -800.0) ? -800.0 : x;  // e^-800 underflows to 0 already; keeps n inside the int range (a NaN stays a NaN)
    const double n = __builtin_rint(x * 1.4426950408889634074);
    double r = fma(n, -0.69314718055994528623, x);
    r = fma(n, -2.3190468138462995584e-17, r);
    double p = 1.6059043836821614599e-10;            // 1/13!
    p = fma(p, r, 2.0876756987868098979e-09);        // 1/12!
    p = fma(p, r, 2.5052108385441718775e-08);        // 1/11!
    p = fma(p, r, 2.7557319223985890653e-07);        // 1/10!
    p = fma(p, r, 2.7557319223985892511e-06);        // 1/9!
    p = fma(p, r, 2.4801587301587301566e-05);        // 1/8!
    p = fma(p, r, 1.9841269841269841253e-04);        // 1/7!
    p = fma(p, r, 1.3888888888888889419e-03);        // 1/6!
    p = fma(p, r, 8.3333333333333332177e-03);        // 1/5!
    p = fma(p, r, 4.1666666666666664354e-02);        // 1/4!
    p = fma(p, r, 1.6666666666666665741e-01);        // 1/3!
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

template <typename T> __device__ __forceinline__ T kappa(int kind, T d2) {
    if (kind == 0) return exp_nonpos<T>(T(-0.5) * d2);
    const T d = sqrt(d2);
    if (kind == 1) return exp_nonpos<T>(-d);
    if (kind == 2) {
        const T a = T(1.7320508075688772935) * d;
        return (T(1) + a) * exp_nonpos<T>(-a);
    }
    const T a = T(2.2360679774997896964) * d;
    return (T(1) + a + T(5.0 / 3.0) * d2) * exp_nonpos<T>(-a);
}

// ---- composite kernels (KSum, engine.hpp): the evaluation kmat_sum_kernel / kvec_sum_kernel / kgrad_sum_kernel share (kernels.hpp describes the contract)
__device__ __forceinline__ double sinpi_t(double x) { return sinpi(x); }  // exact argument reduction, as Julia's sinpi
__device__ __forceinline__ float sinpi_t(float x) { return sinpif(x); }
__device__ __forceinline__ double log1p_t(double x) { return log1p(x); }
__device__ __forceinline__ float log1p_t(float x) { return log1pf(x); }

// d² of a non-periodic factor f: the raw r² (no transform), s²·r² (ScaleTransform), Σ_p (v_p t_p)² (ARDTransform)
template <typename T, int DR>
__device__ __forceinline__ T ksum_d2(const KSum& k, int f, const T (&t)[DR], T r2, int d) {
    const int ns = k.ns[f];
    if (ns == 0) return r2;
    if (ns == 1) {
        const T s = (T)k.th[k.so[f]];
        return s * s * r2;
    }
    T d2 = T(0);
#pragma unroll
    for (int p = 0; p < DR; ++p)
        if (p < d) {
            const T u = (T)k.th[k.so[f] + p] * t[p];
            d2 = fma(u, u, d2);
        }
    return d2;
}

// κ_f at the differences t (r2 = Σ t_p², eq: every t_p == 0)
template <typename T, int DR>
__device__ __forceinline__ T ksum_factor(const KSum& k, int f, const T (&t)[DR], T r2, bool eq, int d) {
    const int kind = k.kind[f];
    if (kind == 6) return eq ? T(1) : T(0);
    if (kind == 4) {
        const int ns = k.ns[f];
        T acc = T(0);
#pragma unroll
        for (int p = 0; p < DR; ++p)
            if (p < d) {
                const T sc = ns == 0 ? T(1) : (T)k.th[k.so[f] + (ns == 1 ? 0 : p)];
                const T v = sinpi_t(sc * t[p]) / (T)k.th[k.po[f] + p];
                acc = fma(v, v, acc);
            }
        return exp_nonpos<T>(T(-0.5) * acc);
    }
    const T d2 = ksum_d2<T, DR>(k, f, t, r2, d);
    if (kind == 5) {
        const T a = (T)k.th[k.po[f]];
        return exp_nonpos<T>(-a * log1p_t(d2 / (T(2) * a)));
    }
    return kappa<T>(kind, d2);
}

template <typename T, int DR>
__device__ __forceinline__ void ksum_r2(const T (&t)[DR], T& r2, bool& eq) {
    r2 = T(0);
    eq = true;
#pragma unroll
    for (int p = 0; p < DR; ++p) {
        r2 = fma(t[p], t[p], r2);
        eq = eq && t[p] == T(0);
    }
}

template <typename T, int DR>
__device__ __forceinline__ T ksum_eval(const KSum& k, const T (&t)[DR], int d) {
    T r2;
    bool eq;
    ksum_r2<T, DR>(t, r2, eq);
    T sum = T(0);
    for (int tt = 0; tt < k.nterms; ++tt) {
        T prod = (T)k.th[k.tv[tt]];
        for (int f = k.t0[tt]; f < k.t0[tt + 1]; ++f) prod *= ksum_factor<T, DR>(k, f, t, r2, eq, d);
        sum += prod;
    }
    return sum;
}

// ---- derivatives: κ with dκ/dr² of the four radial kinds, ∂C_ij/∂θ of a composite kernel (kgrad_* in kernels.hpp, batch_grad_kernel in batch.hip) and, last,
// its ∂k/∂t (ksum_gradx: kgradx_sum_kernel / kpgrad_sum_kernel in kernels.hpp, batch_pgrad_kernel in batch.hip)
//   dκ/dr²: SE −κ/2 · Matern12 −κ/(2r), 0 at r = 0 · Matern32 −(3/2)e^{−√3 r} · Matern52 −(5/6)(1+√5 r)e^{−√5 r}
template <typename T> __device__ __forceinline__ void kappa_and_dr2(int kind, T d2, T& kap, T& dk) {
    if (kind == 0) {
        kap = exp_nonpos<T>(T(-0.5) * d2);
        dk = T(-0.5) * kap;
        return;
    }
    const T d = sqrt(d2);
    if (kind == 1) {
        kap = exp_nonpos<T>(-d);
        dk = d > T(0) ? -kap / (T(2) * d) : T(0);
        return;
    }
    if (kind == 2) {
        const T a = T(1.7320508075688772935) * d, e = exp_nonpos<T>(-a);
        kap = (T(1) + a) * e;
        dk = T(-1.5) * e;
        return;
    }
    const T a = T(2.2360679774997896964) * d, e = exp_nonpos<T>(-a);
    kap = (T(1) + a + T(5.0 / 3.0) * d2) * e;
    dk = T(-5.0 / 6.0) * (T(1) + a) * e;
}

// c·∂κ_f/∂θ_q for every parameter q of factor f (scale entries, then r / α), handed to add(θ index, value); kap = κ_f.
//   kinds 0..3: ∂κ/∂d² as kappa_and_dr2;  RQ (q = d²/(2α)): ∂κ/∂d² = −κ/(2(1+q)), ∂κ/∂α = κ (q/(1+q) − log1p q);
//   Periodic: ∂κ/∂r_p = κ sinpi(u_p)²/r_p³, ∂κ/∂u_p = −κ (π/2) sinpi(2u_p)/r_p²;  ∂d²/∂s = 2 s r², ∂d²/∂v_p = 2 v_p t_p², ∂u_p/∂s = t_p.
template <typename T, int DR, class Add>
__device__ __forceinline__ void ksum_factor_grad(const KSum& k, int f, const T (&t)[DR], T r2, T kap, int d, double c, Add& add) {
    const int kind = k.kind[f], ns = k.ns[f];
    if (kind == 6) return;
    const double kp = (double)kap;
    if (kind == 4) {
        double dsum = 0.0;  // ScaleTransform: Σ_p ∂κ/∂u_p · t_p
#pragma unroll
        for (int p = 0; p < DR; ++p)
            if (p < d) {
                const T sc = ns == 0 ? T(1) : (T)k.th[k.so[f] + (ns == 1 ? 0 : p)];
                const T u = sc * t[p];
                const double r = k.th[k.po[f] + p], sp = (double)sinpi_t(u);
                add(k.po[f] + p, c * kp * sp * sp / (r * r * r));
                if (ns != 0) {
                    const double du = -kp * 1.5707963267948966192 * (double)sinpi_t(T(2) * u) / (r * r);
                    if (ns == 1) dsum += du * (double)t[p];
                    else add(k.so[f] + p, c * du * (double)t[p]);
                }
            }
        if (ns == 1) add(k.so[f], c * dsum);
        return;
    }
    const T d2 = ksum_d2<T, DR>(k, f, t, r2, d);
    double dk;
    if (kind == 5) {
        const double a = k.th[k.po[f]], q = (double)d2 / (2.0 * a);
        dk = -kp / (2.0 * (1.0 + q));
        add(k.po[f], c * kp * (q / (1.0 + q) - log1p(q)));
    } else {
        T kk, dkt;
        kappa_and_dr2<T>(kind, d2, kk, dkt);
        dk = (double)dkt;
    }
    if (ns == 1) {
        add(k.so[f], c * dk * 2.0 * k.th[k.so[f]] * (double)r2);
    } else if (ns > 1) {
#pragma unroll
        for (int p = 0; p < DR; ++p)
            if (p < d) add(k.so[f] + p, c * dk * 2.0 * k.th[k.so[f] + p] * (double)t[p] * (double)t[p]);
    }
}

// ∂C_ij/∂θ of one element, times the weight w, handed to add(θ index, value): σ_t² gets Π_f κ_f, a factor's parameters get σ_t² Π_{g≠f} κ_g ∂κ_f/∂θ —
// the product over the other factors as a running prefix times a suffix product (dividing by κ_f would fail where it underflows to 0).  The κ_f of
// the term wait in this thread's LDS slots kf[j][tid] (NTH = the threads of the workgroup, the stride of the slots: 256 in kernels.hpp, batch.hip's own): the factor loop stays a loop (unrolled over 4 factors, the element body of D = 16 grew
// beyond what the compiler inlines and went to a call frame in scratch).
template <typename T, int DR, class Add, int NTH>
__device__ __forceinline__ void ksum_grad(const KSum& k, const T (&t)[DR], int d, double w, Add& add, double (*kf)[NTH], int tid) {
    T r2;
    bool eq;
    ksum_r2<T, DR>(t, r2, eq);
    for (int tt = 0; tt < k.nterms; ++tt) {
        const int f0 = k.t0[tt], nf = k.t0[tt + 1] - f0;
        double prod = 1.0;
        for (int j = 0; j < nf; ++j) {
            const double v = (double)ksum_factor<T, DR>(k, f0 + j, t, r2, eq, d);
            kf[j][tid] = v;
            prod *= v;
        }
        add(k.tv[tt], w * prod);
        const double wv = w * k.th[k.tv[tt]];
        double pre = 1.0;
        for (int j = 0; j < nf; ++j) {
            double suf = 1.0;
            for (int i = j + 1; i < nf; ++i) suf *= kf[i][tid];
            const double kj = kf[j][tid];
            ksum_factor_grad<T, DR>(k, f0 + j, t, r2, (T)kj, d, wv * pre * suf, add);
            pre *= kj;
        }
    }
}

// acc[p] += w · ∂k/∂t_p at the differences t, k = Σ_t σ_t² Π_f κ_f:  ∂k/∂t_p = Σ_t σ_t² Σ_f (Π_{g≠f} κ_g) ∂κ_f/∂t_p, the product over the other factors as
// prefix × suffix with the κ_f in this thread's LDS slots (stride NTH, deduced from the array), as ksum_grad.  With c_p the factor's transform (1, s or v_p):
//   kinds 0..3 and RQ: ∂κ_f/∂t_p = ∂κ/∂d² · 2 c_p² t_p (∂κ/∂d² as ksum_factor_grad; Matern12 at d = 0 taken as 0);  White: 0;
//   Periodic (u_p = c_p t_p): ∂κ_f/∂t_p = −κ (π/2) sinpi(2u_p)/r_p² · c_p.
// Factors without a transform or with a ScaleTransform share the direction t: their coefficients add up in one scalar, applied once at the end.
template <typename T, int DR, int NTH>
__device__ __forceinline__ void ksum_gradx(const KSum& k, const T (&t)[DR], int d, double w, double (&acc)[DR], double (*kf)[NTH], int tid) {
    T r2;
    bool eq;
    ksum_r2<T, DR>(t, r2, eq);
    double iso = 0.0;
    for (int tt = 0; tt < k.nterms; ++tt) {
        const int f0 = k.t0[tt], nf = k.t0[tt + 1] - f0;
        for (int j = 0; j < nf; ++j) kf[j][tid] = (double)ksum_factor<T, DR>(k, f0 + j, t, r2, eq, d);
        const double wv = w * k.th[k.tv[tt]];
        double pre = 1.0;
        for (int j = 0; j < nf; ++j) {
            double suf = 1.0;
            for (int i = j + 1; i < nf; ++i) suf *= kf[i][tid];
            const double kj = kf[j][tid], c = wv * pre * suf;
            pre *= kj;
            const int f = f0 + j, kind = k.kind[f], ns = k.ns[f];
            if (kind == 6) continue;
            if (kind == 4) {
                const double ck = -c * kj * 1.5707963267948966192;
#pragma unroll
                for (int p = 0; p < DR; ++p)
                    if (p < d) {
                        const T sc = ns == 0 ? T(1) : (T)k.th[k.so[f] + (ns == 1 ? 0 : p)];
                        const double r = k.th[k.po[f] + p];
                        acc[p] += ck * (double)sinpi_t(T(2) * sc * t[p]) * (double)sc / (r * r);
                    }
                continue;
            }
            const T d2 = ksum_d2<T, DR>(k, f, t, r2, d);
            double dk;
            if (kind == 5) {
                dk = -kj / (2.0 * (1.0 + (double)d2 / (2.0 * k.th[k.po[f]])));
            } else {
                T kk, dkt;
                kappa_and_dr2<T>(kind, d2, kk, dkt);
                dk = (double)dkt;
            }
            const double c2 = 2.0 * c * dk;
            if (ns == 0) {
                iso += c2;
            } else if (ns == 1) {
                const double s = k.th[k.so[f]];
                iso += c2 * s * s;
            } else {
#pragma unroll
                for (int p = 0; p < DR; ++p)
                    if (p < d) {
                        const double v = k.th[k.so[f] + p];
                        acc[p] += c2 * v * v * (double)t[p];
                    }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < DR; ++p) acc[p] += iso * (double)t[p];
}

}  // namespace gpmi
