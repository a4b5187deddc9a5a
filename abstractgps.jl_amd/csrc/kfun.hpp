// kfun.hpp — the covariance functions as __device__ code, shared by every translation unit that evaluates a kernel on the device
// (kernels.hpp: kmat / kvec / kgrad and their composite forms; batch.hip: the batched small-problem kernel).
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

}  // namespace gpmi
