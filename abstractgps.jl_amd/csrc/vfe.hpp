// vfe.hpp — VFE / DTC sparse approximation on the device (included by gpmi355.hip).
//
// Reference: posterior(::Union{VFE,DTC}, fx, y)      src/sparse_approximations.jl:58-75
//            update_posterior (new observations)      :87-121      update_posterior (new pseudo-points)  :131-176
//            approx_log_evidence / elbo              :248-254 (VFE), :282-286 (DTC), :289-305
//            predictive mean / cov / var / joint      :183-217
//
// Formulation (S = Σy^-1/2 diagonal, L_z L_zᵀ = K_zz + jitter·I, so U = L_zᵀ), the reference's own:
//   B = U⁻ᵀ (S K_xz)ᵀ,  D = B Bᵀ + I = Λ_ε,  c = B b_y,  m_ε = Λ_ε \ c,  α = U \ m_ε.
//   The N-long pass is streamed in chunks of CH data points and never holds an N×M matrix.  L_z is the same for
//   every chunk, so its inverse is formed once (fp64: I·L_z⁻ᵀ by the blocked TRSM, transposed, rounded to T) and the
//   per-chunk triangular solve becomes ONE MFMA GEMM with a triangular k range (no 64-wide leaf chain per chunk):
//     Xc  = S_c K(x_c, z)                   kmat with a row scale          (CH × M, dtype T)
//     Y   = −inv(L_z) Xcᵀ = −B_c            gemm_nt_dma, beta0 + ktri      (M × CH, data points contiguous)
//     D_acc −= Y Yᵀ                         MFMA gemm (NT), fp64 accumulation (SYRK over the data points)
//     c_acc −= Y b_c,  rowss += rowsumsq(Y) ystats (one pass over Y)
//   (T = f32 or f64).  The M×M side (K_zz, both Choleskys, all vector solves) is always fp64, and so are the
//   accumulators of the N-long reductions (D_acc, c_acc, ‖B‖²_F): in fp32 mode the operands stream in fp32 through
//   the fp32 MFMA in K = 2 048 partial products that are summed into the fp64 accumulator; L_z is rounded to fp32 for
//   the streamed TRSM only.  ‖A‖²_F = tr(B Bᵀ) = Σ rowss (ELBO trace term, :251).
//
// The handle keeps what the reference keeps in its cache (:73, :118): the scaled observations x, Σy^-1/2 and b_y (small
// N-vectors; B_εf itself is never stored), so that both update_posterior forms continue from the resident state:
//   new observations   -> stream only the new points into D_acc / c_acc / rowss, re-finalise the M×M side
//   new pseudo-points  -> bordered Cholesky of K_zz (update_chol, src/util/common_covmat_ops.jl:38-42), then re-stream
//                         the retained observations computing ONLY the new block rows of B Bᵀ, B b_y and ‖B‖²
#pragma once

struct ObsSeg {  // one batch of observations, device resident: T xs[d][npad] (scaled), T rs[npad] = σ⁻¹, T b[brows][npad] = σ⁻¹δ per column of
                 // observations (brows = 1 for a one-column handle, else the columns rounded up to 16: the MFMA blocks of ystats_cols_kernel; rows beyond
                 // the columns and entries beyond n are zero)
    gp_ctx* ctx = nullptr;
    void *xs = nullptr, *rs = nullptr, *b = nullptr;
    long n = 0, npad = 0;
    int brows = 1;
    ~ObsSeg() {  // runs under the ctx lock (gp_vfe_free / error paths of a locked call)
        ctx_release(ctx, xs, 0);
        ctx_release(ctx, rs, 0);
        ctx_release(ctx, b, 0);
    }
};

struct gp_vfe {
    gp_ctx* ctx = nullptr;
    int dtype = 0;
    long m = 0, mp = 0, ld = 0;
    int d = 0;
    KernelRec kern;  // single-kind: VFE / DTC take no composite kernel
    double jitter = 0;
    void *Lz = nullptr, *Ld = nullptr;  // (mp + 256) × ld doubles: chol(K_zz + jitter I), Λ_ε factor
    void* zs = nullptr;                 // scaled inducing inputs, double [d][mp]
    void* vec = nullptr;                // double [4][vrows·mp]: rows c, m_ε, α, spare — each [vrows][mp], one mp-long vector per column of observations
    int approx = 0;
    int ncols = 1;                      // columns of observations (gp_vfe_fit_cols); 1 for every handle of the single-column calls
    int vrows = 1;                      // rows of b / cacc / the vec blocks: 1 for ncols = 1, else ncols rounded up to 16
    std::vector<double> ddc;            // ncols > 1: ‖b_s‖² per column (dd is column 0's)
    long n_obs = 0;
    long chunk = 16384;  // data points per streamed chunk of THIS handle (chosen by its first fit; its updates / appends / gradient keep it: the retained segments are padded to it)
    // streaming state before the M×M finalisation: −B Bᵀ (lower), B b_y, per-row ‖B‖², inv(L_z) and scaled z in T
    void *Dacc = nullptr, *cacc = nullptr, *rowss = nullptr, *Li = nullptr, *zsT = nullptr;
    std::vector<std::shared_ptr<ObsSeg>> segs;  // every observation seen so far (shared between a posterior and its updates)
    double logdet_sy = 0, dd = 0, tr_kff = 0, trZ = 0;
    DibCache dib_z, dib_d;  // inverse diagonal blocks of Lz / Ld for the predictive solves (built on the first prediction; a new handle after every update)
};

static void vfe_release(gp_vfe* p) {  // under the ctx lock
    gp_ctx* c = p->ctx;
    ctx_release(c, p->Lz, 0);
    ctx_release(c, p->Ld, 0);
    ctx_release(c, p->zs, 0);
    ctx_release(c, p->vec, 0);
    ctx_release(c, p->Dacc, 0);
    ctx_release(c, p->cacc, 0);
    ctx_release(c, p->rowss, 0);
    ctx_release(c, p->Li, 0);
    ctx_release(c, p->zsT, 0);
    if (p->dib_z.w) ctx_release(c, p->dib_z.w, p->dib_z.bytes);
    if (p->dib_d.w) ctx_release(c, p->dib_d.w, p->dib_d.bytes);
    p->dib_z = DibCache();
    p->dib_d = DibCache();
    p->segs.clear();
}

// Iw ((mp + 256) × ld doubles, L_b bytes, zeroed first) ← L⁻ᵀ (upper, row-major) of the lower factor L (gpmi355.hip upper_inverse, the mechanism of the exact
// gradient's L⁻ᵀ), with inverse diagonal blocks of "vfe_inv_nb" columns when that is >= 128.  Used by the fit's prelude (inv(L_z)) and by vfe_grad_impl.
static int32_t vfe_upper_inverse(gp_ctx* c, hipStream_t s, const double* L, long ld, long mp, double* Iw, size_t L_b, DevBufs& bufs) {
    HIPCHK(hipMemsetAsync(Iw, 0, L_b, s));
    const long inb = c->vfe_inv_nb;
    return upper_inverse<double>(c, s, bufs, L, ld, mp, (inb >= 128 && mp >= 2 * inb) ? inb : 0, Iw);
}

enum { VFE_FIT = 0, VFE_UPDATE = 1, VFE_APPEND = 2 };

// mode VFE_FIT:    x, y, noise, z, jitter given; prev == NULL
// mode VFE_UPDATE: x, y, noise = the NEW observations; z == NULL; kernel / jitter / z from prev
// mode VFE_APPEND: z = the NEW pseudo-points; x == NULL; everything else from prev
// ncols columns of observations (gp_vfe_fit_cols; an update / append keeps prev's): yv is n×ncols column-major with leading dimension yld, objective has
// ncols entries.  Everything but the observations is shared: ONE streamed pass, ystats_cols_kernel in place of ystats_kernel, the M×M vector solves as
// blocked solves over the columns' rows.  ncols = 1 issues exactly the single-column launches.
// The two N-long reductions of the streamed pass over rows [row_lo, row_lo + nrows) of Y = −B_c (kernels.hpp ystats_kernel / ystats_cols_kernel): the fit below and
// the device-level entry points gpd_ystats / gpd_ystats_cols (include/gpmi355.h) launch them through these.
//   one column : cacc[row] −= Σ_c Y[row][c] b[c],  rowss[row] += Σ_c Y[row][c]²                 one workgroup per row
//   S columns  : Cacc[s][row] −= Σ_c Y[row][c] By[s][c] for s < 16·SB,  rowss as above           32 rows per workgroup (RT = 2); 16 (RT = 1) where nrows is no
//                multiple of 32 — the fit's nrows always is one (mp and row_lo are multiples of 128) — or with the experiment switch GPMI_YSTATS_COLS_ROWS=16
//                (twice the workgroups, twice the re-reads of the b chunk — timed at C5)
template <typename T>
static int32_t launch_ystats(hipStream_t s, const T* Y, long ldy, long ncols, const T* b, long row_lo, long nrows, double* cacc, double* rowss) {
    hipLaunchKernelGGL(ystats_kernel<T>, dim3((unsigned)nrows), dim3(256), 0, s, Y, ldy, ncols, b, row_lo, cacc, rowss);
    HIPCHK(hipGetLastError());
    return 0;
}
template <typename T>
static int32_t launch_ystats_cols(hipStream_t s, const T* Y, long ldy, long ncols, const T* By, long ldb, int SB, long row_lo, long nrows, double* Cacc, long ldc,
                                  double* rowss) {
    static const bool rows16 = [] { const char* e = getenv("GPMI_YSTATS_COLS_ROWS"); return e && !strcmp(e, "16"); }();
    if (rows16 || nrows % 32)
        hipLaunchKernelGGL((ystats_cols_kernel<T, 1>), dim3((unsigned)(nrows / 16)), dim3(256), 0, s, Y, ldy, ncols, By, ldb, SB, row_lo, Cacc, ldc, rowss);
    else
        hipLaunchKernelGGL((ystats_cols_kernel<T, 2>), dim3((unsigned)(nrows / 32)), dim3(256), 0, s, Y, ldy, ncols, By, ldb, SB, row_lo, Cacc, ldc, rowss);
    HIPCHK(hipGetLastError());
    return 0;
}

template <typename T>
static int32_t vfe_fit_impl(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_points* z, const gp_noise* noise,
                            double jitter, const void* mean_or_null, const void* yv, int approx, gp_vfe* out,
                            double* objective, const gp_vfe* prev, int mode, long yld = 0, int ncols_in = 1) {
    const int S = prev ? prev->ncols : ncols_in;
    const bool cols = S > 1;
    const int VR = cols ? (int)round_up(S, 16) : 1;  // rows of b / c_acc / the vec blocks
    const long m_old = prev ? prev->m : 0;
    const long m2 = (mode == VFE_APPEND) ? z->n : 0;
    const long m = mode == VFE_FIT ? z->n : m_old + m2;
    const long mp = round_up(m, 128);
    const int d = prev ? prev->d : x->d;
    // data points per streamed chunk: the handle's own once it exists; else the ctx parameter "vfe_chunk" (> 0), or automatic (0, the default): 16 384 — measured
    // best at C5 (M = 4 096) — times a power of two that keeps chunk × M at C5's footprint for fewer pseudo-points (M = 64 … 256 and N = 2·10⁶: 123 chunks of
    // 16 384 cost 13.5 / 17.0 ms per fit pass, 16 of 131 072 6.4 / ≈ 12 — launches of a few hundred µs of work each), never more than the batch itself
    long CH = prev ? prev->chunk : c->vfe_chunk;
    if (CH <= 0) {
        long f = 1;
        while (f < 16 && 2 * f * mp <= 4096) f *= 2;
        CH = std::min(16384 * f, round_up(std::max(x ? x->n : 1L, 1L), 16384));
    }
    const long KS = std::min(c->vfe_ks, CH);    // fp32: data points per fp32 partial product
    const int NBAT = (int)(CH / KS);
    if (CH % KS) return set_arg_err(1, "vfe_chunk must be a multiple of vfe_ks");
    if (c->vfe_sk) ++c->sk_scope;
    struct SkOff {
        gp_ctx* c;
        ~SkOff() {
            if (c->vfe_sk) --c->sk_scope;
        }
    } sk_off{c};
    const long n = x ? x->n : 0, npad = round_up(std::max(n, 1L), CH);
    const long ld = mp + c->ldpad;              // M×M matrices and the CH×M chunk
    const T* y = (const T*)yv;
    const T* mean = (const T*)mean_or_null;
    constexpr bool is_f64 = sizeof(T) == 8;
    if (prev) jitter = prev->jitter;

    c->ev_used = 0;
    c->gemm_recs.clear();
    for (auto& e : c->ev_phase)
        if (!e) HIPCHK(hipEventCreate(&e));
    if (!c->info_dev) HIPCHK(hipMalloc((void**)&c->info_dev, sizeof(int)));
    RC(ctx_scal(c, 16 + 128));

    // ---- host marshalling
    std::vector<T> znew_h, host_pageable;
    T *xs_h = nullptr, *rs_h = nullptr, *b_h = nullptr;   // the N-long host vectors: page-locked staging of the ctx when it is to be had (three 16 MB uploads from
                                                          // pageable memory cost ≈ 10 ms at N = 2·10⁶; C5's are 1–3 MB and ride behind the prelude either way)
    double logdet_sy = prev ? prev->logdet_sy : 0, dd = prev ? prev->dd : 0, tr_kff = prev ? prev->tr_kff : 0;
    std::vector<double> ddc = (prev && cols) ? prev->ddc : std::vector<double>(cols ? (size_t)S : 0, 0.0);  // ‖b_s‖² per column
    // the N-long host marshalling (scaled inputs, Σy^-1/2, b_y, the scalar sums: ≈ 1 ms at N = 262 144) runs AFTER the M×M prelude has been queued — the
    // device factors K_zz and inverts L_z meanwhile
    auto marshal_x = [&]() -> int32_t {
        if (!x) return 0;
        const size_t cnt = (size_t)(d + 1 + S) * (size_t)npad;   // (the rows of b beyond the S columns are zeroed on the device, not staged)
        xs_h = (T*)ctx_pinned(c, sizeof(T) * cnt);
        if (!xs_h) {
            host_pageable.resize(cnt);
            xs_h = host_pageable.data();
        }
        rs_h = xs_h + (size_t)d * npad;   // s_i = σ_i⁻¹
        b_h = rs_h + npad;                // b_i = s_i δ_i  (b_y, :66)
        scale_points_into<T>(k, x, npad, xs_h);
        std::fill(rs_h + n, rs_h + npad, T(0));
        std::fill(b_h + n, b_h + npad, T(0));
        if (cols) {  // b_y of every column (rows of b_h; the entries beyond n stay zero), Σy shared
            const bool iso = noise->kind == 0;
            if (iso && !(noise->s > 0)) return n > 0 ? 1 : 0;
            const double si_iso = iso ? 1.0 / std::sqrt(noise->s) : 0.0;
            std::vector<double> si_d(iso ? 0 : (size_t)n);   // σ_i⁻¹ in double, formed once for all columns
            for (long i = 0; i < n; ++i) {
                const double s2 = iso ? noise->s : (double)((const T*)noise->diag)[i];
                if (!(s2 > 0)) return 1 + (int32_t)i;
                const double si = 1.0 / std::sqrt(s2);
                rs_h[i] = (T)si;
                if (!iso) {
                    si_d[i] = si;
                    logdet_sy += std::log(s2);
                    tr_kff += k->variance / s2;
                }
            }
            if (iso) {
                logdet_sy += (double)n * std::log(noise->s);
                tr_kff += (double)n * (k->variance / noise->s);
            }
            // the N × S values: the columns dealt to up to 8 host threads (a column's b_y and ‖b_s‖² are formed by one thread, in the order of the
            // single-column loop: the same bits whatever the thread count)
            auto do_cols = [&](int c0, int c1) {
                for (int col = c0; col < c1; ++col) {
                    const T* yc = y + (size_t)col * (size_t)yld;
                    T* bc = b_h + (size_t)col * npad;
                    double acc = 0;
                    for (long i = 0; i < n; ++i) {
                        const double si = iso ? si_iso : si_d[i];
                        const T bi = (T)((double)(T)(yc[i] - (mean ? mean[i] : T(0))) * si);
                        bc[i] = bi;
                        acc += (double)bi * (double)bi;
                    }
                    std::fill(bc + n, bc + npad, T(0));
                    ddc[col] += acc;
                }
            };
            const int nth = (long)S * n >= (1L << 20) ? std::min(S, 8) : 1;
            if (nth == 1) {
                do_cols(0, S);
            } else {
                std::vector<std::thread> th;
                for (int t = 0; t < nth; ++t) th.emplace_back(do_cols, (int)((long)S * t / nth), (int)((long)S * (t + 1) / nth));
                for (auto& t : th) t.join();
            }
            dd = ddc[0];
            return 0;
        }
        if (noise->kind == 0) {  // Σy = σ² I: one square root, one logarithm (the general loop below spends ≈ 15 ns per observation on them: 30 ms at N = 2·10⁶)
            const double s2 = noise->s;
            if (!(s2 > 0)) return n > 0 ? 1 : 0;  // chol(Σy) fails at the first observation (reference :61 / :296)
            const double si = 1.0 / std::sqrt(s2);
            std::fill(rs_h, rs_h + n, (T)si);
            double acc = 0;
            if (mean) {
                for (long i = 0; i < n; ++i) {
                    const T bi = (T)((double)(T)(y[i] - mean[i]) * si);
                    b_h[i] = bi;
                    acc += (double)bi * (double)bi;
                }
            } else {
                for (long i = 0; i < n; ++i) {
                    const T bi = (T)((double)y[i] * si);
                    b_h[i] = bi;
                    acc += (double)bi * (double)bi;
                }
            }
            dd += acc;
            logdet_sy += (double)n * std::log(s2);
            tr_kff += (double)n * (k->variance / s2);  // tr_Cf_invΣy :307-313
            return 0;
        }
        for (long i = 0; i < n; ++i) {
            const double s2 = (double)((const T*)noise->diag)[i];
            if (!(s2 > 0)) return 1 + (int32_t)i;  // chol(Σy) fails at i (reference :61 / :296)
            const double delta = (double)(T)(y[i] - (mean ? mean[i] : T(0)));
            const double si = 1.0 / std::sqrt(s2);
            rs_h[i] = (T)si;
            b_h[i] = (T)(delta * si);
            logdet_sy += std::log(s2);
            dd += (double)b_h[i] * (double)b_h[i];
            tr_kff += k->variance / s2;  // tr_Cf_invΣy :307-313
        }
        return 0;
    };
    const long m2p = round_up(std::max(m2, 1L), 128);
    const long znp = mode == VFE_FIT ? mp : m2p;  // leading dimension of the freshly scaled inducing inputs
    if (z) scale_points<T>(k, z, znp, znew_h);
    std::vector<double> znewD_h(znew_h.begin(), znew_h.end());
    std::vector<double> jit_h((size_t)mp, 0.0);
    for (long i = 0; i < m; ++i) jit_h[i] = jitter;

    const size_t zsT_b = sizeof(T) * (size_t)d * mp, zsD_b = sizeof(double) * (size_t)d * mp;
    const size_t D_b = sizeof(double) * (size_t)(mp + 128) * ld;
    const long ldy = CH + c->ldpad;             // Y = −B_c (M × CH)
    const size_t X_b = sizeof(T) * (size_t)(CH + 128) * ld, L_b = sizeof(double) * (size_t)(mp + 128 + 128) * ld;
    const size_t Y_b = sizeof(T) * (size_t)(mp + 128) * ldy, Li_b = sizeof(T) * (size_t)(mp + 128) * ld;
    const long vst = (long)VR * mp;  // one block of vec / c_acc: a vector of mp entries per column
    const size_t vT_b = sizeof(double) * (size_t)mp, cT_b = sizeof(double) * (size_t)vst, vD_b = sizeof(double) * (size_t)vst * 4, jit_b = sizeof(double) * (size_t)mp;
    const size_t R_b = sizeof(double) * (size_t)256 * ld;  // cols: the columns' vectors as 128 right-hand-side rows (+ 128 slack rows) of the blocked solves
    void *zsT_v = 0, *zsD_v = 0, *D_v = 0, *X_v = 0, *Lz_v = 0, *Ld_v = 0, *cT_v = 0, *rss_v = 0, *vec_v = 0, *jit_v = 0, *Y_v = 0,
         *Li_v = 0, *I_v = 0, *S_v = 0, *zn_v = 0, *znD_v = 0, *X2_v = 0, *Y2_v = 0, *S2_v = 0;
    DevBufs bufs(c);
    std::shared_ptr<ObsSeg> seg;
    if (x) {
        seg = std::make_shared<ObsSeg>();
        seg->ctx = c;
        seg->n = n;
        seg->npad = npad;
        RC(ctx_alloc(c, sizeof(T) * (size_t)d * (size_t)npad, &seg->xs));
        RC(ctx_alloc(c, sizeof(T) * (size_t)npad, &seg->rs));
        RC(ctx_alloc(c, sizeof(T) * (size_t)VR * (size_t)npad, &seg->b));
        seg->brows = VR;
    }
    void *R_v = nullptr, *R2_v = nullptr, *q_v = nullptr;
    std::vector<double> quad_h(128, 0.0);  // cols: ‖L_D⁻¹ c_s‖² per column
    struct Dibs {  // cols: the inverse diagonal blocks the blocked solves build — the handle's once it is made, released otherwise
        gp_ctx* c;
        DibCache z, d;
        ~Dibs() {
            if (z.w) ctx_release(c, z.w, z.bytes);
            if (d.w) ctx_release(c, d.w, d.bytes);
        }
    } dibs{c, DibCache(), DibCache()};
    if (cols) {
        RC(bufs.get(R_b, &R_v));
        RC(bufs.get(R_b, &R2_v));
        RC(bufs.get(sizeof(double) * 128, &q_v));
    }
    RC(bufs.get(zsT_b, &zsT_v));
    RC(bufs.get(zsD_b, &zsD_v));
    RC(bufs.get(D_b, &D_v));
    RC(bufs.get(X_b, &X_v));
    RC(bufs.get(L_b, &Lz_v));
    RC(bufs.get(L_b, &Ld_v));
    RC(bufs.get(Y_b, &Y_v));
    RC(bufs.get(Li_b, &Li_v));
    if (mode != VFE_UPDATE) RC(bufs.get(L_b, &I_v));
    if (!is_f64) RC(bufs.get((size_t)NBAT * Li_b, &S_v));
    if (c->vfe_overlap) {  // second set of chunk buffers for the overlapped helpers
        RC(bufs.get(X_b, &X2_v));
        RC(bufs.get(Y_b, &Y2_v));
        if (!is_f64) RC(bufs.get((size_t)NBAT * Li_b, &S2_v));
    }
    RC(bufs.get(cT_b, &cT_v));
    RC(bufs.get(vT_b, &rss_v));
    RC(bufs.get(vD_b, &vec_v));
    RC(bufs.get(jit_b, &jit_v));
    if (z && mode == VFE_APPEND) {
        RC(bufs.get(sizeof(T) * znew_h.size(), &zn_v));
        RC(bufs.get(sizeof(double) * znewD_h.size(), &znD_v));
    }
    double* Lz = (double*)Lz_v;
    double* Ld = (double*)Ld_v;
    double* vec = (double*)vec_v;  // rows: [0] c , [1] w→m_ε , [2] α , [3] spare
    double scal_h[16] = {0};
    std::vector<double> rss_h((size_t)mp, 0.0);
    int info_h = 0;
    hipStream_t s = c->sm;
    if (prev && mode == VFE_UPDATE && (prev->mp != mp || prev->ld != ld)) return set_arg_err(1, "stale gp_vfe state");
    for (auto& sg : (prev ? prev->segs : std::vector<std::shared_ptr<ObsSeg>>()))
        if (sg->npad % CH) return set_arg_err(1, "gp_vfe was built with a different vfe_chunk");
    const long n_all = (prev ? prev->n_obs : 0) + n;
    // rows of D_acc / c_acc / rowss that the streamed pass (re)computes: everything for a fit / new observations (the
    // accumulators continue), the block rows from the first new pseudo-point's 128-tile on for an append
    const long row_lo = (mode == VFE_APPEND) ? (m_old / 128) * 128 : 0;

    // One chunk loop over a batch of observations: rows >= row_lo of D_acc, c_acc, rowss.  The two MFMA GEMMs of a chunk run
    // back to back on the main stream; the bandwidth-bound helpers run on the ctx's second stream beside them, on double
    // buffers: kmat of chunk c+1 and the partial-sum adds of chunk c overlap the GEMMs of their neighbours ("vfe_overlap").
    hipStream_t sa = c->vfe_overlap ? c->sp : s;
    const bool ovl = sa != s;
    // "vfe_dual" (experiment switch, default 0): the triangular products Y(c) = −inv(L_z) X(c)ᵀ on a third, HIGH-priority stream sy, the chunk SYRKs on the main
    // stream — Y(c+1) is independent of SYRK(c), and the idea was that each launch's last partial round of workgroups (SYRK: 528 lower tiles × 8 partials = 4 224
    // workgroups = 8.25 rounds of the 512 slots) is filled by the other launch.  Measured at C5 in one process (tools/c5_ab.py, profiles/r6/c5_ab*.jsonl): with
    // the priority +0.4…0.7 ms, with both launches at equal priority −0.45 ms of 79.5 — the single-stream pass has no idle tail worth filling (the helper
    // kernels of the second stream already run in it).  Same buffers, same arithmetic, same order of the sums into D_acc either way.
    hipStream_t sy = s;
    if (ovl && c->vfe_dual) RC(ctx_third_stream(c, &sy));
    const bool dual = sy != s;
    hipEvent_t evSy[2] = {nullptr, nullptr};  // SYRK(c) has finished reading Y[bb]
    void* Xb[2] = {X_v, X2_v};
    void* Yb[2] = {Y_v, Y2_v};
    void* Sb[2] = {S_v, S2_v};
    hipEvent_t evK[2] = {nullptr, nullptr}, evYs[2] = {nullptr, nullptr}, evAdd[2] = {nullptr, nullptr};
    hipEvent_t ev_z = nullptr;      // the scaled pseudo-inputs are on the device (fit mode)
    bool first_kmat_done = false;   // chunk 0's kmat was issued beside the prelude
    long cidx = 0;
    auto kmat_chunk = [&](const ObsSeg& sg, long c0, int bb) -> int32_t {
        GridMap g = plain_map(0, c0, 0);
        dim3 grid((unsigned)(mp / 128), (unsigned)(CH / 128));
        launch_kmat<T>(grid, sa, (T*)Xb[bb], ld, (const T*)sg.xs, sg.npad, (const T*)zsT_v, mp, d,
                           k->kind, (T)k->variance, (const T*)nullptr, sg.n, m, 0, g, (const T*)nullptr, (const T*)sg.rs);
        HIPCHK(hipGetLastError());
        if (ovl) {
            RC(ctx_event(c, &evK[bb], false));
            HIPCHK(hipEventRecord(evK[bb], sa));
        }
        return 0;
    };
    auto stream_seg = [&](const ObsSeg& sg, const ObsSeg* next_sg) -> int32_t {
        for (long c0 = 0; c0 < sg.npad; c0 += CH) {
            if (c0 >= sg.n) break;  // nothing but padding in the remaining chunks
            const int bb = ovl ? (int)(cidx & 1) : 0;
            if (!ovl || (cidx == 0 && !first_kmat_done)) RC(kmat_chunk(sg, c0, bb));  // (overlapped mode: later chunks were prefetched below, the first beside the prelude)
            if (ovl) {
                HIPCHK(hipStreamWaitEvent(sy, evK[bb], 0));
                if (evYs[bb]) HIPCHK(hipStreamWaitEvent(sy, evYs[bb], 0));  // chunk cidx−2 is done with Y[bb]
                if (dual && evSy[bb]) HIPCHK(hipStreamWaitEvent(sy, evSy[bb], 0));  // ... its SYRK too
            }
            {
                GridMap gy = plain_map(0, 0, 0);
                gy.beta0 = 1;
                gy.ktri = 1;
                RC(launch_gemm<T>(c, sy, (T*)Yb[bb], ldy, (const T*)Li_v, ld, (const T*)Xb[bb], ld, mp, CH, mp, gy));   // Y = −B_c
            }
            if (ovl) {
                hipEvent_t e;
                RC(ctx_event(c, &e, false));
                HIPCHK(hipEventRecord(e, sy));
                HIPCHK(hipStreamWaitEvent(sa, e, 0));
                if (dual) HIPCHK(hipStreamWaitEvent(s, e, 0));
            }
            if (cols)  // every column's c_s += B_c b_cs and the ‖B‖² rows in one pass over Y (launch_ystats_cols above)
                RC(launch_ystats_cols<T>(sa, (const T*)Yb[bb], ldy, CH, (const T*)sg.b + c0, sg.npad, VR / 16, row_lo, mp - row_lo, (double*)cT_v, mp, (double*)rss_v));
            else
                RC(launch_ystats<T>(sa, (const T*)Yb[bb], ldy, CH, (const T*)sg.b + c0, row_lo, mp - row_lo, (double*)cT_v, (double*)rss_v));   // c += B_c b_c ; ‖B‖² rows (fp64)
            if (ovl) {
                RC(ctx_event(c, &evYs[bb], false));
                HIPCHK(hipEventRecord(evYs[bb], sa));
                // prefetch the next chunk's S·K(x_c, z) into the other X buffer (its last reader, the previous Y GEMM, is done)
                const long c1 = c0 + CH;
                if (c1 < sg.npad && c1 < sg.n) RC(kmat_chunk(sg, c1, bb ^ 1));
                else if (next_sg) RC(kmat_chunk(*next_sg, 0, bb ^ 1));
            }
            const T* Yr = (const T*)Yb[bb] + row_lo * ldy;
            if constexpr (is_f64) {
                RC((launch_gemm<T, double>(c, s, (double*)D_v + row_lo * ld, ld, Yr, ldy, (const T*)Yb[bb], ldy, mp - row_lo, mp, CH,
                                           plain_map(1, row_lo, 0))));
                if (dual) {
                    RC(ctx_event(c, &evSy[bb], false));
                    HIPCHK(hipEventRecord(evSy[bb], s));
                }
            } else {
                // fp32: the chunk's SYRK runs on the LDS-DMA kernel into fp32 scratch — NBAT partial products over KS data points
                // each in ONE launch (blockIdx.z) — which one pass then adds into the fp64 accumulator: fp64 sums across
                // partials and chunks, fp32 MFMA within a partial
                GridMap gs = plain_map(1, row_lo, 0);
                gs.beta0 = 1;
                gs.nbatch = NBAT;
                gs.cstride = (long)(mp + 128) * ld;
                if (ovl && evAdd[bb]) HIPCHK(hipStreamWaitEvent(s, evAdd[bb], 0));  // chunk cidx−2's partials have been added
                RC(launch_gemm<T>(c, s, (T*)Sb[bb] + row_lo * ld, ld, Yr, ldy, (const T*)Yb[bb], ldy, mp - row_lo, mp, KS, gs));
                if (ovl) {
                    hipEvent_t e;
                    RC(ctx_event(c, &e, false));
                    HIPCHK(hipEventRecord(e, s));
                    HIPCHK(hipStreamWaitEvent(sa, e, 0));
                    if (dual) evSy[bb] = e;
                }
                hipLaunchKernelGGL(add_lower_batched_kernel<T>, dim3((unsigned)((mp + 1023) / 1024), (unsigned)(mp - row_lo)), dim3(256),
                                   0, sa, (const T*)Sb[bb], gs.cstride, NBAT, ld, (double*)D_v, ld, mp, row_lo);
                HIPCHK(hipGetLastError());
                if (ovl) {
                    RC(ctx_event(c, &evAdd[bb], false));
                    HIPCHK(hipEventRecord(evAdd[bb], sa));
                }
            }
            ++cidx;
        }
        return 0;
    };
    auto stream_join = [&]() -> int32_t {  // everything the helpers accumulated is visible to the main stream
        if (!ovl) return 0;
        hipEvent_t e;
        RC(ctx_event(c, &e, false));
        HIPCHK(hipEventRecord(e, sa));
        HIPCHK(hipStreamWaitEvent(s, e, 0));
        if (dual) {
            RC(ctx_event(c, &e, false));
            HIPCHK(hipEventRecord(e, sy));
            HIPCHK(hipStreamWaitEvent(s, e, 0));
        }
        return 0;
    };

    const int32_t rc = run_drained(c, [&]() -> int32_t {
        HIPCHK(hipEventRecord(c->ev_phase[0], s));
        HIPCHK(hipMemcpyAsync(jit_v, jit_h.data(), jit_b, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(c->info_dev, 0, sizeof(int), s));
        HIPCHK(hipMemsetAsync(c->scal_dev, 0, sizeof(double) * 16, s));
        HIPCHK(hipMemsetAsync(D_v, 0, D_b, s));
        HIPCHK(hipMemsetAsync(cT_v, 0, cT_b, s));
        if (cols) HIPCHK(hipMemsetAsync(R_v, 0, R_b, s));
        HIPCHK(hipMemsetAsync(rss_v, 0, vT_b, s));
        HIPCHK(hipMemsetAsync(vec_v, 0, vD_b, s));
        if (mode == VFE_UPDATE) {  // resume: factor of K_zz, its inverse, the scaled inducing inputs and the running sums come from prev
            HIPCHK(hipMemcpyAsync(Lz_v, prev->Lz, L_b, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(Li_v, prev->Li, Li_b, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(zsT_v, prev->zsT, zsT_b, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(zsD_v, prev->zs, zsD_b, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(D_v, prev->Dacc, D_b, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(cT_v, prev->cacc, cT_b, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(rss_v, prev->rowss, vT_b, hipMemcpyDeviceToDevice, s));
        } else {
            if (mode == VFE_FIT) {
                HIPCHK(hipMemcpyAsync(zsT_v, znew_h.data(), zsT_b, hipMemcpyHostToDevice, s));
                HIPCHK(hipMemcpyAsync(zsD_v, znewD_h.data(), zsD_b, hipMemcpyHostToDevice, s));
                if (ovl) {  // the first chunk's K(x_c, z) needs the pseudo-inputs only: the helper stream may start it while the prelude runs
                    RC(ctx_event(c, &ev_z, false));
                    HIPCHK(hipEventRecord(ev_z, s));
                }
                // ---- L_z = chol(K_zz + jitter I), fp64                                                :62
                GridMap g = plain_map(1, 0, 0);
                dim3 grid((unsigned)(mp / 128), (unsigned)(mp / 128));
                launch_kmat<double>(grid, s, Lz, ld, (const double*)zsD_v, mp,
                                   (const double*)zsD_v, mp, d, k->kind, k->variance, (const double*)jit_v, m, m, 1, g,
                                   (const double*)nullptr, (const double*)nullptr);
                HIPCHK(hipGetLastError());
                RC(potrf_full<double>(c, Lz, ld, mp, mp, c->info_dev, m, c->scal_dev + 0));
            } else {  // VFE_APPEND: z = vcat(z_old, z_new); U = update_chol(U11, C12, C22)               :131-141
                const long mpo = prev->mp, ldo = prev->ld;
                HIPCHK(hipMemcpyAsync(zn_v, znew_h.data(), sizeof(T) * znew_h.size(), hipMemcpyHostToDevice, s));
                HIPCHK(hipMemcpyAsync(znD_v, znewD_h.data(), sizeof(double) * znewD_h.size(), hipMemcpyHostToDevice, s));
                HIPCHK(hipMemsetAsync(zsT_v, 0, zsT_b, s));
                HIPCHK(hipMemsetAsync(zsD_v, 0, zsD_b, s));
                HIPCHK(hipMemcpy2DAsync(zsT_v, sizeof(T) * mp, prev->zsT, sizeof(T) * mpo, sizeof(T) * m_old, d, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpy2DAsync((T*)zsT_v + m_old, sizeof(T) * mp, zn_v, sizeof(T) * m2p, sizeof(T) * m2, d, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpy2DAsync(zsD_v, sizeof(double) * mp, prev->zs, sizeof(double) * mpo, sizeof(double) * m_old, d, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpy2DAsync((double*)zsD_v + m_old, sizeof(double) * mp, znD_v, sizeof(double) * m2p, sizeof(double) * m2, d, hipMemcpyDeviceToDevice, s));
                // X = K(z_new, z_old) L11⁻ᵀ = U12ᵀ (in Ld's storage, free until the finalisation), S = C22 − U12ᵀU12 (in I's)
                double* Xb = Ld;
                double* Sb = (double*)I_v;
                const long ldx = ldo, lds = m2p + c->ldpad;
                {
                    GridMap g = plain_map(0, 0, 0);
                    dim3 grid((unsigned)(mpo / 128), (unsigned)(m2p / 128));
                    launch_kmat<double>(grid, s, Xb, ldx, (const double*)znD_v, m2p,
                                       (const double*)prev->zs, mpo, d, k->kind, k->variance, (const double*)nullptr, m2, m_old, 0, g,
                                       (const double*)nullptr, (const double*)nullptr);
                    HIPCHK(hipGetLastError());
                }
                RC(trsm_rec<double>(c, s, Xb, ldx, m2p, (const double*)prev->Lz, ldo, mpo));
                {
                    GridMap g = plain_map(1, 0, 0);
                    dim3 grid((unsigned)(m2p / 128), (unsigned)(m2p / 128));
                    // C22 = _symmetric(cov(prior, z_new)) carries NO jitter in the reference (src/sparse_approximations.jl:138)
                    launch_kmat<double>(grid, s, Sb, lds, (const double*)znD_v, m2p,
                                       (const double*)znD_v, m2p, d, k->kind, k->variance, (const double*)nullptr, m2, m2, 1, g,
                                       (const double*)nullptr, (const double*)nullptr);
                    HIPCHK(hipGetLastError());
                }
                RC(launch_gemm<double>(c, s, Sb, lds, Xb, ldx, Xb, ldx, m2p, m2p, mpo, plain_map(1, 0, 0)));
                RC(potrf_full<double>(c, Sb, lds, m2p, m2p, c->info_dev, m2, c->scal_dev + 0));
                HIPCHK(hipMemsetAsync(Lz_v, 0, L_b, s));
                HIPCHK(hipMemcpy2DAsync(Lz, sizeof(double) * ld, prev->Lz, sizeof(double) * ldo, sizeof(double) * m_old, m_old, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpy2DAsync(Lz + m_old * ld, sizeof(double) * ld, Xb, sizeof(double) * ldx, sizeof(double) * m_old, m2, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpy2DAsync(Lz + m_old * ld + m_old, sizeof(double) * ld, Sb, sizeof(double) * lds, sizeof(double) * m2, m2, hipMemcpyDeviceToDevice, s));
                if (mp > m) {
                    hipLaunchKernelGGL(pad_identity_kernel<double>, dim3((unsigned)((mp + 255) / 256), (unsigned)(mp - m)), dim3(256), 0, s,
                                       Lz, ld, m, mp);
                    HIPCHK(hipGetLastError());
                }
                // the finished block rows of the accumulators carry over (rows < row_lo; D_acc is lower, so columns < row_lo too)
                if (row_lo > 0) {
                    HIPCHK(hipMemcpy2DAsync(D_v, sizeof(double) * ld, prev->Dacc, sizeof(double) * ldo, sizeof(double) * row_lo, row_lo, hipMemcpyDeviceToDevice, s));
                    if (cols) HIPCHK(hipMemcpy2DAsync(cT_v, sizeof(double) * mp, prev->cacc, sizeof(double) * mpo, sizeof(double) * row_lo, VR, hipMemcpyDeviceToDevice, s));
                    else HIPCHK(hipMemcpyAsync(cT_v, prev->cacc, sizeof(double) * row_lo, hipMemcpyDeviceToDevice, s));
                    HIPCHK(hipMemcpyAsync(rss_v, prev->rowss, sizeof(double) * row_lo, hipMemcpyDeviceToDevice, s));
                }
            }
            // ---- inv(L_z): W = I · L_z⁻ᵀ (upper), transposed into Ld's storage (free until the SYRK is done), rounded to T
            double* Iw = (double*)I_v;
            RC(vfe_upper_inverse(c, s, Lz, ld, mp, Iw, L_b, bufs));
            hipLaunchKernelGGL(transpose_f64_kernel, dim3((unsigned)(mp / 32), (unsigned)(mp / 32)), dim3(256), 0, s, Iw, ld, Ld, ld, mp);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemsetAsync(Li_v, 0, Li_b, s));
            hipLaunchKernelGGL((convert_kernel<double, T>), convert_grid((long)mp * ld), dim3(256), 0, s, Ld,
                               (T*)Li_v, (long)mp * ld, 1.0);
            HIPCHK(hipGetLastError());
        }
        // ---- the observations: marshalled on the host while the device works through the prelude queued above, uploaded on the helper stream (the first
        //      consumers — kmat, ystats — run there; the main stream joins through their events)
        RC(marshal_x());
        if (x) {
            HIPCHK(hipMemcpyAsync(seg->xs, xs_h, sizeof(T) * (size_t)d * (size_t)npad, hipMemcpyHostToDevice, sa));
            HIPCHK(hipMemcpyAsync(seg->rs, rs_h, sizeof(T) * (size_t)npad, hipMemcpyHostToDevice, sa));
            if (VR > S) HIPCHK(hipMemsetAsync((T*)seg->b + (size_t)S * npad, 0, sizeof(T) * (size_t)(VR - S) * (size_t)npad, sa));  // the MFMA block's rows beyond the columns
            HIPCHK(hipMemcpyAsync(seg->b, b_h, sizeof(T) * (size_t)S * (size_t)npad, hipMemcpyHostToDevice, sa));
        }
        if (ev_z && x && mode == VFE_FIT && n > 0) {  // chunk 0's kmat beside the prelude (0.34 ms at C5); everything else of the helper stream waits for the prelude below
            HIPCHK(hipStreamWaitEvent(sa, ev_z, 0));
            RC(kmat_chunk(*seg, 0, 0));
            first_kmat_done = true;
        }
        HIPCHK(hipEventRecord(c->ev_phase[1], s));
        // ---- streamed pass over the data points                                                   :64-71
        if (ovl) {  // the helper stream starts after the M×M prelude and the uploads
            hipEvent_t e;
            RC(ctx_event(c, &e, false));
            HIPCHK(hipEventRecord(e, s));
            HIPCHK(hipStreamWaitEvent(sa, e, 0));
            if (dual) HIPCHK(hipStreamWaitEvent(sy, e, 0));
        }
        if (mode == VFE_APPEND) {
            for (size_t si = 0; si < prev->segs.size(); ++si)
                RC(stream_seg(*prev->segs[si], si + 1 < prev->segs.size() ? prev->segs[si + 1].get() : nullptr));
        } else {
            RC(stream_seg(*seg, nullptr));
        }
        RC(stream_join());
        HIPCHK(hipEventRecord(c->ev_phase[2], s));
        if (!cols) {
            hipLaunchKernelGGL((convert_kernel<double, double>), convert_grid(mp), dim3(256), 0, s,
                               (const double*)cT_v, vec, mp, 1.0);                                                          // c = B b_y
            HIPCHK(hipGetLastError());
        }
        // ---- D = I + B Bᵀ (fp64, symmetric), Λ_ε = chol(D)                                       :68-69
        hipLaunchKernelGGL(neg_sym_to_f64_kernel<double>, dim3((unsigned)((mp + 255) / 256), (unsigned)mp), dim3(256), 0, s,
                           (const double*)D_v, ld, Ld, ld, mp);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(diag_shift_trace_kernel, dim3(1), dim3(256), 0, s, Ld, ld, mp, m, 1.0, c->scal_dev + 2);
        HIPCHK(hipGetLastError());
        RC(potrf_full<double>(c, Ld, ld, mp, mp, c->info_dev + 0, mp, c->scal_dev + 1));
        // ---- vectors
        if (cols) {
            // every column at once: the c_s are the rows of R (128 right-hand-side rows, zero beyond S) of the blocked solves the predictions use —
            // forward against Λ_ε's factor (quad_s = ‖w_s‖²), backward against it (m_ε), backward against L_z (α); the inverse diagonal blocks they build
            // stay with the handle
            double* R = (double*)R_v;
            const size_t rowb = sizeof(double) * (size_t)mp;
            HIPCHK(hipMemcpy2DAsync(vec, rowb, cT_v, rowb, rowb, VR, hipMemcpyDeviceToDevice, s));                                 // c_s = B b_ys
            HIPCHK(hipMemcpy2DAsync(R, sizeof(double) * ld, cT_v, rowb, rowb, VR, hipMemcpyDeviceToDevice, s));
            RC(trsm_cached<double>(c, s, R, ld, 128, Ld, ld, mp, mp, dibs.d, bufs));                                               // w_s = L_D⁻¹ c_s
            hipLaunchKernelGGL(rowsumsq_kernel<double>, dim3(128), dim3(256), 0, s, (const double*)R, ld, mp, (double*)q_v);
            HIPCHK(hipGetLastError());
            BackWs wb;
            RC(trsm_back_cached<double>(c, s, R, ld, 128, S, Ld, ld, mp, dibs.d, bufs, wb));                                       // m_εs = L_D⁻ᵀ w_s
            HIPCHK(hipMemcpy2DAsync(vec + vst, rowb, R, sizeof(double) * ld, rowb, VR, hipMemcpyDeviceToDevice, s));
            // the backward solve uses the inverse diagonal blocks a forward solve leaves: one over zero rows builds L_z's (the first prediction would anyway)
            HIPCHK(hipMemsetAsync(R2_v, 0, R_b, s));
            RC(trsm_cached<double>(c, s, (double*)R2_v, ld, 128, Lz, ld, mp, m, dibs.z, bufs));
            RC(trsm_back_cached<double>(c, s, R, ld, 128, S, Lz, ld, mp, dibs.z, bufs, wb));                                     // α_s = L_z⁻ᵀ m_εs
            HIPCHK(hipMemcpy2DAsync(vec + 2 * vst, rowb, R, sizeof(double) * ld, rowb, VR, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(quad_h.data(), q_v, sizeof(double) * 128, hipMemcpyDeviceToHost, s));
        } else {
        HIPCHK(hipMemcpyAsync(vec + mp, vec, sizeof(double) * mp, hipMemcpyDeviceToDevice, s));
        RC(trsv<double>(c, s, Ld, ld, mp, vec + mp, mp, 1, true));                // w = L_D⁻¹ c
        hipLaunchKernelGGL(rowsumsq_kernel<double>, dim3(1), dim3(256), 0, s, vec + mp, mp, mp, c->scal_dev + 3);
        HIPCHK(hipGetLastError());
        RC(trsv<double>(c, s, Ld, ld, mp, vec + mp, mp, 1, false));               // m_ε = L_D⁻ᵀ w      :71
        HIPCHK(hipMemcpyAsync(vec + 2 * mp, vec + mp, sizeof(double) * mp, hipMemcpyDeviceToDevice, s));
        RC(trsv<double>(c, s, Lz, ld, mp, vec + 2 * mp, mp, 1, false));           // α = L_z⁻ᵀ m_ε      :73
        }
        HIPCHK(hipEventRecord(c->ev_phase[3], s));
        HIPCHK(hipMemcpyAsync(&info_h, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(scal_h, c->scal_dev, sizeof(double) * 16, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(rss_h.data(), rss_v, vT_b, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        // gp_timings: assemble_ms = the M×M prelude (K_zz, its Cholesky, inv(L_z)), potrf_ms = the streamed pass over the data points, solve_ms = the M×M side
        // after it (Λ_ε = chol(I + B Bᵀ), the vector solves)
        return fit_timings(c);
    });
    if (rc != 0) return rc;
    // a failing factorisation: K_zz (+ the bordered block of an append) or Λ_ε — reported like the reference's cholesky calls
    if (info_h != 0) return (mode == VFE_APPEND && info_h <= m2) ? (int32_t)(m_old + info_h) : info_h;
    // objective: dtc = -½ (N log2π + logdet Σy + logdet Λ_ε + ‖δ_s‖² − ‖Λ_ε.U⁻ᵀ A δ_s‖²)          :302-303
    //            elbo = dtc − ½ (tr(K_ff Σy⁻¹) − ‖A‖²_F),  ‖A‖²_F = ‖B‖²_F                          :251
    double trZ = 0;
    for (long i = 0; i < m; ++i) trZ += rss_h[i];
    const double logdet_lam = 2.0 * scal_h[1], quad = scal_h[3];
    double obj = -0.5 * ((double)n_all * LOG2PI + logdet_sy + logdet_lam + dd - quad);
    if (approx == 0) obj -= 0.5 * (tr_kff - trZ);
    if (objective) *objective = obj;
    if (cols && objective)  // a column's objective differs in ‖b_s‖² and ‖L_D⁻¹ B b_s‖² only
        for (int col = 0; col < S; ++col) {
            double o = -0.5 * ((double)n_all * LOG2PI + logdet_sy + logdet_lam + ddc[col] - quad_h[col]);
            if (approx == 0) o -= 0.5 * (tr_kff - trZ);
            objective[col] = o;
        }
    if (out) {
        out->ncols = S;
        out->vrows = VR;
        out->ddc = ddc;
        if (cols) {
            out->dib_z = dibs.z;
            out->dib_d = dibs.d;
            dibs.z = DibCache();
            dibs.d = DibCache();
        }
        out->ctx = c;
        out->dtype = k->dtype;
        out->m = m; out->mp = mp; out->ld = ld; out->d = d; out->jitter = jitter;
        out->kern = KernelRec(k, nullptr);
        out->Lz = bufs.keep(Lz_v);
        out->Ld = bufs.keep(Ld_v);
        out->zs = bufs.keep(zsD_v);
        out->vec = bufs.keep(vec_v);
        out->approx = approx;
        out->n_obs = n_all;
        out->chunk = CH;
        out->Dacc = bufs.keep(D_v);
        out->cacc = bufs.keep(cT_v);
        out->rowss = bufs.keep(rss_v);
        out->Li = bufs.keep(Li_v);
        out->zsT = bufs.keep(zsT_v);
        out->segs.clear();
        if (prev) out->segs = prev->segs;
        if (seg) out->segs.push_back(seg);
        out->logdet_sy = logdet_sy; out->dd = dd; out->tr_kff = tr_kff; out->trZ = trZ;
    }
    return 0;
}

// X (nsp × mp, leading dimension p->ld) = K(x*, z) L_z⁻ᵀ, the rows Aᵀ every predictive formula starts from (:187-195); xs_dev: the staged test points, [d][nsp]
static int32_t vfe_cross_solve(gp_vfe* p, hipStream_t s, DevBufs& bufs, const double* xs_dev, long ns, long nsp, double* X) {
    const long mp = p->mp, ld = p->ld;
    GridMap g = plain_map(0, 0, 0);
    dim3 grid((unsigned)(mp / 128), (unsigned)(nsp / 128));
    launch_kmat<double>(grid, s, X, ld, xs_dev, nsp, (const double*)p->zs, mp, p->d, p->kern.kind, p->kern.variance, (const double*)nullptr, ns, p->m, 0, g,
                        (const double*)nullptr, (const double*)nullptr);
    HIPCHK(hipGetLastError());
    return trsm_cached<double>(p->ctx, s, X, ld, nsp, (const double*)p->Lz, ld, mp, p->m, p->dib_z, bufs);
}

// Joint predictive distribution of the approximate posterior at x* on the device (always fp64 on the M side):
//   A = U⁻ᵀ K_z*  ->  rows X1 = K_*z L_z⁻ᵀ,  X2 = X1 L_D⁻ᵀ;   cov = K** − X1 X1ᵀ + X2 X2ᵀ (+ Σy*)        :187-190, :205-210
template <typename T>
static int32_t vfe_joint(gp_vfe* p, const gp_points* xs, const void* pm, const gp_noise* noise, long R, DevBufs& bufs,
                         Joint<double>& J) {
    gp_ctx* c = p->ctx;
    SkScope sk(c);
    const long m = p->m, mp = p->mp, ld = p->ld;
    const long ns = xs->n, nsp = round_up(ns, 128);
    const int d = p->d;
    const gp_kernel k = p->kern.view(0);
    StagedPoints<T, double> sx;  // inputs arrive in T; scaled in T (as the fit did), then widened
    std::vector<double> nz_h;
    noise_to<double, T>(noise, ns, nsp, nz_h);
    const double* vec = (const double*)p->vec;
    const long ldc = nsp + c->ldpad;
    const size_t X_b = sizeof(double) * (size_t)(nsp + 128) * ld;
    void *nz_v = 0, *m_v = 0, *X1_v = 0, *X2_v = 0, *X2n_v = 0;
    RC(sx.stage(c, bufs, &k, xs, nsp));
    RC(bufs.get(sizeof(double) * (size_t)nsp, &nz_v));
    RC(bufs.get(sizeof(double) * (size_t)nsp, &m_v));
    RC(bufs.get(X_b, &X1_v));
    RC(bufs.get(X_b, &X2_v));
    RC(bufs.get(X_b, &X2n_v));
    RC(bufs.get(sizeof(double) * (size_t)(nsp + R + 128) * ldc, &J.C));
    J.ns = ns; J.nsp = nsp; J.ld = ldc; J.R = R;
    double* X1 = (double*)X1_v;
    double* X2 = (double*)X2_v;
    double* Cm = (double*)J.C;
    hipStream_t s = c->sm;
    c->ev_used = 0;
    c->gemm_recs.clear();
    std::vector<double> m_h((size_t)ns);
    HIPCHK(hipMemcpyAsync(nz_v, nz_h.data(), sizeof(double) * (size_t)nsp, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(kvec_kernel<double>, dim3((unsigned)ns), dim3(256), 0, s, sx.ptr(), nsp, (const double*)p->zs, mp, d,
                       p->kern.kind, p->kern.variance, m, vec + 2 * mp, (double*)m_v);                                     // K_*z α
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(m_h.data(), m_v, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
    RC(vfe_cross_solve(p, s, bufs, sx.ptr(), ns, nsp, X1));
    HIPCHK(hipMemcpyAsync(X2_v, X1_v, X_b, hipMemcpyDeviceToDevice, s));
    RC(trsm_cached<double>(c, s, X2, ld, nsp, (const double*)p->Ld, ld, mp, p->m, p->dib_d, bufs));
    {
        const long cnt = (long)(nsp + 128) * ld;
        hipLaunchKernelGGL((convert_kernel<double, double>), convert_grid(cnt), dim3(256), 0, s, (const double*)X2,
                           (double*)X2n_v, cnt, -1.0);
        HIPCHK(hipGetLastError());
    }
    {
        GridMap g = plain_map(1, 0, 0);
        dim3 grid((unsigned)(nsp / 128), (unsigned)(nsp / 128));
        launch_kmat<double>(grid, s, Cm, ldc, sx.ptr(), nsp, sx.ptr(), nsp, d,
                           p->kern.kind, p->kern.variance, (const double*)nz_v, ns, ns, 1, g, (const double*)nullptr, (const double*)nullptr);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(Cm + nsp * ldc, 0, sizeof(double) * (size_t)(R + 128) * ldc, s));
    RC(launch_gemm<double>(c, s, Cm, ldc, X1, ld, X1, ld, nsp, nsp, mp, plain_map(1, 0, 0)));                     // − AᵀA
    RC(launch_gemm<double>(c, s, Cm, ldc, (const double*)X2n_v, ld, X2, ld, nsp, nsp, mp, plain_map(1, 0, 0)));  // + (Λ_ε.U⁻ᵀA)ᵀ(·)
    if (noise_dense(noise)) RC((dense_add<double, T>(c, bufs, Cm, ldc, noise, ns)));                              // a dense Σy* (host array in T)
    HIPCHK(hipStreamSynchronize(s));
    const T* prior = (const T*)pm;
    J.mean.resize((size_t)ns);
    for (long i = 0; i < ns; ++i) J.mean[i] = (prior ? (double)prior[i] : 0.0) + m_h[i];
    return 0;
}

template <typename T>
static int32_t vfe_predict_impl(gp_vfe* p, const gp_points* xs, const void* pm, int what, void* mean_out, void* var_out,
                                void* cov_out) {
    gp_ctx* c = p->ctx;
    if (what & 4) {  // full covariance (+ mean): the joint, copied out and mirrored on the host                :187-190, :205-210
        DevBufs bufs(c);
        Joint<double> J;
        const int32_t rc = vfe_joint<T>(p, xs, pm, nullptr, 0, bufs, J);
        if (rc != 0) {
            ctx_drain(c);
            return rc;
        }
        const long ns = J.ns;
        std::vector<double> Ch((size_t)ns * ns);
        HIPCHK(hipMemcpy2DAsync(Ch.data(), sizeof(double) * ns, J.C, sizeof(double) * J.ld, sizeof(double) * ns, ns, hipMemcpyDeviceToHost,
                                c->sm));
        HIPCHK(hipStreamSynchronize(c->sm));
        T* co = (T*)cov_out;
        for (long i = 0; i < ns; ++i)
            for (long j = 0; j <= i; ++j) co[i + j * ns] = co[j + i * ns] = (T)Ch[(size_t)i * ns + j];
        if (what & 1)
            for (long i = 0; i < ns; ++i) ((T*)mean_out)[i] = (T)J.mean[i];
        if (what & 2)
            for (long i = 0; i < ns; ++i) ((T*)var_out)[i] = (T)Ch[(size_t)i * ns + i];
        return 0;
    }
    const long m = p->m, mp = p->mp, ld = p->ld;
    const long ns = xs->n, nsp = round_up(ns, 128);
    const int d = p->d;
    const gp_kernel k = p->kern.view(0);
    StagedPoints<T, double> sx;  // inputs arrive in T; scaled in T (as the fit did), then widened
    const double* vec = (const double*)p->vec;
    const size_t X_b = sizeof(double) * (size_t)(nsp + 128) * ld, o_b = sizeof(double) * (size_t)nsp * 3;
    void *X_v = 0, *o_v = 0;
    DevBufs bufs(c);
    hipStream_t s = c->sm;
    c->ev_used = 0;
    c->gemm_recs.clear();
    std::vector<double> oh((size_t)nsp * 3, 0.0);
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        RC(sx.stage(c, bufs, &k, xs, nsp));
        RC(bufs.get(X_b, &X_v));
        RC(bufs.get(o_b, &o_v));
        double* X = (double*)X_v;
        double* o = (double*)o_v;
        if (what & 1) {  // mean = m(x*) + K_*z α                                                  :183-185
            hipLaunchKernelGGL(kvec_kernel<double>, dim3((unsigned)ns), dim3(256), 0, s, sx.ptr(), nsp,
                               (const double*)p->zs, mp, d, p->kern.kind, p->kern.variance, m, vec + 2 * mp, o);
            HIPCHK(hipGetLastError());
        }
        if (what & 2) {  // var = k** − ‖A‖²_col + ‖Λ_ε.U⁻ᵀ A‖²_col, Aᵀ = K_*z L_z⁻ᵀ                 :192-195
            RC(vfe_cross_solve(p, s, bufs, sx.ptr(), ns, nsp, X));
            hipLaunchKernelGGL(rowsumsq_kernel<double>, dim3((unsigned)nsp), dim3(256), 0, s, X, ld, mp, o + nsp);
            HIPCHK(hipGetLastError());
            RC(trsm_cached<double>(c, s, X, ld, nsp, (const double*)p->Ld, ld, mp, p->m, p->dib_d, bufs));
            hipLaunchKernelGGL(rowsumsq_kernel<double>, dim3((unsigned)nsp), dim3(256), 0, s, X, ld, mp, o + 2 * nsp);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(oh.data(), o, o_b, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
    if (rc != 0) return rc;
    const T* prior = (const T*)pm;
    if (what & 1)
        for (long i = 0; i < ns; ++i) ((T*)mean_out)[i] = (T)((prior ? (double)prior[i] : 0.0) + oh[i]);
    if (what & 2)
        for (long i = 0; i < ns; ++i) ((T*)var_out)[i] = (T)(p->kern.variance - oh[nsp + i] + oh[2 * nsp + i]);
    return 0;
}

// gp_vfe_predict_cols: the means of every column, mean_out (ns × ncols column-major) = m(x*) + K(x*, z) A with A = the M × ncols matrix of the α_s, by ONE
// kmul launch over the pseudo-points (gpmi355.hip kmul: K_*z evaluated once for all columns, fixed-order partial sums); variance and covariance do not
// depend on y and come from vfe_predict_impl.  fp64 on the device whatever the handle's dtype, as every prediction of the sparse path.
template <typename T>
static int32_t vfe_predict_cols_impl(gp_vfe* p, const gp_points* xs, const void* pm, int what, void* mean_out, void* var_out, void* cov_out) {
    gp_ctx* c = p->ctx;
    if (p->ncols == 1) return vfe_predict_impl<T>(p, xs, pm, what, mean_out, var_out, cov_out);  // one column: the call IS gp_vfe_predict
    if (what & 1) {
        const long mp = p->mp, ns = xs->n, nsp = round_up(ns, 128);
        const int S = p->ncols;
        const gp_kernel k = p->kern.view(0);
        StagedPoints<T, double> sx;
        DevBufs bufs(c);
        void* m_v = nullptr;
        hipStream_t s = c->sm;
        c->ev_used = 0;
        c->gemm_recs.clear();
        std::vector<double> mh((size_t)ns * S);
        const double* alpha = (const double*)p->vec + 2 * (long)p->vrows * mp;
        const int32_t rc = run_drained(c, [&]() -> int32_t {
            RC(sx.stage(c, bufs, &k, xs, nsp));
            RC(bufs.get(sizeof(double) * (size_t)nsp * S, &m_v));
            RC(kmul<double>(c, bufs, p->kern.desc(), ns, s, sx.ptr(), nsp, (const double*)p->zs, mp, p->d, p->m, alpha, mp, S, (double*)m_v, nsp));
            HIPCHK(hipMemcpy2DAsync(mh.data(), sizeof(double) * ns, m_v, sizeof(double) * nsp, sizeof(double) * ns, S, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            return 0;
        });
        if (rc != 0) return rc;
        const T* prior = (const T*)pm;
        for (int col = 0; col < S; ++col)
            for (long i = 0; i < ns; ++i) ((T*)mean_out)[(size_t)col * ns + i] = (T)((prior ? (double)prior[i] : 0.0) + mh[(size_t)col * ns + i]);
    }
    if (what & 6) return vfe_predict_impl<T>(p, xs, pm, what & 6, nullptr, var_out, cov_out);
    return 0;
}

// Predictive mean / variance of a sparse posterior AND their gradients w.r.t. the test inputs (include/gpmi355.h gp_vfe_predict_grad), next to
// vfe_predict_impl and with its buffers (fp64 whatever the handle's dtype; results rounded to T).  With A_j = L_z⁻¹ K(z, x*_j) a row of X1 = K_*z L_z⁻ᵀ:
//   ∂mean_j = Σ_m α_m ∂k(x*_j, z_m),   ∂var_j = −2 Σ_m u_jm ∂k(x*_j, z_m),   u_j = L_z⁻ᵀ (A_j − Λ_ε⁻¹ A_j)
// Both forward solves as in vfe_predict_impl (X2 = X1 L_d⁻ᵀ), then X2 ← X2 L_d⁻¹ (= (Λ_ε⁻¹A)ᵀ), X2 ← X1 − X2, X2 ← X2 L_z⁻¹ (all M-wide, trsm_back_cached) and
// kpgrad_kernel over the pseudo-points.
template <typename T>
static int32_t vfe_predict_grad_impl(gp_vfe* p, const gp_points* xs, const void* pm, int what, void* mean_out, void* var_out, void* dmean_out,
                                     void* dvar_out) {
    gp_ctx* c = p->ctx;
    const long m = p->m, mp = p->mp, ld = p->ld;
    const long ns = xs->n, nsp = round_up(ns, 128);
    const int d = p->d;
    const gp_kernel k = p->kern.view(0);
    const KDesc kd = p->kern.desc();
    StagedPoints<T, double> sx;
    DevScales sc;
    const double* vec = (const double*)p->vec;
    const bool want_gm = (what & 1) && dmean_out, want_gv = (what & 2) && dvar_out, side_v = (what & 2) != 0;
    const size_t X_b = sizeof(double) * (size_t)(nsp + 128) * ld, o_b = sizeof(double) * (size_t)nsp * 3, g_b = sizeof(double) * (size_t)2 * d * nsp;
    void *X1_v = 0, *X2_v = 0, *o_v = 0, *g_v = 0;
    DevBufs bufs(c);
    hipStream_t s = c->sm;
    c->ev_used = 0;
    c->gemm_recs.clear();
    std::vector<double> oh((size_t)nsp * 3, 0.0), g_h((want_gm || want_gv) ? (size_t)2 * d * nsp : 0);
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        RC(sx.stage(c, bufs, &k, xs, nsp));
        RC(bufs.get(o_b, &o_v));
        RC(bufs.get(g_b, &g_v));
        RC(sc.stage(bufs, k.nscale, k.scale, s));
        if (side_v) RC(bufs.get(X_b, &X1_v));
        if (want_gv) RC(bufs.get(X_b, &X2_v));
        double* X1 = (double*)X1_v;
        double* X2 = want_gv ? (double*)X2_v : X1;
        double* o = (double*)o_v;
        double* gm = want_gm ? (double*)g_v : nullptr;
        double* gv = want_gv ? (double*)g_v + (size_t)d * nsp : nullptr;
        HIPCHK(hipMemsetAsync(o, 0, o_b, s));
        // the 128 slack rows below the test points are operand over-read of the solves' GEMMs: finite, whatever the recycled block held
        if (side_v) HIPCHK(hipMemsetAsync(X1 + (size_t)nsp * ld, 0, sizeof(double) * (size_t)128 * ld, s));
        if (want_gv) HIPCHK(hipMemsetAsync(X2 + (size_t)nsp * ld, 0, sizeof(double) * (size_t)128 * ld, s));
        if ((what & 1) && mean_out) {
            hipLaunchKernelGGL(kvec_kernel<double>, dim3((unsigned)ns), dim3(256), 0, s, sx.ptr(), nsp, (const double*)p->zs, mp, d, p->kern.kind,
                               p->kern.variance, m, vec + 2 * mp, o);
            HIPCHK(hipGetLastError());
        }
        if (want_gm && !want_gv)
            RC(launch_kpgrad<double>(kd, k.nscale, sc.ptr(), ns, s, sx.ptr(), nsp, (const double*)p->zs, mp, d, m, vec + 2 * mp,
                                     (const double*)nullptr, 0, gm, (double*)nullptr, nsp, 0));
        if (side_v) {
            RC(vfe_cross_solve(p, s, bufs, sx.ptr(), ns, nsp, X1));
            hipLaunchKernelGGL(rowsumsq_kernel<double>, dim3((unsigned)nsp), dim3(256), 0, s, X1, ld, mp, o + nsp);
            HIPCHK(hipGetLastError());
            if (want_gv) HIPCHK(hipMemcpyAsync(X2, X1, sizeof(double) * (size_t)nsp * ld, hipMemcpyDeviceToDevice, s));
            RC(trsm_cached<double>(c, s, X2, ld, nsp, (const double*)p->Ld, ld, mp, p->m, p->dib_d, bufs));
            hipLaunchKernelGGL(rowsumsq_kernel<double>, dim3((unsigned)nsp), dim3(256), 0, s, X2, ld, mp, o + 2 * nsp);
            HIPCHK(hipGetLastError());
            if (want_gv) {
                BackWs wb;  // one transpose scratch for both sweeps (same M, same block width)
                RC(trsm_back_cached<double>(c, s, X2, ld, nsp, ns, (const double*)p->Ld, ld, mp, p->dib_d, bufs, wb));
                hipLaunchKernelGGL(rsub_kernel, dim3((unsigned)ns), dim3(256), 0, s, (const double*)X1, X2, ld, mp);
                HIPCHK(hipGetLastError());
                RC(trsm_back_cached<double>(c, s, X2, ld, nsp, ns, (const double*)p->Lz, ld, mp, p->dib_z, bufs, wb));
                RC(launch_kpgrad<double>(kd, k.nscale, sc.ptr(), ns, s, sx.ptr(), nsp, (const double*)p->zs, mp, d, m, vec + 2 * mp,
                                         (const double*)X2, ld, gm, gv, nsp, 0));
            }
        }
        HIPCHK(hipMemcpyAsync(oh.data(), o, o_b, hipMemcpyDeviceToHost, s));
        if (want_gm || want_gv) HIPCHK(hipMemcpyAsync(g_h.data(), g_v, g_b, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
    if (rc != 0) return rc;
    const T* prior = (const T*)pm;
    if ((what & 1) && mean_out)
        for (long i = 0; i < ns; ++i) ((T*)mean_out)[i] = (T)((prior ? (double)prior[i] : 0.0) + oh[i]);
    if (side_v && var_out)
        for (long i = 0; i < ns; ++i) ((T*)var_out)[i] = (T)(p->kern.variance - oh[nsp + i] + oh[2 * nsp + i]);
    if (want_gm) grad_to_layout<T>(xs->layout, ns, d, g_h.data(), nsp, dmean_out);
    if (want_gv) grad_to_layout<T>(xs->layout, ns, d, g_h.data() + (size_t)d * nsp, nsp, dvar_out);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Gradient of the sparse objective of a fitted handle (gp_vfe_grad): elbo (VFE, src/sparse_approximations.jl:248-254) or approx_log_evidence (DTC, :282-286)
// against the kernel variance, the Scale / ARD parameters, the noise variances, y, the pseudo-inputs z and (optionally) the inputs x — what an AD backend
// computes when examples/0-intro-1d/script.jl:385-394 maximises the ELBO over kernel parameters and pseudo-points.
//   With ψ = K_zf Σy⁻¹ K_fz, φ = K_zf Σy⁻¹ δ, Q = K_zz + ψ = L_z A L_zᵀ (A = I + B Bᵀ = Λ_ε) and ν = Q⁻¹φ = α (the posterior's own α):
//     L = −½ [N log 2π + log|Q| − log|K_zz| + log|Σy| + δᵀΣy⁻¹δ − φᵀQ⁻¹φ] − ½ [tr(Σy⁻¹K_ff) − tr(K_zz⁻¹ψ)]         (second bracket: VFE only)
//     G_ψ  = ∂L/∂ψ    = ½ [W H_ψ Wᵀ − ααᵀ],   H_ψ  = I − A⁻¹ (VFE) | −A⁻¹ (DTC),            W = L_z⁻ᵀ
//     G_zz = ∂L/∂K_zz = ½ [W H_zz Wᵀ − ααᵀ],  H_zz = I − A⁻¹ − B Bᵀ (VFE) | I − A⁻¹ (DTC)
//     ∂L/∂K_fz = Σy⁻¹ (2 K_fz G_ψ + δ αᵀ),   ∂L/∂k_ii = −½/σ_i² (VFE)
//     ∂L/∂σ_i² = −½/σ_i² + ½ δ_i²/σ_i⁴ [+ ½ k_ii/σ_i⁴ VFE] − (k_iᵀ G_ψ k_i)/σ_i⁴ − (αᵀk_i) δ_i/σ_i⁴,     ∂L/∂y_i = −(δ_i − αᵀk_i)/σ_i²
//   The M×M side is fp64 (two triangular inverses, A⁻¹, two conjugations: ≈ 10 M³ flops); the N-long side streams the retained observations once more in the
//   fit's chunks: kmat (S K_c) → ONE MFMA GEMM T̃ = (S K_c) G_ψ (2·CH·M² flops) → vgrad_kernel (κ, dκ recomputed; every reduction fp64).  The pass is fp64 for
//   fp32 handles too (their retained inputs are widened chunk by chunk): G_ψ carries K_zz⁻¹ (entries up to 1/jitter) against which S K_c cancels to O(1) —
//   rounded to fp32 it cost 6–8 % of the variance / pseudo-input gradients at N = 3 000 already (measured, round 6), at the fp32 MFMA rate that is not a trade.
//   (oracle: gp_oracle.elbo_grad — dense N×N calculus on the textbook form; tests/test_gpu_vfe_grad.py)
// ------------------------------------------------------------------------------------------------
template <typename T, bool XG>
static int32_t launch_vgrad(hipStream_t s, dim3 grid, const T* Cm, long ldc, int explicit_w, const T* xr, long ldxr, const T* xc, long ldxc, int d, int kind,
                            double variance, int nscale, const double* scale, const T* rs, const T* bv, const double* nu, long nr, long nc, double* g,
                            double* gz, long ldgz, double zfac, double* rowq, double* rowp, double* gx, long ldgx) {
#define GPMI_VGRAD_FAST(ND_)                                                                                                                                  \
    hipLaunchKernelGGL((vgrad_fast_kernel<T, ND_, XG>), grid, dim3(256), 0, s, Cm, ldc, explicit_w, xr, ldxr, xc, ldxc, d, kind, (T)variance, nscale, scale, \
                       rs, bv, nu, nr, nc, g, gz, ldgz, zfac, rowq, rowp, gx, ldgx)
    if (d <= 16 && (ldc & 1) == 0) {   // the scratch-free form (16-byte loads of the weights: even leading dimension)
        if (d <= 4) GPMI_VGRAD_FAST(4);
        else if (d <= 8) GPMI_VGRAD_FAST(8);
        else GPMI_VGRAD_FAST(16);
        HIPCHK(hipGetLastError());
        return 0;
    }
#undef GPMI_VGRAD_FAST
    for (int p0 = 0; p0 < d; p0 += 16) {
        hipLaunchKernelGGL((vgrad_kernel<T, 16, true, XG>), grid, dim3(256), 0, s, Cm, ldc, explicit_w, xr, ldxr, xc, ldxc, d, kind, (T)variance, nscale, scale,
                           rs, bv, nu, nr, nc, g, gz, ldgz, zfac, rowq, rowp, gx, ldgx, p0);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

template <typename T>
static int32_t vfe_grad_impl(gp_vfe* p, double* dvar, double* dscale, double* dnoise_sum, void* dnoise, void* dy, double* dz, int z_layout, void* dx,
                             int x_layout) {
    gp_ctx* c = p->ctx;
    const long m = p->m, mp = p->mp, ld = p->ld, CH = p->chunk;
    const int d = p->d;
    const bool vfe = p->approx == 0;
    constexpr bool is_f64 = sizeof(T) == 8;
    for (auto& sg : p->segs)
        if (sg->npad % CH) return set_arg_err(1, "gp_vfe was built with a different vfe_chunk");
    hipStream_t s = c->sm;
    c->ev_used = 0;
    c->gemm_recs.clear();
    for (auto& e : c->ev_phase)
        if (!e) HIPCHK(hipEventCreate(&e));
    const int nsc = std::max(p->kern.nscale(), 1);
    const size_t L_b = sizeof(double) * (size_t)(mp + 128 + 128) * ld;
    const size_t X_b = sizeof(double) * (size_t)(CH + 128) * ld, g_b = sizeof(double) * (size_t)(2 + nsc + 2), gz_b = sizeof(double) * (size_t)d * mp;
    void *W_v = 0, *V_v = 0, *H_v = 0, *R_v = 0, *E_v = 0, *Gp_v = 0, *Gz_v = 0, *X_v = 0, *X2_v = 0, *C2_v = 0, *xc_v = 0, *rc_v = 0, *bc_v = 0, *C_v = 0, *g_v = 0, *gz_v = 0;
    DevBufs bufs(c);
    RC(bufs.get(L_b, &W_v));
    RC(bufs.get(L_b, &V_v));
    RC(bufs.get(L_b, &H_v));
    RC(bufs.get(L_b, &R_v));
    RC(bufs.get(L_b, &E_v));
    RC(bufs.get(L_b, &Gp_v));
    RC(bufs.get(L_b, &Gz_v));
    RC(bufs.get(X_b, &X_v));
    if (!is_f64) {  // the chunk's inputs, Σy^-1/2 and b_y widened to fp64
        RC(bufs.get(sizeof(double) * (size_t)d * CH * 2, &xc_v));
        RC(bufs.get(sizeof(double) * (size_t)CH * 2, &rc_v));
        RC(bufs.get(sizeof(double) * (size_t)CH * 2, &bc_v));
    }
    RC(bufs.get(X_b, &C_v));
    RC(bufs.get(X_b, &X2_v));  // double buffers in either mode ("vfe_overlap" = 0 issues the same sequence to one stream)
    RC(bufs.get(X_b, &C2_v));
    RC(bufs.get(g_b, &g_v));
    RC(bufs.get(gz_b, &gz_v));
    // Columns (gp_vfe_grad_cols: the gradient of Σ_s objective_s; dy is then dY, n × S column-major).  The M×M algebra with the column sums folded in:
    //   G = ½[S·W H Wᵀ − A Aᵀ] (A = the M × S matrix of the α_s): one rank-S MFMA GEMM E −= (A/√S)(A/√S)ᵀ before the combination, weight S/2.
    // Per chunk two skinny MFMA GEMMs beside T̃ = (S K_c) G_ψ: the rank-S term of the weights, C −= (½√S b_c)(A/√S)ᵀ — so the chunk's −C is T̃ + ½ b_c Aᵀ and
    // vgrad runs unchanged with ν = 0 — and Pt = −Aᵀ(S K_c)ᵀ (128 × CH), the per-column row sums; vgrad_finish_cols_kernel finishes ∂/∂σ_i², ∂/∂Y per chunk.
    const int S = p->ncols;
    const bool cols = S > 1;
    const long ldt = 128 + c->ldpad, ldpt = CH + c->ldpad;
    const size_t At_b = sizeof(double) * (size_t)256 * ld, A2_b = sizeof(double) * (size_t)(mp + 128) * ldt, Bt_b = sizeof(double) * (size_t)(CH + 128) * ldt,
                 Pt_b = sizeof(double) * (size_t)256 * ldpt;
    void *At_v = 0, *Ats_v = 0, *A2_v = 0, *Bt_v = 0, *Pt_v = 0, *nu0_v = 0;
    if (cols) {
        RC(bufs.get(At_b, &At_v));    // rows α_s
        RC(bufs.get(At_b, &Ats_v));   // rows α_s/√S
        RC(bufs.get(A2_b, &A2_v));    // its transpose: mp × 128
        RC(bufs.get(Bt_b, &Bt_v));    // the chunk's ½√S b_y columns, CH × 128
        RC(bufs.get(Pt_b, &Pt_v));
        RC(bufs.get(sizeof(double) * (size_t)mp, &nu0_v));
    }
    DevScales sc;
    double *W = (double*)W_v, *V = (double*)V_v, *H = (double*)H_v, *R = (double*)R_v, *E = (double*)E_v, *Gp = (double*)Gp_v, *Gz = (double*)Gz_v;
    const double* Lz = (const double*)p->Lz;
    const double* Ld = (const double*)p->Ld;
    const double* alpha = (const double*)p->vec + 2 * (long)p->vrows * mp;   // (columns: the rows α_s, mp apart)
    std::vector<double> g_h((size_t)(2 + nsc + 2), 0.0), gz_h((size_t)d * mp, 0.0);   // [0] ∂/∂variance, [2 + p] ∂/∂scale_p, [2 + nsc] Σ ∂/∂σ_i², [3 + nsc] Σ σ_i⁻²
    // per observation (concatenated over the segments, arrival order): what the host needs to finish ∂/∂σ_i², ∂/∂y_i, ∂/∂x_i
    long n_all = 0;
    for (auto& sg : p->segs) n_all += sg->n;
    std::vector<double> gx_all(dx ? (size_t)n_all * d : 0);
    const dim3 sq((unsigned)((mp + 255) / 256), (unsigned)mp);
    auto conj = [&](const double* Hm, double* G) -> int32_t {  // G (full, symmetric) = ½ W Hm Wᵀ − ½ ααᵀ
        GridMap gr = plain_map(0, 0, 0);
        gr.beta0 = 1;
        gr.ktri = 2;                                                                           // W upper: k starts at the row tile
        RC(launch_gemm<double>(c, s, R, ld, W, ld, Hm, ld, mp, mp, mp, gr));                   // R = −W Hm        (Hm symmetric)
        GridMap ge = plain_map(1, 0, 0);
        ge.beta0 = 1;
        RC(launch_gemm<double>(c, s, E, ld, R, ld, W, ld, mp, mp, mp, ge));                    // E = −R Wᵀ = W Hm Wᵀ (lower)
        if (cols) {  // G = (S/2) [W Hm Wᵀ − (A/√S)(A/√S)ᵀ]
            RC(launch_gemm<double>(c, s, E, ld, (const double*)A2_v, ldt, (const double*)A2_v, ldt, mp, mp, 128, plain_map(1, 0, 0)));
            hipLaunchKernelGGL(sym_combine_kernel, sq, dim3(256), 0, s, G, ld, mp, (const double*)E, ld, 0.5 * S, (const double*)nullptr, 0L, 0.0, 0.0,
                               (const double*)nullptr, 0.0);
        } else {
            hipLaunchKernelGGL(sym_combine_kernel, sq, dim3(256), 0, s, G, ld, mp, (const double*)E, ld, 0.5, (const double*)nullptr, 0L, 0.0, 0.0, alpha, -0.5);
        }
        HIPCHK(hipGetLastError());
        return 0;
    };
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        HIPCHK(hipEventRecord(c->ev_phase[0], s));
        RC(sc.stage(bufs, p->kern.nscale(), p->kern.scale.data(), s));
        HIPCHK(hipMemsetAsync(g_v, 0, g_b, s));
        HIPCHK(hipMemsetAsync(gz_v, 0, gz_b, s));
        for (void* q : {H_v, R_v, E_v, Gp_v, Gz_v}) HIPCHK(hipMemsetAsync(q, 0, L_b, s));   // the GEMMs over-read whole operand tiles: defined slack rows
        HIPCHK(hipMemsetAsync(C_v, 0, X_b, s));
        if (C2_v) HIPCHK(hipMemsetAsync(C2_v, 0, X_b, s));
        HIPCHK(hipMemsetAsync(X_v, 0, X_b, s));
        if (X2_v) HIPCHK(hipMemsetAsync(X2_v, 0, X_b, s));
        if (cols) {
            for (void* q : {At_v, Ats_v}) HIPCHK(hipMemsetAsync(q, 0, At_b, s));
            HIPCHK(hipMemsetAsync(A2_v, 0, A2_b, s));
            HIPCHK(hipMemsetAsync(Bt_v, 0, Bt_b, s));
            HIPCHK(hipMemsetAsync(Pt_v, 0, Pt_b, s));
            HIPCHK(hipMemsetAsync(nu0_v, 0, sizeof(double) * (size_t)mp, s));
            HIPCHK(hipMemcpy2DAsync(At_v, sizeof(double) * ld, alpha, sizeof(double) * mp, sizeof(double) * mp, S, hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL((convert_kernel<double, double>), convert_grid(256 * ld), dim3(256), 0, s, (const double*)At_v, (double*)Ats_v, 256 * ld,
                               1.0 / std::sqrt((double)S));
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(transpose_rect_kernel<double>, dim3((unsigned)((mp + 31) / 32), 4), dim3(256), 0, s, (const double*)Ats_v, ld, (double*)A2_v, ldt,
                               128L, mp, 0);
            HIPCHK(hipGetLastError());
        }
        // ---- M×M side, fp64
        RC(vfe_upper_inverse(c, s, Lz, ld, mp, W, L_b, bufs));                                  // W = L_z⁻ᵀ
        RC(vfe_upper_inverse(c, s, Ld, ld, mp, V, L_b, bufs));                                  // V = Λ_ε.L⁻ᵀ
        {
            GridMap gw = plain_map(1, 0, 0);
            gw.ktri = 2;
            gw.beta0 = 1;
            RC(launch_gemm<double>(c, s, E, ld, V, ld, V, ld, mp, mp, mp, gw));                 // E = −V Vᵀ = −A⁻¹ (lower)
        }
        // H_ψ, then H_zz (padding rows: A⁻¹ = I and B Bᵀ = 0 there, so the VFE forms vanish on the padding; the DTC H_ψ keeps −1 on the padded diagonal,
        // which only reaches padded columns of T̃ and padded entries of G — never read)
        hipLaunchKernelGGL(sym_combine_kernel, sq, dim3(256), 0, s, H, ld, mp, (const double*)E, ld, 1.0, (const double*)nullptr, 0L, 0.0, vfe ? 1.0 : 0.0,
                           (const double*)nullptr, 0.0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(V, E, L_b, hipMemcpyDeviceToDevice, s));                          // −A⁻¹ (lower) survives the first conjugation in V's storage
        RC(conj(H, Gp));
        hipLaunchKernelGGL(sym_combine_kernel, sq, dim3(256), 0, s, H, ld, mp, (const double*)V, ld, 1.0, vfe ? (const double*)p->Dacc : (const double*)nullptr, ld,
                           1.0, 1.0, (const double*)nullptr, 0.0);                              // Dacc = −B Bᵀ (lower)
        HIPCHK(hipGetLastError());
        RC(conj(H, Gz));
        HIPCHK(hipEventRecord(c->ev_phase[1], s));
        // ---- the observations, chunk by chunk: the MFMA GEMMs back to back on one stream; the next chunk's kmat (and, for fp32 handles, the widening of its
        //      inputs) and the previous chunk's vgrad on another beside them, on double buffers ("vfe_overlap")
        struct Ck {
            const ObsSeg* sg;
            long c0;
            double *rq, *rp, *gx;
            size_t si;  // its segment
        };
        std::vector<Ck> cks;
        std::vector<std::array<void*, 3>> segb;
        std::vector<std::array<void*, 2>> segc;  // columns: per segment ∂/∂σ_i² [npad] and ∂/∂Y [S][npad] in T
        for (auto& sgp : p->segs) {
            const ObsSeg& sg = *sgp;
            void *rq_v = 0, *rp_v = 0, *gx_v = 0;
            const size_t r_b = sizeof(double) * (size_t)std::max(sg.npad, 1L);
            RC(bufs.get(r_b, &rq_v));
            RC(bufs.get(r_b, &rp_v));
            if (dx) RC(bufs.get(r_b * d, &gx_v));
            HIPCHK(hipMemsetAsync(rq_v, 0, r_b, s));
            HIPCHK(hipMemsetAsync(rp_v, 0, r_b, s));
            if (dx) HIPCHK(hipMemsetAsync(gx_v, 0, r_b * d, s));
            segb.push_back({rq_v, rp_v, gx_v});
            void *dn_v = 0, *dY_v = 0;
            if (cols && sg.n > 0) {  // ∂/∂σ_i² and ∂/∂Y of the segment, written chunk by chunk
                RC(bufs.get(sizeof(T) * (size_t)sg.npad, &dn_v));
                if (dy) RC(bufs.get(sizeof(T) * (size_t)S * (size_t)sg.npad, &dY_v));
            }
            segc.push_back({dn_v, dY_v});
            for (long c0 = 0; c0 < sg.npad && c0 < sg.n; c0 += CH)
                cks.push_back({&sg, c0, (double*)rq_v + c0, (double*)rp_v + c0, dx ? (double*)gx_v + c0 : nullptr, segc.size() - 1});
        }
        // One stream.  The two-stream forms were measured at C5 (fp64 handle, tools/c5_grad_probe.py): helpers on the ctx's high-priority stream beside the GEMMs
        // 146.8 ms against 142.5 serial; GEMMs on the high-priority stream, helpers on the main one 142.6 / 143.3; and after the helper kernel lost its scratch
        // traffic (vgrad_fast_kernel: 1.1 -> 0.25 ms per chunk) 132.4 with two streams against 129.1 with one — what is left beside the GEMM (kmat + vgrad ≈ 0.4 ms
        // of 8.1 per chunk) costs more as a co-runner than in line.  The double buffers and events below stay for the experiment switch GPMI_VGRAD_STREAMS=2.
        static const bool two_streams = [] { const char* e = getenv("GPMI_VGRAD_STREAMS"); return e && e[0] == '2'; }();
        const bool ovl = two_streams && c->vfe_overlap != 0 && !cols;  // (the column form has one chunk-weight operand buffer: one stream)
        hipStream_t sa = s, sg = ovl ? c->sp : s;
        void* Xb[2] = {X_v, X2_v};
        void* Cb[2] = {C_v, C2_v};
        hipEvent_t evK[2] = {nullptr, nullptr}, evG[2] = {nullptr, nullptr}, evV[2] = {nullptr, nullptr};
        struct In {
            const double *xr, *rs, *b;
            long ldxr, nr;
        } in[2];
        if (ovl) {  // the GEMM stream starts after the M×M side (G_ψ) and the zeroing above
            hipEvent_t e;
            RC(ctx_event(c, &e, false));
            HIPCHK(hipEventRecord(e, s));
            HIPCHK(hipStreamWaitEvent(sg, e, 0));
        }
        auto prep = [&](size_t ci) -> int32_t {  // S K(x_c, z) of chunk ci into X[ci & 1], on the helper stream
            const int bb = (int)(ci & 1);
            const ObsSeg& sg = *cks[ci].sg;
            const long c0 = cks[ci].c0;
            if (ovl && evG[bb]) HIPCHK(hipStreamWaitEvent(sa, evG[bb], 0));  // the GEMM of chunk ci − 2 has read X[bb]
            In& I = in[bb];
            I.nr = std::min(CH, sg.n - c0);
            if constexpr (is_f64) {
                I.xr = (const double*)sg.xs + c0; I.ldxr = sg.npad; I.rs = (const double*)sg.rs + c0; I.b = (const double*)sg.b + c0;
            } else {
                double* xc = (double*)xc_v + (size_t)bb * d * CH;
                double* rc2 = (double*)rc_v + (size_t)bb * CH;
                double* bc2 = (double*)bc_v + (size_t)bb * CH;
                for (int q = 0; q < d; ++q) {
                    hipLaunchKernelGGL((convert_kernel<T, double>), convert_grid(CH), dim3(256), 0, sa, (const T*)sg.xs + (long)q * sg.npad + c0, xc + (long)q * CH, CH, 1.0);
                    HIPCHK(hipGetLastError());
                }
                hipLaunchKernelGGL((convert_kernel<T, double>), convert_grid(CH), dim3(256), 0, sa, (const T*)sg.rs + c0, rc2, CH, 1.0);
                HIPCHK(hipGetLastError());
                hipLaunchKernelGGL((convert_kernel<T, double>), convert_grid(CH), dim3(256), 0, sa, (const T*)sg.b + c0, bc2, CH, 1.0);
                HIPCHK(hipGetLastError());
                I.xr = xc; I.ldxr = CH; I.rs = rc2; I.b = bc2;
            }
            GridMap g = plain_map(0, 0, 0);
            dim3 grid((unsigned)(mp / 128), (unsigned)(CH / 128));
            launch_kmat<double>(grid, sa, (double*)Xb[bb], ld, I.xr, I.ldxr, (const double*)p->zs, mp, d, p->kern.kind, p->kern.variance, (const double*)nullptr, I.nr, m, 0, g,
                                (const double*)nullptr, I.rs);
            HIPCHK(hipGetLastError());
            if (ovl) {
                RC(ctx_event(c, &evK[bb], false));
                HIPCHK(hipEventRecord(evK[bb], sa));
            }
            return 0;
        };
        if (!cks.empty()) RC(prep(0));
        for (size_t ci = 0; ci < cks.size(); ++ci) {
            const int bb = (int)(ci & 1);
            if (ovl) {
                HIPCHK(hipStreamWaitEvent(sg, evK[bb], 0));
                if (evV[bb]) HIPCHK(hipStreamWaitEvent(sg, evV[bb], 0));  // vgrad of chunk ci − 2 has read C[bb]
            }
            {
                GridMap g = plain_map(0, 0, 0);
                g.beta0 = 1;
                RC(launch_gemm<double>(c, sg, (double*)Cb[bb], ld, (const double*)Xb[bb], ld, (const double*)Gp, ld, CH, mp, mp, g));   // C = −(S K_c) G_ψ
            }
            if (ovl) {
                RC(ctx_event(c, &evG[bb], false));
                HIPCHK(hipEventRecord(evG[bb], sg));
            }
            const In I = in[bb];
            const double* nuv = cols ? (const double*)nu0_v : alpha;
            if (cols) {
                const ObsSeg& sgc = *cks[ci].sg;
                hipLaunchKernelGGL(bt_cols_kernel<T>, dim3(4, (unsigned)(CH / 32)), dim3(256), 0, sg, (const T*)sgc.b + cks[ci].c0, sgc.npad, S, CH,
                                   0.5 * std::sqrt((double)S), (double*)Bt_v, ldt);
                HIPCHK(hipGetLastError());
                RC(launch_gemm<double>(c, sg, (double*)Cb[bb], ld, (const double*)Bt_v, ldt, (const double*)A2_v, ldt, CH, mp, 128, plain_map(0, 0, 0)));  // C −= ½ b_c Aᵀ
                GridMap gp = plain_map(0, 0, 0);
                gp.beta0 = 1;
                RC(launch_gemm<double>(c, sg, (double*)Pt_v, ldpt, (const double*)At_v, ld, (const double*)Xb[bb], ld, 128, CH, mp, gp));                  // Pt = −Aᵀ (S K_c)ᵀ
            }
            if (ci + 1 < cks.size()) RC(prep(ci + 1));  // beside this chunk's GEMM
            if (ovl) HIPCHK(hipStreamWaitEvent(sa, evG[bb], 0));
            dim3 grid((unsigned)(mp / 128), (unsigned)((I.nr + 127) / 128));
            if (dx)
                RC((launch_vgrad<double, true>(sa, grid, (const double*)Cb[bb], ld, 0, I.xr, I.ldxr, (const double*)p->zs, mp, d, p->kern.kind, p->kern.variance, p->kern.nscale(),
                                               sc.ptr(), I.rs, I.b, nuv, I.nr, m, (double*)g_v, (double*)gz_v, mp, 1.0, cks[ci].rq, cks[ci].rp,
                                               cks[ci].gx, cks[ci].sg->npad)));
            else
                RC((launch_vgrad<double, false>(sa, grid, (const double*)Cb[bb], ld, 0, I.xr, I.ldxr, (const double*)p->zs, mp, d, p->kern.kind, p->kern.variance, p->kern.nscale(),
                                                sc.ptr(), I.rs, I.b, nuv, I.nr, m, (double*)g_v, (double*)gz_v, mp, 1.0, cks[ci].rq, cks[ci].rp,
                                                (double*)nullptr, 0L)));
            if (cols) {  // the chunk's rows of rq are complete: ∂/∂σ_i², ∂/∂Y of its observations
                const ObsSeg& sgc = *cks[ci].sg;
                const long c0 = cks[ci].c0;
                T* dYs = (T*)segc[cks[ci].si][1];
                hipLaunchKernelGGL(vgrad_finish_cols_kernel<T>, dim3((unsigned)std::min<long>((I.nr + 255) / 256, 2048)), dim3(256), 0, sa, (const T*)sgc.rs + c0,
                                   (const T*)sgc.b + c0, sgc.npad, S, (const double*)cks[ci].rq, (const double*)Pt_v, ldpt, I.nr, p->kern.variance, vfe ? 1 : 0,
                                   (T*)segc[cks[ci].si][0] + c0, dYs ? dYs + c0 : (T*)nullptr, sgc.npad, (double*)g_v + 2 + nsc);
                HIPCHK(hipGetLastError());
            }
            if (ovl) {
                RC(ctx_event(c, &evV[bb], false));
                HIPCHK(hipEventRecord(evV[bb], sa));
            }
        }
        // (every GEMM is followed by its vgrad on the main stream, which waited for it: nothing to join)
        // ---- per observation: ∂/∂σ_i², ∂/∂y_i and the two N-long sums on the device; only what the caller asked for comes back
        long off = 0;
        for (size_t si = 0; si < p->segs.size(); ++si) {
            const ObsSeg& sg = *p->segs[si];
            if (sg.n == 0) continue;
            if (cols) {  // finished chunk by chunk above; dY: n_all × S column-major on the host
                if (dnoise) HIPCHK(hipMemcpyAsync((T*)dnoise + off, segc[si][0], sizeof(T) * (size_t)sg.n, hipMemcpyDeviceToHost, s));
                if (dy)
                    HIPCHK(hipMemcpy2DAsync((T*)dy + off, sizeof(T) * (size_t)n_all, segc[si][1], sizeof(T) * (size_t)sg.npad, sizeof(T) * (size_t)sg.n, (size_t)S,
                                            hipMemcpyDeviceToHost, s));
            } else {
            void *dn_v = 0, *dy_v = 0;
            RC(bufs.get(sizeof(T) * (size_t)sg.n, &dn_v));
            RC(bufs.get(sizeof(T) * (size_t)sg.n, &dy_v));
            hipLaunchKernelGGL(vgrad_finish_kernel<T>, dim3((unsigned)std::min<long>((sg.n + 255) / 256, 2048)), dim3(256), 0, s, (const T*)sg.rs, (const T*)sg.b,
                               (const double*)segb[si][0], (const double*)segb[si][1], sg.n, p->kern.variance, vfe ? 1 : 0, (T*)dn_v, (T*)dy_v, (double*)g_v + 2 + nsc);
            HIPCHK(hipGetLastError());
            if (dnoise) HIPCHK(hipMemcpyAsync((T*)dnoise + off, dn_v, sizeof(T) * (size_t)sg.n, hipMemcpyDeviceToHost, s));
            if (dy) HIPCHK(hipMemcpyAsync((T*)dy + off, dy_v, sizeof(T) * (size_t)sg.n, hipMemcpyDeviceToHost, s));
            }
            if (dx) {
                std::vector<double> gx_h((size_t)sg.npad * d);
                HIPCHK(hipMemcpyAsync(gx_h.data(), segb[si][2], sizeof(double) * (size_t)sg.npad * d, hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                for (int q = 0; q < d; ++q)
                    for (long i = 0; i < sg.n; ++i) gx_all[(size_t)q * n_all + off + i] = gx_h[(size_t)q * sg.npad + i];
            }
            off += sg.n;
        }
        HIPCHK(hipEventRecord(c->ev_phase[2], s));
        // ---- K_zz: explicit weights G_zz over the full square; z_j enters through both arguments (factor 2 on the column role)
        {
            dim3 grid((unsigned)(mp / 128), (unsigned)((m + 127) / 128));
            RC((launch_vgrad<double, false>(s, grid, (const double*)Gz, ld, 1, (const double*)p->zs, mp, (const double*)p->zs, mp, d, p->kern.kind, p->kern.variance, p->kern.nscale(),
                                            sc.ptr(), (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, m, m, (double*)g_v,
                                            (double*)gz_v, mp, 2.0, (double*)nullptr, (double*)nullptr, (double*)nullptr, 0L)));
        }
        HIPCHK(hipMemcpyAsync(g_h.data(), g_v, g_b, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(gz_h.data(), gz_v, gz_b, hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(c->ev_phase[3], s));
        HIPCHK(hipStreamSynchronize(s));
        return phase_timings(c);  // gp_timings: assemble_ms = the M×M side, potrf_ms = the streamed pass, solve_ms = the K_zz term
    });
    if (rc != 0) return rc;
    if (dvar) *dvar = g_h[0] - (vfe ? 0.5 * (double)S * g_h[3 + nsc] : 0.0);   // − ½ Σ_i ∂k_ii/∂σ_k² / σ_i²: the trace term (once per column)
    if (dscale)
        for (int q = 0; q < p->kern.nscale(); ++q) dscale[q] = g_h[2 + q];
    if (dnoise_sum) *dnoise_sum = g_h[2 + nsc];
    // the container layouts of the pseudo-inputs and the inputs (src/finite_gp_projection.jl:32-37): 0 vector, 1 ColVecs (D×M column-major), 2 RowVecs (M×D column-major)
    if (dz) grad_to_layout<double>(z_layout, m, d, gz_h.data(), mp, dz);
    if (dx) grad_to_layout<T>(x_layout, n_all, d, gx_all.data(), n_all, dx);
    return 0;
}
