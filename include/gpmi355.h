/* gpmi355.h — C ABI of libgpmi355.so: MI355X-native (gfx950) exact / sparse GP inference.
 *
 * This is the drop-in boundary for ONE hot path of AbstractGPs.jl (reference paths are relative
 * to the upstream repo): logpdf(fx, y)   src/finite_gp_projection.jl:306-311
 *                         posterior(fx,y) src/exact_gpr_posterior.jl:29-35
 * plus what callers do next (predictive mean/var/cov, src/exact_gpr_posterior.jl:60-90) and the
 * VFE/DTC sparse variant (src/sparse_approximations.jl:58-75, 183-217, 248-313).
 *
 * The reference has no FFI of its own (pure Julia); its documented plug-in point is "subtype
 * AbstractGP and implement the FiniteGP primary API" (docs/src/api.md:18-30, 49-73).  The Julia
 * shim that does that with `ccall` into these entry points is abstractgps.jl_amd/julia/HipGPs.jl;
 * a line-for-line Python ctypes mirror (abstractgps.jl_amd/api.py) is what the test-suite runs.
 *
 * Conventions
 *  - plain C, no C++/torch types; every function returns int32 status:
 *        0      success
 *        k > 0  LAPACK-style info: leading minor of order k is not positive definite
 *               (the shim throws LinearAlgebra.PosDefException(k) exactly like `cholesky` at
 *               src/finite_gp_projection.jl:308 / src/exact_gpr_posterior.jl:31)
 *        -i     (1 <= i < 1000) argument i invalid
 *        -1000-e HIP error e;  text in gp_last_error() (thread-local)
 *  - host pointers are borrowed for the duration of the call only; outputs are caller-allocated
 *    host buffers; device memory, streams and workspaces are owned by the handles.
 *  - dtype: 0 = f64, 1 = f32.  All host arrays of one call share the kernel's dtype
 *    (Float32 in -> Float32 out is a tested reference property, test/finite_gp_projection.jl:180-191).
 *  - matrices handed back to the host are COLUMN-MAJOR (Julia layout).
 *  - functions taking a gp_ctx are serialised per ctx by an internal mutex and may be called from
 *    any OS thread (hipSetDevice is issued on entry).
 */
#ifndef GPMI355_H
#define GPMI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPMI355_ABI_VERSION 4

typedef struct gp_ctx gp_ctx;   /* device + streams + workspace                          */
typedef struct gp_post gp_post; /* PosteriorGP state: device-resident factor, alpha, x   */
typedef struct gp_vfe gp_vfe;   /* ApproxPosteriorGP state (VFE / DTC)                    */

/* Kernel descriptor: variance * base(kind) ∘ transform.   Replaces KernelFunctions.kernelmatrix
 * at src/base_gp.jl:70,72,74.  kind: 0 SqExponential exp(-d²/2); 1 Matern12 exp(-d);
 * 2 Matern32 (1+√3d)exp(-√3d); 3 Matern52 (1+√5d+5d²/3)exp(-√5d).
 * nscale: 0 none; 1 ScaleTransform(scale[0]) (with_lengthscale(k,ℓ) ≡ scale = 1/ℓ); D ARDTransform(scale[0..D)). */
typedef struct {
    int32_t kind;
    int32_t dtype;
    double variance;
    int32_t nscale;
    const double* scale;
} gp_kernel;

/* Composite kernel: Σ_t σ_t² · Π_f κ_f — the normal form of any KernelSum / KernelProduct / ScaledKernel tree (products
 * distributed over sums, the ScaledKernel factors on a path multiplied into σ_t²).  A FACTOR is a base kernel behind its own
 * transform T_f (nscale / scale as in gp_kernel: none, ScaleTransform(s), ARDTransform(v)); u = T_f(x) − T_f(x'), d² = ‖u‖²:
 *   kind 0..3  as gp_kernel (SqExponential, Matern12, Matern32, Matern52)                            nparam 0
 *   kind 4     PeriodicKernel(; r), metric Sinus(r):  exp(−½ Σ_p (sinpi(u_p) / r_p)²),  r_p > 0        nparam D (param = r)
 *              (with_lengthscale(Per, p) = ScaleTransform(1/p) gives period p)
 *   kind 5     RationalQuadraticKernel(; α):  (1 + d²/(2α))^(−α) = exp(−α·log1p(d²/(2α))),  α > 0  nparam 1 (param = α)
 *   kind 6     WhiteKernel():  1 if x and x' are equal in every coordinate, else 0; takes no transform  nparam 0
 * Every κ_f(x, x) = 1, so the prior variance is Σ_t σ_t²; White adds to a cross-covariance wherever a test point equals a training
 * point exactly (as KernelFunctions does).
 * Limits: 1..8 terms, 1..4 factors per term, at most 16 factors in all, D <= 16, at most 64 entries in θ.  Outside them, or with a
 * malformed descriptor (variance <= 0, a param count or value that breaks the table, a transform on White), the *_sum calls return
 * −2 (the descriptor argument) with the reason in gp_last_error().
 * θ (the flat parameter vector of gp_logpdf_grad_sum): term by term σ_t², then for each of its factors scale[0..nscale) and then
 * param[0..nparam). */
typedef struct {
    int32_t kind;
    int32_t nscale;
    const double* scale;
    int32_t nparam;
    const double* param;
} gp_kfactor;
typedef struct {
    double variance;
    int32_t nfactors;
    const gp_kfactor* factors;
} gp_kterm;
typedef struct {
    int32_t dtype;
    int32_t nterms;
    const gp_kterm* terms;
} gp_ksum;

/* Inputs (host).  layout: 0 = Vector{T} (d must be 1); 1 = ColVecs(X), X is d×n column-major
 * (point-contiguous); 2 = RowVecs(X), X is n×d column-major (dimension-contiguous).
 * src/finite_gp_projection.jl:32-37. */
typedef struct {
    const void* data;
    int64_t n;
    int32_t d;
    int32_t layout;
} gp_points;

/* Observation noise Σy.  kind 0: σ²·I (Fill, src/finite_gp_projection.jl:19-21); kind 1: Diagonal(diag)
 * (length n, host, kernel dtype) (:13-15).
 * Dense Σy (any matrix, :2-11; cov(fx) = cov(f, x) + Σy, factored as cholesky(_symmetric(K + Σy)), :96, :308): `diag` points to an n×n COLUMN-MAJOR
 * contiguous host array (leading dimension n) of the kernel's dtype, n = the number of points of the call the noise belongs to (x->n, x2->n, xs->n); `s` is
 * ignored.
 *   kind 2: only the UPPER triangle (row <= column) is read — Symmetric(Σy) = :U, what _symmetric does (src/util/common_covmat_ops.jl:5);
 *   kind 3: only the LOWER triangle (row >= column) is read.  A C-ordered (row-major) array handed over as it lies is the column-major array of its
 *           transpose, so kind 3 is the zero-copy form of "the upper triangle of a row-major matrix".
 * Nothing outside the named triangle is read (it may hold anything).  The triangle is streamed host -> page-locked staging -> device staging -> the resident
 * K in pieces of at most "dense_stage_mb" MiB and added before the factorisation: no second N×N buffer on either side, 8·N(N+1)/2 bytes (fp64) over the bus
 * up to piece padding; the upload and the adds count into gp_timings.assemble_ms.  No atomics: "deterministic" = 1 covers dense fits.  The copy into the
 * page-locked buffer is the slowest stage (it runs on GPMI_DENSE_THREADS host threads, environment, 1..16, default 4): an upload costs 1.1-1.6 times a
 * plain hipMemcpy of the triangle (profiles/r8/).
 * Accepted by every exact-path call that takes a gp_noise (gp_logpdf, gp_logpdf_terms, gp_posterior_fit, gp_logpdf_grad, their *_sum forms,
 * gp_posterior_update, gp_posterior_logpdf, gp_posterior_rand) and by gp_vfe_logpdf / gp_vfe_rand (Σy* of the ns×ns joint).  gp_vfe_fit / gp_vfe_update
 * refuse kinds 2 / 3 (argument error, reason in gp_last_error()): the reference needs cholesky(Σy) there — an N×N factorisation that defeats the sparse
 * cost (src/sparse_approximations.jl:61, :97) — and its elbo has no method for a dense Σy (:307-313).
 * On a multi-device ctx a fit with a dense Σy runs on the single-device engine of the ctx's first device (like composite and fp32 fits): the 2-D
 * block-cyclic driver takes kinds 0 / 1 only; a sequential update with a dense Σy2 gathers the factor first. */
typedef struct {
    int32_t kind;
    double s;
    const void* diag;
} gp_noise;

/* Per-phase wall times (ms, HIP events on the ctx streams) of the last fit/logpdf call, and the
 * accumulated duration / algorithmic FLOPs of the dominant kernel (gemm_nt trailing update) when
 * parameter "time_kernels" is 1.  Exact fits: assemble = Gram phase, potrf = factorisation, solve = vector solves.
 * Sparse fits (gp_vfe_fit / _update / _append): assemble = the M×M prelude (K_zz, its Cholesky, inv(L_z)), potrf = the streamed pass
 * over the data points, solve = the M×M side after it (Λ_ε = chol(I + B Bᵀ), the vector solves). */
typedef struct {
    double assemble_ms;
    double potrf_ms;
    double solve_ms;
    double total_ms;
    double gemm_ms;        /* Σ per-launch durations of gemm_nt_sub launches (time_kernels=1)  */
    double gemm_flops;     /* Σ algorithmic flops of those launches                               */
    int64_t gemm_launches;
    double gemm_bytes;     /* Σ algorithmic bytes of those launches: C read + C write + both operand panels once */
} gp_timings;

/* ---- context ------------------------------------------------------------------------------ */
/* stream_or_null: a hipStream_t owned by the caller to issue the main-stream work on (e.g. the
 * current torch stream in the multi-process driver); NULL = the ctx creates its own. */
int32_t gp_ctx_create(gp_ctx** out, int32_t device, void* stream_or_null);
/* Multi-device context: ONE caller thread (the Julia process of docs/src/api.md:18-30) drives ndev devices of a node.
 * devices[r] is the HIP device of rank r = p·Q + q of the P×Q process grid over which gp_posterior_fit / gp_logpdf partition
 * K + Σy 2D block-cyclically in nb×nb blocks (one internal host thread per rank; panel traffic by RCCL grouped send/recv over
 * xGMI, or by peer copies — environment GPMI_COMM=rccl|p2p overrides the automatic choice).  P = Q = 0: grid chosen for the
 * fabric (P = ndev, Q = 1 on the full-mesh xGMI node, see multi.hip); nb = 0: 1024.  The same device may be listed several
 * times ("virtual ranks": the full schedule on one GPU with same-device copies — how CI exercises it).  Every other entry
 * point works unchanged on such a ctx: fp64 fits are distributed, everything else (and everything downstream of a fit:
 * predictions, updates, sampling — the factor is gathered onto devices[0] on first need) runs on devices[0].
 * fp32 fits, fits with more than 128 right-hand-side columns and fits with a dense Σy (gp_noise kind 2 / 3) also run on devices[0] (single-device engine).
 * Extra parameters: "lookahead_depth" (1..3, default 2), "dist_nb", "multi_gemm_streamk" (stream-K cuts inside the rank
 * contexts, default 0), "multi_timeout_s" (a rank that waits longer for a peer or for its own streams fails the fit instead
 * of hanging, default 600), "multi_check" (diagnostics: 1 marker/checker kernels around every event record / wait, 2 operand
 * buffers compared with the owners' blocks before every update, 4 NaN-poisoned operand buffers; findings fail the fit with
 * status -1990).  Environment: GPMI_COMM=rccl|p2p, GPMI_RCCL_LIB=<library to dlopen instead of librccl>, GPMI_COMM_PRIO=1
 * (high-priority comm stream), GPMI_TRACE_SCHEDULE=<file> (JSON-lines schedule trace of the last fit). */
int32_t gp_ctx_create_multi(gp_ctx** out, const int32_t* devices, int32_t ndev, int32_t P, int32_t Q, int32_t nb);
/* Grid / transport of a ctx (1×1, nb 0, comm 0 for a single-device ctx).  comm: 1 RCCL, 2 peer / same-device copies. */
int32_t gp_ctx_multi_info(gp_ctx* ctx, int32_t* P, int32_t* Q, int32_t* nb, int32_t* comm, int32_t* depth);
/* Multi-device fits check their result before handing it out ("multi_verify", default 1: δᵀα against ‖L⁻¹δ‖², and (K + Σy)α = δ on
 * every row with K·α recomputed from the inputs on the devices) and are repeated once when the check or the factorisation fails; a second failure is the
 * error (-1991, or the LAPACK info).  fits = fit attempts so far, retries = repetitions (0 on a healthy stack); any pointer may be NULL. */
int32_t gp_ctx_multi_stats(gp_ctx* ctx, int64_t* fits, int64_t* retries, int64_t* solves);
/* Predictive variances — and full covariances for up to 4 096 test points — of a multi-device posterior (gp_posterior_predict) are
 * computed on the distributed factor: a block forward solve with the factor left where the fit put it, N*×nb blocks of the solution
 * travelling, one SYRK per rank for the covariance — and with them gp_posterior_logpdf / gp_posterior_rand for up to 4 096 test points
 * ("multi_dist_predict", default 1; `solves` above counts the passes over the pieces).  On the pieces as well:
 *   gp_posterior_solve  (<= 128 columns): the columns travel as rows — forward pass, then one backward block sweep per column;
 *   gp_posterior_update (<= 4 096 new observations): the factor is EXTENDED where it lives — K(x2, x1) L11⁻ᵀ by the forward pass, every
 *                       rank keeping the rows of the new blocks it owns; chol(C22 − U12ᵀU12) on devices[0], its blocks sent to their
 *                       owners; α by a forward + backward pass over the extended pieces.  The new posterior is again a multi-device
 *                       posterior (each batch of observations ends in its own padded blocks).
 *   gp_posterior_factor_mul (<= 1 024 columns): every rank multiplies the blocks it holds with its share of ξ, the process rows'
 *                       partial products are summed on the host — no exchange between the ranks.
 * C.U (gp_posterior_get_factor), covariances of more than 4 096 test points and the variance side of gp_posterior_predict_grad gather the
 * factor onto devices[0] (real points only: the padding inside the blocks is dropped).
 * gp_multi_solve_trace / _ex write the schedule of such a pass for a P×Q grid (dry run of the real rank threads, like
 * gp_multi_schedule_trace); flags: 1 = given right-hand sides, 2 = rows kept for an extended factor (sequential update),
 * 4 = followed by two backward sweeps. */
int32_t gp_multi_solve_trace(int32_t P, int32_t Q, int32_t nblk, const char* path);
int32_t gp_multi_solve_trace_ex(int32_t P, int32_t Q, int32_t nblk, int32_t flags, const char* path);
/* The schedule the multi-device driver issues for a P×Q grid over nblk block columns (look-ahead depth 1..3; comm 1 =
 * send/recv transport, 2 = copies; + 16 = the schedule of "multi_trsm_inv" = 0, + 32 = that of "multi_chain_cus" > 0), written as JSON lines to `path`: every stream operation with its block footprint, every
 * event record / wait, every transfer — produced by the SAME rank-thread code that drives the devices, run without a device
 * (works on a machine without a GPU).  tools/multi_schedule_check.py checks happens-before on it. */
int32_t gp_multi_schedule_trace(int32_t P, int32_t Q, int32_t nblk, int32_t depth, int32_t comm, const char* path);
int32_t gp_ctx_destroy(gp_ctx* ctx);
/* Tuning / diagnostic parameters (all optional; the GPMI_PARAMS="name=value,..." environment variable applies the same
 * names at gp_ctx_create):
 *   "nb"             outer panel width: −1 = automatic ("nb_small" for matrices below "lookahead_min_n", "nb_large" from there on, "nb_huge" from "nb_huge_min_n" on), 0 = purely
 *                    recursive, > 0 = that width (multiple of 128) at every size                default −1
 *   "nb_small", "nb_large"  the automatic widths: below the look-ahead threshold the schedule is one stream and 4 096-column panels halve the
 *                    passes over the trailing matrix (C2 −2.5 %); above it 2 048 / 4 096 / 8 192 measure within ± 0.5 %   default 4096, 2048
 *   "nb_huge", "nb_huge_min_n"  third automatic tier: fits of padded order >= nb_huge_min_n take panels of nb_huge columns whatever the two widths above say.
 *                    The Strassen products of the bulk update then run at K/2 = nb_huge/2, and what a product costs beyond its flops does not grow with K: at
 *                    N = 65 536 4 096 measures 1.8 % faster than 2 048, 3 072 and 6 144 in between; at N = 32 768 4 096 and 2 048 measure the same and the other
 *                    two slower (profiles/r26/nb_sweep.txt), hence the floor between the two sizes; nb_huge_min_n = 0: no such tier   default 4096, 49152
 *   "lookahead"      next panel on a second, high-priority stream (0/1)                   default 1
 *   "lookahead_min_n" ... for matrices of at least this (padded) order                    default 24576
 *   "time_kernels"   bracket every MFMA GEMM launch with HIP events (gp_get_timings)      default 0
 *   "xcd_swizzle", "xcd_min_tiles"  XCD-aware super-tile workgroup order for large GEMM grids   default 0, 256
 *   "strassen_min_rows"  fp64 exact fits (and gpd_gemm_nt): smallest side of an off-diagonal block of the bulk trailing update that runs as seven
 *                    half-size products (one level of Strassen, ordered launches, no atomics: DESIGN.md §4); rounded up to 256; 0 = never   default 8192
 *   "strassen_min_rows_large"  the same threshold for fits whose padded order is at least "lookahead_min_n" (the two-stream schedule), used as long as
 *                    "strassen_min_rows" has not been set on the ctx: once the caller sets that one — to any value, its default included — it applies at
 *                    every size.  4 096 measures faster than 8 192 at N = 65 536 and 32 768 and slower at 16 384 (profiles/r18/strassen_sweep.txt)   default 4096
 *   "strassen_group", "strassen_group_min_rows"  a bulk update (or gpd_gemm_nt lower SYRK) of side >= strassen_group_min_rows that is split at all runs as
 *                    FOUR grouped launches over the tiles of all its pieces — launch i of every Strassen block and the classical pieces write disjoint
 *                    parts of C — instead of four launches per block and one per piece (csrc/bulk_plan.hpp, gemm_nt_grp_kernel: a device table of
 *                    problems per launch, no atomics, bitwise equal to the per-block sequence under "deterministic"); every block then has its own
 *                    sum panels.  0 / below the floor / with "xcd_swizzle": the per-block sequence.  The floor is rounded up to 256 and is at least 256   default 1, 8192
 *   "strassen_u1_min_rows", "strassen_u1_min_k"  fp64 exact fits: U1, the update of the next panel's columns, is one launch over a lower trapezoid.  With this set, the whole 256-row
 *                    quadrants of its rectangle below the panel's square run as ONE Strassen block when they are at least strassen_u1_min_rows rows (rounded up to 256), the
 *                    panel — the K of this update — has at least strassen_u1_min_k columns and
 *                    "strassen_min_rows" of the fit is not 0: the square, the remainder strip and the carried rows stay classical, and all of it runs as four
 *                    grouped launches after two sums launches (csrc/bulk_plan.hpp u1_plan_build); 0 = the single launch.  At N = 65 536 with 4 096-column
 *                    panels floors of 8 192 and 16 384 measure the same, 0.9 % faster than the single launch, 32 768 half of that (profiles/r26/u1_floor_sweep.txt); with 2 048-column panels the form is 0.9 % SLOWER at
 *                    N = 32 768 (profiles/r26/bench_c2_c3_ab.txt: halves of K/2 = 1 024), hence the floor on K   default 16384, 4096
 *   "gemm_streamk"   persistent-grid GEMM with a stream-K tail on launches of <= sk_max_tiles tiles   default 1
 *                    (0 in the rank contexts of a multi-device ctx: "multi_gemm_streamk").  The tail adds its k-slices into C with
 *                    hardware floating-point atomics, so the order of summation depends on scheduling: results agree with the
 *                    oracle at the stated tolerances but are NOT bitwise reproducible from run to run; 0 removes this source of
 *                    variation from the factorisation (hardware-dispatched GEMMs only, 1-5 % slower at N <= 32 768; the backward
 *                    vector sweep still adds four partial products per column with atomics)
 *   "deterministic"  1: the exact path (gp_logpdf, gp_logpdf_terms, gp_posterior_fit and every method of its posterior) uses no
 *                    floating-point atomics — no stream-K tails whatever "gemm_streamk" says, one thread per column in the backward
 *                    sweep — so two calls with the same inputs on the same ctx return the same BITS (tests/test_gpu_api.py; the leaf's one
 *                    Σ log L_ii add per launch is issued by a single thread and the leaves of a fit are totally ordered, so its order is fixed).  The bits
 *                    do not depend on the schedule either: the same fit on one stream and with the two-stream look-ahead, and with grouped and with
 *                    per-block Strassen updates, returns the same logpdf, α and factor (tests/test_gpu_schedule_matrix.py); another panel width or
 *                    another "strassen_min_rows" is another order of operations.  The VFE
 *                    path, the gradient kernels and the multi-device backward sweep keep their atomics.  1-5 % slower at N <= 32 768.   default 0
 *   "leaf_v2", "leaf_xr"  fp64 leaves by the register-resident panel64v2_kernel (csrc/leaf.hpp) / rows of X per leaf workgroup (0 auto)   default 1, 0
 *   "leaf_cols"      columns per register-resident leaf launch (64 or 128; 128 = one workgroup chain per 128 columns)   default 128
 *   "upd128", "updk_max_k"  in-panel updates C[m×N] −= P·P[0:N]ᵀ of the panel recursion by panel_updk_kernel (csrc/leaf.hpp: register chain, 16-row
 *                    wave tiles) instead of the tile GEMM: K = N = 128 (on/off) and 256 <= K = N <= updk_max_k; K above "updk_tall_k" only
 *                    while at most "updk_tall_m" rows are below                          default 1, 512, 256, 8192
 *   "updk_rt"        rows per workgroup / 16 of that kernel (0 auto: tallest tile giving one workgroup per CU; 4, 2, 1)   default 0
 *   "sk_min_k"       smallest inner dimension that may use the stream-K GEMM                default 0
 *   "leaf_group"     columns factored left-looking by consecutive fused leaves (64/128/256/512)   default 128
 *   "trsv_nb"        diagonal block of the vector solves handled by one workgroup (128..1024)    default 256
 *   "gemm_pad_lds"   extra dynamic LDS bytes per GEMM workgroup; 20480 = one workgroup per CU (fp64: same speed on one
 *                    large launch, 4-7 % slower over a whole factorisation)                 default 0
 *   "gemm_pad_f32"   the same for the fp32 GEMMs unless "gemm_pad_lds" was set (0: two workgroups per CU — 1 % faster at C5 with the
 *                    pipelined k loop; with "gemm_pipe" = 0 one workgroup per CU, 20480, was 5 % faster)   default 0
 *   "gemm_pipe"      k loop of the MFMA GEMMs software-pipelined across the step boundary (csrc/kernels.hpp gemm_kloop_pipe: the fragments of
 *                    the next half-step are in registers before the barrier, operand DMA issued between MFMAs); 0 = the round-2 loop   default 1
 *   "kmat_rows"      Gram tiles row by row (distance, κ, store; one kernel instance per dimension bucket D <= 4 / 8 / 16, few registers) instead of
 *                    all 64 squared distances of a thread accumulated first (the form D > 16 always takes); process-wide   default 1
 *   "dib_nb"         forward solves X L⁻ᵀ against a resident factor (predictive variances / covariances, held-out logpdf, sampling, sequential
 *                    conditioning, the gradient's L⁻ᵀ; both factors of a VFE / DTC prediction): column blocks of at most this width are solved by ONE triangular-k MFMA GEMM with the
 *                    explicit inverse of the diagonal block — built once per posterior handle (np × (dib_nb + 32) elements, 3 % of the factor at
 *                    N = 65 536) on its first forward solve; 0 = the recursion down to 64-column TRSM leaves.  A product with an explicit inverse
 *                    carries an error of order cond(L_bb)·ε where substitution is backward stable: a handle whose factor has max |L_ii| / min |L_ii|
 *                    above 1e5 (cond(K + Σy) >= 1e10) keeps the substitution leaves                   default 2048
 *                    What is NOT behind that guard (tests/test_gpu_backward_error.py measures both against componentwise rounding bounds): every Cholesky / TRSM leaf
 *                    multiplies the rows below a 16×16 diagonal block T by inv(T), so the factor satisfies |A − LLᵀ| <= γ_{n+1} |L||L|ᵀ + 2γ_16 |L_iJ Tᵀ||T⁻ᵀ||Tᵀ| and
 *                    not the first term alone — 68 times the first term when the factor's diagonal falls by 1e5 inside ONE 64-column tile (64 points of a smooth kernel at
 *                    σ² = 1e-10), 1.4 at N = 320, below it from N ≈ 1 000; and the vector solves multiply by inv of every 64×64 diagonal tile, which is backward stable in
 *                    the forward direction only: the backward sweep (α, gp_posterior_solve) carries γ_64·cond(T) of such a tile — 29 times substitution's bound at
 *                    128 points under the same conditions, 0.04 at 1 024.  α's residual |Cα − δ| reached 2.9 times Theorem 10.4's bound at 130 such points and stayed
 *                    below 0.02 of it in every other measured case.
 *                    (tests/test_illcond_cpu.py reproduces both excesses with a NumPy emulation of the two designs.)
 *   "ldpad"          row padding in elements (multiple of 16)                             default 32
 *   "dense_stage_mb" dense Σy (gp_noise kind 2 / 3): MiB per staging buffer of the streamed upload and of the gradient's download (two page-locked and two
 *                    device buffers of this size; 1..256; a piece is never shorter than 128 rows / columns of the matrix)   default 64
 *   "vfe_chunk"      data points per streamed VFE chunk (multiple of vfe_ks); 0 = automatic: 16 384 for M > 2 048 pseudo-points (measured best at C5),
 *                    × 2 … 16 for fewer (chunk × M kept at C5's footprint), at most the batch; a handle keeps the chunk of its first fit        default 0
 *   "vfe_ks"         fp32 VFE: data points per fp32 partial product of the chunk SYRK      default 2048
 *   "vfe_overlap"    VFE: kmat / reductions / partial-sum adds on a second stream beside the chunk GEMMs   default 1
 *   "vfe_dual"       VFE experiment switch: 1 = the triangular products of the chunks on a high-priority third stream beside the chunk SYRKs on the main stream
 *                    (needs "vfe_overlap").  Measured at C5 and left off: +0.4…0.7 ms (profiles/r6/c5_ab2.jsonl; both launches at equal priority: −0.45 ms)   default 0
 *   "vfe_inv_nb"     VFE prelude: inv(L_z) through inverse diagonal blocks of this width, built in one batched launch sequence, the levels above them one
 *                    triangular-k GEMM per block (≈ 40 launches at M = 4 096 instead of 127); 0 = the recursion down to 64-wide leaves   default 512
 *   "sk_max_tiles"   largest launch (in 128×128 tiles) that takes the persistent stream-K GEMM    default 4096
 *   "vfe_sk"         VFE: stream-K GEMM tails for the M×M side (K_zz / Λ_ε factorisations, inv(L_z))   default 0
 *   "copy_kernel"    multi-device: block copies by a kernel instead of hipMemcpy2DAsync            default 0
 *   "multi_leaf_cols"  multi-device: columns per register-resident leaf inside the rank contexts — 64 (46 KB of LDS: starts beside the bulk
 *                    update) rather than the single-device 128 (152 KB: waits for an empty CU, i.e. for the end of a GEMM launch)   default 64
 *   "multi_window"   multi-device: block steps a rank thread may queue ahead of its device         default 16
 *   "multi_trsm_inv" multi-device: the diagonal owner of block column k forms −inv(L_kk) (kept in a slot of its own) and THAT travels to the column's other
 *                    owners instead of L_kk; every owner then solves its rows below the block with ONE triangular-k MFMA GEMM + one copy instead of the
 *                    substitution recursion's nb/64 latency-bound leaf launches and as many few-tile GEMMs (nb = 1 024: 31 launches per rank and step -> 2).
 *                    Same conditioning rule as "dib_nb", decided from the inputs before the fit: every pivot of K + Σy lies in
 *                    [min Σy_ii, variance + max Σy_ii], and a fit with sqrt((variance + max Σy) / min Σy) > 1e5 keeps the substitution solve.  1: the owner forms the inverse
 *                    level by level (−inv and its transpose of every 64×64 tile, then 3 batched GEMMs per level: 13 launches at nb = 1 024; nb = 64·2^m), 2: by the
 *                    restricted-row recursion on the identity (33 launches; what 1 falls back to for other nb).   default 1
 *   "multi_chain_cus" multi-device: r > 0 reserves r CUs (r/8 of every XCD; multiple of 8, at most half the device) of every rank's GPU for the diagonal
 *                    block's chain (Cholesky of the nb×nb block + its inverse) on a CU-masked stream of its own; the panel and main streams' work then
 *                    runs on streams masked to the other CUs.  Measured on one GPU (profiles/r5/cumask_chain_probe.jsonl): a 1 024-column chain beside the bulk
 *                    update 3.6 ms unmasked -> 0.46 ms on 16 CUs, the update 4 % slower; masked HIP streams carry no priority, so the look-ahead update
 *                    loses its priority over the bulk update — the trade-off a multi-GPU run has to price (tools/scale_sweep.sh A/Bs it).   default 0
 *   "multi_debug_sync", "multi_inject_fault"  multi-device diagnostics: host synchronisation points of the rank threads (bit mask) /
 *                    hand the next fit's self-check a spoiled α once (tests/test_gpu_multi.py)      default 0, 0
 *   "pool_cap_mb"    device bytes (MiB) the ctx keeps cached for reuse after *_free; ONE block larger than the cap may stay cached (the 137 GB factor
 *                    of N = 131 072: 17.2 s per pair when it is returned to the driver and allocated again every fit, 11.0 s cached) — it takes the
 *                    place of everything else in the cache and is the last block to go; 0 caches nothing; gp_ctx_trim empties the cache; an
 *                    allocation that fails drops the cache and retries.   default 98304
 *   "alloc_poison"   diagnostic: 1 = every device block the ctx hands out (recycled or fresh, over its true size) and the ctx's scalar / inverse-tile
 *                    workspaces when they are created or grown are filled with 0xFF bytes first — NaN read as fp64 or fp32, −1 as int32 — by a memset
 *                    on the main stream that is waited for.  No entry point may return anything that depends on what a block held before it wrote it
 *                    (tests/test_gpu_poisoned_blocks.py); forwarded to the rank contexts of a multi-device ctx; one not-taken branch per allocation when 0.   default 0
 *   "pool_cached_mb", "pool_blocks"   read-only (gp_ctx_get_param): MiB and number of blocks in the cache now
 *   "batch_grad_kernel_problems"      read-only (gp_ctx_get_param): the problems the gradient kernels of gp_logpdf_grad_batch / _sum have served on this ctx
 *                    since it was created (the problems routed to the single path do not count): which path ran, for tests and measurements
 *   "batch_gradx_kernel_problems"     read-only: the same for the input-gradient kernels of gp_logpdf_grad_batch_x / _sum_x (problems whose dx they computed)
 *   "batch_joint_kernel_problems"     read-only: the same for the kernels of gp_joint_batch / _sum
 *   "batch_loo_kernel_problems", "batch_loo_grad_kernel_problems"   read-only: the same for the kernels of gp_loo_batch / _sum and of gp_loo_grad_batch / _sum
 *   "cols_kernel_calls", "cols_kernel_splits"   read-only: kmul launches gp_posterior_predict_cols has served on this ctx since it was created, and the workgroups
 *                    along the training range of the last of them (1 = unsplit, 0 = none yet): which path ran, for tests and measurements */
/* The defaults above, machine-readable (single-device parameters; gp_ctx_get_param reads the same names): the test-suite asserts before
 * every GPU test that the shared default context still has exactly these values, so that no test can leave a non-production setting
 * behind for the tests that follow it (tests/conftest.py). */
#define GPMI355_PARAM_DEFAULTS                                                                                                   \
    "nb=-1,nb_small=4096,nb_large=2048,nb_huge=4096,nb_huge_min_n=49152,strassen_u1_min_rows=16384,strassen_u1_min_k=4096,lookahead=1,lookahead_min_n=24576,time_kernels=0,xcd_swizzle=0,xcd_min_tiles=256,gemm_streamk=1,sk_max_tiles=4096," \
    "sk_min_k=0,gemm_pipe=1,gemm_pad_f32=0,gemm_pad_lds=0,trsv_nb=256,deterministic=0,leaf_v2=1,leaf_xr=0,leaf_cols=128,"    \
    "updk_max_k=512,updk_rt=0,updk_tall_k=256,updk_tall_m=8192,upd128=1,leaf_group=128,ldpad=32,vfe_ks=2048,vfe_sk=0,"          \
    "vfe_overlap=1,vfe_dual=0,vfe_inv_nb=512,vfe_chunk=0,kmat_rows=1,dib_nb=2048,pool_cap_mb=98304,dense_stage_mb=64,alloc_poison=0,strassen_min_rows=8192,strassen_min_rows_large=4096,strassen_group=1,strassen_group_min_rows=8192"
int32_t gp_ctx_set_param(gp_ctx* ctx, const char* name, int64_t value);
/* Read a parameter back (same names; "gemm_pad_lds" reads 0 until it has been set explicitly).  Used by the test-suite to assert that
 * every GPU test starts from the documented defaults. */
int32_t gp_ctx_get_param(gp_ctx* ctx, const char* name, int64_t* value_out);
/* Return every cached (free) device block of the ctx to the HIP allocator — e.g. after freeing an N = 65 536 posterior
 * (34 GB) when another allocator in the process needs the memory. */
int32_t gp_ctx_trim(gp_ctx* ctx);
int32_t gp_get_timings(gp_ctx* ctx, gp_timings* out);
const char* gp_last_error(void);
int32_t gp_abi_version(void);

/* ---- kernelmatrix (parity / small N) ------------------------------------------------------- */
/* out (host, column-major): n×n for y == NULL (exactly symmetric), else x.n × y.n.
 * KernelFunctions.kernelmatrix(k, x[, y]) — src/base_gp.jl:70,74. */
int32_t gp_kernelmatrix(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_points* y_or_null,
                        void* out);

/* ---- exact GP: logpdf / posterior --------------------------------------------------------- */
/* logpdf(f(x, Σy), Y): Y is n×ncols column-major with leading dimension ldy; out has ncols entries.
 * mean_or_null: prior mean vector m (length n) evaluated on the host, NULL = ZeroMean.
 * src/finite_gp_projection.jl:306-311, 325-326. */
int32_t gp_logpdf(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_noise* noise,
                  const void* mean_or_null, const void* Y, int64_t ldy, int32_t ncols, void* out);

/* The two terms of logpdf separately — sqmahal(fx, Y) (src/finite_gp_projection.jl:313-326: ‖U⁻ᵀ(y_s − m)‖² per column) and
 * logdet(cov(fx)) (:310) — from ONE factorisation.  Y may be NULL (logdet only; sqmahal_out must then be NULL too).
 * logdet_out: 1 entry, sqmahal_out: ncols entries, kernel dtype; either may be NULL.  (gradlogpdf(fx, y), :328-337, is −α of
 * gp_posterior_fit.) */
int32_t gp_logpdf_terms(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null,
                        const void* Y_or_null, int64_t ldy, int32_t ncols, void* logdet_out_or_null, void* sqmahal_out_or_null);

/* posterior(f(x, Σy), y): ONE Gram assembly + ONE factorisation serve both results.
 * alpha_out_or_null: length n (α = C \ (y - m));  logpdf_out_or_null: 1 entry (= logpdf(fx, y)).
 * The factor stays on the device inside *out.  src/exact_gpr_posterior.jl:29-35. */
int32_t gp_posterior_fit(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_noise* noise,
                         const void* mean_or_null, const void* y, gp_post** out, void* alpha_out_or_null,
                         void* logpdf_out_or_null);

/* Predictive quantities at xs (src/exact_gpr_posterior.jl:60-90).  what: bit0 mean, bit1 var,
 * bit2 full cov (ns×ns column-major).  prior_mean_xs_or_null: m(x*) evaluated on the host.
 * mean = m(x*) + K_*x α;  var = k** - colsumsq(U⁻ᵀ K_x*);  cov = K** - VᵀV. */
int32_t gp_posterior_predict(gp_post* post, const gp_points* xs, const void* prior_mean_xs_or_null,
                             int32_t what, void* mean_out, void* var_out, void* cov_out);
/* Predictive mean / variance AND their gradients w.r.t. the test inputs: what an AD backend computes when a caller differentiates
 * mean(f_post, x*) / var(f_post, x*) (src/exact_gpr_posterior.jl:60-90) — acquisition functions, the test-time half of a deep kernel, input
 * uncertainty.  For every test point j independently, with k_j = K(X, x*_j), alpha and the factor L of C resident:
 *     dmean[j, p] =      sum_i alpha_i dk(x*_j, x_i)/dx*_jp
 *     dvar[j, p]  = -2 * sum_i w_ji    dk(x*_j, x_i)/dx*_jp,     w_j = C^-1 k_j = L^-T (L^-1 k_j)
 * k(x*, x*) is constant (every kappa(x, x) = 1), and the prior mean counts as constant in x* (as dx_out of gp_logpdf_grad does): a caller whose mean
 * function depends on x adds its derivative to dmean.  Matern12 at distance 0 contributes 0; a White factor contributes 0.
 * what: bit 0 the mean side, bit 1 the variance side (0 or any other bit: argument error).  A side that is asked for writes its value (mean_out / var_out,
 * ns entries) and / or its gradient (dmean_out / dvar_out: ns * d entries in the container layout of xs, in the handle's dtype) — each pointer may be
 * NULL, not both of a side.  Values and gradients come from ONE pass: mean side alone needs no Gram matrix and no solve; the variance side runs, per
 * 4 096 test points, Gram -> forward solve (the variance, as gp_posterior_predict) -> backward solve X <- X L^-1 in place -> one fused kernel that
 * contracts the weights with dk/dx* (fp64 sums, one writer per output, no atomics: the gradient kernel is bitwise reproducible at any setting).
 * The backward solve uses the inverse diagonal blocks of the forward solve ("dib_nb").  A handle without them ("dib_nb" = 0, fewer than "dib_nb" padded
 * points, or a factor whose diagonal ratio trips the conditioning guard) takes the vector back-substitution once per test point: SERIAL in the number
 * of test points.
 * Multi-device ctx: the variance side gathers the factor onto devices[0] and runs the single-device path (like covariances of more than 4 096 points).
 * Cost against gp_posterior_predict(what = 3) on the same handle: a second triangular solve of the same flops plus bandwidth passes, a ratio near 2 by
 * design ON THE BLOCKED PATH.  Measured (tools/predict_grad_profile.py, 4 096 test points, profiles/r17/predict_grad_profile.json): 2.07 at N = 16 384
 * (17.9 -> 37.0 ms; GEMM event times 17.3 ms forward, 17.6 ms backward), 2.06 at N = 65 536 (256 -> 528 ms); gp_vfe_predict_grad 2.10 at M = 4 096
 * (3.2 -> 6.6 ms).  These figures do NOT hold for the back-substitution path — which every handle below "dib_nb" (2 048) padded points takes on a default
 * ctx, and any call whose scratch cannot be allocated: measured at N = 1 920, 4 096 test points 1.3 -> 282 ms (a ratio of 212, 69 us per test point);
 * a caller with many test points on a small handle lowers "dib_nb" (128 at least) on its ctx to get the blocked path. */
int32_t gp_posterior_predict_grad(gp_post* post, const gp_points* xs, const void* prior_mean_xs_or_null, int32_t what,
                                  void* mean_out_or_null, void* var_out_or_null, void* dmean_out_or_null, void* dvar_out_or_null);
/* logpdf(post(x*, Σy*), Y*) on the device: the FiniteGP-over-PosteriorGP path of the reference — mean_and_cov
 * (src/exact_gpr_posterior.jl:78-83) + Σy* (src/finite_gp_projection.jl:133-136), cholesky (:308), logdet + _sqmahal
 * (:310, :325-326).  Y: ns × ncols column-major, leading dimension ldy; out: ncols entries.  The N*×N* predictive
 * covariance is built and factored in HBM against the resident N×N factor; nothing is refitted. */
int32_t gp_posterior_logpdf(gp_post* post, const gp_points* xs, const void* prior_mean_xs_or_null, const gp_noise* noise,
                            const void* Y, int64_t ldy, int32_t ncols, void* out);
/* rand(rng, post(x*, Σy*), ncols) with the standard normals supplied by the caller (src/finite_gp_projection.jl:233-237):
 * out[:, s] = m* + chol(C*).U' xi[:, s]; xi and out are ns × ncols column-major (leading dimension ns). */
int32_t gp_posterior_rand(gp_post* post, const gp_points* xs, const void* prior_mean_xs_or_null, const gp_noise* noise,
                          const void* xi, int32_t ncols, void* out);

/* Value and gradient of logpdf(f(x, Σy), y) — the pullback a ChainRules rrule for the accelerated logpdf needs (the
 * reference differentiates logpdf by AD: test/finite_gp_projection.jl:152-178 and the examples).  One factorisation, then
 * C⁻¹ = L⁻ᵀL⁻¹ (blocked TRSM on the identity + MFMA SYRK) and one fused pass over the lower triangle:
 *   ∂/∂θ = ½ Σ_ij (α_i α_j − C⁻¹_ij) ∂C_ij/∂θ.
 * Outputs (all optional except logpdf_out; kernel dtype unless noted):
 *   dvariance_out  double[1]        ∂/∂(kernel variance)
 *   dscale_out     double[nscale]   ∂/∂scale (ScaleTransform s, or ARDTransform v_p; any D: 16 dimensions per pass)
 *   dnoise_out     noise.kind 0: 1 entry ∂/∂σ² = ½(αᵀα − tr C⁻¹);  kind 1: n entries ½(α_i² − C⁻¹_ii)
 *                  kind 2 / 3 (dense Σy): n×n entries, column-major, the FULL symmetric matrix G = ½(α αᵀ − C⁻¹) — the gradient in the sense
 *                  d logpdf = ⟨G, dΣy⟩ = Σ_ij G_ij dΣy_ij for SYMMETRIC dΣy, so a parametric Σy(φ) chains as ∂logpdf/∂φ = ⟨G, ∂Σy/∂φ⟩.  It is NOT what AD
 *                  through Symmetric(Σy, :U) returns entry by entry (that puts 2·G_ij on the named off-diagonal entries and 0 on the others).  Streamed to
 *                  the host in row blocks ("dense_stage_mb"); skipped when dnoise_out is NULL.
 *   dy_out         n entries ∂/∂y = −α   (∂/∂m = +α for a mean vector m)
 *   dx_out         n×d entries ∂/∂x in the container layout of x (what a deep-kernel model back-propagates into its feature
 *                  map, examples/2-deep-kernel-learning/script.jl); the prior mean is taken as constant in x */
int32_t gp_logpdf_grad(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null,
                       const void* y, void* logpdf_out, double* dvariance_out, double* dscale_out, void* dnoise_out,
                       void* dy_out, void* dx_out);

/* ---- exact GP with a composite kernel (gp_ksum above) ------------------------------------------------------------------ */
/* The same contracts as gp_kernelmatrix / gp_logpdf / gp_posterior_fit / gp_logpdf_grad with a gp_ksum in place of the gp_kernel.
 * Assembly, the predictive mean and the gradient pass evaluate the composite kernel on the device (kmat_sum_kernel, kvec_sum_kernel,
 * kgrad_sum_kernel); everything after the Gram matrix is the single-kind path.  A handle from gp_posterior_fit_sum keeps its composite
 * kernel: every gp_posterior_* entry point works on it unchanged.  The assembly and mean kernels use no floating-point atomics, so
 * "deterministic" = 1 covers composite fits as well.  On a multi-device ctx these calls run on the single-device engine of the ctx's
 * first device (the 2-D block-cyclic driver is single-kind).
 * gp_logpdf_grad_sum: dtheta_out (fp64, one entry per θ entry in the order documented at gp_ksum) = ∂logpdf/∂θ; dnoise_out and dy_out
 * as in gp_logpdf_grad.  gp_logpdf_grad_sum_x is the same call with gp_logpdf_grad's dx_out behind it (n×d entries ∂/∂x in the container
 * layout of x, kernel dtype, the prior mean taken as constant in x; kgradx_sum_kernel: one more pass over the full square of C⁻¹); with
 * dx_out NULL it does exactly what gp_logpdf_grad_sum does.  A Matern12 factor's derivative at coincident inputs is taken as 0.
 * gp_logpdf_terms_sum: the contract of gp_logpdf_terms for a composite kernel.  VFE / DTC stay single-kind. */
int32_t gp_kernelmatrix_sum(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_points* y_or_null, void* out);
int32_t gp_logpdf_sum(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null,
                      const void* Y, int64_t ldy, int32_t ncols, void* out);
int32_t gp_posterior_fit_sum(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null,
                             const void* y, gp_post** out, void* alpha_out_or_null, void* logpdf_out_or_null);
int32_t gp_logpdf_grad_sum(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null,
                           const void* y, void* logpdf_out, double* dtheta_out_or_null, void* dnoise_out_or_null,
                           void* dy_out_or_null);
int32_t gp_logpdf_grad_sum_x(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null,
                             const void* y, void* logpdf_out, double* dtheta_out_or_null, void* dnoise_out_or_null,
                             void* dy_out_or_null, void* dx_out_or_null);
int32_t gp_logpdf_terms_sum(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null,
                            const void* Y_or_null, int64_t ldy, int32_t ncols, void* logdet_out_or_null, void* sqmahal_out_or_null);

/* ---- one factorisation for a matrix of observations ("columns") ------------------------------------------------------------------ */
/* S = ncols independent GPs that share x, kernel, Σy and the prior-mean vector and differ in y — the columns of Y (n×ncols column-major, leading
 * dimension ldy), as logpdf(fx, Y::AbstractMatrix) takes them (src/finite_gp_projection.jl:313-326): emulators with many PCA outputs, multi-objective
 * surrogates, many series on one grid.  ONE Gram assembly and ONE factorisation serve all columns: the right-hand sides ride below the factor as
 * gp_logpdf's do, at no extra cost up to GPMI355_COLS_MAX = 128 columns (one block of right-hand-side rows); more columns are an argument error
 * (argument 8) — the caller groups them.
 * gp_posterior_fit_cols / _sum: posterior(fx, Y[:, s]) for every s (src/exact_gpr_posterior.jl:29-35).  alpha_out_or_null: n×ncols column-major, leading
 *   dimension n (α_s = C \ (Y[:, s] − m));  logpdf_out_or_null: ncols entries.  A failed factorisation returns the LAPACK info and no handle.
 *   Column 0 goes through the code of gp_posterior_fit; with ncols = 1 the call IS gp_posterior_fit.
 *   On a multi-device ctx a fit with ncols > 1 runs on the single-device engine of the ctx's first device (like composite fits).
 * gp_posterior_ncols: the columns of a handle — 1 for every handle made by the other calls.
 * gp_posterior_predict_cols: gp_posterior_predict for every column (src/exact_gpr_posterior.jl:60-90).  mean_out: ns×ncols column-major, column s =
 *   m(x*) + K_*x α_s, prior_mean_xs_or_null (ns entries) shared by the columns; var_out (ns) and cov_out (ns×ns) do not depend on y and are what
 *   gp_posterior_predict returns.  The means come from ONE launch of kmul_kernel / kmul_sum_kernel (csrc/kernels.hpp): K_*x is evaluated once for all
 *   columns and never stored, the products run on the 16×16×4 MFMA (fp64 and fp32 alike), the training range is split over workgroups when the test
 *   points are few and the partial sums are added in a fixed order: no floating-point atomics, bitwise repeatable, a column's bits independent of what
 *   the other columns hold, at any "deterministic" setting.  Single-kind kernels with D > 16 take one kvec launch per column instead.  On a one-column
 *   handle the call works and equals gp_posterior_predict.
 *   Read-only ctx parameters (gp_ctx_get_param): "cols_kernel_calls" = kmul launches served since the ctx was created (the per-column kvec launches of
 *   D > 16 do not count), "cols_kernel_splits" = workgroups along the training range of the last such launch (1 = unsplit; the rule: about 512
 *   workgroups, at least 128 training points each — the smallest n that splits is 225).
 * A handle with ncols > 1 serves unchanged everything that does not use α: gp_posterior_predict with what ⊆ {var, cov}, the variance side of
 *   gp_posterior_predict_grad, gp_posterior_solve, gp_posterior_factor_mul, gp_posterior_get_factor, gp_posterior_logdet, gp_posterior_n, gp_posterior_free.
 *   The mean bit of gp_posterior_predict, the mean side of gp_posterior_predict_grad, gp_posterior_logpdf, gp_posterior_rand and gp_posterior_update
 *   return −1 (the handle argument) with the reason in gp_last_error() and write nothing.
 * gp_logpdf_grad_cols / _sum: logpdf_out[s] = logpdf(fx, Y[:, s]) (ncols entries) and the gradient of Σ_s logpdf(fx, Y[:, s]), outputs as gp_logpdf_grad /
 *   gp_logpdf_grad_sum / gp_logpdf_grad_sum_x (every noise kind; dx_out may be NULL) except dY_out: n×ncols column-major, column s = −α_s.  One
 *   factorisation and one C⁻¹: ∂/∂θ = ½ Σ_ij (Σ_s α_is α_js − S·C⁻¹_ij) ∂C_ij/∂θ — cols_weight_kernel folds the sum over the columns into the −C⁻¹
 *   buffer, then the gradient kernels of gp_logpdf_grad run once.  With ncols = 1 the call IS gp_logpdf_grad. */
#define GPMI355_COLS_MAX 128
int32_t gp_posterior_fit_cols(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null, const void* Y,
                              int64_t ldy, int32_t ncols, gp_post** out, void* alpha_out_or_null, void* logpdf_out_or_null);
int32_t gp_posterior_fit_cols_sum(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null, const void* Y,
                                  int64_t ldy, int32_t ncols, gp_post** out, void* alpha_out_or_null, void* logpdf_out_or_null);
int32_t gp_posterior_ncols(gp_post* post, int32_t* out);
int32_t gp_posterior_predict_cols(gp_post* post, const gp_points* xs, const void* prior_mean_xs_or_null, int32_t what, void* mean_out, void* var_out,
                                  void* cov_out);
int32_t gp_logpdf_grad_cols(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null, const void* Y,
                            int64_t ldy, int32_t ncols, void* logpdf_out, double* dvariance_out, double* dscale_out, void* dnoise_out, void* dY_out,
                            void* dx_out);
int32_t gp_logpdf_grad_cols_sum(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null, const void* Y,
                                int64_t ldy, int32_t ncols, void* logpdf_out, double* dtheta_out_or_null, void* dnoise_out_or_null, void* dY_out_or_null,
                                void* dx_out_or_null);

/* ---- leave-one-out cross-validation ---------------------------------------------------------------------------------------------- */
/* How well f(x, Σy) predicts each observation from all the others (Rasmussen & Williams, GPML §5.4.2) without n refits.  With C = K + Σy,
 * α = C⁻¹(y − m) and c_i = [C⁻¹]_ii:
 *   mean_out[i] = μ_i = y_i − α_i / c_i          the predictive mean of y_i given y_−i
 *   var_out[i]  = v_i = 1 / c_i                  its predictive variance, the noise of observation i included
 *   lp_out[i]   = ℓ_i = −½ log 2π + ½ log c_i − ½ α_i² / c_i = log p(y_i | y_−i)
 *   value_out[0] = L = Σ_i ℓ_i                   the LOO log predictive density (a diagnostic, and a training objective: gp_loo_grad)
 * for any noise kind, a dense Σy included; n = 1 gives the prior prediction.  All outputs in the kernel's dtype, n entries each, any of the three
 * arrays may be NULL.
 * gp_loo / gp_loo_sum: one factorisation, W = L⁻ᵀ (the triangular inversion gp_logpdf_grad starts with), c_i = Σ_{k ≥ i} W_ik² and the terms by two
 *   bandwidth-bound kernels (fp64 sums in a fixed order, no floating-point atomics: "deterministic" = 1 covers the call).  No product with C⁻¹:
 *   2n³/3 flops, twice gp_logpdf's.
 * gp_loo_grad / gp_loo_grad_sum: value_out = L and its gradient, outputs as gp_logpdf_grad / gp_logpdf_grad_sum_x (all optional except value_out).
 *   dL = ⟨G, dC⟩ with a_i = ½(1/c_i + α_i²/c_i²), b_i = α_i/c_i, β = C⁻¹b and
 *     G = −C⁻¹ diag(a) C⁻¹ + ½(β αᵀ + α βᵀ):
 *   ∂/∂θ = Σ_ij G_ij ∂K_ij/∂θ;  dnoise_out: kind 0 tr G, kind 1 G_ii, kind 2 / 3 the full symmetric G (n×n, the convention of gp_logpdf_grad);
 *   dy_out = −β (∂/∂m = +β);  dx_out through ∂K/∂x with the same weights.  On the device 2G = −Z Zᵀ + β αᵀ + α βᵀ with Z = C⁻¹ diag(√(2a)) takes the
 *   place of −C⁻¹ in gp_logpdf_grad's buffers (one more n³ product on the MFMA GEMM and two bandwidth-bound passes: loo_mirror_scale_kernel,
 *   loo_fold_kernel), then gp_logpdf_grad's gradient kernels run as they are: 2n³ flops, twice gp_logpdf_grad's, and no more device memory.
 * Argument numbers and status codes as gp_logpdf_grad (a failed factorisation returns the LAPACK info and writes nothing).  On a multi-device ctx
 * the calls run on the single-device engine of the ctx's first device, as gp_logpdf_grad does. */
int32_t gp_loo(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null, const void* y, void* value_out,
               void* lp_out_or_null, void* mean_out_or_null, void* var_out_or_null);
int32_t gp_loo_sum(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null, const void* y, void* value_out,
                   void* lp_out_or_null, void* mean_out_or_null, void* var_out_or_null);
int32_t gp_loo_grad(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null, const void* y,
                    void* value_out, double* dvariance_out, double* dscale_out, void* dnoise_out, void* dy_out, void* dx_out);
int32_t gp_loo_grad_sum(gp_ctx* ctx, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean_or_null, const void* y,
                        void* value_out, double* dtheta_out_or_null, void* dnoise_out_or_null, void* dy_out_or_null, void* dx_out_or_null);

/* ---- many small exact GPs in one call ------------------------------------------------------------------------------------------ */
/* nb independent problems (k_b, x_b, Σy_b, m_b, y_b), each with its own size n_b: logpdf_out[b] = logpdf(f_b(x_b, Σy_b), y_b)
 * (src/finite_gp_projection.jl:306-311, once per problem — what a sampler over hyper-parameters, a multi-start optimiser, a grid search or a
 * set of cross-validation folds evaluates again and again) and, where alpha_out_or_null[b] is not NULL, α_b = C_b \ (y_b − m_b)
 * (src/exact_gpr_posterior.jl:29-35; n_b entries).  Value and weights only: no gradient, no posterior handle.
 *   k, noise, logpdf_out, info_out: arrays of nb;  x: nx entries, y: ny pointers (n_b entries each), nx, ny ∈ {1, nb} — 1 = every problem shares
 *   that x (resp. y; the problems then have one size), which is uploaded once;  mean_or_null, alpha_out_or_null: NULL, or nb pointers each of
 *   which may be NULL (ZeroMean / α not wanted).  One dtype per call (that of k[0]; a descriptor that differs is an argument error).
 * A failing problem is data, not a status: info_out[b] = 0, or the order of the first leading minor that is not positive definite (what
 * gp_logpdf returns for the same problem) with logpdf_out[b] = NaN and α_b filled with NaN — the other problems are not affected.  The return
 * value reports argument errors only (−i, reason in gp_last_error(); nb = 0 returns 0 and touches nothing).
 * fp64 problems with noise kind 0 / 1, n_b <= GPMI355_BATCH_MAX_N and D <= 16 are served by the batch kernel (csrc/batch.hip): one workgroup
 * per problem, inputs of a launch in ONE packed host -> device copy, results in one copy back, a bounded workspace from the ctx's block cache
 * (a larger batch runs in waves).  No floating-point atomics and a fixed schedule per problem: its result is the same bits whatever batch it
 * rides in.  Every other problem (fp32, a dense Σy, a larger n_b or D) is answered inside the same call by the single path; which path serves a
 * problem depends on that problem alone.  On a multi-device ctx the batch kernel runs on the first device.
 * GPMI355_BATCH_MAX_N: the largest multiple of 128 of the measured sweep (tools/batch_profile.py, profiles/r9/batch_profile.json: n = 64 … 2 048 ×
 * nb = 1, 8, 64, 512) for which one batch call beat the loop of gp_logpdf calls in every cell with nb >= 8.  The nb = 8 cells decide it: 768 points
 * 3.06 ms against 3.64 ms, 896 points 4.39 ms against 3.68 ms — one workgroup per problem stops paying where eight of them leave most of the chip idle
 * for longer than eight whole-chip fits take.  (The environment variable GPMI_BATCH_MAX_N, 0 … 2 048 = what the kernel admits, read per call, overrides
 * it for measurements.) */
#define GPMI355_BATCH_MAX_N 768
int32_t gp_logpdf_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                        const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                        void* const* alpha_out_or_null);
/* The same with one composite kernel (gp_ksum) per problem. */
int32_t gp_logpdf_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                            const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                            void* const* alpha_out_or_null);

/* The predictive half of the batch call: the same nb problems, each with its own test points, answered by ONE call — what a set of cross-validation
 * folds, a grid, a multi-start optimiser or independent outputs sharing one x want next (gp_posterior_fit + gp_posterior_predict + gp_posterior_free
 * per problem otherwise).  Per problem the semantics are those of gp_posterior_fit followed by gp_posterior_predict (src/exact_gpr_posterior.jl:29-35,
 * 60-70):  mean = m(x*) + K_*x α;  var = k(x*, x*) − colsumsq(L⁻¹ K_x*), not clamped.
 *   The arguments up to y are those of gp_logpdf_batch.  xs: nxs entries, nxs ∈ {1, nb} — 1 = ONE set of test points shared by every problem (uploaded
 *   once); problem b has ns_b = xs_b.n >= 0 test points of the D of its x (ns_b = 0 is legal: nothing of that problem's xs or outputs is touched).
 *   prior_mean_xs_or_null: NULL, or nb pointers each NULL or m(x*_b) evaluated on the host (ns_b entries).  what: bit 0 the mean, bit 1 the variance, as
 *   in gp_posterior_predict (0 or any other bit: argument error).  mean_out / var_out: nb pointers to ns_b entries each, in the call's dtype; the array
 *   of a side that is asked for must not be NULL (nor its entries where ns_b > 0), the other one is not read.  logpdf_out_or_null: nb entries
 *   (logpdf(f_b(x_b, Σy_b), y_b), from the same factorisation) or NULL;  info_out: nb entries.
 * Failure is data, as in gp_logpdf_batch: info_out[b] is the order of the first leading minor that is not positive, that problem's logpdf, mean and var
 * are NaN, the other problems are not affected.  The return value reports argument errors only (−i, reason in gp_last_error(); nb = 0 returns 0 and
 * touches nothing).
 * Problems the batch kernel takes (fp64, noise kind 0 / 1, n_b <= GPMI355_BATCH_MAX_N, D <= 16 — the routing of gp_logpdf_batch, decided by the problem
 * alone) run as two kernels per wave: batch_logpdf_kernel, then batch_predict_kernel on the slices it left (csrc/batch.hip) — one workgroup per tile of
 * 128 test points of one problem (cross-Gram rows and the mean in one pass, a left-looking forward solve against the read-only factor, the variance), so
 * a problem with many test points spreads over many workgroups.  One packed copy in, one copy back; the workspace (slices plus one strip per predict
 * workgroup) stays within the budget of a wave, and a wave with more tiles than one launch takes runs several predict launches against the same slices.
 * No floating-point atomics, no waits between workgroups; every test point's arithmetic touches no other row, so its mean and variance are the same bits
 * alone, among other test points, and in any batch.  Every other problem is answered inside the same call by gp_posterior_fit(_sum) +
 * gp_posterior_predict + gp_posterior_free.  Measured against that loop: tools/batch_predict_profile.py, DESIGN.md §4. */
int32_t gp_predict_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                         const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                         const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out, void* const* var_out,
                         void* logpdf_out_or_null, int32_t* info_out);
/* The same with one composite kernel (gp_ksum) per problem: k** = Σ_t σ_t². */
int32_t gp_predict_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                             const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                             const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out, void* const* var_out,
                             void* logpdf_out_or_null, int32_t* info_out);

/* gp_predict_batch with the gradients of its outputs w.r.t. the test inputs: what every gradient-based acquisition step over many independent
 * surrogates asks for (multi-start UCB / EI, one local GP per trust region, independent outputs sharing one x, per-fold sensitivity) — per problem
 * gp_posterior_fit + gp_posterior_predict_grad + gp_posterior_free otherwise.
 *   Everything up to `what` means what it means in gp_predict_batch (nxs ∈ {1, nb}, ns_b = 0 legal, what bit 0 the mean side, bit 1 the variance side).
 *   Per side the conventions are those of gp_posterior_predict_grad: a side that is asked for writes its values (mean_out / var_out: nb pointers to ns_b
 *   entries) and / or its gradient (dmean_out / dvar_out: nb pointers to ns_b * d entries in the container layout of xs_b, in the call's dtype).  Each of
 *   the four arrays may be NULL, not both of a side that is asked for; an array that is given holds a non-NULL pointer wherever ns_b > 0.
 *     dmean[j, p] = sum_i alpha_i dk(x*_j, x_i)/dx*_jp,     dvar[j, p] = -2 sum_i w_ji dk(x*_j, x_i)/dx*_jp,     w_j = C^-1 k_j.
 *   The prior mean counts as constant in x*, k(x*, x*) is constant, Matern12 at distance 0 contributes 0, a White factor contributes 0.
 * Failure is data: info_out[b] > 0 means NaN in every output of that problem (logpdf included), the other problems are not affected.  The return value
 * reports argument errors only (−i, reason in gp_last_error(); nb = 0 returns 0 and touches nothing).
 * fp64 problems with noise kind 0 / 1, D <= 16 and n_b <= GPMI355_BATCH_PGRAD_MAX_N run on the batch kernels (csrc/batch.hip), per wave: batch_logpdf_kernel,
 * batch_inv_kernel (S = L⁻ᵀ beside the slice, only for problems with a variance-side gradient and ns_b > 0), then per predict launch group
 * batch_predict_kernel (mean, variance, V = K* L⁻ᵀ left in the tile's strip) and directly behind it batch_pgrad_kernel over the same tiles: the weights
 * W = V Sᵀ by fp64 MFMA IN PLACE on the strip (64-column blocks ascending; accumulate, barrier, store, barrier), then the contraction with dk/dx*
 * re-evaluated from the packed inputs — one wave per test point, lanes striding over the training points, fp64 sums, a butterfly, one writer per (j, p).
 * No atomics, no waits between workgroups: a test point's gradient is the same bits alone, among other test points, in any batch and on repetition;
 * mean, var and logpdf are the bits of gp_predict_batch (the same kernels).  The mean side alone needs no strip, no S and no product.  Every other problem
 * is answered inside the same call by gp_posterior_fit(_sum) + gp_posterior_predict_grad + gp_posterior_free.  The read-only ctx parameter
 * "batch_pgrad_kernel_problems" counts the problems the kernels served.
 * GPMI355_BATCH_PGRAD_MAX_N: chosen by the rule that fixed the other two — the largest multiple of 128 of the measured sweep (tools/batch_predict_grad_profile.py,
 * profiles/r22/batch_predict_grad_profile.json: n = 64 … 2 048 × nb = 1, 8, 64, 512 × ns = 1, 64, 1 024, SE, D = 3, scalar noise, what = 3 with all four outputs) at which ONE
 * gp_predict_grad_batch call beat the loop of gp_posterior_fit + gp_posterior_predict_grad + gp_posterior_free in every cell with nb >= 8, the loop run twice — on a default ctx and
 * on a ctx with "dib_nb" = 128 (the blocked single path) — and the faster of the two taken.  The nb = 8, ns = 1 cells decide it (the default-ctx loop is the opponent there):
 * 1 152 points 11.43 ms (11.42 – 11.44) against 11.46 ms (11.45 – 11.47) — a win by 0.3 %, the ranges disjoint — 1 280 points 14.63 ms against 12.85 ms; 1 024 points is the last
 * size won by more than 5 % in every such cell (8.83 against 9.50 ms).  At nb = 64 the batch call wins every size but 2 048 points with 1 024 test points (291 against 177 ms), at
 * nb = 512 every size of the sweep (1 152 points, ns = 1 024: 198 against 1 088 ms); a single problem loses from 128 points on (ns = 64: 0.42 against 0.41 ms), as in the other
 * batch calls.
 * (The environment variable GPMI_BATCH_PGRAD_MAX_N, 0 … 2 048 = what the kernels admit, read per call, overrides it for measurements.) */
#define GPMI355_BATCH_PGRAD_MAX_N 1152
int32_t gp_predict_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                              const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                              const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out_or_null, void* const* var_out_or_null,
                              void* const* dmean_out_or_null, void* const* dvar_out_or_null, void* logpdf_out_or_null, int32_t* info_out);
/* The same with one composite kernel (gp_ksum) per problem. */
int32_t gp_predict_grad_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                                  const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                                  const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out_or_null, void* const* var_out_or_null,
                                  void* const* dmean_out_or_null, void* const* dvar_out_or_null, void* logpdf_out_or_null, int32_t* info_out);

/* The JOINT predictive distribution of the same nb problems at their test points, in ONE call: the latent covariance, the held-out log density
 * logpdf(post_b(x*_b, Σy*_b), y*_b) — the score of a cross-validation fold, the scoring rule of a grid search — and joint samples rand(post_b(x*_b, Σy*_b)) for
 * Thompson sampling and q-acquisitions over many surrogates (gp_posterior_fit + gp_posterior_predict(what = 5) / gp_posterior_logpdf / gp_posterior_rand +
 * gp_posterior_free per problem otherwise).  Per problem the semantics are those of that sequence (src/exact_gpr_posterior.jl:29-35, 78-83;
 * src/finite_gp_projection.jl:133-136, 233-237, 306-311, 325-326).
 *   The arguments up to prior_mean_xs_or_null are those of gp_predict_batch (nx, ny, nxs ∈ {1, nb}; ns_b = 0 is legal and touches nothing of that problem but
 *   its logpdf and info entries).  noise_xs_or_null: nb entries Σy*_b for the ns_b test points of each problem, NULL = zero.
 *   what: bit 0 the mean; bit 2 the latent covariance K** − VᵀV with no Σy* added, as in gp_posterior_predict; bit 3 the held-out logpdf; bit 4 samples.  Bit 1
 *   and every other bit are an argument error (marginal variances: gp_predict_batch), and so is 0.
 *   mean_out_or_null: nb pointers to ns_b entries.  cov_out_or_null: nb pointers to ns_b × ns_b entries, column-major with leading dimension ns_b, both
 *   triangles written and exactly symmetric.  ys_or_null: nb pointers to the ns_b held-out observations; hlogpdf_out_or_null: nb entries.  xi_or_null /
 *   samples_out_or_null: nb pointers to ns_b × nsamp entries each, column-major with leading dimension ns_b — the caller's standard normals and the draws, as
 *   in gp_posterior_rand: out[:, s] = mean + L* xi[:, s] with L* L*ᵀ = C* + Σy* (nsamp >= 0; 0 draws nothing).  The arrays of a bit that is asked for must not be
 *   NULL (nor their entries where ns_b > 0).  logpdf_out_or_null: the training logpdf, as in gp_predict_batch.  info_out: nb entries, the training
 *   factorisation; info_joint_out_or_null: nb entries, the order of the first leading minor of C*_b + Σy*_b that is not positive, or 0.
 * Failure is data: a failed training fit gives NaN in every output of that problem; a failed joint factorisation gives NaN in that problem's held-out logpdf and
 * samples only — its mean and covariance stay valid.  Other problems are never affected.  The return value reports argument errors only (−i, reason in
 * gp_last_error(); nb = 0 returns 0 and touches nothing).
 * fp64 problems with noise kind 0 / 1, D <= 16, n_b <= GPMI355_BATCH_JOINT_MAX_N, ns_b <= GPMI355_BATCH_JOINT_MAX_NS and a Σy*_b that is absent or of kind 0 / 1
 * run on the batch kernels (csrc/batch.hip), per wave: batch_logpdf_kernel; batch_predict_kernel with one strip per tile of 128 test points, a problem's strips
 * one behind the other — together V_b = K* L⁻ᵀ; batch_jcov_kernel, one workgroup per 64×64 tile (ti >= tj) of a problem's ns_b × ns_b matrix: K(x*_I, x*_J) from
 * the packed test points, minus V_I V_Jᵀ by fp64 MFMA, stored into the covariance (tile and mirror image) and, with Σy* on the diagonal, into a joint slice;
 * batch_jfact_kernel, one workgroup per problem: the blocked Cholesky of batch_logpdf_kernel on the joint slice with δ* = y* − mean riding along, the logpdf off
 * the carried row, the samples one wave per row.  No atomics, no waits between workgroups: every output is the same bits alone, anywhere in any batch and on
 * repetition; mean and training logpdf are the bits of gp_predict_batch.  Every other problem is answered inside the same call by the single-path sequence
 * above; which path serves a problem depends on that problem alone.  The read-only ctx parameter "batch_joint_kernel_problems" counts the problems the kernels
 * served.
 * GPMI355_BATCH_JOINT_MAX_N / GPMI355_BATCH_JOINT_MAX_NS: chosen by the rule that fixed the other three — each the largest multiple of 128 of the measured sweep
 * (tools/batch_joint_profile.py, profiles/r25/batch_joint_profile.json: n = 64 … 2 048 × nb = 1, 8, 64, 512 × ns = 64, 256, 1 024, SE, D = 3, scalar noise, scalar Σy*, what = 29
 * with 4 samples) at which ONE gp_joint_batch call beat the loop of gp_posterior_fit + gp_posterior_predict(what = 5) + gp_posterior_logpdf + gp_posterior_rand +
 * gp_posterior_free in every cell with nb >= 8, the loop run twice — on a default ctx and on a ctx with "dib_nb" = 128 — and the faster of the two taken.  The nb = 8 cells
 * decide MAX_N (the default-ctx loop is the opponent there): 1 536 points win at every ns — 19.84 ms (19.84 – 19.86) against 29.60 ms (29.55 – 29.80) at ns = 64, 31.01 ms
 * (30.94 – 31.20) against 37.04 ms (36.98 – 37.13) at ns = 1 024 — and 2 048 points lose at every ns: 40.54 ms (40.43 – 40.56) against 27.13 ms (27.07 – 27.21) at ns = 64,
 * 53.25 against 34.80 ms at ns = 1 024 — eight workgroups factor for longer than eight whole-chip fits take, as in gp_logpdf_batch.  (1 536 is the largest size of the sweep below
 * 2 048; nothing between them was measured.)  MAX_NS is the top of the sweep: 1 024 test points win every cell with nb >= 8 up to 1 536 points, the closest ones at nb = 8 (1 536 points
 * as above, a factor 1.19; 128 points 9.71 ms (9.59 – 9.73) against 12.08 ms (12.06 – 12.60), 1.24); more test points were not measured, and the joint slice of a problem is factored by
 * ONE workgroup, so ns_b is held to what was.  At nb = 64 the call wins every cell by 1.8 (2 048 points, ns = 1 024: 152 against 276 ms) to 118 (64 points, ns = 64), at nb = 512 by
 * 2.9 to 198 (1 536 points, ns = 1 024: 481 against 2 625 ms); a single problem wins only up to 256 points with 64 test points and up to 128 points with 256, and loses everywhere else
 * (ns = 1 024: 6.5 against 1.5 ms at 64 points), as in the other batch calls.
 * (The environment variables GPMI_BATCH_JOINT_MAX_N / GPMI_BATCH_JOINT_MAX_NS, 0 … 2 048 = what the kernels admit, read per call, override them for measurements.) */
#define GPMI355_BATCH_JOINT_MAX_N 1536
#define GPMI355_BATCH_JOINT_MAX_NS 1024
int32_t gp_joint_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                       const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                       const void* const* prior_mean_xs_or_null, const gp_noise* noise_xs_or_null, int32_t what, void* const* mean_out_or_null,
                       void* const* cov_out_or_null, const void* const* ys_or_null, void* hlogpdf_out_or_null, int32_t nsamp, const void* const* xi_or_null,
                       void* const* samples_out_or_null, void* logpdf_out_or_null, int32_t* info_out, int32_t* info_joint_out_or_null);
/* The same with one composite kernel (gp_ksum) per problem. */
int32_t gp_joint_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                           const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                           const void* const* prior_mean_xs_or_null, const gp_noise* noise_xs_or_null, int32_t what, void* const* mean_out_or_null,
                           void* const* cov_out_or_null, const void* const* ys_or_null, void* hlogpdf_out_or_null, int32_t nsamp,
                           const void* const* xi_or_null, void* const* samples_out_or_null, void* logpdf_out_or_null, int32_t* info_out,
                           int32_t* info_joint_out_or_null);

/* The training half of the batch calls: value AND gradient of logpdf for the same nb problems in ONE call — what multi-start hyper-parameter
 * optimisation, gradient-based samplers over hyper-parameters, per-fold training and independent outputs sharing one x evaluate at every step (one
 * gp_logpdf_grad call per problem otherwise).  Per problem the semantics are those of gp_logpdf_grad / gp_logpdf_grad_sum:
 *   ∂/∂θ = ½ Σ_ij (α_i α_j − C⁻¹_ij) ∂C_ij/∂θ.
 *   The arguments up to y are those of gp_logpdf_batch (same sharing through nx, ny ∈ {1, nb}, same checks); logpdf_out and info_out: nb entries.
 *   Every gradient output is optional: a NULL array means that side is not wanted; an array that is given holds a pointer for every problem (a NULL
 *   entry is an argument error, except in dscale_out where nscale_b = 0):
 *     dvariance_out_or_null   double[nb]                          ∂/∂(kernel variance) of problem b
 *     dscale_out_or_null      nb pointers, double[nscale_b] each   ∂/∂scale (may be NULL where nscale_b = 0)
 *     dtheta_out_or_null      (gp_logpdf_grad_batch_sum) nb pointers, one double per θ entry of k_b in the order documented at gp_ksum
 *     dnoise_out_or_null      nb pointers, call dtype: 1 entry (noise kind 0) ½(αᵀα − tr C⁻¹), n_b entries (kind 1) ½(α_i² − C⁻¹_ii), n_b × n_b entries
 *                             (kind 2 / 3, as gp_logpdf_grad; such a problem runs on the single path)
 *     dy_out_or_null          nb pointers, call dtype, n_b entries: ∂/∂y = −α_b
 *   ∂/∂x: gp_logpdf_grad_batch_x / gp_logpdf_grad_batch_sum_x below are the same calls with one more array, dx_out_or_null, behind dy_out_or_null.
 * Failure is data, as in the other batch calls: info_out[b] is the order of the first leading minor that is not positive, that problem's logpdf and every
 * one of its gradient outputs are NaN, the other problems are not affected.  The return value reports argument errors only (−i, reason in
 * gp_last_error(); nb = 0 returns 0 and touches nothing).
 * fp64 problems with noise kind 0 / 1, D <= 16 and n_b <= GPMI355_BATCH_GRAD_MAX_N run as four kernels per wave (csrc/batch.hip): batch_logpdf_kernel (the
 * fit, α always), then on the slices it left batch_inv_kernel — one workgroup per tile of 128 rows of S = L⁻ᵀ, the left-looking solve of the predict
 * kernel on identity rows, into a strip beside the slice — batch_grad_kernel — one workgroup per 64×64 tile of the lower triangle: C⁻¹_tile = S_i S_jᵀ by
 * fp64 MFMA, the weights ½(α_i α_j − C⁻¹_ij) (off-diagonal pairs doubled) contracted with ∂C_ij/∂θ re-evaluated from the packed inputs, partial sums per
 * tile reduced in a fixed order — and batch_gsum_kernel, which adds a problem's tiles in index order.  A problem spreads over many workgroups, launch
 * boundaries are the only synchronisation; no floating-point atomics, no waits between workgroups: a problem's gradient is the same bits alone, at any
 * position of any batch, and on repetition.  The workspace of a wave (slices, S strips, per-tile sums) stays within the budget of the other batch calls.
 * Every other problem (fp32, a dense Σy, a larger n_b or D) is answered inside the same call by gp_logpdf_grad / gp_logpdf_grad_sum; which path serves a
 * problem depends on that problem alone.  The read-only ctx parameter "batch_grad_kernel_problems" counts the problems the kernels served.
 * GPMI355_BATCH_GRAD_MAX_N: chosen by the rule that fixed GPMI355_BATCH_MAX_N — the largest multiple of 128 of the measured sweep
 * (tools/batch_grad_profile.py, profiles/r20/batch_grad_profile.json: n = 64 … 2 048 × nb = 1, 8, 64, 512, SE, D = 3, scalar noise) for which ONE
 * gp_logpdf_grad_batch call beat the loop of gp_logpdf_grad calls in every cell with nb >= 8.  The nb = 8 cells decide it: 1 024 points 8.13 ms against
 * 9.74 ms, 2 048 points 44.0 ms against 18.5 ms (no size between the two was measured); at nb = 64 and 512 the batch call wins every size of the sweep (2 048
 * points: 121.6 against 148.2 ms, 680 against 1 186 ms), a single problem loses from 256 points on (0.65 against 0.43 ms), as it does in the other batch calls.  (The environment variable
 * GPMI_BATCH_GRAD_MAX_N, 0 … 2 048 = what the kernels admit, read per call, overrides it for measurements.) */
#define GPMI355_BATCH_GRAD_MAX_N 1024
int32_t gp_logpdf_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                             const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                             double* dvariance_out_or_null, double* const* dscale_out_or_null, void* const* dnoise_out_or_null,
                             void* const* dy_out_or_null);
/* The same with one composite kernel (gp_ksum) per problem. */
int32_t gp_logpdf_grad_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                                 const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                                 double* const* dtheta_out_or_null, void* const* dnoise_out_or_null, void* const* dy_out_or_null);

/* gp_logpdf_grad_batch / gp_logpdf_grad_batch_sum with the gradient w.r.t. the inputs — what a deep-kernel model back-propagates into its feature map
 * (examples/2-deep-kernel-learning/script.jl) when one GP per output, task, fold or start sits behind it, and what a caller who optimises input or latent
 * locations needs; one gp_logpdf_grad (dx_out) / gp_logpdf_grad_sum_x call per problem otherwise.  Per problem the semantics are theirs:
 *     ∂logpdf/∂x_ip = Σ_{j ≠ i} (α_i α_j − C⁻¹_ij) ∂k/∂t_p (t = x_i − x_j)
 *   — both orders of the symmetric pair folded in, the prior mean taken as constant in x, noise independent of x; the diagonal contributes nothing, Matern12
 *   at distance 0 is taken as 0 (for coincident distinct points too), a White factor contributes 0.
 *   dx_out_or_null: NULL, or nb pointers; entry b receives n_b × d_b values in the container layout of x_b (as dx_out of gp_logpdf_grad), in the call's
 *   dtype.  With the array NULL the call does exactly what the entry point without _x does (kernel-served problems: the same bits in every output).  An
 *   array that is given with a NULL entry is an argument error at that argument's position.  With a shared x (nx = 1) every problem still gets its own
 *   n × d gradient w.r.t. the shared inputs; summing them is the caller's business.  Failure is data: info_out[b] > 0 means NaN in every entry of dx_out[b]
 *   as in that problem's other outputs, the neighbours are not affected.
 * With dx, fp64 problems with noise kind 0 / 1, D <= 16 and n_b <= GPMI355_BATCH_GRADX_MAX_N run on the kernels of gp_logpdf_grad_batch and, behind them on
 * the S strips and α they leave, two more (csrc/batch.hip): batch_gradx_kernel — one workgroup per 64×64 tile of the FULL square of a problem: C⁻¹_tile =
 * S_i S_jᵀ by fp64 MFMA over k >= 64·max(ti, tj), the weights α_i α_j − C⁻¹_ij (zero on the diagonal and in the padding) contracted with ∂k/∂t re-evaluated
 * from the packed inputs, lane = column, every (row, p) summed over the tile's 64 columns by a butterfly and stored in the tile's own table, one writer per
 * entry — and batch_gxsum_kernel — one workgroup per 64-row block, which adds the block's tables in column-tile order.  No floating-point atomics, no waits
 * between workgroups, every sum in an order the problem's size alone fixes: a problem's dx is the same bits alone, at any position of any batch, and on
 * repetition; its other outputs are the bits of the call without dx (the same kernels, launched the same way).  The tables (n_b²/64 × d_b doubles) count
 * towards the workspace budget of a wave.  Every other problem is answered inside the same call by gp_logpdf_grad (dx_out) / gp_logpdf_grad_sum_x; which
 * path serves a problem depends on that problem alone and on whether dx is asked for.  The read-only ctx parameter "batch_gradx_kernel_problems" counts the
 * problems the two kernels served.
 * GPMI355_BATCH_GRADX_MAX_N: chosen by the rule that fixed the other three — the largest multiple of 128 of the measured sweep (tools/batch_gradx_profile.py,
 * profiles/r24/batch_gradx_profile.json: n = 64 … 2 048 × nb = 1, 8, 64, 512, SE, D = 3, scalar noise, all outputs) at which ONE gp_logpdf_grad_batch_x call
 * beat the loop of gp_logpdf_grad calls with dx_out in every cell with nb >= 8.  The nb = 8 cells decide it: 1 152 points 11.20 ms (11.19 – 11.25) against
 * 13.03 ms (12.86 – 13.04), 1 280 points 14.57 ms (14.56 – 14.57) against 14.22 ms (14.19 – 14.49), 1 536 points 22.8 against 16.9 ms.  The limit lies above
 * GPMI355_BATCH_GRAD_MAX_N because the opponent pays more for dx than the batch call does: the loop's 1 024-point call costs 1.38 ms with dx (1.22 ms
 * without, r20), the batch call 7 % more than without dx at nb = 8.  At nb = 64 and 512 the batch call wins every size of the sweep (2 048 points: 142.6
 * against 160.8 ms, 854 against 1 263 ms); a single problem loses from 256 points on (0.71 against 0.57 ms), as in the other batch calls.  The batch call
 * with dx against the batch call without it, same cells: 1.06 – 1.11 at nb = 8 from 256 points on (1.34 at 64 points), 1.18 – 1.35 at nb = 64, 1.26 – 1.57
 * at nb = 512 (the full square of a problem is twice the tiles of batch_grad_kernel's triangle, each with its own S product).
 * (The environment variable GPMI_BATCH_GRADX_MAX_N, 0 … 2 048 = what the kernels admit, read per call, overrides it for measurements.) */
#define GPMI355_BATCH_GRADX_MAX_N 1152
int32_t gp_logpdf_grad_batch_x(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                               const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                               double* dvariance_out_or_null, double* const* dscale_out_or_null, void* const* dnoise_out_or_null,
                               void* const* dy_out_or_null, void* const* dx_out_or_null);
/* The same with one composite kernel (gp_ksum) per problem. */
int32_t gp_logpdf_grad_batch_sum_x(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                                   const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                                   double* const* dtheta_out_or_null, void* const* dnoise_out_or_null, void* const* dy_out_or_null,
                                   void* const* dx_out_or_null);

/* Leave-one-out cross-validation of nb independent problems in one call — the model-selection quantity a grid of hyper-parameters, a multi-start optimiser
 * or a set of independent outputs over one x evaluates again and again; one gp_loo / gp_loo_grad call per problem otherwise.  The arguments up to y, the
 * sharing through nx, ny ∈ {1, nb} and their checks are those of gp_logpdf_batch; per problem the semantics are those of gp_loo / gp_loo_sum and of
 * gp_loo_grad / gp_loo_grad_sum:
 *     value_out[b] = L_b (call dtype);  lp_out / mean_out / var_out: NULL, or nb pointers to n_b entries each (ℓ_i, μ_i, v_i; call dtype)
 *     dvariance_out / dscale_out / dtheta_out: as in gp_logpdf_grad_batch (double; dscale_out[b] may be NULL where nscale_b = 0)
 *     dnoise_out: nb pointers, call dtype: tr G (noise kind 0), n_b entries G_ii (kind 1), the full n_b × n_b G (kind 2 / 3);  dy_out: n_b entries −β
 *     dx_out: nb pointers to n_b × d_b entries in the container layout of x_b, as dx_out of gp_loo_grad
 *   Every output array is optional; an array that is given holds one non-NULL pointer per problem.  Failure is data: info_out[b] is the order of the
 *   first leading minor that is not positive, that problem's value and every one of its outputs are NaN, the other problems are not affected.  The return
 *   value reports argument errors only (−i, reason in gp_last_error(); nb = 0 returns 0 and touches nothing).
 * fp64 problems with noise kind 0 / 1, D <= 16 and n_b <= GPMI355_BATCH_LOO_MAX_N (values) resp. GPMI355_BATCH_LOO_GRAD_MAX_N (gradients) run on the batch
 * kernels (csrc/batch.hip), per wave: batch_logpdf_kernel (the fit, α always) and batch_inv_kernel (S = L⁻ᵀ in a strip beside the slice) as in
 * gp_logpdf_grad_batch; batch_loo_kernel — one workgroup per 128 rows of the strip, one wave per row: c_i = Σ_{k ≥ i} S_ik² by lane-strided sums and a
 * butterfly, then μ_i, v_i, ℓ_i and the tile's Σ ℓ_i — and batch_loo_sum_kernel, which adds a problem's tiles in order.  The gradient calls go on with
 * batch_loo_z_kernel — one workgroup per 64×64 tile of the full square: Z = C⁻¹ diag(√(2a)) with C⁻¹_tile = S_i S_kᵀ by fp64 MFMA, into a second strip —
 * batch_loo_beta_kernel — β_i = Σ_k Z_ik b_k / d_k, one wave per row — and the tile and sum kernels of gp_logpdf_grad_batch with the weights
 * (β_i α_j + α_i β_j − (Z Zᵀ)_ij)·(i = j ? ½ : 1) in place of logpdf's (a template parameter of batch_grad_kernel; the contraction with ∂C/∂θ and the ordered
 * sums are the same code).  No floating-point atomics, no waits between workgroups, every sum in an order the problem's size alone fixes: a problem's
 * outputs are the same bits alone, at any position of any batch, and on repetition.  Both strips, the vectors and the per-tile sums count towards the
 * workspace budget of a wave.  Every other problem — fp32, a dense Σy, a larger n_b or D, and EVERY problem of a call that asks for dx (the kernels have no
 * ∂/∂x yet) — is answered inside the same call by gp_loo[_sum] / gp_loo_grad[_sum]; which path serves a problem depends on that problem alone and on
 * whether dx is asked for.  The read-only ctx parameters "batch_loo_kernel_problems" and "batch_loo_grad_kernel_problems" count the problems the kernels
 * served.
 * GPMI355_BATCH_LOO_MAX_N / GPMI355_BATCH_LOO_GRAD_MAX_N: chosen by the rule that fixed the other four — each the largest multiple of 128 of the measured sweep
 * (tools/batch_loo_profile.py, profiles/r32/batch_loo_profile.json: n = 64 … 2 048 × nb = 1, 8, 64, 512, SE, D = 3, scalar noise, all outputs except dx) at which
 * ONE batch call beat the loop of gp_loo resp. gp_loo_grad calls in every cell with nb >= 8, a cell counting only where every sample of the batch call lies
 * below every sample of the loop.  The nb = 8 cells decide both.  Values: 1 024 points 7.96 ms (7.96 – 7.96) against 8.47 ms (8.47 – 8.48); 1 152 points
 * 10.49 ms (10.46 – 10.51) against 10.99 ms (10.47 – 11.20): the medians still favour the batch call, the ranges overlap, so the cell decides nothing and the
 * limit stays at 1 024; 1 280 points 13.52 against 11.67 ms.  Gradients: 1 280 points 14.79 ms (14.77 – 14.80) against 16.95 ms (16.80 – 17.26), 1 536 points
 * 23.42 against 19.35 ms (no size between the two was measured).  The gradient limit lies above the value limit because the opponent pays more for the
 * gradient than the batch call does: at 1 024 points and nb = 8 the loop goes from 8.47 to 12.57 ms, the batch call from 7.96 to 8.80 ms.  At nb = 64 and
 * 512 the batch call wins every size of the sweep (2 048 points: values 112.4 against 130.6 ms and 610 against 1 046 ms, gradients 153.1 against 187.3 ms
 * and 1 095 against 1 527 ms; 64 points × 512: 0.39 against 124.8 ms and 0.44 against 223.8 ms).  A single problem loses to the one single call from 128
 * points on for values (0.29 against 0.25 ms; 2 048 points: 41.6 against 2.0 ms) and from 256 points on for gradients (0.75 against 0.62 ms; 2 048 points:
 * 42.6 against 2.9 ms), as in the other batch calls: one workgroup factors the whole problem.
 * (The environment variables GPMI_BATCH_LOO_MAX_N and GPMI_BATCH_LOO_GRAD_MAX_N, 0 … 2 048 = what the kernels admit, read per call, override them for
 * measurements.) */
#define GPMI355_BATCH_LOO_MAX_N 1024
#define GPMI355_BATCH_LOO_GRAD_MAX_N 1280
int32_t gp_loo_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                     const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                     void* const* lp_out_or_null, void* const* mean_out_or_null, void* const* var_out_or_null);
int32_t gp_loo_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                         const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                         void* const* lp_out_or_null, void* const* mean_out_or_null, void* const* var_out_or_null);
int32_t gp_loo_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                          const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                          double* dvariance_out_or_null, double* const* dscale_out_or_null, void* const* dnoise_out_or_null,
                          void* const* dy_out_or_null, void* const* dx_out_or_null);
int32_t gp_loo_grad_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                              const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                              double* const* dtheta_out_or_null, void* const* dnoise_out_or_null, void* const* dy_out_or_null,
                              void* const* dx_out_or_null);

/* Sequential conditioning, posterior(fx::FiniteGP{<:PosteriorGP}, y) (src/exact_gpr_posterior.jl:46-56): the resident
 * factor of `old` is extended by the bordered-Cholesky step update_chol (src/util/common_covmat_ops.jl:38-42):
 *   U12 = U11'\C12  (here: rows K(x2,x1)·L11⁻ᵀ by the blocked MFMA TRSM),  U22 = chol(C22 − U12'U12).
 * x2 / noise2: the new inputs and their noise;  delta_all: δ = vcat(δ_old, y2 − m(x2)) (length n_old + n2, host).
 * `old` stays valid.  alpha_out (n_old + n2) and logpdf_out (logpdf of all observations under the prior) optional. */
int32_t gp_posterior_update(gp_post* old, const gp_points* x2, const gp_noise* noise2, const void* delta_all,
                            gp_post** out, void* alpha_out_or_null, void* logpdf_out_or_null);

/* out[:, s] = C.U' * xi[:, s] (n×ncols column-major host arrays, leading dimension n): the sampling transform of
 * rand / _rand! (src/finite_gp_projection.jl:233-237, 271-277); the caller draws xi = randn(rng, n, ncols). */
int32_t gp_posterior_factor_mul(gp_post* post, const void* xi, int32_t ncols, void* out);

/* out[:, s] = C \ B[:, s] (n×ncols column-major host arrays) by forward + backward sweeps over the resident factor — what
 * gradlogpdf(fx, X) = C \ (m .- X) (src/finite_gp_projection.jl:328-337) needs for the columns beyond the fitted one, and
 * `post.data.C \ v` of user code. */
int32_t gp_posterior_solve(gp_post* post, const void* B, int32_t ncols, void* out);

/* C.U (n×n column-major upper, strictly-lower part zero) to the host — parity / debugging only. */
int32_t gp_posterior_get_factor(gp_post* post, void* U_out);
/* logdet(post.data.C) = 2 Σ log U_ii, kept from the fit (always double). */
int32_t gp_posterior_logdet(gp_post* post, double* out);
int64_t gp_posterior_n(gp_post* post);
int32_t gp_posterior_free(gp_post* post); /* NULL or already-freed handle: returns -1, never UB-free twice */

/* ---- VFE / DTC sparse approximation -------------------------------------------------------- */
/* posterior(VFE(f(z, jitter)), f(x, Σy), y)  (src/sparse_approximations.jl:58-75) and
 * approx_log_evidence / elbo (:248-254 VFE, :282-286 DTC) from the same intermediates.
 * approx: 0 VFE, 1 DTC.  objective_out_or_null: 1 entry.  K_xz is streamed in row blocks and never
 * materialised; only M×M matrices live in HBM. */
int32_t gp_vfe_fit(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_points* z,
                   const gp_noise* noise, double jitter, const void* mean_or_null, const void* y,
                   int32_t approx, gp_vfe** out, void* objective_out_or_null);
/* update_posterior(f_post_approx, fx, y) with the same pseudo-points (src/sparse_approximations.jl:87-121): the streamed
 * reductions of `old` (B Bᵀ, B b_y, ‖B‖²_F, the Σy terms) are continued with the new observations and the M×M side is
 * re-finalised — equal to refitting on all observations.  objective_out: ELBO / DTC evidence of all observations. */
int32_t gp_vfe_update(gp_vfe* old, const gp_points* x2, const gp_noise* noise2, const void* mean2_or_null, const void* y2,
                      gp_vfe** out, void* objective_out_or_null);
/* update_posterior(f_post_approx, fz) — append pseudo-points (src/sparse_approximations.jl:131-176): bordered Cholesky of
 * K_zz against the resident factor (update_chol, src/util/common_covmat_ops.jl:38-42), then the retained observations are
 * streamed once more to form ONLY the new block rows of B Bᵀ / B b_y / ‖B‖²_F (the reference keeps B_εf, x, Σy, b_y in its
 * cache for this; here x, Σy^-1/2 and b_y stay on the device and B is never stored).  As in the reference (:138) the new
 * diagonal block C22 = cov(prior, z2) carries no jitter.  `old` stays valid.  objective_out: ELBO / DTC evidence with the enlarged pseudo-point set. */
int32_t gp_vfe_append(gp_vfe* old, const gp_points* z2, gp_vfe** out, void* objective_out_or_null);
/* mean / var / cov / mean_and_var / mean_and_cov (src/sparse_approximations.jl:183-217).  what: bit0 mean, bit1 var,
 * bit2 full cov (ns×ns column-major) = K** − AᵀA + (Λ_ε.U⁻ᵀA)ᵀ(Λ_ε.U⁻ᵀA). */
int32_t gp_vfe_predict(gp_vfe* post, const gp_points* xs, const void* prior_mean_xs_or_null, int32_t what,
                       void* mean_out, void* var_out, void* cov_out);
/* The sparse counterpart of gp_posterior_predict_grad (same `what`, outputs, conventions; src/sparse_approximations.jl:183-217).  With
 * A_j = L_z^-1 K(z, x*_j), Lambda_eps = L_d L_d^T and alpha over the M pseudo-points:
 *     dmean[j, p] =      sum_m alpha_m dk(x*_j, z_m)/dx*_jp
 *     dvar[j, p]  = -2 * sum_m u_jm    dk(x*_j, z_m)/dx*_jp,     u_j = L_z^-T (A_j - Lambda_eps^-1 A_j)
 * Both forward solves of gp_vfe_predict, then the Lambda_eps backward solve, the subtraction and the L_z backward solve (all M wide), then the same
 * kernel over z.  fp64 on the device whatever the handle's dtype, like gp_vfe_predict. */
int32_t gp_vfe_predict_grad(gp_vfe* post, const gp_points* xs, const void* prior_mean_xs_or_null, int32_t what,
                            void* mean_out_or_null, void* var_out_or_null, void* dmean_out_or_null, void* dvar_out_or_null);
/* logpdf(f_post_approx(x*, Σy*), Y*) and rand(...) — same contracts as gp_posterior_logpdf / gp_posterior_rand. */
int32_t gp_vfe_logpdf(gp_vfe* post, const gp_points* xs, const void* prior_mean_xs_or_null, const gp_noise* noise,
                      const void* Y, int64_t ldy, int32_t ncols, void* out);
int32_t gp_vfe_rand(gp_vfe* post, const gp_points* xs, const void* prior_mean_xs_or_null, const gp_noise* noise,
                    const void* xi, int32_t ncols, void* out);
int64_t gp_vfe_m(gp_vfe* post); /* number of pseudo-points */
/* α = U \ m_ε (length M) and m_ε — cache fields of src/sparse_approximations.jl:73. */
int32_t gp_vfe_get(gp_vfe* post, void* alpha_out_or_null, void* m_eps_out_or_null);
/* The two M×M factors of the cache (src/sparse_approximations.jl:73: `U` = cholesky(cov(fz)).U and `Λ_ε.U`, read field by field by
 * test/sparse_approximations.jl:48-55, 76-83): M×M column-major UPPER triangular host arrays in the posterior's dtype (the strictly
 * lower part is zero-filled); either pointer may be NULL.  The device keeps both as fp64 row-major lower factors — byte-identical. */
int32_t gp_vfe_get_factors(gp_vfe* post, void* U_out_or_null, void* Lambda_U_out_or_null);
int64_t gp_vfe_n(gp_vfe* post); /* observations seen so far (fit + every update_posterior) */
/* b_y = U_y⁻ᵀ (y − m) of every observation seen so far, length gp_vfe_n(post) (cache field b_y, :66, :102), posterior's dtype. */
int32_t gp_vfe_get_by(gp_vfe* post, void* b_y_out);
/* Gradient of the objective the handle was fitted with — elbo for VFE (src/sparse_approximations.jl:248-254), approx_log_evidence for DTC (:282-286) — at the
 * handle's own parameters, after any number of gp_vfe_update / gp_vfe_append calls (the observations are retained on the device; B_εf is never stored: they are
 * streamed once more, one MFMA GEMM per chunk).  The reference has no hand-written adjoint: this is what an AD backend computes when
 * examples/0-intro-1d/script.jl:385-394 maximises the ELBO over kernel parameters and pseudo-points.  Every output may be NULL.
 *   dvariance      ∂/∂σ_k² (the ScaledKernel factor)             dscale [nscale]  ∂/∂s (ScaleTransform) or ∂/∂v_p (ARDTransform)
 *   dnoise_sum     Σ_i ∂/∂Σy_ii (the gradient for a scalar σ²)   dnoise_diag [n]  ∂/∂Σy_ii, the handle's dtype, n = gp_vfe_n(post), arrival order
 *   dy [n]         ∂/∂y_i (= −∂/∂m_i of the prior mean), the handle's dtype
 *   dz [m·d]       ∂/∂z in the container layout z_layout (0 vector, 1 ColVecs D×M column-major, 2 RowVecs M×D column-major), fp64.  fp64 handles only (status −7
 *                  otherwise): ∂/∂z is the small difference of the K_zz and K_fz terms, and the B Bᵀ an fp32 fit accumulated from fp32 products does not carry it
 *                  (measured at C5: 69 % off; the other outputs of an fp32 handle are within 2e-3 of the fp64 oracle's — the backward pass itself is always fp64)
 *   dx [n·d]       ∂/∂x in the container layout x_layout, the handle's dtype (adds one row reduction per observation to the streamed pass)
 * gp_get_timings afterwards: assemble = the M×M side, potrf = the streamed pass, solve = the K_zz term. */
int32_t gp_vfe_grad(gp_vfe* post, double* dvariance_or_null, double* dscale_or_null, double* dnoise_sum_or_null, void* dnoise_diag_or_null, void* dy_or_null,
                    double* dz_or_null, int32_t z_layout, void* dx_or_null, int32_t x_layout);

/* ---- VFE / DTC for a matrix of observations ("columns") --------------------------------------------------------------------------- */
/* S = ncols <= GPMI355_COLS_MAX sparse GPs that share x, z, kernel, jitter, Σy (scalar or diagonal) and the prior-mean vector and differ in y — the columns
 * of Y (n×ncols column-major, leading dimension ldy) — fitted, updated, predicted and differentiated from ONE streamed pass over the data: K(x_c, z), the
 * triangular product and the SYRK of a chunk do not depend on y, only the product c_s = B b_ys does.  Single-kind kernels; composite kernels and a dense
 * Σy are refused as on the rest of the sparse path.  fp64 and fp32 handles.
 * gp_vfe_fit_cols: gp_vfe_fit for every column.  objective_out_or_null: ncols entries (elbo for approx 0, approx_log_evidence for 1).  ncols outside
 *   1..GPMI355_COLS_MAX is an argument error (argument 10), ldy < n argument 9.  A failed factorisation returns the LAPACK info and no handle.  Per chunk
 *   ystats_cols_kernel (csrc/kernels.hpp) reads Y = −B_c once and forms ‖B‖² per row and B_c b_cs for every column on the fp64 16×16×4 MFMA (fp32
 *   operands widened: the sums over the data points are fp64 for either dtype); a workgroup owns 32 rows for all data points and all columns, its four
 *   waves split the data points by a rule that reads neither ncols nor the data, and their partial sums are added in wave order: no floating-point
 *   atomics, bitwise repeatable, a column's bits independent of what the other columns hold.  After the pass the M×M side solves all columns at once
 *   (the blocked solves of the predictions over the columns' rows).  The handle retains b_y of every column: round_up(ncols, 16) × npad values of the
 *   handle's dtype on the device (npad = n rounded up to the chunk; N = 2·10⁶, ncols = 128, fp32: about 1 GB).
 *   With ncols = 1 the call IS gp_vfe_fit (the same launches, the same bits), and so is every *_cols call below its single-column counterpart.
 * gp_vfe_update_cols / gp_vfe_append_cols: gp_vfe_update / gp_vfe_append on such a handle; Y2 (n2×ncols column-major, leading dimension ldy2) must have
 *   the handle's ncols; objective_out_or_null: ncols entries.
 * gp_vfe_ncols: the columns of a handle — 1 for every handle made by the single-column calls.
 * gp_vfe_predict_cols: `what` bits as gp_vfe_predict.  mean_out: ns×ncols column-major, column s = m(x*) + K(x*, z) α_s, from ONE kmul_kernel launch over
 *   the pseudo-points (K_*z evaluated once for all columns; counted in "cols_kernel_calls"; D > 16: one kvec launch per column); var_out (ns) and cov_out
 *   (ns×ns) do not depend on y and are what gp_vfe_predict returns.
 * gp_vfe_get_cols: α and m_ε of every column, both M×ncols column-major.   gp_vfe_get_by_cols: b_y of every column, n×ncols column-major, n = gp_vfe_n.
 * gp_vfe_grad_cols: the gradient of Σ_s objective_s at the handle's parameters; outputs as gp_vfe_grad with dy replaced by dY (n×ncols column-major,
 *   column s = ∂/∂Y[:, s]).  The M×M algebra of gp_vfe_grad with the column sums folded in — G_ψ = ½[S·W H_ψ Wᵀ − A Aᵀ], G_zz likewise, A = the M×ncols
 *   matrix of the α_s — and per chunk two skinny MFMA GEMMs beside T̃ = (S K_c) G_ψ: the rank-S term ½ b_c Aᵀ into the chunk's weights and the per-column
 *   row sums (S K_c) A.  fp64 pass for fp32 handles; dz on an fp32 handle stays refused (−7).
 * A handle with ncols > 1 serves unchanged everything that does not use α: gp_vfe_predict with what ⊆ {var, cov}, the variance side of gp_vfe_predict_grad,
 *   gp_vfe_get_factors, gp_vfe_m, gp_vfe_n, gp_vfe_free.  The mean bit of gp_vfe_predict, the mean side of gp_vfe_predict_grad, gp_vfe_get, gp_vfe_get_by,
 *   gp_vfe_logpdf, gp_vfe_rand, gp_vfe_update, gp_vfe_append and gp_vfe_grad return −1 (the handle argument) with the reason in gp_last_error() and write
 *   nothing. */
int32_t gp_vfe_fit_cols(gp_ctx* ctx, const gp_kernel* k, const gp_points* x, const gp_points* z, const gp_noise* noise, double jitter,
                        const void* mean_or_null, const void* Y, int64_t ldy, int32_t ncols, int32_t approx, gp_vfe** out, void* objective_out_or_null);
int32_t gp_vfe_update_cols(gp_vfe* old, const gp_points* x2, const gp_noise* noise2, const void* mean2_or_null, const void* Y2, int64_t ldy2, gp_vfe** out,
                           void* objective_out_or_null);
int32_t gp_vfe_append_cols(gp_vfe* old, const gp_points* z2, gp_vfe** out, void* objective_out_or_null);
int32_t gp_vfe_ncols(gp_vfe* post, int32_t* out);
int32_t gp_vfe_predict_cols(gp_vfe* post, const gp_points* xs, const void* prior_mean_xs_or_null, int32_t what, void* mean_out, void* var_out,
                            void* cov_out);
int32_t gp_vfe_get_cols(gp_vfe* post, void* alpha_out_or_null, void* m_eps_out_or_null);
int32_t gp_vfe_get_by_cols(gp_vfe* post, void* B_out);
int32_t gp_vfe_grad_cols(gp_vfe* post, double* dvariance_or_null, double* dscale_or_null, double* dnoise_sum_or_null, void* dnoise_diag_or_null,
                         void* dY_or_null, double* dz_or_null, int32_t z_layout, void* dx_or_null, int32_t x_layout);
int32_t gp_vfe_free(gp_vfe* post);

/* ---- device-level building blocks ------------------------------------------------------------ */
/* The operations the in-library multi-device driver composes (csrc/multi.hip calls the same engine functions), exposed on DEVICE
 * memory so that they can be unit-tested one by one (tests/test_gpu_units.py) and driven by a caller that keeps its own
 * device-resident data.  All pointers below are DEVICE pointers (double* in the entry points declared first, float* in their
 * _f32 twins), row-major with the given leading dimension, i.e.
 * a row-major lower factor L — memory-identical to Julia's column-major C.U.  Work is issued on the
 * ctx main stream and NOT synchronised (gpd_sync, or order it against your own stream work).
 * m, n multiples of 64 (gpd_trsv: np multiple of 128); k multiple of 16 (gemm; 32 in gpd_gemm_nt_f32).
 * Every entry point with matrix / vector data has an fp32 twin gpd_X_f32 (declared below, after the fp64 ones): the same arguments with float* data, the same kernels
 * instantiated for float — what every fp32 fit runs (tests/test_gpu_units_f32.py).  info_dev stays int32*, logdet_dev and the row sums stay double*. */

/* Fill local tiles of K + Σy.  rows: global indices row0 + i (i < m) mapped through the block-cyclic
 * map (global tile-row of local 128-tile t is ((t / tb) * P + p) * tb + t % tb); same for columns with
 * (Q, q).  x_dev is n_total×d in RowVecs layout (dimension-contiguous) already on the device;
 * noise_dev has n_total entries (padding rows get identity).  */
typedef struct {
    int32_t P, p, Q, q; /* process grid and my coordinates                                */
    int32_t tb;         /* 128-tiles per distribution block (NB / 128)                       */
    int32_t lower;      /* 1: skip 128-tiles strictly above the global diagonal             */
} gp_grid;

int32_t gpd_assemble(gp_ctx* ctx, const gp_kernel* k, const double* x_dev, int64_t n_valid, int64_t n_pad,
                     int32_t d, const double* noise_dev, const gp_grid* g, double* a_loc, int64_t lda,
                     int64_t m_loc, int64_t n_loc);
/* In-place lower Cholesky of the n×n diagonal block at a (rows/cols [0,n)), and of the m-n rows
 * below it (X ← X L⁻ᵀ) when m > n.  info_dev: device int32, set to (col0 + failing column, 1-based)
 * on the first non-positive pivot.  logdet_dev += Σ log L_ii over columns col0+i < n_valid.
 * m, n multiples of 64; `a` 16-byte aligned and lda even (the leaf kernels move rows as 16-byte pieces): anything else is refused (−2 / −3). */
int32_t gpd_potrf(gp_ctx* ctx, double* a, int64_t lda, int64_t m, int64_t n, int32_t* info_dev, int32_t col0,
                  int64_t n_valid, double* logdet_dev);
/* X (m×n) ← X · L⁻ᵀ with L the n×n lower factor (row-major, ldl). */
int32_t gpd_trsm(gp_ctx* ctx, double* x, int64_t ldx, int64_t m, const double* l, int64_t ldl, int64_t n);
/* The two pieces of the multi-device panel step ("multi_trsm_inv"; csrc/multi.hip):
 *   gpd_inv_lower: W (nb × ldw, lower) ← −inv(L) for the nb×nb lower block L.  W must be zero above its diagonal on entry and, like both scratch blocks, followed by
 *                  128 finite slack rows; scratch1 / scratch2: (nb + 128) × ldw doubles, ZEROED by the caller before the first use (their untouched triangles must stay
 *                  zero).  nb = 64·2^m with scratch2 != NULL: level by level in 1 + 3·log2(nb/64) batched launches; otherwise (scratch2 NULL or another nb, nb a
 *                  multiple of 64): the restricted-row recursion on the identity.
 *   gpd_trsm_inv : X (m × nb) ← X · L⁻ᵀ = −X · Wᵀ with that W as ONE triangular-k GEMM into scratch ((m + 128) × lds doubles) + one copy back. */
int32_t gpd_inv_lower(gp_ctx* ctx, const double* l, int64_t ldl, int64_t nb, double* w, int64_t ldw, double* scratch1, double* scratch2_or_null);
int32_t gpd_trsm_inv(gp_ctx* ctx, double* x, int64_t ldx, int64_t m, const double* w, int64_t ldw, int64_t nb, double* scratch, int64_t lds);
/* C (m×n) -= A (m×k) · B (n×k)ᵀ.  With g != NULL and g->lower, 64×64 sub-tiles strictly above the
 * global diagonal are skipped; row0/col0 = local absolute index of C's first row/column (mapped to
 * global indices through g).  g == NULL: plain rectangular update. */
int32_t gpd_gemm_nt(gp_ctx* ctx, double* c, int64_t ldc, const double* a, int64_t lda, const double* b,
                    int64_t ldb, int64_t m, int64_t n, int64_t k, const gp_grid* g_or_null, int64_t row0,
                    int64_t col0);
/* nrhs vectors stored as rows r[s*ldr + i], i < np: forward (L z = r) or backward (Lᵀ a = r) solve in place. */
int32_t gpd_trsv(gp_ctx* ctx, const double* l, int64_t ldl, int64_t np, double* r, int64_t ldr, int32_t nrhs,
                 int32_t forward);
/* r[j] -= Σ_{i<nrows} l[i*ldl + j] · a[i]  for j < ncols  (block row of Lᵀ times a vector; backward sweep). */
int32_t gpd_gemv_t(gp_ctx* ctx, const double* l, int64_t ldl, int64_t nrows, int64_t ncols, const double* a,
                   double* r);
/* out_dev[i] = Σ_{c<ncols} x[i*ldx + c]² for i < nrows. */
int32_t gpd_rowsumsq(gp_ctx* ctx, const double* x, int64_t ldx, int64_t nrows, int64_t ncols, double* out_dev);
int32_t gpd_sync(gp_ctx* ctx);
/* The fp32 twins.  Contracts, read off the float instantiations (rows move as 16-byte pieces = 4 floats; the GEMM's k step is 32); anything else is refused with a
 * status and a reason (gp_last_error), never run:
 *   gpd_assemble_f32 : m_loc, n_loc multiples of 128 (−11); a_loc 8-byte aligned (−9), lda even and >= n_loc (−10): two columns per store.
 *   gpd_potrf_f32    : m, n multiples of 64, m >= n (−4); a 16-byte aligned (−2); lda a multiple of 4 and >= n (−3).  Every leaf is panel64_kernel<float>
 *                      ("leaf_v2" is fp64-only); (m + 128) rows allocated (the trailing GEMM's operand over-read).
 *   gpd_trsm_f32     : m, n multiples of 64 (−4); x and l 16-byte aligned, ldx and ldl multiples of 4 (−2 / −5).
 *   gpd_gemm_nt_f32  : m, n multiples of 64, k a multiple of 32 (−8); a and b 16-byte aligned, lda and ldb multiples of 4 (−4 / −6); c: any float alignment.
 *                      As in fp64 both operands are over-read up to the next multiple of 128 rows: allocate them.
 *   gpd_trsv_f32     : np a multiple of 128 (−4); l 16-byte aligned, ldl a multiple of 4 (−2); r: any float alignment.
 *   gpd_gemv_t_f32, gpd_rowsumsq_f32 : element-wise access, no alignment contract (gpd_rowsumsq_f32 sums in fp64 and returns doubles). */
int32_t gpd_assemble_f32(gp_ctx* ctx, const gp_kernel* k, const float* x_dev, int64_t n_valid, int64_t n_pad,
                         int32_t d, const float* noise_dev, const gp_grid* g, float* a_loc, int64_t lda,
                         int64_t m_loc, int64_t n_loc);
int32_t gpd_potrf_f32(gp_ctx* ctx, float* a, int64_t lda, int64_t m, int64_t n, int32_t* info_dev, int32_t col0,
                      int64_t n_valid, double* logdet_dev);
int32_t gpd_trsm_f32(gp_ctx* ctx, float* x, int64_t ldx, int64_t m, const float* l, int64_t ldl, int64_t n);
int32_t gpd_gemm_nt_f32(gp_ctx* ctx, float* c, int64_t ldc, const float* a, int64_t lda, const float* b,
                        int64_t ldb, int64_t m, int64_t n, int64_t k, const gp_grid* g_or_null, int64_t row0,
                        int64_t col0);
int32_t gpd_trsv_f32(gp_ctx* ctx, const float* l, int64_t ldl, int64_t np, float* r, int64_t ldr, int32_t nrhs,
                     int32_t forward);
int32_t gpd_gemv_t_f32(gp_ctx* ctx, const float* l, int64_t ldl, int64_t nrows, int64_t ncols, const float* a,
                       float* r);
int32_t gpd_rowsumsq_f32(gp_ctx* ctx, const float* x, int64_t ldx, int64_t nrows, int64_t ncols, double* out_dev);

/* ---- the gradient contractions and the sparse path's N-long reductions, on caller-supplied weights (tests/test_gpu_units_grad.py, test_gpu_units_sparse.py) ----
 * The kernels that turn a factorisation into gradients, reachable without a factorisation: the weights are the caller's, so an error of the contraction is not hidden
 * behind the conditioning of C.  Each entry launches through the function production launches through (csrc/gpmi355.hip launch_kgrad / launch_kgradx, csrc/vfe.hpp
 * launch_vgrad / launch_ystats / launch_ystats_cols): a shape gets the kernel instance here that it gets in gp_logpdf_grad / gp_vfe_grad / gp_vfe_fit.  T = double, or
 * float in the _f32 twins; every sum is fp64 whatever T is.  gpd_grad_contract* and gpd_vgrad* stage the kernel's scales and DRAIN the ctx stream before they
 * return; gpd_ystats* only queue (gpd_sync).  "Read, never used" below means: the location must be addressable, its value — a NaN included — cannot reach an output.
 *
 * gpd_grad_contract: the contraction of gp_logpdf_grad,  Σ_{j<=i<n} w_ij ∂C_ij/∂θ  with  w_ij = (alpha_i alpha_j + ci_ij) · (i == j ? ½ : 1)   (ci = −C⁻¹).
 *   ci    n rows of a row-major LOWER matrix, leading dimension ld >= np, 16-byte aligned.  Used: ci[i][j], j <= i < n.  Read, never used: ci[i][j] for i < n,
 *         i < j < np (the D <= 16 form loads the 2-wide pair (2l, 2l+1) of every 128-tile on or below the diagonal and discards what lies above the diagonal or
 *         beyond n).  Rows >= n are not read.  D <= 16 and ld·sizeof(T) a multiple of 16: kgrad_fast_kernel<T, 4|8|16>; otherwise kgrad_kernel<T>, once per 16 ARD
 *         scales (the only form for D > 16; for D <= 16 the form production never takes, its ld being padded to 16 bytes).  Both must give the same sums.
 *   alpha n entries; entries >= n are not read.
 *   x     the inputs ALREADY multiplied by the scales (u = s∘x), dimension-major [d][np] with leading dimension np, np a multiple of 128.  Columns [n, np) are read,
 *         never used.
 *   k     kind 0..3, variance, nscale ∈ {0, 1, d} with `scale` on the HOST (it divides the scale sums and multiplies gx; x is not scaled again); dtype must be T's.
 *   g     doubles, 2 + max(nscale, 1):  g[0] += Σ w κ (∂/∂variance),  g[1] += Σ_i dn[i],  g[2 + p] += Σ w σ² dκ/dr² ∂r²/∂s_p  (∂r²/∂s = 2r²/s for one scale,
 *         2(u_ip − u_jp)²/s_p for ARD).  With nscale = 0, g[2] is not touched.  Atomic "+=": zero it for the value alone.
 *   dn    T, n entries: dn[i] = ½ (alpha_i² + ci_ii), OVERWRITTEN; entries >= n untouched.
 *   gx    NULL, or doubles [d][np]:  gx[p][i] += 2 s_p σ² Σ_{j≠i, j<n} (alpha_i alpha_j + ci_max(i,j),min(i,j)) dκ/dr² (u_ip − u_jp)  for i < n (kgradx_kernel, once per
 *         16 dimensions); columns >= n untouched.  Atomic "+=".
 *   Matern12 at r = 0 takes dκ/dr² = 0: a coincident pair adds exactly 0 to the scale sums and to gx.
 * gpd_grad_contract_sum: the same for a composite kernel (kgrad_sum_kernel once per 16 θ entries, kgradx_sum_kernel): x holds the RAW inputs, D <= 16,
 *   g[2 + p] += ∂/∂θ_p in the order of gp_logpdf_grad_sum's dtheta (2 + nθ doubles; g[0] is not touched), gx[p][j] += ∂/∂x_jp.
 * Refused: kernel (−2), ci NULL / misaligned (−3), ld < np (−4), alpha / x NULL (−5 / −6), n outside 1..np (−7), np no multiple of 128 (−8), d < 1 (−9), g / dn NULL
 * (−10 / −11). */
int32_t gpd_grad_contract(gp_ctx* ctx, const gp_kernel* k, const double* ci, int64_t ld, const double* alpha, const double* x, int64_t n, int64_t np, int32_t d,
                          double* g, double* dn, double* gx_or_null);
int32_t gpd_grad_contract_f32(gp_ctx* ctx, const gp_kernel* k, const float* ci, int64_t ld, const float* alpha, const float* x, int64_t n, int64_t np, int32_t d,
                              double* g, float* dn, double* gx_or_null);
int32_t gpd_grad_contract_sum(gp_ctx* ctx, const gp_ksum* k, const double* ci, int64_t ld, const double* alpha, const double* x, int64_t n, int64_t np, int32_t d,
                              double* g, double* dn, double* gx_or_null);
int32_t gpd_grad_contract_sum_f32(gp_ctx* ctx, const gp_ksum* k, const float* ci, int64_t ld, const float* alpha, const float* x, int64_t n, int64_t np, int32_t d,
                                  double* g, float* dn, double* gx_or_null);
/* gpd_vgrad: the reverse pass of the sparse objective over one rectangular kernel block K(rows, cols), nr × nc (gp_vfe_grad runs it in fp64 only; the _f32 twin
 * instantiates the same templates for float).  With W_ij = ∂L/∂K_ij, κ and dκ/dr² recomputed from the inputs:
 *     g[0] += Σ W κ,   g[2 + p] += Σ W σ² dκ/dr² ∂r²/∂s_p  (as above; g: 2 + max(nscale, 1) doubles; g[1], and with nscale = 0 g[2], not touched),
 *     gz[p][j] += zfac · Σ_i W_ij σ² dκ/dr² (−2 s_p)(u_ip − w_jp)   for j < nc       (doubles [d][ldgz], ldgz >= nc; required)
 *     gx[p][i] +=        Σ_j W_ij σ² dκ/dr² (+2 s_p)(u_ip − w_jp)   for i < nr       (NULL, or doubles [d][ldgx], ldgx >= nr)
 *   explicit_w = 1: W = cm.  rs, bv, nu, rowq, rowp are not read.
 *   explicit_w = 0: cm = −T̃ and W_ij = rs_i (2 T̃_ij + bv_i nu_j), formed in fp64;  rowq[i] += Σ_j σ² κ_ij T̃_ij,  rowp[i] += Σ_j σ² κ_ij nu_j  for i < nr when rowq is
 *                   non-NULL (rowq and rowp come together).  rs, bv: T, nr entries; nu: doubles, nc entries.
 *   cm    nr rows, leading dimension ldc >= nc rounded up to 128, aligned to two elements.  Used: cm[i][j], i < nr, j < nc.  Read, never used: columns [nc, round_up(nc, 128))
 *         of those rows (the 2-wide loads of the D <= 16 form).  D <= 16 and ldc even: vgrad_fast_kernel<T, 4|8|16, XG>; otherwise vgrad_kernel<T, 16, true, XG> once per
 *         16 dimensions (for D <= 16: the form production never takes).  XG = (gx != NULL).
 *   xr, xc  pre-scaled inputs, dimension-major [d][ldxr] / [d][ldxc], ldxr >= nr and ldxc >= nc rounded up to 128.  Columns beyond nr / nc up to that multiple: read by
 *           vgrad_kernel (D > 16, and D <= 16 with an odd ldc), never used.
 *   Everything is an atomic "+=" (rows / columns beyond nr / nc untouched).
 * Refused: cm (−2), ldc (−3), explicit_w (−4), xr / ldxr (−6), xc / ldxc (−8), d (−9), kernel (−10), rs / bv / nu missing (−11), nr / nc < 1 (−14), g NULL (−16),
 * gz / ldgz (−17), one of rowq / rowp (−20), ldgx (−23). */
int32_t gpd_vgrad(gp_ctx* ctx, const double* cm, int64_t ldc, int32_t explicit_w, const double* xr, int64_t ldxr, const double* xc, int64_t ldxc, int32_t d,
                  const gp_kernel* k, const double* rs, const double* bv, const double* nu, int64_t nr, int64_t nc, double* g, double* gz, int64_t ldgz, double zfac,
                  double* rowq_or_null, double* rowp_or_null, double* gx_or_null, int64_t ldgx);
int32_t gpd_vgrad_f32(gp_ctx* ctx, const float* cm, int64_t ldc, int32_t explicit_w, const float* xr, int64_t ldxr, const float* xc, int64_t ldxc, int32_t d,
                      const gp_kernel* k, const float* rs, const float* bv, const double* nu, int64_t nr, int64_t nc, double* g, double* gz, int64_t ldgz, double zfac,
                      double* rowq_or_null, double* rowp_or_null, double* gx_or_null, int64_t ldgx);
/* gpd_ystats: for every row r in [row_lo, row_lo + nrows) of y (row-major, ldy):   rowss[r] += Σ_{c<ncols} y[r][c]²,   cacc[r] −= Σ_{c<ncols} y[r][c] · b[c]
 *   (ystats_kernel, one workgroup per row; fp64 fused multiply-adds, a fixed order: bitwise repeatable).  Plain read-modify-write: other rows of cacc / rowss are not
 *   touched, columns >= ncols of y and b are not read.  y, b 16-byte aligned and every row of y 16-byte aligned (ldy a multiple of 2 doubles / 4 floats): the body
 *   moves 4 columns per thread as 16-byte loads, the last ncols % 4 columns one by one.
 * gpd_ystats_cols: the same for 16·sb columns of observations at once (ystats_cols_kernel<T, RT> on the fp64 MFMA):
 *     rowss[r] += Σ_c y[r][c]²,   cacc[s][r] −= Σ_c y[r][c] · by[s][c]   for s < 16·sb      (cacc: doubles [16·sb][ldc], ldc >= row_lo + nrows; by: T [16·sb][ldb])
 *   by rows of unused columns must be ZERO (they are multiplied like the others; their cacc rows then keep their values).  ncols a multiple of 16·(16 / sizeof(T)):
 *   32 doubles / 64 floats.  nrows a multiple of 16: 32 rows per workgroup (RT = 2, what the fit launches) when nrows is a multiple of 32, else 16 (RT = 1).  sb in 1..8.
 *   y and by 16-byte aligned with 16-byte rows.  No atomics: bitwise repeatable, and a column's bits do not depend on what the other columns of by hold.
 * Refused: y / ldy (−2), ncols (−4), b / by / ldb (−5), row_lo / nrows (−6; cols: −9), sb (−7), cacc / ldc (−8; cols: −10), rowss (−8; cols: −12). */
int32_t gpd_ystats(gp_ctx* ctx, const double* y, int64_t ldy, int64_t ncols, const double* b, int64_t row_lo, int64_t nrows, double* cacc, double* rowss);
int32_t gpd_ystats_f32(gp_ctx* ctx, const float* y, int64_t ldy, int64_t ncols, const float* b, int64_t row_lo, int64_t nrows, double* cacc, double* rowss);
int32_t gpd_ystats_cols(gp_ctx* ctx, const double* y, int64_t ldy, int64_t ncols, const double* by, int64_t ldb, int32_t sb, int64_t row_lo, int64_t nrows,
                        double* cacc, int64_t ldc, double* rowss);
int32_t gpd_ystats_cols_f32(gp_ctx* ctx, const float* y, int64_t ldy, int64_t ncols, const float* by, int64_t ldb, int32_t sb, int64_t row_lo, int64_t nrows,
                            double* cacc, int64_t ldc, double* rowss);
/* With parameter "time_kernels" = 1 every gpd_gemm_nt launch is bracketed by HIP events on the ctx
 * stream.  This synchronises the stream, returns the summed launch durations (ms) and the launch count since the
 * previous call, and clears the records (the caller knows the algorithmic flops of its own launches). */
int32_t gpd_gemm_time(gp_ctx* ctx, double* ms_out, int64_t* launches_out);

/* The multi-device transport's library on ONE device: dlopen (librccl, or the library GPMI_RCCL_LIB names), the seven entry points,
 * ncclCommInitAll(1) and one grouped ncclSend / ncclRecv pair of `count` doubles from the rank to itself, every element compared.
 * max_abs_err_out_or_null: largest |received − sent| (0 when the element type constant and the posting rules are what the driver
 * assumes).  −1996: the library is unavailable; −1998: an RCCL call failed (text in gp_last_error()). */
int32_t gp_rccl_selftest(int32_t device, int64_t count, double* max_abs_err_out_or_null);

/* ---- probes used by tools/gpu_diag.py and bench.py ------------------------------------------ */
/* D(16×16) = A(16×4)·B(4×16), all row-major host arrays: checks the f64 MFMA lane maps. */
int32_t gp_probe_mfma_f64(gp_ctx* ctx, const double* a_host, const double* b_host, double* d_host);
/* the same for fp32, through the traits every fp32 kernel uses (csrc/kcommon.hpp Tr<float>: v_mfma_f32_16x16x4_f32, row = 4·(lane>>4) + r). */
int32_t gp_probe_mfma_f32(gp_ctx* ctx, const float* a_host, const float* b_host, float* d_host);
/* measured TFLOP/s of back-to-back v_mfma_f64_16x16x4_f64 on all CUs (the roofline's measured ceiling). */
int32_t gp_bench_mfma_f64(gp_ctx* ctx, int32_t iters, double* tflops_out);
/* the same for fp32: variant 0 = v_mfma_f32_16x16x4_f32, 1 = v_mfma_f32_32x32x2_f32 (the C5 roofline's measured ceiling). */
int32_t gp_bench_mfma_f32(gp_ctx* ctx, int32_t variant, int32_t iters, double* tflops_out);

#ifdef __cplusplus
}
#endif
#endif /* GPMI355_H */
