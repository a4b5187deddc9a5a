"""GPU: the argument checks of the C ABI, one row per check.  Every row is an otherwise valid call through ctypes with exactly ONE argument broken; the library
refuses it during validation (nothing reaches the device) with −i for argument i and "invalid argument i: <reason>" in gp_last_error() (csrc/gpmi355.hip
set_arg_err).  The codes and texts are read off the source of the entry points; which error a call with TWO bad arguments reports is not part of the contract,
hence single faults only.

Checks asserted elsewhere, not repeated here: malformed gp_ksum descriptors (test_gpu_composite.py test_malformed_descriptors_are_refused_by_the_library),
misaligned base pointers of the gpd_*_f32 entry points (test_gpu_units_f32.py test_fp32_contracts_are_refused_with_a_reason), the gp_logpdf_batch arguments
(test_gpu_batch.py test_argument_errors_have_their_statuses_and_reasons), dead handles given to the *_free functions (test_abi.py).  Three checks need a handle
that this module's two fits do not give and have no row: gp_vfe_append on a handle without observations, gp_vfe_get_factors on a handle without factors, and
gp_vfe_grad's dz on an fp32 handle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, M = 8, 2, 4


@pytest.fixture(scope="module")
def env(agp):
    import torch

    L = agp._lib
    ctx = agp.default_context(0)
    lib = L.load()
    rng = np.random.default_rng(7)
    keep = []

    def arr(a):
        keep.append(a)
        return a

    def pts(a, n, d, layout):
        return L.gp_points(a.ctypes.data if a is not None else None, n, d, layout)

    dp = C.POINTER(C.c_double)
    X, X3, Z = arr(rng.uniform(0, 1, (N, D))), arr(rng.uniform(0, 1, (N, 3))), arr(rng.uniform(0, 1, (M, D)))
    y, diag, sc = arr(rng.normal(size=N)), arr(np.full(N, 0.1)), arr(np.array([1.0, 2.0]))
    S = arr(np.asfortranarray(0.1 * np.eye(N)))
    buf = arr(np.zeros(4 * N * N))         # every host output / right-hand side of the base calls fits in here
    fac = (L.gp_kfactor * 1)(L.gp_kfactor(0, 0, None, 0, None))
    terms = (L.gp_kterm * 2)(L.gp_kterm(1.0, 1, fac), L.gp_kterm(0.5, 1, fac))
    keep += [fac, terms]
    e = {
        "lib": lib, "h": ctx.handle, "buf": C.c_void_p(buf.ctypes.data), "y": C.c_void_p(y.ctypes.data), "dbl": (C.c_double * 4)(), "i64": C.c_int64(),
        "tm": L.gp_timings(), "new": C.c_void_p(), "name": b"nb", "i32": C.c_int32(),
        "px": pts(X, N, D, 1), "pz": pts(Z, M, D, 1), "kk": L.gp_kernel(0, 0, 1.5, D, sc.ctypes.data_as(dp)), "nz": L.gp_noise(0, 0.1, None),
        "ks": L.gp_ksum(0, 2, terms),
        # the faults
        "px_null": pts(None, N, D, 1), "px_n0": pts(X, 0, D, 1), "px_d0": pts(X, N, 0, 1), "px_layout3": pts(X, N, D, 3), "px_vec_d2": pts(X, N, D, 0),
        "px_d3": pts(X3, N, 3, 1), "kk_kind4": L.gp_kernel(4, 0, 1.5, D, sc.ctypes.data_as(dp)), "kk_dtype2": L.gp_kernel(0, 2, 1.5, D, sc.ctypes.data_as(dp)),
        "kk_var0": L.gp_kernel(0, 0, 0.0, D, sc.ctypes.data_as(dp)), "kk_scale_null": L.gp_kernel(0, 0, 1.5, D, None),
        "ks_dtype2": L.gp_ksum(2, 2, terms), "ks_terms_null": L.gp_ksum(0, 2, None),
        "nz_kind4": L.gp_noise(4, 0.1, diag.ctypes.data), "nz_diag_null": L.gp_noise(1, 0.0, None), "nz_dense_null": L.gp_noise(2, 0.0, None),
        "nz_dense": L.gp_noise(2, 0.0, S.ctypes.data),
    }
    # the two valid handles: one exact fit (n = 8, d = 2, fp64), one VFE fit (n = 8, m = 4)
    post, vfe = C.c_void_p(), C.c_void_p()
    assert lib.gp_posterior_fit(e["h"], C.byref(e["kk"]), C.byref(e["px"]), C.byref(e["nz"]), None, e["y"], C.byref(post), None, None) == 0
    assert lib.gp_vfe_fit(e["h"], C.byref(e["kk"]), C.byref(e["px"]), C.byref(e["pz"]), C.byref(e["nz"]), 1e-6, None, e["y"], 0, C.byref(vfe), None) == 0
    e["post"], e["vfe"] = post, vfe
    # device buffers of the gpd_* rows: real allocations of a legal size, so that nothing in a row but the named argument is wrong
    A64, A32 = torch.zeros(256 + 128, 288, dtype=torch.float64, device="cuda"), torch.zeros(256 + 128, 288, dtype=torch.float32, device="cuda")
    keep += [A64, A32]
    e.update(A64=C.c_void_p(A64.data_ptr()), A32=C.c_void_p(A32.data_ptr()), k32=L.gp_kernel(0, 1, 1.5, 0, None), k64=L.gp_kernel(0, 0, 1.5, 0, None),
             k64_kind4=L.gp_kernel(4, 0, 1.5, 0, None), grid=L.gp_grid(1, 0, 1, 0, 1, 0), ks32=L.gp_ksum(1, 2, terms),
             A64_off8=C.c_void_p(A64.data_ptr() + 8), A32_off8=C.c_void_p(A32.data_ptr() + 8))
    yield e
    assert lib.gp_posterior_free(post) == 0 and lib.gp_vfe_free(vfe) == 0
    del keep


# entry point -> its valid call ("@name": the address of env[name], "name": env[name] itself, anything else literal); argument i is element i − 1
FIT = ["h", "@kk", "@px", "@nz", None]
FIT_SUM = ["h", "@ks", "@px", "@nz", None]
GPD = lambda A, k: {  # noqa: E731  (fp64 / fp32 twins share their argument lists)
    "assemble": ["h", k, A, 200, 256, 3, A, "@grid", A, 288, 256, 256], "potrf": ["h", A, 288, 256, 256, None, 0, 256, None],
    "trsm": ["h", A, 288, 128, A, 288, 128], "gemm_nt": ["h", A, 288, A, 288, A, 288, 128, 128, 32, None, 0, 0], "trsv": ["h", A, 288, 256, A, 256, 1, 1],
    "gemv_t": ["h", A, 288, 128, 128, A, A], "rowsumsq": ["h", A, 288, 128, 128, A]}
GPD_GRAD = lambda A, k: {  # noqa: E731  (the gradient contractions and the sparse reductions: n = 200 of np = 256 points, D = 3; a 200 × 100 rectangle; 4 rows of 100
    # columns; 16 rows of 128 columns.  A dict of their own, and their rows at the END of TABLE: the ids of the earlier rows carry their position)
    "grad_contract": ["h", k, A, 288, A, A, 200, 256, 3, A, A, None],
    "vgrad": ["h", A, 288, 1, A, 256, A, 256, 3, k, None, None, None, 200, 100, A, A, 256, 1.0, None, None, None, 0],
    "ystats": ["h", A, 288, 100, A, 0, 4, A, A], "ystats_cols": ["h", A, 288, 128, A, 288, 1, 0, 16, A, 288, A]}
BASE = {
    "gp_ctx_create": ["@new", 0, None], "gp_ctx_set_param": ["h", "name", -1], "gp_ctx_get_param": ["h", "name", "@i64"], "gp_ctx_trim": ["h"],
    "gp_get_timings": ["h", "@tm"],
    "gp_kernelmatrix": ["h", "@kk", "@px", "@px", "buf"], "gp_kernelmatrix_sum": ["h", "@ks", "@px", "@px", "buf"],
    "gp_logpdf": FIT + ["y", N, 1, "buf"], "gp_logpdf_sum": FIT_SUM + ["y", N, 1, "buf"], "gp_logpdf_terms": FIT + ["y", N, 1, "buf", "buf"],
    "gp_posterior_fit": FIT + ["y", "@new", None, None], "gp_posterior_fit_sum": FIT_SUM + ["y", "@new", None, None],
    "gp_logpdf_grad": FIT + ["y", "buf", None, None, None, None, None], "gp_logpdf_grad_sum": FIT_SUM + ["y", "buf", None, None, None],
    "gp_logpdf_batch": ["h", 1, "@kk", 1, "@px", "@nz", None, 1, "@y", "buf", "@i32", None],
    "gp_posterior_logdet": ["post", "dbl"], "gp_posterior_predict": ["post", "@px", None, 3, "buf", "buf", None],
    "gp_posterior_update": ["post", "@px", "@nz", "buf", "@new", None, None], "gp_posterior_factor_mul": ["post", "buf", 1, "buf"],
    "gp_posterior_solve": ["post", "buf", 1, "buf"], "gp_posterior_get_factor": ["post", "buf"], "gp_posterior_n": ["post"],
    "gp_posterior_logpdf": ["post", "@px", None, "@nz", "y", N, 1, "buf"], "gp_posterior_rand": ["post", "@px", None, "@nz", "buf", 1, "buf"],
    "gp_vfe_fit": ["h", "@kk", "@px", "@pz", "@nz", 1e-6, None, "y", 0, "@new", None],
    "gp_vfe_update": ["vfe", "@px", "@nz", None, "y", "@new", None], "gp_vfe_append": ["vfe", "@pz", "@new", None],
    "gp_vfe_predict": ["vfe", "@px", None, 3, "buf", "buf", None], "gp_vfe_logpdf": ["vfe", "@px", None, "@nz", "y", N, 1, "buf"],
    "gp_vfe_rand": ["vfe", "@px", None, "@nz", "buf", 1, "buf"], "gp_vfe_get": ["vfe", "buf", None], "gp_vfe_get_factors": ["vfe", "buf", None],
    "gp_vfe_get_by": ["vfe", "buf"], "gp_vfe_n": ["vfe"], "gp_vfe_m": ["vfe"],
    "gp_vfe_grad": ["vfe", "dbl", None, None, None, None, "buf", 1, "buf", 1],
    "gp_probe_mfma_f64": ["h", "buf", "buf", "buf"], "gp_probe_mfma_f32": ["h", "buf", "buf", "buf"], "gp_bench_mfma_f64": ["h", 1, "dbl"],
    "gp_bench_mfma_f32": ["h", 0, 1, "dbl"],
    "gpd_inv_lower": ["h", "A64", 288, 64, "A64", 288, "A64", None], "gpd_trsm_inv": ["h", "A64", 288, 128, "A64", 288, 64, "A64", 288],
    "gpd_gemm_time": ["h", "dbl", "@i64"], "gpd_sync": ["h"],
    **{f"gpd_{n}": a for n, a in GPD("A64", "@k64").items()}, **{f"gpd_{n}_f32": a for n, a in GPD("A32", "@k32").items()},
    **{f"gpd_{n}": a for n, a in GPD_GRAD("A64", "@k64").items()}, **{f"gpd_{n}_f32": a for n, a in GPD_GRAD("A32", "@k32").items()},
    "gpd_grad_contract_sum": GPD_GRAD("A64", "@ks")["grad_contract"], "gpd_grad_contract_sum_f32": GPD_GRAD("A32", "@ks32")["grad_contract"],
}

CTX, POST, VFE = "not a live gp_ctx", "not a live gp_post", "not a live gp_vfe"
POINTS = [("@px_null", "points NULL"), ("@px_n0", "n must be > 0"), ("@px_d0", "d must be > 0"), ("@px_layout3", "layout must be 0..2"),
          ("@px_vec_d2", "layout 0 requires d == 1")]
KERNEL = [(None, "kernel is NULL"), ("@kk_kind4", "kernel kind must be 0..3"), ("@kk_dtype2", "dtype must be 0 (f64) or 1 (f32)"),
          ("@kk_var0", "variance must be > 0"), ("@kk_scale_null", "scale is NULL")]
NOISE = [(None, "noise is NULL"), ("@nz_kind4", "noise kind must be 0 (scalar), 1 (diagonal), 2 or 3"), ("@nz_diag_null", "noise diag is NULL"),
         ("@nz_dense_null", "noise diag (the dense matrix) is NULL")]
DENSE = "dense noise (kind 2 / 3) is not offered for VFE / DTC fits"
WHAT = "what must be a combination of 1|2|4"

# (entry point, argument that is broken (1-based), its broken value, expected return code, expected text)
TABLE = [
    ("gp_ctx_create", 1, None, -1, "out is NULL"), ("gp_ctx_create", 2, -1, -2, "no such device"),
    ("gp_ctx_set_param", 2, None, -2, "name is NULL"), ("gp_ctx_set_param", 2, b"no_such_knob", -2, "unknown parameter"),
    ("gp_ctx_set_param", 2, b"lookahead_depth", -2, "multi-device parameter on a single-device ctx"),
    ("gp_ctx_get_param", 2, None, -2, "name is NULL"), ("gp_ctx_get_param", 3, None, -3, "out is NULL"), ("gp_ctx_get_param", 2, b"no_such_knob", -2, "unknown parameter"),
    ("gp_get_timings", 2, None, -2, "out is NULL"),
    # a NULL / never-issued ctx at every entry point that takes one
    *[(fn, 1, bad, -1, CTX) for fn in ["gp_ctx_set_param", "gp_ctx_get_param", "gp_ctx_trim", "gp_get_timings", "gp_kernelmatrix", "gp_kernelmatrix_sum", "gp_logpdf",
                                       "gp_logpdf_sum", "gp_logpdf_terms", "gp_posterior_fit", "gp_posterior_fit_sum", "gp_logpdf_grad", "gp_logpdf_grad_sum",
                                       "gp_logpdf_batch", "gp_vfe_fit", "gp_probe_mfma_f64", "gp_probe_mfma_f32", "gp_bench_mfma_f64", "gp_bench_mfma_f32",
                                       "gpd_inv_lower", "gpd_trsm_inv", "gpd_gemm_time", "gpd_sync", *[f"gpd_{n}{s}" for n in GPD(0, 0) for s in ("", "_f32")]]
      for bad in (None, 0xDEADBEEF)],
    *[(fn, 1, bad, -1, POST) for fn in ["gp_posterior_logdet", "gp_posterior_predict", "gp_posterior_update", "gp_posterior_factor_mul", "gp_posterior_solve",
                                        "gp_posterior_get_factor", "gp_posterior_logpdf", "gp_posterior_rand"] for bad in (None, 0xDEADBEEF)],
    *[(fn, 1, bad, -1, VFE) for fn in ["gp_vfe_update", "gp_vfe_append", "gp_vfe_predict", "gp_vfe_logpdf", "gp_vfe_rand", "gp_vfe_get", "gp_vfe_get_factors",
                                       "gp_vfe_get_by", "gp_vfe_grad"] for bad in (None, 0xDEADBEEF)],
    *[(fn, 1, None, -1, None) for fn in ["gp_posterior_n", "gp_vfe_n", "gp_vfe_m"]],   # int64 getters: −1, no text
    # points / kernel / noise descriptors at each position they are checked at
    *[("gp_kernelmatrix", 3, v, -3, t) for v, t in POINTS], *[("gp_kernelmatrix", 4, v, -4, t) for v, t in POINTS],
    *[("gp_kernelmatrix", 2, v, -2, t) for v, t in KERNEL], ("gp_kernelmatrix", 3, "@px_d3", -2, "nscale must be 0, 1 or D"),
    ("gp_kernelmatrix", 4, "@px_d3", -4, "x and y have different D"), ("gp_kernelmatrix", 5, None, -5, "out is NULL"),
    ("gp_kernelmatrix_sum", 3, "@px_layout3", -3, "layout must be 0..2"), ("gp_kernelmatrix_sum", 2, None, -2, "kernel is NULL"),
    ("gp_kernelmatrix_sum", 2, "@ks_dtype2", -2, "dtype must be 0 (f64) or 1 (f32)"), ("gp_kernelmatrix_sum", 2, "@ks_terms_null", -2, "composite kernel: terms is NULL"),
    ("gp_kernelmatrix_sum", 4, "@px_n0", -4, "n must be > 0"), ("gp_kernelmatrix_sum", 4, "@px_d3", -4, "x and y have different D"),
    ("gp_kernelmatrix_sum", 5, None, -5, "out is NULL"),
    *[(fn, 3, "@px_layout3", -3, "layout must be 0..2") for fn in ["gp_logpdf", "gp_logpdf_sum", "gp_logpdf_terms", "gp_posterior_fit", "gp_posterior_fit_sum",
                                                                   "gp_logpdf_grad", "gp_logpdf_grad_sum", "gp_vfe_fit"]],
    *[(fn, 2, "@kk_kind4", -2, "kernel kind must be 0..3") for fn in ["gp_logpdf", "gp_logpdf_terms", "gp_posterior_fit", "gp_logpdf_grad", "gp_vfe_fit"]],
    *[(fn, 3, "@px_d3", -2, "nscale must be 0, 1 or D") for fn in ["gp_logpdf", "gp_posterior_fit"]],
    *[(fn, 2, "@ks_terms_null", -2, "composite kernel: terms is NULL") for fn in ["gp_logpdf_sum", "gp_posterior_fit_sum", "gp_logpdf_grad_sum"]],
    *[("gp_logpdf", 4, v, -4, t) for v, t in NOISE],
    *[(fn, 4, "@nz_kind4", -4, NOISE[1][1]) for fn in ["gp_logpdf_sum", "gp_logpdf_terms", "gp_posterior_fit", "gp_posterior_fit_sum", "gp_logpdf_grad",
                                                       "gp_logpdf_grad_sum", "gp_posterior_logpdf", "gp_posterior_rand", "gp_vfe_logpdf", "gp_vfe_rand"]],
    # exact fits
    ("gp_logpdf", 6, None, -6, "Y is NULL"), ("gp_logpdf", 8, 0, -8, "ncols must be >= 1"), ("gp_logpdf", 7, N - 1, -7, "ldy < n"), ("gp_logpdf", 9, None, -9, "out is NULL"),
    ("gp_logpdf_sum", 6, None, -6, "Y is NULL"), ("gp_logpdf_sum", 8, 0, -8, "ncols must be >= 1"), ("gp_logpdf_sum", 7, N - 1, -7, "ldy < n"),
    ("gp_logpdf_sum", 9, None, -9, "out is NULL"),
    ("gp_logpdf_terms", 8, 0, -8, "ncols must be >= 1"), ("gp_logpdf_terms", 7, N - 1, -7, "ldy < n"), ("gp_logpdf_terms", 6, None, -6, "sqmahal needs Y"),
    *[(fn, 6, None, -6, "y is NULL") for fn in ["gp_posterior_fit", "gp_posterior_fit_sum", "gp_logpdf_grad", "gp_logpdf_grad_sum"]],
    *[(fn, 7, None, -7, "out is NULL") for fn in ["gp_posterior_fit", "gp_posterior_fit_sum"]],
    *[(fn, 7, None, -7, "logpdf_out is NULL") for fn in ["gp_logpdf_grad", "gp_logpdf_grad_sum"]],
    # the exact posterior
    ("gp_posterior_logdet", 2, None, -2, "out is NULL"),
    *[(fn, 2, "@px_layout3", -2, "layout must be 0..2") for fn in ["gp_posterior_predict", "gp_posterior_update", "gp_posterior_logpdf", "gp_posterior_rand",
                                                                   "gp_vfe_update", "gp_vfe_append", "gp_vfe_predict", "gp_vfe_logpdf", "gp_vfe_rand"]],
    *[(fn, 2, "@px_d3", -2, "xs has a different D than the training inputs") for fn in ["gp_posterior_predict", "gp_posterior_logpdf", "gp_posterior_rand",
                                                                                        "gp_vfe_predict", "gp_vfe_logpdf", "gp_vfe_rand"]],
    *[(fn, 2, "@px_d3", -2, "x2 has a different D than the training inputs") for fn in ["gp_posterior_update", "gp_vfe_update"]],
    *[(fn, 4, w, -4, WHAT) for fn in ["gp_posterior_predict", "gp_vfe_predict"] for w in (0, 8)],
    *[(fn, 5, None, -5, "mean_out is NULL") for fn in ["gp_posterior_predict", "gp_vfe_predict"]],
    *[(fn, 6, None, -6, "var_out is NULL") for fn in ["gp_posterior_predict", "gp_vfe_predict"]],
    *[(fn, 4, 4, -7, "cov_out is NULL") for fn in ["gp_posterior_predict", "gp_vfe_predict"]],   # what = 4 asks for the covariance the base call leaves NULL
    *[("gp_posterior_update", 3, v, -3, t) for v, t in NOISE],
    ("gp_posterior_update", 4, None, -4, "delta_all is NULL"), ("gp_posterior_update", 5, None, -5, "out is NULL"),
    *[(fn, 2, None, -2, t) for fn, t in [("gp_posterior_factor_mul", "xi is NULL"), ("gp_posterior_solve", "B is NULL"), ("gp_posterior_get_factor", "U_out is NULL")]],
    *[(fn, 3, 0, -3, "ncols must be >= 1") for fn in ["gp_posterior_factor_mul", "gp_posterior_solve"]],
    *[(fn, 4, None, -4, "out is NULL") for fn in ["gp_posterior_factor_mul", "gp_posterior_solve"]],
    *[(fn, 5, None, -5, "Y is NULL") for fn in ["gp_posterior_logpdf", "gp_vfe_logpdf"]], *[(fn, 6, N - 1, -6, "ldy < n") for fn in ["gp_posterior_logpdf", "gp_vfe_logpdf"]],
    *[(fn, 7, 0, -7, "ncols must be >= 1") for fn in ["gp_posterior_logpdf", "gp_vfe_logpdf"]],
    *[(fn, 8, None, -8, "out is NULL") for fn in ["gp_posterior_logpdf", "gp_vfe_logpdf"]],
    *[(fn, 5, None, -5, "xi is NULL") for fn in ["gp_posterior_rand", "gp_vfe_rand"]], *[(fn, 6, 0, -6, "ncols must be >= 1") for fn in ["gp_posterior_rand", "gp_vfe_rand"]],
    *[(fn, 7, None, -7, "out is NULL") for fn in ["gp_posterior_rand", "gp_vfe_rand"]],
    # VFE / DTC (gp_vfe_fit reports its noise as argument 4, the position it has in the exact fits)
    ("gp_vfe_fit", 5, "@nz_dense", -4, DENSE), ("gp_vfe_fit", 5, "@nz_kind4", -4, NOISE[1][1]), ("gp_vfe_fit", 4, "@px_n0", -4, "n must be > 0"),
    ("gp_vfe_fit", 4, "@px_d3", -4, "z has a different D than x"), ("gp_vfe_fit", 6, -1.0, -6, "jitter must be >= 0"), ("gp_vfe_fit", 8, None, -8, "y is NULL"),
    ("gp_vfe_fit", 9, 2, -9, "approx must be 0 (VFE) or 1 (DTC)"),
    ("gp_vfe_update", 3, "@nz_dense", -3, DENSE), ("gp_vfe_update", 3, None, -3, "noise is NULL"), ("gp_vfe_update", 5, None, -5, "y2 is NULL"),
    ("gp_vfe_update", 6, None, -6, "out is NULL"), ("gp_vfe_append", 2, "@px_d3", -2, "z2 has a different D than the pseudo-points"),
    ("gp_vfe_append", 3, None, -3, "out is NULL"), ("gp_vfe_get_by", 2, None, -2, "b_y_out is NULL"),
    ("gp_vfe_grad", 8, 3, -8, "z_layout must be 0 (vector, D = 1), 1 (ColVecs) or 2 (RowVecs)"), ("gp_vfe_grad", 8, 0, -8, "z_layout must be 0"),
    ("gp_vfe_grad", 10, 3, -10, "x_layout must be 0 (vector, D = 1), 1 (ColVecs) or 2 (RowVecs)"),
    # device-level building blocks: sizes and leading dimensions
    *[(f"gpd_assemble{s}", 2, v, -2, t) for s in ("", "_f32") for v, t in [(None, "kernel is NULL"), ("@k64_kind4", "kernel kind must be 0..3")]],
    *[(f"gpd_assemble{s}", 11, 96, -11, "m_loc, n_loc must be multiples of 128") for s in ("", "_f32")],
    ("gpd_assemble_f32", 10, 287, -10, "lda must be even and >= n_loc"), ("gpd_assemble_f32", 10, 254, -10, "lda must be even and >= n_loc"),
    *[(f"gpd_potrf{s}", 4, 96, -4, "m, n must be multiples of 64 with m >= n") for s in ("", "_f32")], ("gpd_potrf", 4, 192, -4, "with m >= n"),
    ("gpd_potrf", 3, 287, -3, "lda must be even and >= n"), ("gpd_potrf", 3, 254, -3, "lda must be even and >= n"),
    ("gpd_potrf_f32", 3, 286, -3, "lda must be a multiple of 4 and >= n"),
    *[(f"gpd_trsm{s}", 4, 96, -4, "m, n must be multiples of 64") for s in ("", "_f32")],
    ("gpd_trsm_f32", 3, 286, -2, "x must be 16-byte aligned and ldx a multiple of 4"), ("gpd_trsm_f32", 6, 286, -5, "l must be 16-byte aligned and ldl a multiple of 4"),
    ("gpd_gemm_nt", 8, 96, -8, "m, n multiples of 64 and k multiple of 16 required"), ("gpd_gemm_nt", 10, 8, -8, "k multiple of 16"),
    ("gpd_gemm_nt_f32", 8, 96, -8, "m, n multiples of 64 and k multiple of 32 required"), ("gpd_gemm_nt_f32", 10, 16, -8, "k multiple of 32"),
    ("gpd_gemm_nt_f32", 5, 286, -4, "a must be 16-byte aligned and lda a multiple of 4"), ("gpd_gemm_nt_f32", 7, 286, -6, "b must be 16-byte aligned and ldb a multiple of 4"),
    *[(f"gpd_trsv{s}", 4, 96, -4, "np must be a multiple of 128") for s in ("", "_f32")],
    ("gpd_trsv_f32", 3, 286, -2, "l must be 16-byte aligned and ldl a multiple of 4"),
    ("gpd_inv_lower", 4, 32, -4, "nb must be a multiple of 64"), ("gpd_inv_lower", 4, 96, -4, "nb must be a multiple of 64"),
    *[("gpd_inv_lower", i, None, -2, "l / w / scratch1 is NULL") for i in (2, 5, 7)],
    ("gpd_trsm_inv", 4, 96, -3, "m, nb must be multiples of 64"), ("gpd_trsm_inv", 7, 32, -3, "m, nb must be multiples of 64"),
    # the gradient contractions and the sparse reductions (include/gpmi355.h lists each entry's refusals): a NULL / never-issued ctx, then the arguments
    *[(fn, 1, bad, -1, CTX) for fn in [*[f"gpd_{n}{s}" for n in GPD_GRAD(0, 0) for s in ("", "_f32")], "gpd_grad_contract_sum", "gpd_grad_contract_sum_f32"]
      for bad in (None, 0xDEADBEEF)],
    *[(f"gpd_grad_contract{s}", 8, 200, -8, "np must be a positive multiple of 128") for s in ("", "_f32", "_sum", "_sum_f32")],
    ("gpd_grad_contract", 3, "A64_off8", -3, "ci must be non-NULL and 16-byte aligned"), ("gpd_grad_contract_f32", 3, "A32_off8", -3, "16-byte aligned"),
    ("gpd_grad_contract", 7, 257, -7, "n must be in 1..np"), ("gpd_grad_contract_f32", 4, 255, -4, "ld must be >= np"),
    ("gpd_grad_contract", 2, "@kk", -2, "nscale must be 0, 1 or D"), ("gpd_grad_contract", 2, "@k32", -2, "kernel dtype does not match"),
    ("gpd_grad_contract_sum", 9, 17, -2, "composite kernel: D must be <= 16"), ("gpd_grad_contract_sum_f32", 2, "@ks", -2, "kernel dtype does not match"),
    ("gpd_grad_contract_sum", 2, None, -2, "kernel is NULL"), ("gpd_grad_contract", 10, None, -10, "g is NULL"),
    *[(f"gpd_vgrad{s}", 9, 0, -9, "d must be >= 1") for s in ("", "_f32")], ("gpd_vgrad_f32", 3, 100, -3, "ldc must be >= nc rounded up to 128"),
    ("gpd_vgrad", 10, "@kk", -10, "nscale must be 0, 1 or D"), ("gpd_vgrad", 4, 0, -11, "rs, bv and nu are needed with explicit_w = 0"),
    ("gpd_vgrad", 2, "A64_off8", -2, "aligned to two elements"), ("gpd_vgrad", 17, None, -17, "gz is NULL or ldgz < nc"), ("gpd_vgrad_f32", 20, "A32", -20, "come together"),
    ("gpd_ystats", 3, 287, -2, "16-byte rows"), ("gpd_ystats_f32", 5, None, -5, "b must be non-NULL and 16-byte aligned"), ("gpd_ystats_f32", 3, 286, -2, "16-byte rows"),
    ("gpd_ystats_cols", 7, 9, -7, "sb must be 1..8"), ("gpd_ystats_cols_f32", 7, 0, -7, "sb must be 1..8"), ("gpd_ystats_cols", 9, 8, -9, "nrows a multiple of 16"),
    ("gpd_ystats_cols_f32", 4, 32, -4, "ncols must be a positive multiple"), ("gpd_ystats_cols", 4, 48, -4, "ncols must be a positive multiple"),
    ("gpd_ystats_cols", 11, 8, -10, "cacc is NULL or ldc < row_lo + nrows"),
]


def _value(e, v):
    if isinstance(v, str):
        return C.byref(e[v[1:]]) if v.startswith("@") else e[v]
    return v


@pytest.mark.parametrize("fn,argi,bad,rc,text", TABLE, ids=[f"{i:03d}-{r[0]}-arg{r[1]}" for i, r in enumerate(TABLE)])
def test_one_broken_argument_is_refused_with_its_code_and_reason(env, fn, argi, bad, rc, text):
    lib = env["lib"]
    args = [_value(env, v) for v in BASE[fn]]
    args[argi - 1] = _value(env, bad)
    env["new"].value = None
    assert lib.gp_ctx_set_param(env["h"], b"lookahead_depth", 0) == -2   # leaves a known text behind: a stale reason cannot satisfy the row
    got = getattr(lib, fn)(*args)
    why = lib.gp_last_error().decode()
    assert got == rc, (got, why)
    if text is not None:
        assert why.startswith(f"invalid argument {-rc}: ") and text in why, why
    assert not env["new"].value                                # no handle was handed out
