"""gp_posterior_predict_grad / gp_vfe_predict_grad against the predict call on the SAME handle, in one process (issue: gradients of the predictive mean
and variance w.r.t. the test inputs).

Exact: a fit at the C2 inputs (N = 16 384, D = 3, SE, σ² = 0.01, fp64; --c4 adds N = 65 536), 4 096 test points.  Sparse: VFE at N = 262 144, M = 4 096.
Per handle, at the C ABI with the arguments marshalled beforehand, `repeats` (5) ALTERNATING samples of
    predict        gp_*_predict(what = 3)                      mean + variance: Gram, forward solve
    predict_grad   gp_*_predict_grad(what = 3)                 + backward solve, + the fused contraction kernel
after one warm-up of each (the first call builds the inverse diagonal blocks).  Every call ends in a stream synchronise inside the library, so the host
clock around it is its whole cost.  The ratio of the medians is the headline (PREDICT_GRAD_RATIO): a second solve of the same flops predicts ≈ 2.
Phases, from further calls on the same handle (medians, by difference; the per-kernel split of the backward phase is the rocprofv3 --kernel-trace run):
    mean_side        predict_grad(what = 1): kvec + kpgrad with α only — no Gram, no solve
    gram_forward     predict_grad(what = 2, dvar = NULL): Gram + forward solve + rowsumsq
    backward_kernel  predict_grad(what = 2) − gram_forward: the backward solve (transposes + GEMMs) + kpgrad with the weight rows
Event times of the solves' GEMM launches, from one further pass with the ctx parameter "time_kernels" = 1 (an event pair around every MFMA GEMM launch, read
back with gpd_gemm_time; the launches between them — Gram, transposes, panel copies, rowsumsq, kpgrad — are what remains of the call):
    forward_solve_gemm_ms    the GEMMs of a gram_forward call                      (the forward solve)
    backward_solve_gemm_ms   the GEMMs of a variance_side call minus those         (the backward solve)
--small-n N (default 1920; 0: skip) adds an exact handle BELOW "dib_nb" padded points on the default context: no inverse blocks, so the backward solve is the
row-by-row back-substitution — serial in the test points; its ratio is reported as `substitution` and is NOT near 2.
One JSON object to stdout and to --out.

    python tools/predict_grad_profile.py [--n 16384] [--ns 4096] [--repeats 5] [--c4] [--vfe-n 262144] [--vfe-m 4096] [--no-vfe] [--small-n 1920] [--out FILE]"""
import argparse
import ctypes as C
import json
import socket
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _med(v):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def profile_handle(agp, lib, predict, predict_grad, handle, Xs, repeats, ctx=None):
    m = agp.api._Marshal(np.float64)
    px = m.points(agp.RowVecs(Xs))
    ns, d = Xs.shape
    mean, var, dm, dv = np.empty(ns), np.empty(ns), np.empty((ns, d)), np.empty((ns, d))
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731

    def call(fn, what, *outs):
        rc = fn(handle, C.byref(px), None, what, *[P(o) for o in outs])
        if rc != 0:
            raise RuntimeError(f"status {rc}: {lib.gp_last_error().decode()}")

    calls = {
        "predict": lambda: call(predict, 3, mean, var, None),
        "predict_grad": lambda: call(predict_grad, 3, mean, var, dm, dv),
        "mean_side": lambda: call(predict_grad, 1, mean, None, dm, None),
        "gram_forward": lambda: call(predict_grad, 2, None, var, None, None),
        "variance_side": lambda: call(predict_grad, 2, None, var, None, dv),
    }
    for f in calls.values():
        f()
    m0, v0 = mean.copy(), var.copy()
    calls["predict"]()
    assert np.allclose(mean, m0, rtol=1e-10, atol=1e-12) and np.allclose(var, v0, rtol=1e-8, atol=1e-12), "predict and predict_grad disagree on the values"
    t = {k: [] for k in calls}
    for _ in range(repeats):  # alternating: every sample of one call has a sample of every other call next to it
        for k, f in calls.items():
            t[k].append(_timed(f))
    out = {k: _med(v) for k, v in t.items()}
    out["backward_kernel"] = {"ms": round(out["variance_side"]["ms"] - out["gram_forward"]["ms"], 4)}
    out["ratio"] = round(out["predict_grad"]["ms"] / out["predict"]["ms"], 3)
    out["samples"] = {k: [round(x, 4) for x in v] for k, v in t.items() if k in ("predict", "predict_grad")}
    if ctx is not None:  # event times of the GEMM launches of the two solves
        ms, cnt = C.c_double(), C.c_int64()
        ctx.set_param("time_kernels", 1)
        try:
            g = {}
            for k in ("gram_forward", "variance_side"):
                calls[k]()
                if lib.gpd_gemm_time(ctx.handle, C.byref(ms), C.byref(cnt)) != 0:
                    raise RuntimeError(lib.gp_last_error().decode())
                g[k] = (ms.value, cnt.value)
        finally:
            ctx.set_param("time_kernels", 0)
        out["forward_solve_gemm_ms"] = round(g["gram_forward"][0], 4)
        out["forward_solve_gemm_launches"] = g["gram_forward"][1]
        out["backward_solve_gemm_ms"] = round(g["variance_side"][0] - g["gram_forward"][0], 4)
        out["backward_solve_gemm_launches"] = g["variance_side"][1] - g["gram_forward"][1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--ns", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--c4", action="store_true")
    ap.add_argument("--vfe-n", type=int, default=262144)
    ap.add_argument("--vfe-m", type=int, default=4096)
    ap.add_argument("--no-vfe", action="store_true")
    ap.add_argument("--small-n", type=int, default=1920)
    ap.add_argument("--exact-only-once", action="store_true", help="one predict_grad call on the exact handle and nothing else (the run a kernel trace wraps)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import abstractgps_jl_amd as agp
    from oracle.gp_oracle import synth_inputs

    lib = agp._lib.load()
    res = {"host": socket.gethostname(), "ns": a.ns, "repeats": a.repeats, "exact": [], "sparse": None}
    for name, n, seed in [("C2", a.n, 2)] + ([("C4", 65536, 4)] if a.c4 else []):
        x, y = synth_inputs(n, 3, seed)
        Xs = np.random.default_rng(seed + 100).uniform(x.min(0), x.max(0), size=(a.ns, 3))
        post = agp.posterior(agp.GP(agp.SqExponentialKernel())(agp.RowVecs(x), 0.01), y)
        if a.exact_only_once:
            post.mean_and_var_grad(agp.RowVecs(Xs))
            post.mean_and_var_grad(agp.RowVecs(Xs))
            print("PREDICT_GRAD_TRACE_DONE")
            return
        r = profile_handle(agp, lib, lib.gp_posterior_predict, lib.gp_posterior_predict_grad, post.data.C.handle, Xs, a.repeats, post.data.C.ctx)
        r.update(config=name, n=n, d=3)
        res["exact"].append(r)
        print(f"PREDICT_GRAD_RATIO {name} n={n} ns={a.ns}: predict {r['predict']['ms']} ms, predict_grad {r['predict_grad']['ms']} ms, ratio {r['ratio']}", flush=True)
        del post
    if a.small_n > 0:
        x, y = synth_inputs(a.small_n, 3, 8)
        Xs = np.random.default_rng(108).uniform(x.min(0), x.max(0), size=(a.ns, 3))
        post = agp.posterior(agp.GP(agp.SqExponentialKernel())(agp.RowVecs(x), 0.01), y)
        r = profile_handle(agp, lib, lib.gp_posterior_predict, lib.gp_posterior_predict_grad, post.data.C.handle, Xs, min(a.repeats, 3))
        r.update(config="substitution", n=a.small_n, d=3)
        res["substitution"] = r
        print(f"PREDICT_GRAD_RATIO substitution path n={a.small_n} ns={a.ns}: predict {r['predict']['ms']} ms, predict_grad {r['predict_grad']['ms']} ms, "
              f"ratio {r['ratio']}", flush=True)
        del post
    if not a.no_vfe:
        x, y = synth_inputs(a.vfe_n, 3, 6)
        rng = np.random.default_rng(7)
        z = x[rng.choice(a.vfe_n, a.vfe_m, replace=False)] + 0.01 * rng.standard_normal((a.vfe_m, 3))
        Xs = rng.uniform(x.min(0), x.max(0), size=(a.ns, 3))
        f = agp.GP(agp.SqExponentialKernel())
        vp = agp.posterior(agp.VFE(f(agp.RowVecs(z), 1e-6)), f(agp.RowVecs(x), 0.01), y)
        r = profile_handle(agp, lib, lib.gp_vfe_predict, lib.gp_vfe_predict_grad, vp._state.handle, Xs, a.repeats, vp._state.ctx)
        r.update(config="VFE", n=a.vfe_n, m=a.vfe_m, d=3)
        res["sparse"] = r
        print(f"PREDICT_GRAD_RATIO VFE n={a.vfe_n} m={a.vfe_m} ns={a.ns}: predict {r['predict']['ms']} ms, predict_grad {r['predict_grad']['ms']} ms, ratio {r['ratio']}", flush=True)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(s + "\n")


if __name__ == "__main__":
    main()
