"""One leave-one-out batch call against the loop it replaces, on one box in one process (the method of tools/batch_profile.py and
tools/batch_grad_profile.py).

For every cell n × B (SE kernel, D = 3, fp64, scalar noise, every problem its own seeded x and y) two pairs are timed at the C ABI, with the arguments
marshalled beforehand:
  values     ONE gp_loo_batch call for the B problems (L, ℓ, μ, v of every problem) against B gp_loo calls with the same outputs;
  gradients  ONE gp_loo_grad_batch call (L, ∂/∂variance, ∂/∂scale, ∂/∂noise, ∂/∂y of every problem; no dx) against B gp_loo_grad calls with the same
             outputs.
The opponent is always the loop of the existing single calls.  Every call ends in a stream synchronise inside the library, so the host clock around it is
the whole cost.  Per cell and side: one same-shape warm-up, then `samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s` (0.2 s);
reported: the median with min-max.  The two results of a cell are compared before they are timed (in units of the suite's tolerances), and the ctx's
"batch_loo_kernel_problems" / "batch_loo_grad_kernel_problems" must have counted every problem of the batch call.  GPMI_BATCH_LOO_MAX_N and
GPMI_BATCH_LOO_GRAD_MAX_N are set to the kernels' own limit for the run, so that every size of the sweep is served by them: the sweep is what
GPMI355_BATCH_LOO_MAX_N and GPMI355_BATCH_LOO_GRAD_MAX_N are chosen from — each the largest multiple of 128 of the sweep at which the batch call beat the
loop in every cell with B >= 8 (the output applies that rule twice: to the medians, and counting a cell only where every sample of the batch call lies below
every sample of the loop; the header takes the second).  One JSON object to stdout and to --out.

    python tools/batch_loo_profile.py [--sizes 64,128,256,384,512,640,768,896,1024,1152,1280,1536,2048] [--batches 1,8,64,512] [--samples 5]
                                      [--what values,gradients] [--out profiles/r32/batch_loo_profile.json]
    python tools/batch_loo_profile.py --resummarise old.json --out new.json     # the summary of an earlier run's cells again, without a device"""
import argparse
import ctypes as C
import json
import os
import socket
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.batch_profile import _sample, _stats  # noqa: E402

# The two answers of a cell are recorded in units of the suite's tolerances.  Those are forward tolerances for cond(C) <= 1e3 (tests/loo_cases.py); the sweep's
# problems (noise 1 % of the variance, up to 2 048 points in [0, 4]³) are worse conditioned, and two correct paths may then differ by more: the run stops only
# where they no longer agree to about six digits.
SANITY = 1e4


def limit_by_the_rule(cells, key, disjoint):
    """the largest multiple of 128 among the sizes of the sweep up to which ONE batch call beat the loop in every cell with B >= 8 (0: none); beat: the
    median below the loop's median, or with `disjoint` every sample below every sample of the loop (a cell whose ranges overlap decides nothing)"""
    def beat(v):
        return v["t_batch"]["max"] < v["t_loop"]["min"] if disjoint else v["t_batch"]["ms"] < v["t_loop"]["ms"]

    best = 0
    for n in sorted({c["n"] for c in cells if key in c}):
        if not all(beat(c[key]) for c in cells if key in c and c["n"] == n and c["B"] >= 8):
            break
        if n % 128 == 0:
            best = n
    return best


def summary(cells, what):
    return {"limits_by_medians": {w: limit_by_the_rule(cells, w, False) for w in what}, "limits_by_disjoint_ranges": {w: limit_by_the_rule(cells, w, True) for w in what}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,384,512,640,768,896,1024,1152,1280,1536,2048")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--what", default="values,gradients")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resummarise", default=None, help="no measurement: read this JSON of an earlier run and write it to --out with the summary of its cells")
    a = ap.parse_args()
    what = a.what.split(",")
    if a.resummarise:
        res = json.loads(Path(a.resummarise).read_text())
        res.pop("limits", None)
        res = {**{k: v for k, v in res.items() if k != "cells"}, **summary(res["cells"], what), "cells": res["cells"]}
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(summary(res["cells"], what)))
        return
    os.environ["GPMI_BATCH_LOO_MAX_N"] = "2048"
    os.environ["GPMI_BATCH_LOO_GRAD_MAX_N"] = "2048"
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    lib = ctx.lib
    cells = []
    for n in [int(v) for v in a.sizes.split(",")]:
        for B in [int(v) for v in a.batches.split(",")]:
            rng = np.random.default_rng(n * 1000 + B)
            X = rng.uniform(0, 4, size=(B, n, 3))
            Y = rng.standard_normal((B, n))
            k = 1.3 * agp.SqExponentialKernel() @ agp.ScaleTransform(0.7)
            fxs = [agp.GP(k)(agp.RowVecs(X[b]), 1.3e-2) for b in range(B)]
            (g,) = agp.api._batch_groups(fxs, [Y[b] for b in range(B)])
            cell = {"n": n, "B": B}
            if "values" in what:
                call = agp.api._loo_batch_marshal(g)
                nb, karr, nx, pts, narr, marr, ny, yarr = call.args[:8]
                L1 = np.empty(B)
                lp1, mu1, var1 = np.empty((B, n)), np.empty((B, n)), np.empty((B, n))

                def batch():
                    rc = lib.gp_loo_batch(ctx.handle, *call.args)
                    assert rc == 0, rc

                def loop():
                    for b in range(B):
                        rc = lib.gp_loo(ctx.handle, C.byref(karr[b]), C.byref(pts[b]), C.byref(narr[b]), None, yarr[b], L1.ctypes.data + 8 * b,
                                        lp1.ctypes.data + 8 * n * b, mu1.ctypes.data + 8 * n * b, var1.ctypes.data + 8 * n * b)
                        assert rc == 0, rc

                served = ctx.get_param("batch_loo_kernel_problems")
                batch()
                assert ctx.get_param("batch_loo_kernel_problems") - served == B, "the kernels did not serve the whole batch"
                loop()  # same-shape warm-up of both, and the two answers side by side, in units of the suite's tolerances
                err = {"L": float(np.max(np.abs(call.out - L1) / (1e-10 * np.abs(L1)))),
                       "lp": float(max(np.max(np.abs(call.lp[b] - lp1[b])) / (1e-10 * max(1.0, np.max(np.abs(lp1[b])))) for b in range(B))),
                       "mean": float(max(np.max(np.abs(call.mean[b] - mu1[b])) for b in range(B)) / 1e-8),
                       "var": float(max(np.max(np.abs(call.var[b] - var1[b])) for b in range(B)) / 1e-9)}
                assert max(err.values()) <= SANITY and not call.info.any(), (n, B, err)
                tb, rb = _sample(batch, a.min_s, a.samples)
                tl, rl = _sample(loop, a.min_s, a.samples)
                sb, sl = _stats(tb), _stats(tl)
                cell["values"] = {"t_batch": sb, "t_loop": sl, "reps_batch": rb, "reps_loop": rl, "diff_over_tolerance": {k_: round(v, 4) for k_, v in err.items()},
                                  "speedup_median": round(sl["ms"] / sb["ms"], 2), "disjoint_and_faster": sb["max"] < sl["min"]}
            if "gradients" in what:
                gcall = agp.api._loo_grad_batch_marshal(g)
                nb, karr, nx, pts, narr, marr, ny, yarr = gcall.args[:8]
                L2, dv1, ds1, dn1 = np.empty(B), np.empty(B), np.empty(B), np.empty(B)
                dy1 = np.empty((B, n))

                def gbatch():
                    rc = lib.gp_loo_grad_batch(ctx.handle, *gcall.args)
                    assert rc == 0, rc

                def gloop():
                    for b in range(B):
                        rc = lib.gp_loo_grad(ctx.handle, C.byref(karr[b]), C.byref(pts[b]), C.byref(narr[b]), None, yarr[b], L2.ctypes.data + 8 * b,
                                             C.cast(dv1.ctypes.data + 8 * b, C.POINTER(C.c_double)), C.cast(ds1.ctypes.data + 8 * b, C.POINTER(C.c_double)),
                                             dn1.ctypes.data + 8 * b, dy1.ctypes.data + 8 * n * b, None)
                        assert rc == 0, rc

                served = ctx.get_param("batch_loo_grad_kernel_problems")
                gbatch()
                assert ctx.get_param("batch_loo_grad_kernel_problems") - served == B, "the gradient kernels did not serve the whole batch"
                gloop()
                gb = np.stack([gcall.dvar, np.array([s[0] for s in gcall.dscale]), np.array([d[0] for d in gcall.dnoise])], axis=1)
                gl = np.stack([dv1, ds1, dn1], axis=1)
                ginf = np.max(np.abs(gl), axis=1, keepdims=True)
                err = {"L": float(np.max(np.abs(gcall.out - L2) / (1e-10 * np.abs(L2)))),
                       "theta_noise": float(np.max(np.abs(gb - gl) / (1e-7 * np.abs(gl) + 1e-9 * ginf))),
                       "dy": float(max(np.max(np.abs(gcall.dy[b] - dy1[b]) / (1e-7 * np.abs(dy1[b]) + 1e-9 * np.max(np.abs(dy1[b])))) for b in range(B)))}
                assert max(err.values()) <= SANITY and not gcall.info.any(), (n, B, err)
                tb, rb = _sample(gbatch, a.min_s, a.samples)
                tl, rl = _sample(gloop, a.min_s, a.samples)
                sb, sl = _stats(tb), _stats(tl)
                cell["gradients"] = {"t_batch": sb, "t_loop": sl, "reps_batch": rb, "reps_loop": rl,
                                     "diff_over_tolerance": {k_: round(v, 4) for k_, v in err.items()},
                                     "speedup_median": round(sl["ms"] / sb["ms"], 2), "disjoint_and_faster": sb["max"] < sl["min"]}
            cells.append(cell)
            print(json.dumps(cell), file=sys.stderr, flush=True)
    res = {"host": socket.gethostname(), "kernel": "SE, D = 3, fp64, scalar noise", "samples": a.samples, "min_s": a.min_s,
           **summary(cells, what), "cells": cells}
    txt = json.dumps(res, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
