"""One gradient batch call against the loop it replaces, on one box in one process (the method of tools/batch_profile.py).

For every cell n × B (SE kernel, D = 3, fp64, scalar noise, every problem its own seeded x and y) two things are timed at the C ABI, with the arguments
marshalled beforehand:
  t_batch  ONE gp_logpdf_grad_batch call for the B problems (logpdf, ∂/∂variance, ∂/∂scale, ∂/∂noise, ∂/∂y of every problem);
  t_loop   B gp_logpdf_grad calls with the same outputs, one per problem — the single path.
Both end in a stream synchronise inside the library, so the host clock around them is the whole cost.  Per cell: one same-shape warm-up of each, then
`samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s` (0.2 s); reported: the median with min-max and the achieved fp64 rate over
B·n³ flops (factor, L⁻ᵀ and L⁻ᵀL⁻¹: n³/3 each).  The two results of a cell are compared before they are timed, and the ctx's
"batch_grad_kernel_problems" must have counted every problem of the batch call.  GPMI_BATCH_GRAD_MAX_N is set to the kernels' own limit for the run, so
that every size of the sweep is served by them: the sweep is what GPMI355_BATCH_GRAD_MAX_N is chosen from.  One JSON object to stdout and to --out.

    python tools/batch_grad_profile.py [--sizes 64,128,256,384,512,640,768,896,1024,2048] [--batches 1,8,64,512] [--samples 5] [--out profiles/r20/batch_grad_profile.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,384,512,640,768,896,1024,2048")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true", help="time the batch call alone (a kernel trace of it: four launches per call)")
    a = ap.parse_args()
    os.environ["GPMI_BATCH_GRAD_MAX_N"] = "2048"
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
            call = agp.api._grad_batch_marshal(g)
            nb, karr, nx, pts, narr, marr, ny, yarr, out, info, dvar, dsarr, dnarr, dyarr = call.args
            lp1, dv1, ds1, dn1 = np.empty(B), np.empty(B), np.empty(B), np.empty(B)
            dy1 = np.empty((B, n))

            def batch():
                rc = lib.gp_logpdf_grad_batch(ctx.handle, *call.args)
                assert rc == 0, rc

            def loop():
                for b in range(B):
                    rc = lib.gp_logpdf_grad(ctx.handle, C.byref(karr[b]), C.byref(pts[b]), C.byref(narr[b]), None, yarr[b], lp1.ctypes.data + 8 * b,
                                            C.cast(dv1.ctypes.data + 8 * b, C.POINTER(C.c_double)), C.cast(ds1.ctypes.data + 8 * b, C.POINTER(C.c_double)),
                                            dn1.ctypes.data + 8 * b, dy1.ctypes.data + 8 * n * b, None)
                    assert rc == 0, rc

            served = ctx.get_param("batch_grad_kernel_problems")
            batch()
            assert ctx.get_param("batch_grad_kernel_problems") - served == B, "the gradient kernels did not serve the whole batch"
            if a.batch_only:
                tb, rb = _sample(batch, a.min_s, a.samples)
                cells.append({"n": n, "B": B, "t_batch": _stats(tb), "reps_batch": rb})
                continue
            loop()  # same-shape warm-up of both, and the two answers side by side
            err_lp = float(np.max(np.abs(call.out - lp1) / np.maximum(np.abs(lp1), 1.0)))
            gb = np.stack([call.dvar, np.array([s[0] for s in call.dscale]), np.array([d[0] for d in call.dnoise])], axis=1)
            gl = np.stack([dv1, ds1, dn1], axis=1)
            ginf = np.max(np.abs(gl), axis=1, keepdims=True)
            err_g = float(np.max(np.abs(gb - gl) / (1e-7 * np.abs(gl) + 1e-9 * ginf)))  # in units of the suite's gradient tolerance
            err_dy = float(max(np.linalg.norm(call.dy[b] - dy1[b]) / np.linalg.norm(dy1[b]) for b in range(B)))
            assert err_lp <= 1e-10 and err_g <= 1.0 and err_dy <= 1e-8 and not call.info.any(), (n, B, err_lp, err_g, err_dy)
            tb, rb = _sample(batch, a.min_s, a.samples)
            tl, rl = _sample(loop, a.min_s, a.samples)
            flops = B * float(n) ** 3
            sb, sl = _stats(tb), _stats(tl)
            cell = {"n": n, "B": B, "t_batch": sb, "t_loop": sl, "reps_batch": rb, "reps_loop": rl, "max_rel_diff_logpdf": err_lp,
                    "grad_diff_over_tolerance": round(err_g, 4), "max_rel_diff_dy": err_dy,
                    "speedup_median": round(sl["ms"] / sb["ms"], 2), "disjoint_and_faster": sb["max"] < sl["min"],
                    "batch_tflops": round(flops / (sb["ms"] * 1e-3) / 1e12, 4), "loop_tflops": round(flops / (sl["ms"] * 1e-3) / 1e12, 4)}
            cells.append(cell)
            print(json.dumps(cell), file=sys.stderr, flush=True)
    res = {"host": socket.gethostname(), "kernel": "SE, D = 3, fp64, scalar noise", "samples": a.samples, "min_s": a.min_s, "cells": cells}
    txt = json.dumps(res, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
