"""One gradient batch call WITH the input gradient against the loop it replaces, on one box in one process (the method of tools/batch_grad_profile.py).

For every cell n × B (SE kernel, D = 3, fp64, scalar noise, every problem its own seeded x and y) three things are timed at the C ABI, with the arguments
marshalled beforehand:
  t_batch     ONE gp_logpdf_grad_batch_x call for the B problems (logpdf, ∂/∂variance, ∂/∂scale, ∂/∂noise, ∂/∂y and ∂/∂x of every problem);
  t_loop      B gp_logpdf_grad calls with the same outputs (dx_out included), one per problem — the single path, the opponent;
  t_batch_nox ONE gp_logpdf_grad_batch call (the same outputs without ∂/∂x): what the two input-gradient kernels add to a batch call.
All end in a stream synchronise inside the library, so the host clock around them is the whole cost.  Per cell: one same-shape warm-up of each, then
`samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s` (0.2 s); reported: the median with min-max.  The results of a cell are
compared before they are timed (∂/∂x in units of the suite's tolerance 1e-7·|g| + 1e-8·max(1, max|g|)), and the ctx's "batch_gradx_kernel_problems" must
have counted every problem of the batch call.  GPMI_BATCH_GRADX_MAX_N and GPMI_BATCH_GRAD_MAX_N are set to the kernels' own limit for the run, so that
every size of the sweep is served by them: the sweep is what GPMI355_BATCH_GRADX_MAX_N is chosen from.  One JSON object to stdout and to --out.

    python tools/batch_gradx_profile.py [--sizes 64,128,256,384,512,640,768,896,1024,1152,1280,1536,2048] [--batches 1,8,64,512] [--samples 5]
                                        [--out profiles/r24/batch_gradx_profile.json]"""
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
    ap.add_argument("--sizes", default="64,128,256,384,512,640,768,896,1024,1152,1280,1536,2048")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["GPMI_BATCH_GRADX_MAX_N"] = "2048"
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
            call = agp.api._grad_batch_marshal(g, True)
            nox = agp.api._grad_batch_marshal(g)
            nb, karr, nx, pts, narr, marr, ny, yarr = call.args[:8]
            lp1, dv1, ds1, dn1 = np.empty(B), np.empty(B), np.empty(B), np.empty(B)
            dy1 = np.empty((B, n))
            dx1 = np.empty((B, n, 3))

            def batch():
                rc = lib.gp_logpdf_grad_batch_x(ctx.handle, *call.args)
                assert rc == 0, rc

            def batch_nox():
                rc = lib.gp_logpdf_grad_batch(ctx.handle, *nox.args)
                assert rc == 0, rc

            def loop():
                for b in range(B):
                    rc = lib.gp_logpdf_grad(ctx.handle, C.byref(karr[b]), C.byref(pts[b]), C.byref(narr[b]), None, yarr[b], lp1.ctypes.data + 8 * b,
                                            C.cast(dv1.ctypes.data + 8 * b, C.POINTER(C.c_double)), C.cast(ds1.ctypes.data + 8 * b, C.POINTER(C.c_double)),
                                            dn1.ctypes.data + 8 * b, dy1.ctypes.data + 8 * n * b, dx1.ctypes.data + 8 * 3 * n * b)
                    assert rc == 0, rc

            served = ctx.get_param("batch_gradx_kernel_problems")
            batch()
            assert ctx.get_param("batch_gradx_kernel_problems") - served == B, "the input-gradient kernels did not serve the whole batch"
            batch_nox()
            loop()  # same-shape warm-up of all three, and the answers side by side
            err_lp = float(np.max(np.abs(call.out - lp1) / np.maximum(np.abs(lp1), 1.0)))
            gb = np.stack([call.dvar, np.array([s[0] for s in call.dscale]), np.array([d[0] for d in call.dnoise])], axis=1)
            gl = np.stack([dv1, ds1, dn1], axis=1)
            ginf = np.max(np.abs(gl), axis=1, keepdims=True)
            err_g = float(np.max(np.abs(gb - gl) / (1e-7 * np.abs(gl) + 1e-9 * ginf)))  # in units of the suite's gradient tolerance
            gxb = np.stack(call.dx)  # RowVecs of a C-ordered (n, 3) array: layout 1, (n, 3) as dx1
            gxinf = np.maximum(np.max(np.abs(dx1), axis=(1, 2), keepdims=True), 1.0)
            err_x = float(np.max(np.abs(gxb - dx1) / (1e-7 * np.abs(dx1) + 1e-8 * gxinf)))  # in units of the suite's input-gradient tolerance
            same_bits = call.out.tobytes() == nox.out.tobytes() and call.dvar.tobytes() == nox.dvar.tobytes() and \
                all(p.tobytes() == q.tobytes() for p, q in zip(call.dy + call.dnoise + call.dscale, nox.dy + nox.dnoise + nox.dscale))
            assert err_lp <= 1e-10 and err_g <= 1.0 and err_x <= 1.0 and same_bits and not call.info.any(), (n, B, err_lp, err_g, err_x, same_bits)
            tb, rb = _sample(batch, a.min_s, a.samples)
            tl, rl = _sample(loop, a.min_s, a.samples)
            tn, rn = _sample(batch_nox, a.min_s, a.samples)
            sb, sl, sn = _stats(tb), _stats(tl), _stats(tn)
            cell = {"n": n, "B": B, "t_batch": sb, "t_loop": sl, "t_batch_nox": sn, "reps_batch": rb, "reps_loop": rl, "reps_batch_nox": rn,
                    "max_rel_diff_logpdf": err_lp, "grad_diff_over_tolerance": round(err_g, 4), "dx_diff_over_tolerance": round(err_x, 4),
                    "other_outputs_same_bits_as_without_dx": same_bits, "speedup_median": round(sl["ms"] / sb["ms"], 2),
                    "disjoint_and_faster": sb["max"] < sl["min"], "with_dx_over_without": round(sb["ms"] / sn["ms"], 3)}
            cells.append(cell)
            print(json.dumps(cell), file=sys.stderr, flush=True)
    res = {"host": socket.gethostname(), "kernel": "SE, D = 3, fp64, scalar noise, all outputs", "samples": a.samples, "min_s": a.min_s, "cells": cells}
    txt = json.dumps(res, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
