"""One batch call against the loop it replaces, on one box in one process (issue: batched logpdf for many small exact GPs).

For every cell n × B (SE kernel, D = 3, fp64, scalar noise, every problem its own seeded x and y) two things are timed at the C ABI, with the arguments
marshalled beforehand:
  t_batch  ONE gp_logpdf_batch call for the B problems;
  t_loop   B gp_logpdf calls, one per problem — the single path.
Both end in a stream synchronise inside the library, so the host clock around them is the whole cost.  Per cell: one same-shape warm-up of each, then
`samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s` (0.2 s); reported: the median with min-max, the achieved fp64 rate over
B·n³/3 flops and its share of the MFMA peak of min(B, 256) CUs (78.6 TF/s / 256 each).  The two results of a cell are compared before they are timed.
GPMI_BATCH_MAX_N is set to the kernel's own limit for the run, so that every size of the sweep is served by the batch kernel: the sweep is what
GPMI355_BATCH_MAX_N is chosen from.  One JSON object to stdout and to --out.

    python tools/batch_profile.py [--sizes 64,256,545,640,768,896,1024,2048] [--batches 1,8,64,512] [--samples 5] [--out profiles/r9/batch_profile.json]"""
import argparse
import ctypes as C
import json
import os
import socket
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_PER_CU = 78.6e12 / 256


def _stats(v):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def _sample(fn, min_s, samples):
    t0 = time.perf_counter()
    fn()
    once = max(time.perf_counter() - t0, 1e-6)
    reps = max(1, int(np.ceil(min_s / once)))
    out = []
    for _ in range(samples):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t0) / reps * 1e3)
    return out, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,545,640,768,896,1024,2048")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true", help="time the batch call alone (a kernel trace of it: one launch per call)")
    a = ap.parse_args()
    os.environ["GPMI_BATCH_MAX_N"] = "2048"
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
            call = agp.api._batch_marshal(g, False)
            nb, karr, nx, pts, narr, marr, ny, yarr, out, info, aarr = call.args
            single = np.empty(B)

            def batch():
                rc = lib.gp_logpdf_batch(ctx.handle, *call.args)
                assert rc == 0, rc

            def loop():
                for b in range(B):
                    rc = lib.gp_logpdf(ctx.handle, C.byref(karr[b]), C.byref(pts[b]), C.byref(narr[b]), None, yarr[b], n, 1, single.ctypes.data + 8 * b)
                    assert rc == 0, rc

            batch()
            if a.batch_only:
                tb, rb = _sample(batch, a.min_s, a.samples)
                cells.append({"n": n, "B": B, "t_batch": _stats(tb), "reps_batch": rb})
                continue
            loop()  # same-shape warm-up of both, and the two answers side by side
            err = float(np.max(np.abs(call.out - single) / np.maximum(np.abs(single), 1.0)))
            assert err <= 1e-10 and not call.info.any(), (n, B, err)
            tb, rb = _sample(batch, a.min_s, a.samples)
            tl, rl = _sample(loop, a.min_s, a.samples)
            flops = B * n**3 / 3.0
            sb, sl = _stats(tb), _stats(tl)
            cell = {"n": n, "B": B, "t_batch": sb, "t_loop": sl, "reps_batch": rb, "reps_loop": rl, "max_rel_diff": err,
                    "speedup_median": round(sl["ms"] / sb["ms"], 2), "disjoint_and_faster": sb["max"] < sl["min"],
                    "batch_tflops": round(flops / (sb["ms"] * 1e-3) / 1e12, 4),
                    "batch_share_of_mfma_peak": round(flops / (sb["ms"] * 1e-3) / (min(B, 256) * PEAK_PER_CU), 4),
                    "loop_tflops": round(flops / (sl["ms"] * 1e-3) / 1e12, 4)}
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
