"""One gp_predict_batch call against the loop it replaces, on one box in one process (the predictive half of the batch feature).

For every cell n × B × ns (SE kernel, D = 3, fp64, scalar noise, every problem its own seeded x, y and test points) two things are timed at the C ABI,
with the arguments marshalled beforehand:
  t_batch  ONE gp_predict_batch call (what = 3, logpdf included) for the B problems;
  t_loop   B times gp_posterior_fit + gp_posterior_predict(what = 3) + gp_posterior_free on the same library — the single path.
Both end in a stream synchronise inside the library, so the host clock around them is the whole cost.  Per cell: one same-shape warm-up of each, then
`samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s` (0.2 s); reported: the median with min-max.  The two results of a cell
are compared before they are timed (mean 1e-8, var 1e-9 absolute, logpdf 1e-10 relative).  GPMI_BATCH_MAX_N is set to the kernel's own limit (KERNEL_MAX_N)
for the run, as tools/batch_profile.py does, so that every size up to it is served by the batch kernels.  One JSON object to stdout and to --out.

    python tools/batch_predict_profile.py [--sizes 64,256,545,768] [--batches 1,8,64,512] [--points 64,1024] [--out profiles/r19/batch_predict_profile.json]"""
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

from tools.batch_profile import _sample, _stats  # noqa: E402  (the same sampling method)

KERNEL_MAX_N = 2048  # BATCH_KERNEL_MAX_N of csrc/batch.hip: what the kernels admit, whatever GPMI355_BATCH_MAX_N routes to them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,545,768")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--points", default="64,1024")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true", help="time the batch call alone (a kernel trace of it: two kernels and one copy each way per call)")
    a = ap.parse_args()
    os.environ["GPMI_BATCH_MAX_N"] = str(KERNEL_MAX_N)
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    lib = ctx.lib
    cells = []
    for n in [int(v) for v in a.sizes.split(",")]:
        assert n <= KERNEL_MAX_N, "the sweep covers what the batch kernel is routed"
        for B in [int(v) for v in a.batches.split(",")]:
            for ns in [int(v) for v in a.points.split(",")]:
                rng = np.random.default_rng(n * 1000 + B + 7 * ns)
                X, XS = rng.uniform(0, 4, size=(B, n, 3)), rng.uniform(0, 4, size=(B, ns, 3))
                Y = rng.standard_normal((B, n))
                k = 1.3 * agp.SqExponentialKernel() @ agp.ScaleTransform(0.7)
                fxs = [agp.GP(k)(agp.RowVecs(X[b]), 1.3e-2) for b in range(B)]
                (g,) = agp.api._predict_groups(fxs, [Y[b] for b in range(B)], [agp.RowVecs(XS[b]) for b in range(B)])
                call = agp.api._predict_marshal(g, 3)
                nb, karr, nx, pts, narr, marr, ny, yarr, nxs, xpts, pmarr, what, moarr, voarr, out, info = call.args
                lp1, m1, v1 = np.empty(B), np.empty((B, ns)), np.empty((B, ns))

                def batch():
                    rc = getattr(lib, call.entry)(ctx.handle, *call.args)
                    assert rc == 0, rc

                def loop():
                    for b in range(B):
                        post = C.c_void_p()
                        rc = lib.gp_posterior_fit(ctx.handle, C.byref(karr[b]), C.byref(pts[b]), C.byref(narr[b]), None, yarr[b], C.byref(post), None,
                                                  lp1.ctypes.data + 8 * b)
                        assert rc == 0, rc
                        rc = lib.gp_posterior_predict(post, C.byref(xpts[b]), None, 3, m1[b].ctypes.data, v1[b].ctypes.data, None)
                        assert rc == 0, rc
                        assert lib.gp_posterior_free(post) == 0

                batch()
                if a.batch_only:
                    tb, rb = _sample(batch, a.min_s, a.samples)
                    cells.append({"n": n, "B": B, "ns": ns, "t_batch": _stats(tb), "reps_batch": rb})
                    continue
                loop()  # same-shape warm-up of both, and the two answers side by side
                em = float(np.max(np.abs(np.stack(call.means) - m1)))
                ev = float(np.max(np.abs(np.stack(call.vars) - v1)))
                el = float(np.max(np.abs(call.out - lp1) / np.maximum(np.abs(lp1), 1.0)))
                assert em <= 1e-8 and ev <= 1e-9 and el <= 1e-10 and not call.info.any(), (n, B, ns, em, ev, el)
                tb, rb = _sample(batch, a.min_s, a.samples)
                tl, rl = _sample(loop, a.min_s, a.samples)
                sb, sl = _stats(tb), _stats(tl)
                cell = {"n": n, "B": B, "ns": ns, "t_batch": sb, "t_loop": sl, "reps_batch": rb, "reps_loop": rl, "max_diff": {"mean": em, "var": ev, "logpdf": el},
                        "speedup_median": round(sl["ms"] / sb["ms"], 2), "disjoint_and_faster": sb["max"] < sl["min"],
                        "disjoint_and_slower": sb["min"] > sl["max"]}
                cells.append(cell)
                print(json.dumps(cell), file=sys.stderr, flush=True)
    res = {"host": socket.gethostname(), "kernel": "SE, D = 3, fp64, scalar noise", "what": 3, "samples": a.samples, "min_s": a.min_s, "cells": cells}
    txt = json.dumps(res, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
