"""One gp_predict_grad_batch call against the loops it replaces, on one box in one process (gradients of the batched predictions w.r.t. the test inputs).

For every cell n × B × ns (SE kernel, D = 3, fp64, scalar noise, every problem its own seeded x, y and test points; what = 3, all four outputs) three things
are timed at the C ABI, with the arguments marshalled beforehand:
  t_batch      ONE gp_predict_grad_batch call (logpdf included) for the B problems;
  t_loop       B times gp_posterior_fit + gp_posterior_predict_grad + gp_posterior_free on a default ctx — below "dib_nb" = 2 048 padded points the variance
               side back-substitutes one test point at a time;
  t_loop_dib   the same loop on a ctx with "dib_nb" = 128: the blocked single path.
The faster of the two loops is the opponent (t_opponent) that GPMI355_BATCH_PGRAD_MAX_N is chosen against (include/gpmi355.h).
All end in a stream synchronise inside the library, so the host clock around them is the whole cost.  Per cell: one same-shape warm-up of each, then
`samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s` (0.2 s); reported: [median, min, max] in ms.  --slow-s S: a function whose
same-shape warm-up takes longer than S seconds keeps that run as its only sample (the cell says so: "samples": 1) — what bounds the run
at B = 512 with 1 024 test points, where one pass of the default loop takes tens of seconds.  The answers of a cell are compared before they are timed
(mean 1e-8, var 1e-9 absolute, logpdf 1e-10 relative, gradients rtol 1e-7 / atol 1e-8·max(1, max|g|)), and "batch_pgrad_kernel_problems" must count every
problem of every batch call.  GPMI_BATCH_PGRAD_MAX_N is set to the kernels' own limit (KERNEL_MAX_N) for the run, so that every size up to it is served by
the batch kernels.  The batch sizes are the outer loop, in the order given.  One JSON object to stdout and to --out (rewritten after every cell).

    python tools/batch_predict_grad_profile.py [--sizes 64,128,256,512,768,1024,1536,2048] [--batches 1,8,64,512] [--points 1,64,1024]
                                               [--out profiles/r22/batch_predict_grad_profile.json]"""
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

from tools.batch_profile import _sample, _stats  # noqa: E402  (the same sampling method)

DIFF_KEYS = ("mean", "var", "logpdf", "dmean_of_tol", "dvar_of_tol")  # max_diff of a cell: the worse of the two loops, in this order
KERNEL_MAX_N = 2048  # BATCH_KERNEL_MAX_N of csrc/batch.hip: what the kernels admit, whatever GPMI355_BATCH_PGRAD_MAX_N routes to them


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def _sample_capped(fn, min_s, samples, slow_s, warm):
    """tools.batch_profile._sample, except that a function whose same-shape warm-up took longer than slow_s seconds keeps that run as its only sample"""
    return ([warm * 1e3], 1) if warm > slow_s else _sample(fn, min_s, samples)


def _gerr(g, ref):
    return float(np.max(np.abs(g - ref) / (1e-8 * max(1.0, float(np.abs(ref).max())) + 1e-7 * np.abs(ref))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,512,768,1024,1536,2048")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--points", default="1,64,1024")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--slow-s", type=float, default=float("inf"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true", help="time the batch call alone")
    a = ap.parse_args()
    os.environ["GPMI_BATCH_PGRAD_MAX_N"] = str(KERNEL_MAX_N)
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    dib = agp.Context(0)
    dib.set_param("dib_nb", 128)
    lib = ctx.lib
    cells = []

    def dump():
        res = {"host": socket.gethostname(), "kernel": "SE, D = 3, fp64, scalar noise", "what": 3, "times": "ms: [median, min, max]", "samples_of": "batch, loop, loop_dib",
               "max_diff_of": list(DIFF_KEYS), "samples": a.samples, "min_s": a.min_s,
               "slow_s": a.slow_s if a.slow_s != float("inf") else None, "cells": cells}
        head = json.dumps({k: v for k, v in res.items() if k != "cells"})
        txt = head[:-1] + ', "cells": [\n' + ",\n".join(json.dumps(c) for c in cells) + "\n]}"  # one cell per line
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(txt + "\n")
        return txt

    for B in [int(v) for v in a.batches.split(",")]:
        for n in [int(v) for v in a.sizes.split(",")]:
            assert n <= KERNEL_MAX_N, "the sweep covers what the batch kernels are routed"
            for ns in [int(v) for v in a.points.split(",")]:
                rng = np.random.default_rng(n * 1000 + B + 7 * ns)
                X, XS = rng.uniform(0, 4, size=(B, n, 3)), rng.uniform(0, 4, size=(B, ns, 3))
                Y = rng.standard_normal((B, n))
                k = 1.3 * agp.SqExponentialKernel() @ agp.ScaleTransform(0.7)
                fxs = [agp.GP(k)(agp.RowVecs(X[b]), 1.3e-2) for b in range(B)]
                (g,) = agp.api._predict_groups(fxs, [Y[b] for b in range(B)], [agp.RowVecs(XS[b]) for b in range(B)])
                call = agp.api._predict_grad_marshal(g, 3)
                nb, karr, nx, pts, narr, marr, ny, yarr, nxs, xpts, pmarr, what, moarr, voarr, dmarr, dvarr, out, info = call.args
                lp1, m1, v1 = np.empty(B), np.empty((B, ns)), np.empty((B, ns))
                dm1, dv1 = np.empty((B, ns, 3)), np.empty((B, ns, 3))  # RowVecs: the container layout is (ns, d) per problem

                def batch():
                    rc = getattr(lib, call.entry)(ctx.handle, *call.args)
                    assert rc == 0, rc

                def loop_on(c):
                    def loop():
                        for b in range(B):
                            post = C.c_void_p()
                            rc = lib.gp_posterior_fit(c.handle, C.byref(karr[b]), C.byref(pts[b]), C.byref(narr[b]), None, yarr[b], C.byref(post), None,
                                                      lp1.ctypes.data + 8 * b)
                            assert rc == 0, rc
                            rc = lib.gp_posterior_predict_grad(post, C.byref(xpts[b]), None, 3, m1[b].ctypes.data, v1[b].ctypes.data, dm1[b].ctypes.data,
                                                               dv1[b].ctypes.data)
                            assert rc == 0, rc
                            assert lib.gp_posterior_free(post) == 0
                    return loop

                served = ctx.get_param("batch_pgrad_kernel_problems")
                batch()  # the first call of a shape takes its blocks from the driver; the second is the warm run
                warm = {"batch": _timed(batch)}
                assert ctx.get_param("batch_pgrad_kernel_problems") - served == 2 * B and not call.info.any()
                if a.batch_only:
                    tb, rb = _sample(batch, a.min_s, a.samples)
                    cells.append({"n": n, "B": B, "ns": ns, "t_batch": _stats(tb), "reps_batch": rb})
                    dump()
                    continue
                diffs = {}
                for name, c in (("loop", ctx), ("loop_dib", dib)):  # same-shape warm-up of each loop, and its answers beside the batch call's
                    warm[name] = _timed(loop_on(c))
                    diffs[name] = {"mean": float(np.max(np.abs(np.stack(call.means) - m1))), "var": float(np.max(np.abs(np.stack(call.vars) - v1))),
                                   "logpdf": float(np.max(np.abs(call.out - lp1) / np.maximum(np.abs(lp1), 1.0))),
                                   "dmean_of_tol": _gerr(np.stack(call.dmeans), dm1), "dvar_of_tol": _gerr(np.stack(call.dvars), dv1)}
                    e = diffs[name]
                    assert e["mean"] <= 1e-8 and e["var"] <= 1e-9 and e["logpdf"] <= 1e-10 and e["dmean_of_tol"] <= 1.0 and e["dvar_of_tol"] <= 1.0, (n, B, ns, name, e)
                tb, rb = _sample_capped(batch, a.min_s, a.samples, a.slow_s, warm["batch"])
                tl, rl = _sample_capped(loop_on(ctx), a.min_s, a.samples, a.slow_s, warm["loop"])
                td, rd = _sample_capped(loop_on(dib), a.min_s, a.samples, a.slow_s, warm["loop_dib"])
                sb, sl, sd = _stats(tb), _stats(tl), _stats(td)
                trio = lambda st: [st["ms"], st["min"], st["max"]]  # noqa: E731
                cell = {"n": n, "B": B, "ns": ns, "t_batch": trio(sb), "t_loop": trio(sl), "t_loop_dib": trio(sd), "opponent": "loop" if sl["ms"] <= sd["ms"] else "loop_dib",
                        "samples": [len(tb), len(tl), len(td)], "max_diff": [float(f"{max(d[k] for d in diffs.values()):.1e}") for k in DIFF_KEYS]}
                cells.append(cell)
                dump()
                print(json.dumps(cell), file=sys.stderr, flush=True)
    print(dump())
    dib.close()


if __name__ == "__main__":
    main()
