"""One gp_joint_batch call against the loops it replaces, on one box in one process (joint predictions of many small exact GPs).

For every cell n × B × ns (SE kernel, D = 3, fp64, scalar noise, scalar Σy* = 1.3e-2, every problem its own seeded x, y, test points, held-out observations and
standard normals; what = 29: mean, latent covariance, held-out logpdf and nsamp = 4 samples) three things are timed at the C ABI, with the arguments
marshalled beforehand:
  t_batch      ONE gp_joint_batch call (training logpdf included) for the B problems;
  t_loop       B times gp_posterior_fit + gp_posterior_predict(what = 5) + gp_posterior_logpdf + gp_posterior_rand + gp_posterior_free on a default ctx;
  t_loop_dib   the same loop on a ctx with "dib_nb" = 128: the blocked solves of the single path on small handles.
The faster of the two loops is the opponent that GPMI355_BATCH_JOINT_MAX_N / _MAX_NS are chosen against (include/gpmi355.h).
All end in a stream synchronise inside the library, so the host clock around them is the whole cost.  Per cell: one same-shape warm-up of each, then
`samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s`; reported: [median, min, max] in ms.  --slow-s S: a function whose same-shape
warm-up takes longer than S seconds keeps that run as its only sample (the cell says so in "samples").  The answers of a cell are compared during the
warm-up of each loop (mean 1e-8, cov 1e-9 absolute, logpdf and held-out logpdf 1e-10 relative to max(|.|, 1), samples 1e-8), and
"batch_joint_kernel_problems" must count every problem of every batch call.  GPMI_BATCH_JOINT_MAX_N / _MAX_NS are set to the kernels' own limit for the run,
so that every size up to it is served by the batch kernels.  The batch sizes are the outer loop, in the order given.  One JSON object to stdout and to --out
(rewritten after every cell).

    python tools/batch_joint_profile.py [--sizes 64,128,256,512,768,1024,1536,2048] [--batches 1,8,64,512] [--points 64,256,1024]
                                        [--out profiles/r25/batch_joint_profile.json]"""
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

DIFF_KEYS = ("mean", "cov", "logpdf", "heldout_logpdf", "samples")  # max_diff of a cell: the worse of the two loops, in this order
DIFF_TOLS = (1e-8, 1e-9, 1e-10, 1e-10, 1e-8)
KERNEL_MAX_N = 2048  # BATCH_KERNEL_MAX_N of csrc/batch.hip: what the kernels admit, whatever the header constants route to them
NSAMP = 4


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def _sample_capped(fn, min_s, samples, slow_s, warm):
    """tools.batch_profile._sample, except that a function whose same-shape warm-up took longer than slow_s seconds keeps that run as its only sample"""
    return ([warm * 1e3], 1) if warm > slow_s else _sample(fn, min_s, samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,512,768,1024,1536,2048")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--points", default="64,256,1024")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--slow-s", type=float, default=float("inf"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["GPMI_BATCH_JOINT_MAX_N"] = os.environ["GPMI_BATCH_JOINT_MAX_NS"] = str(KERNEL_MAX_N)
    import abstractgps_jl_amd as agp
    from abstractgps_jl_amd._lib import gp_noise

    ctx = agp.default_context(0)
    dib = agp.Context(0)
    dib.set_param("dib_nb", 128)
    lib = ctx.lib
    cells = []

    def dump():
        res = {"host": socket.gethostname(), "kernel": "SE, D = 3, fp64, scalar noise, scalar noise on the test points", "what": 29, "nsamp": NSAMP,
               "times": "ms: [median, min, max]", "samples_of": "batch, loop, loop_dib", "max_diff_of": list(DIFF_KEYS), "samples": a.samples, "min_s": a.min_s,
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
                Y, YS, XI = rng.standard_normal((B, n)), rng.standard_normal((B, ns)), np.asfortranarray(rng.standard_normal((B, ns, NSAMP)).transpose(1, 2, 0))
                k = 1.3 * agp.SqExponentialKernel() @ agp.ScaleTransform(0.7)
                fxs = [agp.GP(k)(agp.RowVecs(X[b]), 1.3e-2) for b in range(B)]
                (g,) = agp.api._predict_groups(fxs, [Y[b] for b in range(B)], [agp.RowVecs(XS[b]) for b in range(B)])
                call = agp.api._joint_marshal(g, 29, [1.3e-2] * B, [YS[b] for b in range(B)], [XI[:, :, b] for b in range(B)])
                (nb, karr, nx, pts, narr, marr, ny, yarr, nxs, xpts, pmarr, nzarr, what, moarr, coarr, ysarr, hl, nsamp, xiarr, soarr, out, info, ij) = call.args
                nzs = gp_noise(0, 1.3e-2, None)
                lp1, hl1 = np.empty(1), np.empty(1)  # the loop's outputs: one problem's worth, compared (check) and overwritten
                m1, C1, s1 = np.empty(ns), np.empty((ns, ns), order="F"), np.empty((ns, NSAMP), order="F")

                def batch():
                    rc = getattr(lib, call.entry)(ctx.handle, *call.args)
                    assert rc == 0, rc

                def loop_on(c, diffs=None):
                    def loop():
                        for b in range(B):
                            post = C.c_void_p()
                            rc = lib.gp_posterior_fit(c.handle, C.byref(karr[b]), C.byref(pts[b]), C.byref(narr[b]), None, yarr[b], C.byref(post), None, lp1.ctypes.data)
                            assert rc == 0, rc
                            rc = lib.gp_posterior_predict(post, C.byref(xpts[b]), None, 5, m1.ctypes.data, None, C1.ctypes.data)
                            assert rc == 0, rc
                            rc = lib.gp_posterior_logpdf(post, C.byref(xpts[b]), None, C.byref(nzs), ysarr[b], ns, 1, hl1.ctypes.data)
                            assert rc == 0, rc
                            rc = lib.gp_posterior_rand(post, C.byref(xpts[b]), None, C.byref(nzs), xiarr[b], NSAMP, s1.ctypes.data)
                            assert rc == 0, rc
                            assert lib.gp_posterior_free(post) == 0
                            if diffs is not None:
                                e = (float(np.max(np.abs(call.means[b] - m1))), float(np.max(np.abs(call.covs[b] - C1))),
                                     abs(call.out[b] - lp1[0]) / max(abs(lp1[0]), 1.0), abs(call.heldout[b] - hl1[0]) / max(abs(hl1[0]), 1.0),
                                     float(np.max(np.abs(call.samples[b] - s1))))
                                diffs[:] = [max(u, float(v)) for u, v in zip(diffs, e)]
                    return loop

                served = ctx.get_param("batch_joint_kernel_problems")
                batch()  # the first call of a shape takes its blocks from the driver; the second is the warm run
                warm = {"batch": _timed(batch)}
                assert ctx.get_param("batch_joint_kernel_problems") - served == 2 * B and not call.info.any() and not call.info_joint.any()
                worst = [0.0] * 5
                for name, c in (("loop", ctx), ("loop_dib", dib)):  # same-shape warm-up of each loop, and its answers beside the batch call's
                    d = [0.0] * 5
                    warm[name] = _timed(loop_on(c, d))
                    assert all(v <= t for v, t in zip(d, DIFF_TOLS)), (n, B, ns, name, d)
                    worst = [max(u, v) for u, v in zip(worst, d)]
                tb, rb = _sample_capped(batch, a.min_s, a.samples, a.slow_s, warm["batch"])
                tl, rl = _sample_capped(loop_on(ctx), a.min_s, a.samples, a.slow_s, warm["loop"])
                td, rd = _sample_capped(loop_on(dib), a.min_s, a.samples, a.slow_s, warm["loop_dib"])
                sb, sl, sd = _stats(tb), _stats(tl), _stats(td)
                trio = lambda st: [st["ms"], st["min"], st["max"]]  # noqa: E731
                cell = {"n": n, "B": B, "ns": ns, "t_batch": trio(sb), "t_loop": trio(sl), "t_loop_dib": trio(sd), "opponent": "loop" if sl["ms"] <= sd["ms"] else "loop_dib",
                        "samples": [len(tb), len(tl), len(td)], "max_diff": [float(f"{v:.1e}") for v in worst]}
                cells.append(cell)
                dump()
                print(json.dumps(cell), file=sys.stderr, flush=True)
    print(dump())
    dib.close()


if __name__ == "__main__":
    main()
