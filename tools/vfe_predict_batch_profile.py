"""One gp_vfe_predict_batch call against the loop of gp_vfe_fit + gp_vfe_predict + gp_vfe_free it replaces, on one box in one process (modelled on
tools/vfe_grad_batch_profile.py).

For every cell M × n × B × {shared, per-problem (x, y, xs)} × ns (SE kernel with a ScaleTransform, D = 3, fp64, scalar noise, VFE, what = 3; every problem
its own seeded lengthscale and pseudo-inputs; ns test points per problem, ONE shared set in the shared mode) two things are timed at the C ABI, with the
arguments marshalled beforehand:
  t_batch  ONE gp_vfe_predict_batch call for the B problems: objective, mean and variance;
  t_loop   B times gp_vfe_fit with a handle + gp_vfe_predict (what = 3) + gp_vfe_free — what agp.posterior(...).mean_and_var does.
Both sides end in a stream synchronise inside the library, so the host clock around them is the whole cost.  Per cell: one same-shape warm-up of each (their
objectives, means and variances are compared), then `samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s`; reported: the median with
min-max.  GPMI_VFE_PREDICT_BATCH_MAX_N is set above the largest n for the run, so that every cell is served by the kernels: the sweep is what
GPMI355_VFE_PREDICT_BATCH_MAX_N is chosen from ("threshold": the largest n at which the batch call's slowest sample beat the loop's fastest in every measured
cell with B >= 8 up to that n).  The cells run in ascending n; --budget-s ends the sweep cleanly and lists the cells it did not reach under "skipped".

--segs 128,512,2048 is the other measurement: the batch call alone at M = 128 under each GPMI_VFE_PREDICT_BATCH_SEG (the test points per predict workgroup;
read per call), the settings alternating inside every sample — what GPMI355_VFE_PREDICT_BATCH_SEG is chosen from.

    python tools/vfe_predict_batch_profile.py [--ms 16,64,128] [--sizes 1024,4096,16384,65536,262144] [--batches 1,8,64,512] [--ns 64,1024] [--out profiles/r37/vfe_predict_batch_profile.json]
    python tools/vfe_predict_batch_profile.py --segs 128,512,2048 --ms 128 --sizes 4096 --batches 8,64 --ns 64,4096 --out profiles/r37/vfe_predict_batch_seg.json"""
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
from tools.batch_profile import _sample, _stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="16,64,128")
    ap.add_argument("--sizes", default="1024,4096,16384,65536,262144")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--modes", default="shared,per_problem")
    ap.add_argument("--ns", default="64,1024")
    ap.add_argument("--segs", default=None)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--max-obs", type=int, default=1 << 28)
    ap.add_argument("--budget-s", type=float, default=float("inf"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",")]  # noqa: E731
    sizes, segs = sorted(ints(a.sizes)), ints(a.segs) if a.segs else None
    os.environ["GPMI_VFE_PREDICT_BATCH_MAX_N"] = str(max(sizes))
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    lib = ctx.lib
    start, cells, skipped = time.perf_counter(), [], []

    def result():
        deciding = [c for c in cells if c["B"] >= 8 and "t_loop" in c]
        wins = [n for n in sizes if any(c["n"] == n for c in deciding) and not any(s["n"] <= n and s["B"] >= 8 for s in skipped)
                and all(c["disjoint_and_faster"] for c in deciding if c["n"] <= n)]
        return {"host": socket.gethostname(), "kernel": "SE ∘ ScaleTransform, D = 3, fp64, scalar noise, VFE, what = 3", "samples": a.samples, "min_s": a.min_s,
                "segs": segs, "threshold": None if segs else max(wins, default=0), "losing_cells": [c for c in deciding if not c["disjoint_and_faster"]],
                "skipped": skipped, "cells": cells}

    for n in sizes:
        for M in ints(a.ms):
            for B in ints(a.batches):
                for mode in a.modes.split(","):
                    key = {"M": M, "n": n, "B": B, "mode": mode}
                    if (mode == "per_problem" and B * n > a.max_obs) or time.perf_counter() - start > a.budget_s:
                        skipped += [dict(key, ns=ns) for ns in ints(a.ns)]
                        continue
                    rng = np.random.default_rng(M * 7 + n * 1000 + B)
                    nd = 1 if mode == "shared" else B
                    X = [agp.RowVecs(rng.uniform(-2, 2, (n, 3))) for _ in range(nd)]
                    Y = [np.sin(x.X.sum(1)) + 0.1 * rng.standard_normal(n) for x in X]
                    fs = [agp.GP(1.3 * agp.SqExponentialKernel() @ agp.ScaleTransform(float(rng.uniform(0.5, 1.5)))) for _ in range(B)]
                    fxs = [f(X[b % nd], 0.05) for b, f in enumerate(fs)]
                    approxs = [agp.VFE(f(agp.RowVecs(X[b % nd].X[rng.permutation(n)[:M]] + 0.01 * rng.standard_normal((M, 3))), 1e-4)) for b, f in enumerate(fs)]
                    (g,) = agp.api._vfe_batch_groups(approxs, fxs, [Y[b % nd] for b in range(B)])
                    call = agp.api._vfe_batch_marshal(g, False, False)
                    nb, karr, nx, pts, nz, zs, narr, jit, marr, ny, yarr, kinds, out, info, aarr, earr = call.args
                    assert (nx, ny) == ((1, 1) if mode == "shared" else (B, B)) or B == 1
                    for ns in ints(a.ns):
                        T = [np.ascontiguousarray(rng.uniform(-2, 2, (ns, 3))) for _ in range(nd)]
                        xpts = (agp._lib.gp_points * nd)(*[call.keep.points(agp.RowVecs(t)) for t in T])
                        res = np.empty((2, 2, B, ns))  # [batch, loop][mean, var]
                        optr = [(C.c_void_p * B)(*[res[0, s, b].ctypes.data for b in range(B)]) for s in (0, 1)]

                        def batch():
                            rc = lib.gp_vfe_predict_batch(ctx.handle, *call.args[:12], nd, xpts, None, 3, optr[0], optr[1], out, info)
                            assert rc == 0, rc

                        single = np.empty(B)

                        def loop():
                            for b in range(B):
                                h = C.c_void_p()
                                rc = lib.gp_vfe_fit(ctx.handle, C.byref(karr[b]), C.byref(pts[b % nx]), C.byref(zs[b]), C.byref(narr[b]), jit[b], None,
                                                    yarr[b % ny], 0, C.byref(h), single.ctypes.data + 8 * b)
                                assert rc == 0, rc
                                rc = lib.gp_vfe_predict(h, C.byref(xpts[b % nd]), None, 3, res[1, 0, b].ctypes.data, res[1, 1, b].ctypes.data, None)
                                assert rc == 0 and lib.gp_vfe_free(h) == 0, rc

                        served = ctx.get_param("vfe_predict_batch_kernel_problems")
                        batch()
                        assert ctx.get_param("vfe_predict_batch_kernel_problems") - served == B
                        loop()  # same-shape warm-up of both, and the two answers side by side
                        err = {"objective": float(np.max(np.abs(call.out - single) / np.abs(single))), "mean": float(np.max(np.abs(res[0, 0] - res[1, 0]))),
                               "var": float(np.max(np.abs(res[0, 1] - res[1, 1])))}
                        assert err["objective"] <= 1e-8 and err["mean"] <= 1e-7 and err["var"] <= 1e-8 and not call.info.any(), (M, n, B, ns, err)
                        cell = dict(key, ns=ns, max_abs_diff=err)
                        if segs:  # the batch call alone under each segment length, alternating inside every sample
                            _, reps = _sample(batch, a.min_s, 1)
                            ts = {s: [] for s in segs}
                            for _ in range(a.samples):
                                for s in segs:
                                    os.environ["GPMI_VFE_PREDICT_BATCH_SEG"] = str(s)
                                    batch()
                                    t0 = time.perf_counter()
                                    for _ in range(reps):
                                        batch()
                                    ts[s].append((time.perf_counter() - t0) / reps * 1e3)
                            del os.environ["GPMI_VFE_PREDICT_BATCH_SEG"]
                            cell["t_batch_by_seg"] = {str(s): _stats(v) for s, v in ts.items()}
                        else:
                            tb, rb = _sample(batch, a.min_s, a.samples)
                            tl, rl = _sample(loop, a.min_s, a.samples)
                            sb, sl = _stats(tb), _stats(tl)
                            cell.update(t_batch=sb, t_loop=sl, reps_batch=rb, reps_loop=rl, speedup_median=round(sl["ms"] / sb["ms"], 2),
                                        disjoint_and_faster=sb["max"] < sl["min"])
                        cells.append(cell)
                        print(json.dumps(cell), file=sys.stderr, flush=True)
                        if a.out:  # what is measured so far survives a run that is ended from outside
                            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                            Path(a.out).write_text(json.dumps(result(), indent=1) + "\n")
    print(json.dumps(result(), indent=1))


if __name__ == "__main__":
    main()
