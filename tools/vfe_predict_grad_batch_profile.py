"""One gp_vfe_predict_grad_batch call against the loop of gp_vfe_fit + gp_vfe_predict_grad + gp_vfe_free it replaces, on one box in one process (modelled on
tools/vfe_predict_batch_profile.py).

For every cell M × n × B × {shared, per-problem (x, y, xs)} × ns (SE kernel with a ScaleTransform, D = 3, fp64, scalar noise, VFE, what = 3 with all four
outputs; every problem its own seeded lengthscale and pseudo-inputs; ns test points per problem, ONE shared set in the shared mode) three things are timed at
the C ABI, with the arguments marshalled beforehand:
  t_batch  ONE gp_vfe_predict_grad_batch call for the B problems: objective, mean, variance and both gradients;
  t_loop   B times gp_vfe_fit with a handle + gp_vfe_predict_grad (what = 3) + gp_vfe_free — what agp.posterior(...).mean_and_var_grad does;
  t_values ONE gp_vfe_predict_batch call (what = 3) on the same cell: "grad_over_values" is the cost of the gradients as a ratio — written down, not asserted.
Every side ends in a stream synchronise inside the library, so the host clock around it is the whole cost.  Per cell: one same-shape warm-up of each (the
objectives, means, variances and gradients of batch and loop are compared), then `samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s`;
reported: the median with min-max (--loop-samples takes fewer samples of the loop alone, whose repetitions take seconds at B = 512).  GPMI_VFE_PREDICT_GRAD_BATCH_MAX_N and GPMI_VFE_PREDICT_BATCH_MAX_N are set above the largest n for the run, so that every
cell is served by the kernels: the sweep is what GPMI355_VFE_PREDICT_GRAD_BATCH_MAX_N is chosen from ("threshold": the largest n at which the batch call's
slowest sample beat the loop's fastest in every measured cell with B >= 8 up to that n).  The cells run in ascending n; --budget-s ends the sweep cleanly and
lists the cells it did not reach under "skipped".

A long sweep may be split by n into several runs (--sizes), one process and one file each: the threshold rule reads their cells together.

    python tools/vfe_predict_grad_batch_profile.py [--ms 16,64,128] [--sizes 1024,4096,16384,65536,262144] [--batches 1,8,64,512] [--ns 64,1024] [--out profiles/r38/vfe_predict_grad_batch_profile.json]"""
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
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--loop-samples", type=int, default=None, help="samples of the loop (default: --samples); the loop at B = 512 takes seconds per repetition")
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--max-obs", type=int, default=1 << 28)
    ap.add_argument("--budget-s", type=float, default=float("inf"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",")]  # noqa: E731
    sizes = sorted(ints(a.sizes))
    os.environ["GPMI_VFE_PREDICT_GRAD_BATCH_MAX_N"] = os.environ["GPMI_VFE_PREDICT_BATCH_MAX_N"] = str(max(sizes))
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    lib = ctx.lib
    start, cells, skipped = time.perf_counter(), [], []

    def result():
        deciding = [c for c in cells if c["B"] >= 8 and "t_loop" in c]
        wins = [n for n in sizes if any(c["n"] == n for c in deciding) and not any(s["n"] <= n and s["B"] >= 8 for s in skipped)
                and all(c["disjoint_and_faster"] for c in deciding if c["n"] <= n)]
        return {"host": socket.gethostname(), "kernel": "SE ∘ ScaleTransform, D = 3, fp64, scalar noise, VFE, what = 3, all four outputs", "samples": a.samples,
                "loop_samples": a.loop_samples or a.samples, "min_s": a.min_s, "threshold": max(wins, default=0), "losing_cells": [c for c in deciding if not c["disjoint_and_faster"]],
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
                        res, grd = np.empty((2, 2, B, ns)), np.empty((2, 2, B, ns, 3))  # [batch, loop][mean, var] and their gradients (RowVecs: ns × d)
                        optr = [(C.c_void_p * B)(*[v[0, s, b].ctypes.data for b in range(B)]) for v in (res, grd) for s in (0, 1)]

                        def batch():
                            rc = lib.gp_vfe_predict_grad_batch(ctx.handle, *call.args[:12], nd, xpts, None, 3, *optr, out, info)
                            assert rc == 0, rc

                        def values():
                            rc = lib.gp_vfe_predict_batch(ctx.handle, *call.args[:12], nd, xpts, None, 3, optr[0], optr[1], out, info)
                            assert rc == 0, rc

                        single = np.empty(B)

                        def loop():
                            for b in range(B):
                                h = C.c_void_p()
                                rc = lib.gp_vfe_fit(ctx.handle, C.byref(karr[b]), C.byref(pts[b % nx]), C.byref(zs[b]), C.byref(narr[b]), jit[b], None,
                                                    yarr[b % ny], 0, C.byref(h), single.ctypes.data + 8 * b)
                                assert rc == 0, rc
                                rc = lib.gp_vfe_predict_grad(h, C.byref(xpts[b % nd]), None, 3, res[1, 0, b].ctypes.data, res[1, 1, b].ctypes.data,
                                                             grd[1, 0, b].ctypes.data, grd[1, 1, b].ctypes.data)
                                assert rc == 0 and lib.gp_vfe_free(h) == 0, rc

                        served = ctx.get_param("vfe_predict_grad_batch_kernel_problems")
                        batch()
                        assert ctx.get_param("vfe_predict_grad_batch_kernel_problems") - served == B
                        loop()  # same-shape warm-up of both, and the two answers side by side
                        gscale = [max(1.0, float(np.max(np.abs(grd[1, s])))) for s in (0, 1)]
                        err = {"objective": float(np.max(np.abs(call.out - single) / np.abs(single))), "mean": float(np.max(np.abs(res[0, 0] - res[1, 0]))),
                               "var": float(np.max(np.abs(res[0, 1] - res[1, 1]))), "dmean_rel": float(np.max(np.abs(grd[0, 0] - grd[1, 0]))) / gscale[0],
                               "dvar_rel": float(np.max(np.abs(grd[0, 1] - grd[1, 1]))) / gscale[1]}
                        assert err["objective"] <= 1e-8 and err["mean"] <= 1e-7 and err["var"] <= 1e-8 and not call.info.any(), (M, n, B, ns, err)
                        assert err["dmean_rel"] <= 1e-7 and err["dvar_rel"] <= 1e-7, (M, n, B, ns, err)
                        values()
                        tb, rb = _sample(batch, a.min_s, a.samples)
                        tl, rl = _sample(loop, a.min_s, a.loop_samples or a.samples)
                        tv, _ = _sample(values, a.min_s, a.samples)
                        sb, sl, sv = _stats(tb), _stats(tl), _stats(tv)
                        cell = dict(key, ns=ns, max_abs_diff=err, t_batch=sb, t_loop=sl, t_values=sv, reps_batch=rb, reps_loop=rl,
                                    speedup_median=round(sl["ms"] / sb["ms"], 2), grad_over_values=round(sb["ms"] / sv["ms"], 2),
                                    disjoint_and_faster=sb["max"] < sl["min"])
                        cells.append(cell)
                        print(json.dumps(cell), file=sys.stderr, flush=True)
                        if a.out:  # what is measured so far survives a run that is ended from outside
                            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                            Path(a.out).write_text(json.dumps(result(), indent=1) + "\n")
    if a.out:  # the final state: the cells a budget did not reach are listed only now
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result(), indent=1) + "\n")
    print(json.dumps(result(), indent=1))


if __name__ == "__main__":
    main()
