"""One gp_vfe_joint_batch call against the loop of gp_vfe_fit + gp_vfe_predict(what = 5) + gp_vfe_logpdf + gp_vfe_rand + gp_vfe_free it replaces, on one box in
one process (modelled on tools/vfe_predict_batch_profile.py).

For every cell M × n × B × {shared, per-problem (x, y, xs)} × ns (SE kernel with a ScaleTransform, D = 3, fp64, scalar noise, VFE, what = 29 with 4 samples,
scalar Σy* = 0.02; every problem its own seeded lengthscale and pseudo-inputs; ns test points per problem, ONE shared set in the shared mode) two things are
timed at the C ABI, with the arguments marshalled beforehand:
  t_batch  ONE gp_vfe_joint_batch call for the B problems: objective, mean, latent covariance, held-out logpdf and samples;
  t_loop   B times gp_vfe_fit with a handle + gp_vfe_predict (what = 5) + gp_vfe_logpdf + gp_vfe_rand + gp_vfe_free — what agp.posterior(...) with mean_and_cov,
           logpdf and rand of post(xs, Σy*) does.
Both sides end in a stream synchronise inside the library, so the host clock around them is the whole cost.  Per cell: one same-shape warm-up of each (their
five outputs are compared), then `samples` samples, each the mean of enough repetitions to fill `min_s`; reported: the median with min-max.
GPMI_VFE_JOINT_BATCH_MAX_N / _MAX_NS are set above the largest n and ns for the run, so that every cell is served by the kernels: the sweep is what
GPMI355_VFE_JOINT_BATCH_MAX_N / _MAX_NS are chosen from ("threshold_n": the largest n at which the batch call's slowest sample beat the loop's fastest in every
measured cell with B >= 8 up to that n; "threshold_ns": the largest ns swept, where every such cell won).  The cells run in ascending n; --budget-s ends the
sweep cleanly and lists the cells it did not reach under "skipped".

    python tools/vfe_joint_batch_profile.py [--ms 16,64,128] [--sizes 1024,4096,16384,65536,262144] [--batches 1,8,64,512] [--ns 64,256,1024] [--out profiles/r39/vfe_joint_batch_profile.json]"""
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

NSAMP, NOISE_XS = 4, 0.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="16,64,128")
    ap.add_argument("--sizes", default="1024,4096,16384,65536,262144")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--modes", default="shared,per_problem")
    ap.add_argument("--ns", default="64,256,1024")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--max-obs", type=int, default=1 << 28)
    ap.add_argument("--budget-s", type=float, default=float("inf"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",")]  # noqa: E731
    sizes, nss = sorted(ints(a.sizes)), sorted(ints(a.ns))
    os.environ["GPMI_VFE_JOINT_BATCH_MAX_N"] = str(max(sizes))
    os.environ["GPMI_VFE_JOINT_BATCH_MAX_NS"] = str(max(nss))
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    lib = ctx.lib
    start, cells, skipped = time.perf_counter(), [], []

    def result():
        deciding = [c for c in cells if c["B"] >= 8]
        wins = [n for n in sizes if any(c["n"] == n for c in deciding) and not any(s["n"] <= n and s["B"] >= 8 for s in skipped)
                and all(c["disjoint_and_faster"] for c in deciding if c["n"] <= n)]
        tn = max(wins, default=0)
        wins_ns = [ns for ns in nss if all(c["disjoint_and_faster"] for c in deciding if c["n"] <= tn and c["ns"] <= ns)]
        return {"host": socket.gethostname(), "kernel": f"SE ∘ ScaleTransform, D = 3, fp64, scalar noise, VFE, what = 29, {NSAMP} samples, Σy* = {NOISE_XS}",
                "samples": a.samples, "min_s": a.min_s, "threshold_n": tn, "threshold_ns": max(wins_ns, default=0) if tn else 0,
                "losing_cells": [c for c in deciding if not c["disjoint_and_faster"]], "skipped": skipped, "cells": cells}

    for n in sizes:
        for M in ints(a.ms):
            for B in ints(a.batches):
                for mode in a.modes.split(","):
                    key = {"M": M, "n": n, "B": B, "mode": mode}
                    if (mode == "per_problem" and B * n > a.max_obs) or time.perf_counter() - start > a.budget_s:
                        skipped += [dict(key, ns=ns) for ns in nss]
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
                    for ns in nss:
                        T = [np.ascontiguousarray(rng.uniform(-2, 2, (ns, 3))) for _ in range(nd)]
                        xpts = (agp._lib.gp_points * nd)(*[call.keep.points(agp.RowVecs(t)) for t in T])
                        nzs = (agp._lib.gp_noise * B)(*[call.keep.noise(NOISE_XS, ns) for _ in range(B)])
                        ys, xi = rng.standard_normal((B, ns)), np.asfortranarray(rng.standard_normal((ns, NSAMP)))
                        mean, hl, smp = np.empty((2, B, ns)), np.empty((2, B)), np.empty((2, B, NSAMP, ns))  # [batch, loop]
                        cov, cov1 = np.empty((B, ns, ns)), np.empty((min(B, 8), ns, ns))  # the loop keeps the covariances of its last eight problems
                        ptrs = lambda v: (C.c_void_p * B)(*[v[b].ctypes.data for b in range(B)])  # noqa: E731
                        mo, co, so, ysp, xip = ptrs(mean[0]), ptrs(cov), ptrs(smp[0]), ptrs(ys), (C.c_void_p * B)(*[xi.ctypes.data] * B)
                        infj = np.zeros(B, dtype=np.int32)

                        def batch():
                            rc = lib.gp_vfe_joint_batch(ctx.handle, *call.args[:12], nd, xpts, None, nzs, 29, mo, co, ysp, hl[0].ctypes.data, NSAMP, xip, so, out, info,
                                                        infj.ctypes.data_as(C.POINTER(C.c_int32)))
                            assert rc == 0, rc

                        single = np.empty(B)

                        def loop():
                            for b in range(B):
                                h, px = C.c_void_p(), C.byref(xpts[b % nd])
                                rc = lib.gp_vfe_fit(ctx.handle, C.byref(karr[b]), C.byref(pts[b % nx]), C.byref(zs[b]), C.byref(narr[b]), jit[b], None,
                                                    yarr[b % ny], 0, C.byref(h), single.ctypes.data + 8 * b)
                                assert rc == 0, rc
                                rc = lib.gp_vfe_predict(h, px, None, 5, mean[1, b].ctypes.data, None, cov1[b % len(cov1)].ctypes.data)
                                assert rc == 0, rc
                                rc = lib.gp_vfe_logpdf(h, px, None, C.byref(nzs[b]), ys[b].ctypes.data, ns, 1, hl[1].ctypes.data + 8 * b)
                                assert rc == 0, rc
                                rc = lib.gp_vfe_rand(h, px, None, C.byref(nzs[b]), xi.ctypes.data, NSAMP, smp[1, b].ctypes.data)
                                assert rc == 0 and lib.gp_vfe_free(h) == 0, rc

                        served = ctx.get_param("vfe_joint_batch_kernel_problems")
                        batch()
                        assert ctx.get_param("vfe_joint_batch_kernel_problems") - served == B
                        loop()  # same-shape warm-up of both, and the two answers side by side
                        err = {"objective": float(np.max(np.abs(call.out - single) / np.abs(single))), "mean": float(np.max(np.abs(mean[0] - mean[1]))),
                               "cov": float(np.max(np.abs(cov[B - len(cov1):] - cov1))), "hlogpdf": float(np.max(np.abs(hl[0] - hl[1]) / np.maximum(np.abs(hl[1]), 1))),
                               "samples": float(np.max(np.abs(smp[0] - smp[1])))}
                        assert err["objective"] <= 1e-8 and err["mean"] <= 1e-7 and err["cov"] <= 1e-8 and err["hlogpdf"] <= 1e-8 and err["samples"] <= 1e-7, (M, n, B, ns, err)
                        assert not call.info.any() and not infj.any()
                        tb, rb = _sample(batch, a.min_s, a.samples)
                        tl, rl = _sample(loop, a.min_s, a.samples)
                        sb, sl = _stats(tb), _stats(tl)
                        cell = dict(key, ns=ns, max_abs_diff=err, t_batch=sb, t_loop=sl, reps_batch=rb, reps_loop=rl, speedup_median=round(sl["ms"] / sb["ms"], 2),
                                    disjoint_and_faster=sb["max"] < sl["min"])
                        cells.append(cell)
                        print(json.dumps(cell), file=sys.stderr, flush=True)
                        if a.out:  # what is measured so far survives a run that is ended from outside
                            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                            Path(a.out).write_text(json.dumps(result(), indent=1) + "\n")
    print(json.dumps(result(), indent=1))


if __name__ == "__main__":
    main()
