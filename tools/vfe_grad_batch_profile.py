"""One gp_vfe_grad_batch call against the loop of gp_vfe_fit + gp_vfe_grad + gp_vfe_free it replaces, on one box in one process (modelled on
tools/vfe_batch_profile.py).

For every cell M × n × B × {shared, per-problem (x, y)} (SE kernel with a ScaleTransform, D = 3, fp64, scalar noise, VFE; every problem its own seeded
lengthscale and pseudo-inputs) two things are timed at the C ABI, with the arguments marshalled beforehand:
  t_batch  ONE gp_vfe_grad_batch call for the B problems: objective, d/dvariance, d/dscale, d/dnoise, d/dy, d/dz (with --dx also d/dx);
  t_loop   B times gp_vfe_fit with a handle + gp_vfe_grad with the same outputs + gp_vfe_free — what agp.elbo_and_grad does.
Both sides end in a stream synchronise inside the library, so the host clock around them is the whole cost.  Per cell: one same-shape warm-up of each (their
objectives and d/dvariance, d/dz are compared), then `samples` (>= 5) samples, each the mean of enough repetitions to fill `min_s`; reported: the median with
min-max.  GPMI_VFE_GRAD_BATCH_MAX_N is set above the largest n for the run, so that every cell is served by the kernels: the sweep is what
GPMI355_VFE_GRAD_BATCH_MAX_N is chosen from ("threshold": the largest n at which the batch call's slowest sample beat the loop's fastest in every measured
cell with B >= 8).

    python tools/vfe_grad_batch_profile.py [--ms 16,64,128] [--sizes 1024,4096,16384,65536,262144] [--batches 1,8,64,512] [--dx] [--out profiles/r36/vfe_grad_batch_profile.json]"""
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
    ap.add_argument("--ms", default="16,64,128")
    ap.add_argument("--sizes", default="1024,4096,16384,65536,262144")
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--modes", default="shared,per_problem")
    ap.add_argument("--dx", action="store_true")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--max-obs", type=int, default=1 << 28)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    os.environ["GPMI_VFE_GRAD_BATCH_MAX_N"] = str(max(sizes))
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    lib = ctx.lib
    cells, skipped = [], []
    for M in [int(v) for v in a.ms.split(",")]:
        for n in sizes:
            for B in [int(v) for v in a.batches.split(",")]:
                for mode in a.modes.split(","):
                    if mode == "per_problem" and B * n > a.max_obs:
                        skipped.append({"M": M, "n": n, "B": B, "mode": mode})
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
                    # the outputs of both sides: [batch, loop]; the loop reuses one set of per-observation arrays, as a caller's loop would
                    dvar, dsc, dns = np.empty((2, B)), np.empty((2, B)), np.empty((2, B))
                    dy, dz = np.empty((B, n)), np.empty((2, B, M * 3))
                    dx = np.empty((B, n * 3)) if a.dx else None
                    arr = lambda rows, T=C.c_void_p: (T * B)(*[r.ctypes.data for r in rows])  # noqa: E731
                    bptrs = [arr(dsc[0][:, None]), arr(dns[0][:, None]), arr(dy), arr(dz[0]), arr(dx) if a.dx else None]

                    def batch():
                        rc = lib.gp_vfe_grad_batch(ctx.handle, *call.args[:14], dvar[0].ctypes.data_as(C.POINTER(C.c_double)), *bptrs)
                        assert rc == 0, rc

                    single = np.empty(B)
                    pd = C.POINTER(C.c_double)

                    def loop():
                        for b in range(B):
                            h = C.c_void_p()
                            rc = lib.gp_vfe_fit(ctx.handle, C.byref(karr[b]), C.byref(pts[b % nx]), C.byref(zs[b]), C.byref(narr[b]), jit[b], None,
                                                yarr[b % ny], 0, C.byref(h), single.ctypes.data + 8 * b)
                            assert rc == 0, rc
                            rc = lib.gp_vfe_grad(h, dvar[1, b:].ctypes.data_as(pd), dsc[1, b:].ctypes.data_as(pd), dns[1, b:].ctypes.data_as(pd), None,
                                                 dy[0].ctypes.data, dz[1, b].ctypes.data, zs[b].layout, dx[0].ctypes.data if a.dx else None, pts[b % nx].layout)
                            assert rc == 0 and lib.gp_vfe_free(h) == 0, rc

                    served = ctx.get_param("vfe_grad_batch_kernel_problems")
                    batch()
                    assert ctx.get_param("vfe_grad_batch_kernel_problems") - served == B
                    loop()  # same-shape warm-up of both, and the two answers side by side
                    rel = lambda u, v: float(np.max(np.abs(u - v)) / max(np.max(np.abs(v)), 1.0))  # noqa: E731
                    err = {"objective": rel(call.out, single), "variance": rel(dvar[0], dvar[1]), "scale": rel(dsc[0], dsc[1]), "noise": rel(dns[0], dns[1]),
                           "z": rel(dz[0], dz[1])}
                    assert max(err.values()) <= 1e-6 and not call.info.any(), (M, n, B, err)
                    tb, rb = _sample(batch, a.min_s, a.samples)
                    tl, rl = _sample(loop, a.min_s, a.samples)
                    sb, sl = _stats(tb), _stats(tl)
                    cell = {"M": M, "n": n, "B": B, "mode": mode, "dx": a.dx, "t_batch": sb, "t_loop": sl, "reps_batch": rb, "reps_loop": rl,
                            "max_rel_diff": err, "speedup_median": round(sl["ms"] / sb["ms"], 2), "disjoint_and_faster": sb["max"] < sl["min"]}
                    cells.append(cell)
                    print(json.dumps(cell), file=sys.stderr, flush=True)
    deciding = [c for c in cells if c["B"] >= 8]
    wins = [n for n in sizes if any(c["n"] == n for c in deciding) and all(c["disjoint_and_faster"] for c in deciding if c["n"] <= n)]
    res = {"host": socket.gethostname(), "kernel": "SE ∘ ScaleTransform, D = 3, fp64, scalar noise, VFE", "samples": a.samples, "min_s": a.min_s,
           "threshold": max(wins, default=0), "losing_cells": [c for c in deciding if not c["disjoint_and_faster"]], "skipped": skipped, "cells": cells}
    txt = json.dumps(res, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
