"""Sparse column calls against the loop of single-column calls they replace, in one process on one library (VFE, SE kernel, D = 3, seeded inputs as
bench.py's C5 row).

Per configuration (N, M, dtype) and S, at the mirror (marshalling included on both sides; every call ends in a stream synchronise inside the library, so the
host clock around it is its whole cost):
    fit           posterior_columns(VFE(fz), fx, Y)                          against  S × posterior(VFE(fz), fx, Y[:, s])
    fit_predict   … + mean_and_var(xs), ns = 4 096                            against  S × (… + mean_and_var(xs))
    value_grad    elbo_and_grad_columns(VFE(fz), fx, Y)                       against  S × elbo_and_grad(VFE(fz), fx, Y[:, s])
`single_ms` is ONE single-column call (median).  The column side is the median of `repeats` samples after a warm-up.  The loop side runs
min(S, --loop-cap) columns once and is scaled to S columns (`loop_columns_run` says how many ran; 0 = the whole loop).  ratio = loop / cols.
`cols_over_single` = what the S columns cost in units of one single-column call.  `by_bytes` = the device memory the handle's retained b_y takes
(round_up(S, 16) × npad × sizeof(dtype)).  One JSON line per cell to stdout; --out FILE also writes the whole object.

    python tools/vfe_cols_profile.py [--configs 262144x4096xf32,262144x4096xf64,2000000x256xf32] [--s 2,16,128] [--repeats 3] [--loop-cap 0] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _ms(fn, repeats):
    v = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        v.append((time.perf_counter() - t0) * 1e3)
    v.sort()
    return round(v[len(v) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="262144x4096xf32,262144x4096xf64,2000000x256xf32")
    ap.add_argument("--s", default="2,16,128")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=0)
    ap.add_argument("--ns", type=int, default=4096)
    ap.add_argument("--out", default="", help="also write the JSON object to this file")
    a = ap.parse_args()
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    cells = []
    for cfg in a.configs.split(","):
        n, m, dts = cfg.split("x")
        n, m, dt = int(n), int(m), (np.float32 if dts == "f32" else np.float64)
        rng = np.random.default_rng(5)
        X = (rng.uniform(0, 1, (n, 3)) * 4).astype(dt)
        z = X[rng.permutation(n)[:m]].copy()
        xs = agp.RowVecs((rng.uniform(0, 1, (a.ns, 3)) * 4).astype(dt))
        f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
        fx = f(agp.RowVecs(X), dt(0.1))
        approx = agp.VFE(f(agp.RowVecs(z), 1e-4))
        base = np.sin(X.sum(1))

        def one_fit(y):
            return agp.posterior(approx, fx, y)

        def one_fit_predict(y):
            return one_fit(y).mean_and_var(xs)

        def one_grad(y):
            return agp.elbo_and_grad(approx, fx, y)

        y0 = (base + 0.3 * rng.standard_normal(n)).astype(dt)
        one_grad(y0)
        one_fit_predict(y0)  # warm-up (workspaces, code objects, the inverse blocks' build path)
        single = {"fit": _ms(lambda: one_fit(y0), a.repeats), "fit_predict": _ms(lambda: one_fit_predict(y0), a.repeats),
                  "value_grad": _ms(lambda: one_grad(y0), a.repeats)}
        for S in [int(v) for v in a.s.split(",")]:
            Y = np.asfortranarray((base[:, None] * (1.0 + 0.1 * np.arange(S)[None, :]) + 0.3 * rng.standard_normal((n, S))).astype(dt))
            run = S if a.loop_cap <= 0 else min(S, a.loop_cap)
            agp.elbo_and_grad_columns(approx, fx, Y)
            agp.posterior_columns(approx, fx, Y).mean_and_var(xs)
            cols = {"fit": _ms(lambda: agp.posterior_columns(approx, fx, Y), a.repeats),
                    "fit_predict": _ms(lambda: agp.posterior_columns(approx, fx, Y).mean_and_var(xs), a.repeats),
                    "value_grad": _ms(lambda: agp.elbo_and_grad_columns(approx, fx, Y), a.repeats)}
            ph = ctx.timings()
            loop = {}
            for name, fn in (("fit", one_fit), ("fit_predict", one_fit_predict), ("value_grad", one_grad)):
                t0 = time.perf_counter()
                for s in range(run):
                    fn(Y[:, s])
                loop[name] = round((time.perf_counter() - t0) * 1e3 * S / run, 3)
            chunk_pad = -(-n // 16384) * 16384
            cell = {"n": n, "m": m, "dtype": dts, "S": S, "single_ms": single, "cols_ms": cols, "loop_ms": loop, "loop_columns_run": 0 if run == S else run,
                    "ratio": {k: round(loop[k] / cols[k], 2) for k in cols}, "cols_over_single": {k: round(cols[k] / single[k], 3) for k in cols},
                    "by_bytes_at_16384_chunks": -(-S // 16) * 16 * chunk_pad * np.dtype(dt).itemsize, "last_call_phases_ms": ph}
            cells.append(cell)
            print(json.dumps(cell), flush=True)
        ctx.trim()
    out = {"tool": "tools/vfe_cols_profile.py", "cells": cells}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
