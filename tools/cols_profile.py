"""Column calls against the loop of single-column calls they replace, in one process on one library (issue: one factorisation for a matrix of observations).

Inputs as C2 (D = 3, SE, σ² = 0.01, fp64, seeded).  For n ∈ {2 048, 16 384} × S ∈ {2, 16, 64, 128} × ns ∈ {64, 4 096}, at the mirror (marshalling
included on both sides; every call ends in a stream synchronise inside the library, so the host clock around it is its whole cost):
    fit_predict   posterior_columns(fx, Y) + mean_and_var(xs)            against  S × (posterior(fx, Y[:, s]) + mean_and_var(xs))
    kmul          gp_posterior_predict_cols(what = 1) on the cols handle against  S × gp_posterior_predict(what = 1) on a one-column handle
                  (ONE kmul launch against S kvec launches; both sides upload xs and download their means)
    grad          logpdf_and_grad_columns(fx, Y)                         against  S × logpdf_and_grad(fx, Y[:, s])          (once per (n, S): no test points)
The column side is the median of `repeats` samples after a warm-up; the loop side is timed `loop_repeats` times (it is S times as long).  ratio = loop / cols.
"cols_kernel_splits" of the kmul launch is recorded with every cell.  One JSON object to stdout and to --out.

    python tools/cols_profile.py [--n 2048,16384] [--s 2,16,64,128] [--ns 64,4096] [--repeats 5] [--loop-repeats 1] [--out profiles/r27/cols_profile.json]"""
import argparse
import json
import socket
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
    ap.add_argument("--n", default="2048,16384")
    ap.add_argument("--s", default="2,16,64,128")
    ap.add_argument("--ns", default="64,4096")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-repeats", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r27" / "cols_profile.json"))
    a = ap.parse_args()
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    f = agp.GP(agp.SqExponentialKernel())
    rng = np.random.default_rng(27)
    cells = []
    for n in [int(v) for v in a.n.split(",")]:
        X = rng.uniform(0.0, 4.0, size=(n, 3))
        fx = f(agp.RowVecs(X), 0.01)
        for S in [int(v) for v in a.s.split(",")]:
            Y = np.asfortranarray(np.sin(X.sum(1))[:, None] + 0.1 * rng.standard_normal((n, S)))
            agp.logpdf_and_grad_columns(fx, Y)  # warm-up (workspaces, code objects)
            g_cols = _ms(lambda: agp.logpdf_and_grad_columns(fx, Y), max(1, a.repeats // 2))
            g_loop = _ms(lambda: [agp.logpdf_and_grad(fx, Y[:, s]) for s in range(S)], a.loop_repeats)
            for ns in [int(v) for v in a.ns.split(",")]:
                xs = agp.RowVecs(rng.uniform(0.0, 4.0, size=(ns, 3)))

                def cols_fp():
                    p = agp.posterior_columns(fx, Y)
                    p.mean_and_var(xs)
                    p.data.C.free()

                def loop_fp():
                    for s in range(S):
                        p = agp.posterior(fx, Y[:, s])
                        p.mean_and_var(xs)
                        p.data.C.free()

                cols_fp()
                fp_cols = _ms(cols_fp, a.repeats)
                fp_loop = _ms(loop_fp, a.loop_repeats)
                pc, p1 = agp.posterior_columns(fx, Y), agp.posterior(fx, Y[:, 0])
                mc = pc.mean(xs)
                splits = ctx.get_param("cols_kernel_splits")
                m1 = p1.mean(xs)
                assert np.max(np.abs(mc[:, 0] - m1)) <= 1e-8 * max(1.0, np.max(np.abs(m1)))
                k_cols = _ms(lambda: pc.mean(xs), a.repeats)
                k_loop = _ms(lambda: [p1.mean(xs) for _ in range(S)], max(a.loop_repeats, 3))
                pc.data.C.free()
                p1.data.C.free()
                cell = {"n": n, "S": S, "ns": ns, "splits": splits,
                        "fit_predict": {"cols_ms": fp_cols, "loop_ms": fp_loop, "ratio": round(fp_loop / fp_cols, 2)},
                        "kmul": {"cols_ms": k_cols, "loop_ms": k_loop, "ratio": round(k_loop / k_cols, 2)},
                        "grad": {"cols_ms": g_cols, "loop_ms": g_loop, "ratio": round(g_loop / g_cols, 2)}}
                print(json.dumps(cell), flush=True)
                cells.append(cell)
    out = {"host": socket.gethostname(), "what": "loop of S single-column calls / one column call, host clock, ms", "cells": cells}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"written": a.out, "cells": len(cells)}))


if __name__ == "__main__":
    main()
