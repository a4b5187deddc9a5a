"""K-fold cross-validation from one factorisation against the loop of refits it replaces and against leave-one-out, in one process on one library.

Inputs as C2 (D = 3, SE, σ² = 0.01, fp64, seeded), folds i mod K.  For n ∈ {2 048, 8 192, 16 384} × K ∈ {5, 10, 16, 64}, wherever every fold holds at most
GPMI355_KFOLD_MAX_FOLD observations, at the mirror (marshalling included on both sides; every call ends in a stream synchronise inside the library, so the
host clock around it is its whole cost):
    kfold   kfold_logpdf(fx, y, folds)
    loop    K × (posterior on the other folds + logpdf of the held-out fold under it + free)
    loo     loo_logpdf(fx, y) on the same data
Each figure is the median of `repeats` samples after a warm-up, the three alternating within a sample.  The loop's value is compared with kfold's and goes
into the cell.  Cells where a fold would be above the limit are listed as skipped.  One JSON object to stdout and to --out.

    python tools/kfold_profile.py [--n 2048,8192,16384] [--k 5,10,16,64] [--repeats 5] [--out profiles/r40/kfold_profile.json]"""
import argparse
import json
import socket
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="2048,8192,16384")
    ap.add_argument("--k", default="5,10,16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r40" / "kfold_profile.json"))
    a = ap.parse_args()
    import abstractgps_jl_amd as agp

    f = agp.GP(agp.SqExponentialKernel())
    rng = np.random.default_rng(40)
    cells, skipped = [], []
    for n in [int(v) for v in a.n.split(",")]:
        X = rng.uniform(0.0, 4.0, size=(n, 3))
        fx = f(agp.RowVecs(X), 0.01)
        y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
        for K in [int(v) for v in a.k.split(",")]:
            if -(-n // K) > agp._lib.kfold_max_fold():
                skipped.append({"n": n, "K": K, "why": f"folds of {-(-n // K)} observations"})
                continue
            folds = np.arange(n) % K

            def loop():
                total = 0.0
                for k in range(K):
                    r, h = folds != k, folds == k
                    p = agp.posterior(f(agp.RowVecs(X[r]), 0.01), y[r])
                    try:
                        total += float(agp.logpdf(p(agp.RowVecs(X[h]), 0.01), y[h]))
                    finally:
                        p.data.C.free()
                return total

            fns = {"kfold_ms": lambda: agp.kfold_logpdf(fx, y, folds), "loop_ms": loop, "loo_ms": lambda: agp.loo_logpdf(fx, y)}
            v, vl = float(agp.kfold_logpdf(fx, y, folds)), loop()  # warm-up of two of the three (workspaces, code objects) and the comparison
            agp.loo_logpdf(fx, y)
            t = {k: [] for k in fns}
            for _ in range(a.repeats):
                for k, fn in fns.items():
                    t[k].append(_ms(fn))
            med = {k: round(sorted(s)[len(s) // 2], 3) for k, s in t.items()}
            cell = {"n": n, "K": K, **med, "loop_over_kfold": round(med["loop_ms"] / med["kfold_ms"], 2),
                    "kfold_over_loo": round(med["kfold_ms"] / med["loo_ms"], 2), "value_rel_diff_loop": abs(v - vl) / abs(vl)}
            print(json.dumps(cell), flush=True)
            cells.append(cell)
    out = {"host": socket.gethostname(), "what": "host clock, ms, median; loop_over_kfold = the loop of K refits / kfold_logpdf (above 1: the one call wins)",
           "cells": cells, "skipped": skipped}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"written": a.out, "cells": len(cells), "skipped": len(skipped)}))


if __name__ == "__main__":
    main()
