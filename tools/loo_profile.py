"""Leave-one-out cross-validation against the calls it is built from and against the host recipe it replaces, in one process on one library.

Inputs as C2 (D = 3, SE, σ² = 0.01, fp64, seeded).  For n ∈ {2 048, 8 192, 16 384}, at the mirror (marshalling included on both sides; every call ends in a
stream synchronise inside the library, so the host clock around it is its whole cost):
    value   loo_logpdf(fx, y)            against  logpdf(fx, y)            by flops 2× (fit + L⁻ᵀ = 2n³/3 against n³/3)
    grad    loo_logpdf_and_grad(fx, y)   against  logpdf_and_grad(fx, y)   by flops 2× (one more n³ product: 2n³ against n³), plus two n² passes
    host    the recipe without gp_loo: posterior(fx, y) + data.C.solve(I) (n² numbers over the bus) + NumPy for μ, v, ℓ — no gradient
Each figure is the median of `repeats` samples after a warm-up.  The host recipe's L is compared with loo_logpdf's.  One JSON object to stdout and to --out.

    python tools/loo_profile.py [--n 2048,8192,16384] [--repeats 5] [--out profiles/r28/loo_profile.json]"""
import argparse
import json
import math
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
    ap.add_argument("--n", default="2048,8192,16384")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r28" / "loo_profile.json"))
    a = ap.parse_args()
    import abstractgps_jl_amd as agp

    f = agp.GP(agp.SqExponentialKernel())
    rng = np.random.default_rng(28)
    cells = []
    for n in [int(v) for v in a.n.split(",")]:
        X = rng.uniform(0.0, 4.0, size=(n, 3))
        fx = f(agp.RowVecs(X), 0.01)
        y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)

        def host_recipe():
            p = agp.posterior(fx, y)
            try:
                c = np.diag(p.data.C.solve(np.eye(n))).copy()
            finally:
                p.data.C.free()
            al = p.data.alpha
            return y - al / c, 1.0 / c, float(np.sum(-0.5 * math.log(2.0 * math.pi) + 0.5 * np.log(c) - 0.5 * al**2 / c))

        for fn in (lambda: agp.logpdf(fx, y), lambda: agp.loo_logpdf(fx, y), lambda: agp.logpdf_and_grad(fx, y), lambda: agp.loo_logpdf_and_grad(fx, y)):
            fn()  # warm-up (workspaces, code objects)
        L = float(agp.loo_logpdf(fx, y))
        Lh = host_recipe()[2]
        assert abs(L - Lh) <= 1e-6 * abs(Lh), (L, Lh)  # (cond(C) reaches 1e6 here: the figure itself goes into the cell)
        t = {"logpdf_ms": _ms(lambda: agp.logpdf(fx, y), a.repeats), "loo_logpdf_ms": _ms(lambda: agp.loo_logpdf(fx, y), a.repeats),
             "logpdf_and_grad_ms": _ms(lambda: agp.logpdf_and_grad(fx, y), a.repeats),
             "loo_logpdf_and_grad_ms": _ms(lambda: agp.loo_logpdf_and_grad(fx, y), a.repeats),
             "host_recipe_ms": _ms(host_recipe, max(1, a.repeats // 2))}
        cell = {"n": n, **t, "value_ratio": round(t["loo_logpdf_ms"] / t["logpdf_ms"], 2),
                "grad_ratio": round(t["loo_logpdf_and_grad_ms"] / t["logpdf_and_grad_ms"], 2),
                "host_over_value": round(t["host_recipe_ms"] / t["loo_logpdf_ms"], 2),
                "host_over_grad": round(t["host_recipe_ms"] / t["loo_logpdf_and_grad_ms"], 2), "L_rel_diff_host": abs(L - Lh) / abs(Lh)}
        print(json.dumps(cell), flush=True)
        cells.append(cell)
    out = {"host": socket.gethostname(), "what": "host clock, ms, median; value_ratio = loo_logpdf / logpdf, grad_ratio = loo_logpdf_and_grad / logpdf_and_grad",
           "cells": cells}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"written": a.out, "cells": len(cells)}))


if __name__ == "__main__":
    main()
