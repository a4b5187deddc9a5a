"""Composite kernels against the single kind on one box, in one process.  Timed unit: `logpdf(fx, y)` followed by `posterior(fx, y)` — two separate
calls, so two Gram assemblies and two factorisations (bench.py's C4 step is ONE fit serving both: about half of this) — at N = 65 536, D = 1 with
GP(SqExponentialKernel()) and with the Mauna Loa form of examples/1-mauna-loa (SE + Per·SE + RQ + (SE + White): five terms, seven factors) on the
same inputs, alternated; then the value + gradient at N = 32 768, gp_logpdf_grad (SE) against gp_logpdf_grad_sum (Mauna Loa form), alternated.
Prints one JSON line: ms per unit (median), its spread (min / max over the repetitions), and assemble_ms of gp_get_timings (the Gram phase; median
over the repetitions, summed over the two calls of a pair).
    python tools/composite_bench.py [n=65536] [n_grad=32768] [reps=5]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import abstractgps_jl_amd as agp  # noqa: E402


def mauna_loa():
    se, per, rq = agp.SqExponentialKernel(), agp.PeriodicKernel(r=[1.0]), agp.RationalQuadraticKernel(alpha=1.5)
    return (agp.with_lengthscale(se, 50.0) + 0.5 * (agp.with_lengthscale(per, 1.0) * agp.with_lengthscale(se, 100.0))
            + 0.1 * agp.with_lengthscale(rq, 1.2) + (0.05 * agp.with_lengthscale(se, 0.1) + 0.01 * agp.WhiteKernel()))


def data(n):
    rng = np.random.default_rng(0)
    x = np.linspace(0.0, 65.0, n)  # years since 1958
    y = 0.02 * x**2 + 1.3 * x + 3.0 * np.sin(2 * np.pi * x) + 0.3 * rng.standard_normal(n)
    return x, (y - y.mean()) / y.std()


def stats(v):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3), "spread": round((v[-1] - v[0]) / v[len(v) // 2], 4)}


def main():
    opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
    n, ng, reps = int(opt.get("n", 65536)), int(opt.get("n_grad", 32768)), int(opt.get("reps", 5))
    ctx = agp.default_context(0)
    kernels = {"se": agp.SqExponentialKernel(), "mauna_loa": mauna_loa()}
    x, y = data(n)

    def pair(k):
        f = agp.GP(k)
        t0 = time.perf_counter()
        agp.logpdf(f(x, 0.1), y)
        asm = ctx.timings()["assemble_ms"]
        p = agp.posterior(f(x, 0.1), y)
        asm += ctx.timings()["assemble_ms"]
        dt = (time.perf_counter() - t0) * 1e3
        p.data.C.free()
        return dt, asm

    res = {"n": n, "reps": reps}
    t = {k: [] for k in kernels}
    a = {k: [] for k in kernels}
    for k in kernels.values():  # warm-up of both shapes
        pair(k)
    for _ in range(reps):
        for name, k in kernels.items():
            dt, asm = pair(k)
            t[name].append(dt)
            a[name].append(asm)
    for name in kernels:
        res["pair_" + name] = {**stats(t[name]), "assemble_ms": round(float(np.median(a[name])), 3)}
    res["pair_ratio"] = round(res["pair_mauna_loa"]["ms"] / res["pair_se"]["ms"], 4)

    xg, yg = data(ng)

    def grad(k):
        f = agp.GP(k)
        t0 = time.perf_counter()
        agp.logpdf_and_grad(f(xg, 0.1), yg)
        return (time.perf_counter() - t0) * 1e3, ctx.timings()["assemble_ms"]

    tg = {k: [] for k in kernels}
    ag = {k: [] for k in kernels}
    for k in kernels.values():
        grad(k)
    for _ in range(reps):
        for name, k in kernels.items():
            dt, asm = grad(k)
            tg[name].append(dt)
            ag[name].append(asm)
    res["n_grad"] = ng
    for name in kernels:
        res["grad_" + name] = {**stats(tg[name]), "assemble_ms": round(float(np.median(ag[name])), 3)}
    res["grad_ratio"] = round(res["grad_mauna_loa"]["ms"] / res["grad_se"]["ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
