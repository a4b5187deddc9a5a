"""What a dense Σy costs against the vector noise diag(Σy), on one box in one run (issue: exact GPs with a dense observation-noise covariance).

Timed unit: `logpdf(fx, y)` followed by `posterior(fx, y)` — two separate calls, so two Gram assemblies, two factorisations and, with a dense Σy, TWO
uploads of its triangle.  fp64, SE kernel, D = 3; per size one same-size warm-up, then the median of `reps` (3) repetitions:
  t_vec     the pair with the vector noise diag(Σy) — in child processes that alternate between the PARENT commit's library (--parent-lib, selected
            through GPMI355_LIB) and this tree's;
  t_copy    one plain hipMemcpy of 8·N(N+1)/2 bytes from pageable host memory to the device (what a caller cannot avoid, once);
  t_dense2  the pair with Σy as a Fortran-ordered array (gp_noise kind 2: a block of matrix rows per piece, straight add);
  t_dense3  the pair with Σy as a C-ordered array (kind 3: a block of matrix columns per piece, transposing add),
both with the phases of gp_get_timings (summed over the two calls) and the bytes moved, computed from the shapes.
Condition of the issue: t_dense <= 1.10 · (t_vec(parent) + t_copy); and t_vec of this tree inside the spread of the parent's own repetitions.
Every child runs under its own time limit; the first one that fails ends the run.  One JSON object to stdout and to --out.

    python tools/dense_noise_profile.py --parent-lib /path/to/parent/libgpmi355.so [--sizes 16384,32768] [--reps 3] [--out profiles/r8/dense_noise_profile.json]"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _stats(v):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2), "all": [round(t, 2) for t in v]}


def _sigma(n):
    """A dense positive definite Σy that costs nothing to build: 1e-3 everywhere + 0.05 on the diagonal (every page of the array is touched)."""
    S = np.full((n, n), 1e-3)
    S[np.diag_indices(n)] += 0.05
    return S


def child(n, reps, what):
    import abstractgps_jl_amd as agp

    ctx = agp.default_context(0)
    rng = np.random.default_rng(n)
    X = agp.RowVecs(rng.uniform(0, 3, size=(n, 3)))
    y = rng.standard_normal(n)
    f = agp.GP(1.3 * agp.with_lengthscale(agp.SqExponentialKernel(), 0.7))
    res = {"n": n, "lib": os.environ.get("GPMI355_LIB", "tree")}

    def pair(noise):
        ph = {"assemble_ms": 0.0, "potrf_ms": 0.0, "solve_ms": 0.0}
        t0 = time.perf_counter()
        agp.logpdf(f(X, noise), y)
        for k in ph:
            ph[k] += ctx.timings()[k]
        p = agp.posterior(f(X, noise), y)
        for k in ph:
            ph[k] += ctx.timings()[k]
        dt = (time.perf_counter() - t0) * 1e3
        p.data.C.free()
        return dt, ph

    def timed(noise):
        pair(noise)  # same-size warm-up
        ts, phs = [], []
        for _ in range(reps):
            dt, ph = pair(noise)
            ts.append(dt)
            phs.append(ph)
        out = _stats(ts)
        out["phases_ms"] = {k: round(float(np.median([p[k] for p in phs])), 2) for k in phs[0]}
        return out

    res["t_vec"] = timed(np.full(n, 0.051))
    if what == "all":
        tflops = C.c_double()
        agp._lib.check(ctx.lib.gp_bench_mfma_f64(ctx.handle, 2000, C.byref(tflops)))
        res["mfma_f64_tflops"] = round(tflops.value, 1)
        S = _sigma(n)
        tri = 8 * n * (n + 1) // 2
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
        dev = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev), tri) == 0
        ts = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            assert hip.hipMemcpy(dev, S.ctypes.data, tri, 1) == 0  # hipMemcpyHostToDevice, blocking, pageable source
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
        hip.hipFree(dev)
        res["t_copy"] = {**_stats(ts), "bytes": tri, "gb_per_s": round(tri / 1e6 / sorted(ts)[len(ts) // 2], 2)}
        piece = ctx.get_param("dense_stage_mb")
        res["t_dense3"] = {**timed(S), "kind": 3, "bytes_uploaded_per_fit": tri, "fits_per_pair": 2, "dense_stage_mb": piece}
        res["t_dense2"] = {**timed(S.T),  # S is symmetric: its transposed view is the Fortran-ordered array, no copy
                            "kind": 2, "bytes_uploaded_per_fit": tri, "fits_per_pair": 2, "dense_stage_mb": piece}
    print("RESULT " + json.dumps(res), flush=True)


def run_child(n, reps, what, lib, limit):
    env = dict(os.environ)
    env.pop("GPMI355_LIB", None)
    if lib:
        env["GPMI355_LIB"] = str(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--child", what, "--n", str(n), "--reps", str(reps)]
    pr = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if pr.returncode != 0:
        sys.stderr.write(pr.stdout[-2000:] + pr.stderr[-4000:])
        raise SystemExit(f"child {what} n={n} lib={lib} ended with status {pr.returncode}: nothing more is started")
    line = next(ln for ln in pr.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--sizes", default="16384,32768")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r8" / "dense_noise_profile.json"))
    ap.add_argument("--child")
    ap.add_argument("--n", type=int)
    a = ap.parse_args()
    if a.child:
        return child(a.n, a.reps, a.child)
    if not a.parent_lib or not Path(a.parent_lib).exists():
        raise SystemExit("--parent-lib: the library built from the parent commit is needed for t_vec")
    out = {"host": socket.gethostname(), "started": time.strftime("%Y-%m-%dT%H:%M:%S%z"), "reps": a.reps, "dtype": "float64", "kernel": "1.3*SE(l=0.7)", "d": 3,
           "unit": "logpdf(fx, y) + posterior(fx, y): two fits", "sizes": {}}
    for n in [int(s) for s in a.sizes.split(",")]:
        limit = 120 + int(60 * (n / 16384) ** 2)
        p1 = run_child(n, a.reps, "vec", a.parent_lib, limit)
        new = run_child(n, a.reps, "all", None, limit + 120)
        p2 = run_child(n, a.reps, "vec", a.parent_lib, limit)
        n2 = run_child(n, a.reps, "vec", None, limit)
        par = p1["t_vec"]["all"] + p2["t_vec"]["all"]
        nw = new["t_vec"]["all"] + n2["t_vec"]["all"]
        r = {"t_vec_parent": _stats(par), "t_vec_new": _stats(nw), "t_vec_phases_ms": new["t_vec"]["phases_ms"], "t_copy": new["t_copy"],
             "t_dense2": new["t_dense2"], "t_dense3": new["t_dense3"], "mfma_f64_tflops": new["mfma_f64_tflops"]}
        bound = 1.10 * (r["t_vec_parent"]["ms"] + r["t_copy"]["ms"])
        r["bound_ms"] = round(bound, 2)
        for k in ("t_dense2", "t_dense3"):
            r[k]["ratio_to_bound"] = round(r[k]["ms"] / bound, 3)
            r[k]["condition_met"] = bool(r[k]["ms"] <= bound)
        r["t_vec_new_inside_parent_spread"] = bool(r["t_vec_parent"]["min"] <= r["t_vec_new"]["ms"] <= r["t_vec_parent"]["max"])
        r["t_vec_new_not_above_parent_spread"] = bool(r["t_vec_new"]["ms"] <= r["t_vec_parent"]["max"])
        out["sizes"][str(n)] = r
        print(f"[dense_noise_profile] n={n}: " + json.dumps(r), file=sys.stderr, flush=True)
    out["c4_n_65536"] = "not measured"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
