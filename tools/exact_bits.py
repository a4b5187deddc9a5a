"""Every output array of the single-problem calls — exact (csrc/gpmi355.hip) and sparse (csrc/vfe.hpp) — on a fixed, seeded set of problems, stored
raw (.npz) beside its SHA-256 (.json): the single-path sibling of tools/batch_bits.py, for changes to the host drivers that must not move a launch.
Unlike the batch kernels the gradient kernels of this path add across workgroups with atomics, so some outputs differ from run to run of ONE build:
run the old build several times, compare the .json files for the outputs that are stable, and the raw arrays numerically for the ones that are not.

The set is the smallest at which the drivers can go wrong: n in {1, 100, 128, 129, 300} (one padded tile, the 128 boundary, three tiles) times D in
{1, 3, 16}, the categories cycling with different periods — the container layouts (vector / point-contiguous / dimension-contiguous), fp64 and fp32,
the four radial kinds with no scale, one scale and ARD, scalar, vector and dense noise, with and without a mean — then one D = 20 ARD problem (the
chunk-of-16 loops) and one composite kernel whose θ is longer than 16 entries, both at n = 129.  Test points ns in {1, 128, 129}, and 4 100 (across
the 4 096-row chunk) at n = 129.  Sparse fits at m in {64, 130} pseudo-points.  Everything runs on a default context and on one with "dib_nb" = 128,
where n = 300 takes the blocked solves and the dib_build branch of the gradient's L⁻ᵀ.

    GPMI355_LIB=<library> python tools/exact_bits.py --out bits.npz           # one process per library; writes bits.npz and bits.json"""
import argparse
import hashlib
import itertools
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SIZES = [1, 100, 128, 129, 300]
DIMS = [1, 3, 16]
POINTS = [1, 128, 129]
NS_CHUNKED = 4100  # n = 129 only
PSEUDO = [64, 130]


def container(agp, X, layout):
    """X (n, d) in the container that marshals to gp_points.layout: 0 a vector (d = 1), 1 point-contiguous, 2 dimension-contiguous"""
    if layout == 0:
        return np.ascontiguousarray(X[:, 0])
    return agp.RowVecs(np.ascontiguousarray(X) if layout == 1 else np.asfortranarray(X))


def problems(agp):
    """dicts with n, d, dt, layout, kernel k, mean, noise sigma2 (scalar / vector / dense), inputs X, observations y (n,) and Y (n, 3), seed"""
    radial = [agp.SqExponentialKernel, agp.Matern12Kernel, agp.Matern32Kernel, agp.Matern52Kernel]
    out = []
    for b, (n, d) in enumerate(itertools.product(SIZES, DIMS)):
        i, j = divmod(b, len(DIMS))  # size and dimension index: every category below meets every D, and the dtypes meet every layout
        rng = np.random.default_rng(2900 + b)
        dt = np.float64 if (i + j) % 2 == 0 else np.float32
        k = 1.3 * radial[b % 4]()
        if (b // 2) % 3 == 1:
            k = k @ agp.ScaleTransform(0.7)
        elif (b // 2) % 3 == 2:
            k = k @ agp.ARDTransform(np.linspace(0.5, 0.9, d))
        X = (rng.uniform(0.0, 4.0, size=(n, d)) / np.sqrt(d)).astype(dt)
        s2 = [1.3e-2, 1.3 * rng.uniform(1e-2, 5e-2, size=n), None][(i + j) % 3]
        if s2 is None:  # dense, SPD: a diagonal plus a rank-one term
            u = rng.standard_normal(n)
            s2 = np.diag(rng.uniform(2e-2, 5e-2, size=n)) + 1e-2 * np.outer(u, u) / n
        out.append(dict(n=n, d=d, dt=dt, layout=((i // 2) % 2 if d == 1 else 1 + i % 2), k=k, mean=(0.4 if b % 5 in (1, 3) else None), sigma2=s2, X=X, seed=b))
    SE, M32 = agp.SqExponentialKernel, agp.Matern32Kernel
    rng = np.random.default_rng(2990)
    out.append(dict(n=129, d=20, dt=np.float64, layout=2, k=1.1 * M32() @ agp.ARDTransform(np.linspace(0.4, 0.8, 20)), mean=None, sigma2=2e-2,
                    X=rng.uniform(0, 4, size=(129, 20)) / np.sqrt(20), seed=90))
    k4 = (0.9 * (SE() @ agp.ARDTransform([0.6, 0.7, 0.8, 0.9]) + M32() @ agp.ARDTransform([0.5, 0.4, 0.3, 0.6]))
          * (agp.PeriodicKernel(r=[1.0, 1.1, 1.2, 1.3]) @ agp.ARDTransform([0.3, 0.2, 0.25, 0.35]))
          + 0.2 * agp.RationalQuadraticKernel(alpha=0.8) @ agp.ScaleTransform(0.9))  # θ: 22 entries
    out.append(dict(n=129, d=4, dt=np.float64, layout=1, k=k4, mean=0.4, sigma2=0.1, X=rng.uniform(0, 3, size=(129, 4)), seed=91))
    for p in out:
        rng = np.random.default_rng(3100 + p["seed"])
        p["y"] = rng.standard_normal(p["n"]).astype(p["dt"])
        p["Y"] = np.asfortranarray(rng.standard_normal((p["n"], 3)).astype(p["dt"]))
    return out


def run_problem(agp, ctx, p, put):
    """put(name, array) for every output of every call on problem p"""
    api = agp.api
    n, d, dt, lay = p["n"], p["d"], p["dt"], p["layout"]
    composite = api._is_composite(p["k"])
    f = agp.GP(p["k"], ctx=ctx) if p["mean"] is None else agp.GP(p["mean"], p["k"], ctx=ctx)
    s2 = p["sigma2"] if np.ndim(p["sigma2"]) == 0 else np.asarray(p["sigma2"], dtype=dt)
    fx = f(container(agp, p["X"], lay), s2)
    y, Y = p["y"], p["Y"]
    rng = np.random.default_rng(3300 + p["seed"])

    def points(ns):
        return container(agp, (rng.uniform(0.0, 4.0, size=(ns, d)) / np.sqrt(d)).astype(dt), lay)

    def put_grad(tag, r):
        put(f"{tag}/value", r[0])
        for key, v in r[1].items():
            if v is not None and key != "mean":
                put(f"{tag}/{key}", v)

    ns_list = [POINTS[p["seed"] % 3], POINTS[(p["seed"] + 1) % 3]] + ([NS_CHUNKED] if n == 129 else [])
    put("kernelmatrix/xx", api.kernelmatrix(p["k"], fx.x, ctx=ctx))
    put("kernelmatrix/xz", api.kernelmatrix(p["k"], fx.x, points(ns_list[0]), ctx=ctx))
    put("logpdf/vector", api.logpdf(fx, y))
    put("logpdf/matrix", api.logpdf(fx, Y))
    ld, sq = api._terms(fx, Y, True, True)
    put("logpdf_terms/logdet", ld)
    put("logpdf_terms/sqmahal", sq)

    post = api.posterior(fx, y)
    put("posterior_fit/alpha", post.data.alpha)
    put("posterior_fit/logpdf", post.logpdf_value)
    for ns in ns_list:
        xs = points(ns)
        for what in (1, 2, 3) + ((7,) if ns != NS_CHUNKED else ()):
            for name, v in zip(("mean", "var", "cov"), post._predict(xs, what)):
                if v is not None:
                    put(f"predict/ns{ns}/what{what}/{name}", v)
        if d <= 16 or not composite:
            for what in (1, 2, 3):
                r = api._predict_grad(ctx.lib.gp_posterior_predict_grad, post.data.C.handle, dt, f.mean_fn, xs, what)
                for name, v in zip(("mean", "var", "dmean", "dvar"), r):
                    if v is not None:
                        put(f"predict_grad/ns{ns}/what{what}/{name}", v)
    xs = points(ns_list[1])
    ns = len(xs)
    s2s = 2e-2 if p["seed"] % 2 == 0 else rng.uniform(1e-2, 5e-2, size=ns).astype(dt)
    put("posterior_logpdf", api.logpdf(post(xs, s2s), rng.standard_normal((ns, 2)).astype(dt)))
    put("posterior_rand", api.rand(post(xs, s2s), 2, xi=rng.standard_normal((ns, 2))))
    put("posterior_solve", post.data.C.solve(rng.standard_normal((n, 2))))
    put("posterior_factor_mul", post.data.C.Ut_mul(rng.standard_normal((n, 2))))
    if np.ndim(p["sigma2"]) < 2:  # sequential conditioning on 5 more observations, then on 130 (two tiles of new rows)
        for n2 in (5, 130):
            up = api.posterior(post(points(n2), 3e-2), rng.standard_normal(n2).astype(dt))
            put(f"update/n{n2}/alpha", up.data.alpha)
            put(f"update/n{n2}/logpdf", up.logpdf_value)

    cp = api.posterior_columns(fx, Y)
    put("fit_cols/alpha", cp.data.alpha)
    put("fit_cols/logpdf", cp.logpdf_values)
    for ns in ns_list:
        put(f"predict_cols/ns{ns}/mean", cp.mean(points(ns)))
    put_grad("logpdf_grad_cols", api.logpdf_and_grad_columns(fx, Y, wrt_x=True))

    for name, v in zip(("value", "lp", "mean", "var"), api._loo(fx, y, "exact_bits")):
        put(f"loo/{name}", v)
    put_grad("loo_grad", api.loo_logpdf_and_grad(fx, y, wrt_x=True))
    put_grad("logpdf_grad", api.logpdf_and_grad(fx, y))
    put_grad("logpdf_grad_x", api.logpdf_and_grad(fx, y, wrt_x=True))

    if composite or np.ndim(p["sigma2"]) == 2:  # the sparse path takes single kinds and diagonal noise
        return
    for m in PSEUDO:
        approx = (agp.VFE if (p["seed"] + m) % 2 == 0 else agp.DTC)(f(points(m), 1e-6 if dt == np.float64 else 1e-3))
        vp = api.posterior(approx, fx, y)
        put(f"vfe/m{m}/objective", vp.objective)
        for ns in ns_list:
            xs = points(ns)
            for what in (1, 2, 3) + ((7,) if ns != NS_CHUNKED else ()):
                for name, v in zip(("mean", "var", "cov"), vp._predict(xs, what)):
                    if v is not None:
                        put(f"vfe/m{m}/predict/ns{ns}/what{what}/{name}", v)
            for what in (1, 2, 3):
                r = api._predict_grad(ctx.lib.gp_vfe_predict_grad, vp._state.handle, dt, f.mean_fn, xs, what)
                for name, v in zip(("mean", "var", "dmean", "dvar"), r):
                    if v is not None:
                        put(f"vfe/m{m}/predict_grad/ns{ns}/what{what}/{name}", v)
        xs = points(ns_list[1])
        put(f"vfe/m{m}/logpdf", api.logpdf(vp(xs, 2e-2), rng.standard_normal((len(xs), 2)).astype(dt)))
        put(f"vfe/m{m}/rand", api.rand(vp(xs, 2e-2), 2, xi=rng.standard_normal((len(xs), 2))))
        for key, v in vp.objective_grad(wrt_x=True).items():
            if v is not None and key != "mean":
                put(f"vfe/m{m}/grad/{key}", v)


def collect(out: Path):
    import abstractgps_jl_amd as agp

    arrays = {}
    for cname, params in (("default", {}), ("dib128", {"dib_nb": 128})):
        ctx = agp.api.Context(0)
        for key, v in params.items():
            ctx.set_param(key, v)
        for i, p in enumerate(problems(agp)):
            tag = f"{cname}/{i:02d}_n{p['n']}_d{p['d']}_l{p['layout']}_{np.dtype(p['dt']).name}"

            def put(name, a, tag=tag):
                assert f"{tag}/{name}" not in arrays, name
                arrays[f"{tag}/{name}"] = np.array(a, copy=True)

            run_problem(agp, ctx, p, put)
        ctx.close()
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez(out, **arrays)
    digests = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in arrays.items()}
    out.with_suffix(".json").write_text(json.dumps(digests, indent=0, sort_keys=True) + "\n")
    print(f"{len(arrays)} outputs -> {out} (+ .json)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    collect(Path(ap.parse_args().out))


if __name__ == "__main__":
    main()
