"""SHA-256 of every output array of the three batch entry points on a fixed, seeded set of problems: what a change that must not move a rounding is
checked with.  The library promises a fixed schedule per problem (csrc/batch.hip), so two builds that compute the same thing write the same file, byte
for byte; a difference names the call, the problem and the output that changed.

The set is the smallest that reaches every branch of the kernels' shared tile code: n in {1, 63, 64, 65, 130, 321, 700} (one block, the block boundary,
three blocks with more than eight trailing wave tiles, inverse tiles from rows 0 / 128 / 256, a second trip of the tid + NT loops), D in {1, 3, 16}, the
four radial kinds with no scale, one scale and ARD, scalar and diagonal noise, with and without a mean, α wanted and not, one problem that fails (a
negative noise entry), two composite kernels (a sum with a product and a Periodic factor; one whose θ is longer than one pass of 16 entries), test
points ns in {0, 1, 33, 128, 129, 300} with what in {1, 2, 3}, and one call with x, y and xs shared by every problem.  The same problems go through
gp_predict_grad_batch and gp_logpdf_grad_batch_x (and their _sum forms) with the containers of xs / x cycling over the layouts, since those gradients
come back in the container's layout.  The GPMI_BATCH_*_MAX_N limits are set to the kernels' own, and the served-problem counter of every gradient
family ("batch_grad_kernel_problems", "batch_pgrad_kernel_problems", "batch_gradx_kernel_problems") must count every problem of its calls.

    GPMI355_LIB=<library> python tools/batch_bits.py --out bits.json      # one process per library; compare the files"""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SIZES = [1, 63, 64, 65, 130, 321, 700]
DIMS = [1, 3, 16]
POINTS = [0, 1, 33, 128, 129, 300]


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def single_kind_problems(agp):
    """(fx, y) per problem: three per size, the categories cycling with different periods; then the one that fails"""
    out = []
    for i, n in enumerate(SIZES):
        for v in range(3):
            b = 3 * i + v
            rng = np.random.default_rng(9000 + b)
            d = DIMS[(b + i) % 3]
            X = rng.uniform(0.0, 4.0, size=(n, d)) / np.sqrt(d)
            y = rng.standard_normal(n)
            k = 1.3 * [agp.SqExponentialKernel, agp.Matern12Kernel, agp.Matern32Kernel, agp.Matern52Kernel][b % 4]()
            if (b // 2) % 3 == 1:
                k = k @ agp.ScaleTransform(0.7)
            elif (b // 2) % 3 == 2:
                k = k @ agp.ARDTransform(np.linspace(0.5, 0.9, d))
            s2 = 1.3e-2 if b % 2 == 0 else 1.3 * rng.uniform(1e-2, 5e-2, size=n)
            f = agp.GP(k) if (b // 3) % 2 == 0 else agp.GP(0.4, k)
            out.append((f(agp.RowVecs(X), s2), y))
    fx, y = out[13]  # n = 130, three blocks: the factorisation stops inside the second one
    s2 = fx.noise_vector().copy()
    s2[int(0.6 * 129)] = -10.0
    out.append((agp.FiniteGP(fx.f, fx.x, s2), y))
    return out


def composite_problems(agp):
    SE, M32 = agp.SqExponentialKernel, agp.Matern32Kernel
    rng = np.random.default_rng(41)
    X1 = rng.uniform(0, 3, size=(130, 1))
    X4 = rng.uniform(0, 3, size=(200, 4))
    k1 = SE() @ agp.ScaleTransform(0.5) + 0.5 * M32() * agp.PeriodicKernel(r=[0.9])
    k4 = (0.9 * (SE() @ agp.ARDTransform([0.6, 0.7, 0.8, 0.9]) + M32() @ agp.ARDTransform([0.5, 0.4, 0.3, 0.6]))
          * (agp.PeriodicKernel(r=[1.0, 1.1, 1.2, 1.3]) @ agp.ARDTransform([0.3, 0.2, 0.25, 0.35]))
          + 0.2 * agp.RationalQuadraticKernel(alpha=0.8) @ agp.ScaleTransform(0.9))
    return [(agp.GP(k1)(agp.RowVecs(X1), 0.05), np.sin(X1[:, 0]) + 0.1 * rng.standard_normal(130)),
            (agp.GP(k4)(agp.RowVecs(X4), 0.1), np.cos(X4[:, 0]) + 0.1 * rng.standard_normal(200))]


def shared_problems(agp):
    """three kernels over ONE x, ONE y and ONE xs object"""
    rng = np.random.default_rng(77)
    x = agp.RowVecs(rng.uniform(0, 4, size=(130, 3)))
    y = rng.standard_normal(130)
    xs = agp.RowVecs(rng.uniform(0, 4, size=(33, 3)))
    ks = [1.3 * agp.SqExponentialKernel(), 0.8 * agp.Matern32Kernel() @ agp.ScaleTransform(0.7), 1.1 * agp.Matern52Kernel() @ agp.ARDTransform([0.5, 0.7, 0.9])]
    return [agp.GP(k)(x, 2e-2) for k in ks], y, xs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.environ["GPMI_BATCH_MAX_N"] = "2048"
    os.environ["GPMI_BATCH_GRAD_MAX_N"] = "2048"
    os.environ["GPMI_BATCH_PGRAD_MAX_N"] = "2048"
    os.environ["GPMI_BATCH_GRADX_MAX_N"] = "2048"
    import abstractgps_jl_amd as agp

    api = agp.api
    ctx = agp.default_context(0)
    digests = {}

    def run(call):
        rc = getattr(ctx.lib, call.entry)(ctx.handle, *call.args)
        assert rc == 0, (call.entry, rc)

    def put(tag, b, name, arr):
        if arr is not None:
            digests[f"{tag}/{b:02d}/{name}"] = sha(arr)

    def fit(tag, fxs, ys):
        for want_alpha in (True, False):
            (g,) = api._batch_groups(fxs, ys)
            call = api._batch_marshal(g, want_alpha)
            run(call)
            for b in range(call.nb):
                t = f"{tag}/{'alpha' if want_alpha else 'value'}"
                put(t, b, "logpdf", call.out[b])
                put(t, b, "info", call.info[b])
                if want_alpha:
                    put(t, b, "alpha", call.alphas[b])
        return call.info

    def predict(tag, fxs, ys, xss):
        for what in (1, 2, 3):
            (g,) = api._predict_groups(fxs, ys, xss)
            call = api._predict_marshal(g, what)
            run(call)
            for b in range(call.nb):
                t = f"{tag}/what{what}"
                put(t, b, "logpdf", call.out[b])
                put(t, b, "info", call.info[b])
                put(t, b, "mean", call.means[b] if call.means is not None else None)
                put(t, b, "var", call.vars[b] if call.vars is not None else None)

    def grad(tag, fxs, ys):
        (g,) = api._batch_groups(fxs, ys)
        call = api._grad_batch_marshal(g)
        before = ctx.get_param("batch_grad_kernel_problems")
        run(call)
        assert ctx.get_param("batch_grad_kernel_problems") - before == call.nb, "the gradient kernels did not serve every problem"
        for b in range(call.nb):
            put(tag, b, "logpdf", call.out[b])
            put(tag, b, "info", call.info[b])
            put(tag, b, "dvariance", call.dvar[b] if call.dvar is not None else None)
            put(tag, b, "dscale", call.dscale[b] if call.dscale is not None else None)
            put(tag, b, "dtheta", call.dtheta[b] if call.dtheta is not None else None)
            put(tag, b, "dnoise", call.dnoise[b])
            put(tag, b, "dy", call.dy[b])

    def relayout(x, b):
        """the points of x in the b-th of the container layouts the ABI knows: point-contiguous, dimension-contiguous, and for D = 1 a vector"""
        X = np.asarray(x.X)
        if X.shape[1] == 1 and b % 3 == 2:
            return np.ascontiguousarray(X[:, 0])
        return agp.RowVecs(np.ascontiguousarray(X) if b % 2 == 0 or X.shape[0] < 2 else np.asfortranarray(X))

    def counted(call, counter):
        before = ctx.get_param(counter)
        run(call)
        assert ctx.get_param(counter) - before == call.nb, f"{counter}: the kernels did not serve every problem"

    def predict_grad(tag, fxs, ys, xss):
        """gp_predict_grad_batch / _sum: the gradients come back in the container layout of each xs_b, so the layouts cycle"""
        xss = xss if not isinstance(xss, list) else [relayout(xs, b) for b, xs in enumerate(xss)]
        for what in (1, 2, 3):
            (g,) = api._predict_groups(fxs, ys, xss)
            call = api._predict_grad_marshal(g, what)
            counted(call, "batch_pgrad_kernel_problems")
            for b in range(call.nb):
                t = f"{tag}/what{what}"
                put(t, b, "logpdf", call.out[b])
                put(t, b, "info", call.info[b])
                for name, arrs in (("mean", call.means), ("var", call.vars), ("dmean", call.dmeans), ("dvar", call.dvars)):
                    put(t, b, name, arrs[b] if arrs is not None else None)

    def gradx(tag, fxs, ys):
        """gp_logpdf_grad_batch_x / _sum_x: dx in the container layout of each x_b (the layouts cycle unless the problems share one x)"""
        if len({id(fx.x) for fx in fxs}) == len(fxs):
            fxs = [agp.FiniteGP(fx.f, relayout(fx.x, b), fx.sigma2) for b, fx in enumerate(fxs)]
        (g,) = api._batch_groups(fxs, ys)
        call = api._grad_batch_marshal(g, wrt_x=True)
        counted(call, "batch_gradx_kernel_problems")
        for b in range(call.nb):
            put(tag, b, "logpdf", call.out[b])
            put(tag, b, "info", call.info[b])
            put(tag, b, "dnoise", call.dnoise[b])
            put(tag, b, "dy", call.dy[b])
            put(tag, b, "dx", call.dx[b])

    def points(fxs, seed, first):
        """ns cycles over POINTS from POINTS[first] on, shifted so that every size of the set meets several of them"""
        rng = np.random.default_rng(seed)
        return [agp.RowVecs(rng.uniform(0, 4, size=(POINTS[(first + b + b // 6) % 6], fx.x.X.shape[1]))) for b, fx in enumerate(fxs)]

    for name, probs in (("single", single_kind_problems(agp)), ("composite", composite_problems(agp))):
        fxs, ys = [p[0] for p in probs], [p[1] for p in probs]
        info = fit(f"fit/{name}", fxs, ys)
        assert np.count_nonzero(info) == (1 if name == "single" else 0), info
        xss = points(fxs, 500, 0 if name == "single" else 4)
        predict(f"predict/{name}", fxs, ys, xss)
        grad(f"grad/{name}", fxs, ys)
        predict_grad(f"predict_grad/{name}", fxs, ys, xss)
        gradx(f"gradx/{name}", fxs, ys)
    fxs, y, xs = shared_problems(agp)
    fit("fit/shared", fxs, y)
    predict("predict/shared", fxs, y, xs)
    grad("grad/shared", fxs, y)
    predict_grad("predict_grad/shared", fxs, y, xs)
    gradx("gradx/shared", fxs, y)

    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(digests, indent=0, sort_keys=True) + "\n")
    print(f"{len(digests)} digests -> {a.out}")


if __name__ == "__main__":
    main()
