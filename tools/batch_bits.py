"""SHA-256 of every output array of the batch entry points on a fixed, seeded set of problems: what a change that must not move a rounding is
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

gp_joint_batch (what in {1, 4, 8, 16, 29}, three draws, Σy* cycling over absent, scalar and diagonal, the test points of the predictions), gp_loo_batch (all
three per-point arrays, ℓ alone, none) and gp_loo_grad_batch go the same way, under their own limits and counters.  A "routed" pass sets every limit to 0 and
the ctx to its deterministic schedule and sends the single-kind and the composite set once through every family, so the single-path loops and their NaN
fills are recorded; no served-problem counter may move there.  It runs twice: an output whose digest differs between the two runs is not bit-stable on the
single path and is listed under "unstable" in --routed-values' file, which also keeps the arrays of both runs, so that such an output can be compared by
value.  An "errors" pass makes one bad call per argument check of the batch drivers — each a valid marshalled call with one argument replaced, refused
before anything is launched or dereferenced — and records (status, gp_last_error()).

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
LIMITS = ["GPMI_BATCH_MAX_N", "GPMI_BATCH_GRAD_MAX_N", "GPMI_BATCH_PGRAD_MAX_N", "GPMI_BATCH_GRADX_MAX_N", "GPMI_BATCH_JOINT_MAX_N", "GPMI_BATCH_JOINT_MAX_NS",
          "GPMI_BATCH_LOO_MAX_N", "GPMI_BATCH_LOO_GRAD_MAX_N"]
COUNTERS = ["batch_grad_kernel_problems", "batch_pgrad_kernel_problems", "batch_gradx_kernel_problems", "batch_joint_kernel_problems",
            "batch_loo_kernel_problems", "batch_loo_grad_kernel_problems"]


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
    ap.add_argument("--routed-values", help="npz: the arrays of both runs of the routed pass, and the keys whose digests differ between them")
    a = ap.parse_args()
    os.environ["GPMI_BATCH_MAX_N"] = "2048"
    os.environ["GPMI_BATCH_GRAD_MAX_N"] = "2048"
    os.environ["GPMI_BATCH_PGRAD_MAX_N"] = "2048"
    os.environ["GPMI_BATCH_GRADX_MAX_N"] = "2048"
    for v in LIMITS[4:]:
        os.environ[v] = "2048"
    import abstractgps_jl_amd as agp

    api = agp.api
    ctx = agp.default_context(0)
    digests, values = {}, {}

    def run(call):
        rc = getattr(ctx.lib, call.entry)(ctx.handle, *call.args)
        assert rc == 0, (call.entry, rc)

    def put(tag, b, name, arr):
        if arr is not None:
            digests[f"{tag}/{b:02d}/{name}"] = sha(arr)
            values[f"{tag}/{b:02d}/{name}"] = np.array(arr)

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
        put_grad(tag, call)

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

    def joint_inputs(fxs, xss):
        """per problem: Σy* (absent, a scalar, a diagonal: cycling; no diagonal over no points), held-out observations and three columns of normals"""
        xss = xss if isinstance(xss, list) else [xss] * len(fxs)
        noises, yh, xi = [], [], []
        for b, xs in enumerate(xss):
            rng = np.random.default_rng(7000 + b)
            ns = xs.X.shape[0]
            noises.append([None, 3e-2, rng.uniform(1e-2, 5e-2, size=ns) if ns else 3e-2][b % 3])
            yh.append(rng.standard_normal(ns))
            xi.append(rng.standard_normal((ns, 3)))
        return noises, yh, xi

    def put_joint(t, call):
        for b in range(call.nb):
            put(t, b, "logpdf", call.out[b])
            put(t, b, "info", call.info[b])
            put(t, b, "info_joint", call.info_joint[b])
            put(t, b, "heldout", call.heldout[b] if call.heldout is not None else None)
            for name, arrs in (("mean", call.means), ("cov", call.covs), ("samples", call.samples)):
                put(t, b, name, arrs[b] if arrs is not None else None)

    def joint(tag, fxs, ys, xss, whats=(1, 4, 8, 16, 29), counter="batch_joint_kernel_problems"):
        noises, yh, xi = joint_inputs(fxs, xss)
        for what in whats:
            (g,) = api._predict_groups(fxs, ys, xss)
            call = api._joint_marshal(g, what, noises, yh, xi)
            counted(call, counter) if counter else run(call)
            put_joint(f"{tag}/what{what}", call)

    def loo(tag, fxs, ys, wants=((True, True), (True, False), (False, False)), counter="batch_loo_kernel_problems"):
        for want_lp, want_pred in wants:
            (g,) = api._batch_groups(fxs, ys)
            call = api._loo_batch_marshal(g, want_lp, want_pred)
            counted(call, counter) if counter else run(call)
            for b in range(call.nb):
                t = f"{tag}/{'all' if want_pred else 'lp' if want_lp else 'value'}"
                put(t, b, "value", call.out[b])
                put(t, b, "info", call.info[b])
                for name, arrs in (("lp", call.lp), ("mean", call.mean), ("var", call.var)):
                    put(t, b, name, arrs[b] if arrs is not None else None)

    def put_grad(tag, call):
        for b in range(call.nb):
            put(tag, b, "logpdf", call.out[b])
            put(tag, b, "info", call.info[b])
            put(tag, b, "dvariance", call.dvar[b] if call.dvar is not None else None)
            put(tag, b, "dscale", call.dscale[b] if call.dscale is not None else None)
            put(tag, b, "dtheta", call.dtheta[b] if call.dtheta is not None else None)
            put(tag, b, "dnoise", call.dnoise[b])
            put(tag, b, "dy", call.dy[b])
            put(tag, b, "dx", call.dx[b] if call.dx is not None else None)

    def loo_grad(tag, fxs, ys, wrt_x=False, counter="batch_loo_grad_kernel_problems"):
        (g,) = api._batch_groups(fxs, ys)
        call = api._loo_grad_batch_marshal(g, wrt_x)
        counted(call, counter) if counter else run(call)
        put_grad(tag, call)

    def routed(fxs, ys, xss, name):
        """every family once on the single path: the limits are 0, so no kernel of this file serves a problem and no counter moves"""
        before = [ctx.get_param(c) for c in COUNTERS]
        (g,) = api._batch_groups(fxs, ys)
        call = api._batch_marshal(g, True)
        run(call)
        for b in range(call.nb):
            put(f"routed/fit/{name}", b, "logpdf", call.out[b])
            put(f"routed/fit/{name}", b, "info", call.info[b])
            put(f"routed/fit/{name}", b, "alpha", call.alphas[b])
        for marshal, fam in ((api._predict_marshal, "predict"), (api._predict_grad_marshal, "predict_grad")):
            (g,) = api._predict_groups(fxs, ys, xss)
            call = marshal(g, 3)
            run(call)
            for b in range(call.nb):
                t = f"routed/{fam}/{name}"
                put(t, b, "logpdf", call.out[b])
                put(t, b, "info", call.info[b])
                for out in ("means", "vars", "dmeans", "dvars"):
                    put(t, b, out[:-1], getattr(call, out)[b] if getattr(call, out, None) is not None else None)
        joint(f"routed/joint/{name}", fxs, ys, xss, whats=(29,), counter=None)
        for wrt_x in (False, True):
            (g,) = api._batch_groups(fxs, ys)
            call = api._grad_batch_marshal(g, wrt_x=wrt_x)
            run(call)
            put_grad(f"routed/{'gradx' if wrt_x else 'grad'}/{name}", call)
        loo(f"routed/loo/{name}", fxs, ys, wants=((True, True),), counter=None)
        loo_grad(f"routed/loo_grad/{name}", fxs, ys, counter=None)
        loo_grad(f"routed/loo_grad_x/{name}", fxs, ys, wrt_x=True, counter=None)
        assert [ctx.get_param(c) for c in COUNTERS] == before, "a served-problem counter moved on the single path"

    def errors(name, fxs, ys, xss):
        """(status, message) of one bad call per argument check.  Positions are those of call.args (the ABI's argument number less 2)."""
        keep = []

        def null_at(arr, j=1):  # a pointer array with element j NULL
            keep.append(type(arr)(*[None if q == j else arr[q] for q in range(len(arr))]))
            return keep[-1]

        def points_with(arr, **fields):  # a gp_points array whose last entry has other fields
            cp = type(arr)(*[type(arr[q])(arr[q].data, arr[q].n, arr[q].d, arr[q].layout) for q in range(len(arr))])
            for f, v in fields.items():
                setattr(cp[len(arr) - 1], f, v)
            keep.append(cp)
            return cp

        def other_dtype(arr):  # a descriptor array whose second entry carries the other dtype
            cp = type(arr)(*[arr[q] for q in range(len(arr))])
            cp[1].dtype = 1 - arr[1].dtype
            keep.append(cp)
            return cp

        def bad(fam, what, call, repl, handle=True):
            args = list(call.args)
            for i, v in repl.items():
                args[i] = v
            rc = getattr(ctx.lib, call.entry)(ctx.handle if handle else None, *args)
            assert rc < 0, (call.entry, what, rc)
            digests[f"errors/{fam}/{name}/{what}"] = [int(rc), ctx.lib.gp_last_error().decode(errors="replace")]

        def head(fam, call, info_at, lp_at=None):
            nb, a = call.nb, call.args
            bad(fam, "handle", call, {}, handle=False)
            bad(fam, "nb", call, {0: -1})
            bad(fam, "k", call, {1: None})
            bad(fam, "nx", call, {2: nb + 1})
            bad(fam, "x", call, {3: None})
            bad(fam, "noise", call, {4: None})
            bad(fam, "ny", call, {6: nb + 1})
            bad(fam, "y", call, {7: None})
            bad(fam, "y_elem", call, {7: null_at(a[7])})
            bad(fam, "info", call, {info_at: None})
            if lp_at is not None:
                bad(fam, "logpdf_out", call, {lp_at: None})

        def test_points(fam, call, outs):
            """nxs, xs and what at positions 8, 9 and what_at; outs: (name, position) of the output arrays every problem with test points needs"""
            a = call.args
            bad(fam, "nxs", call, {8: call.nb + 1})
            bad(fam, "xs", call, {9: None})
            bad(fam, "xs_n", call, {9: points_with(a[9], n=-1)})
            bad(fam, "xs_d", call, {9: points_with(a[9], d=a[9][len(a[9]) - 1].d + 1)})
            for out, at in outs:
                bad(fam, f"{out}_elem", call, {at: null_at(a[at], call.nb - 1)})

        (g,) = api._batch_groups(fxs, ys)
        call = api._batch_marshal(g, True)
        head("fit", call, 9, 8)
        bad("fit", "dtype", call, {1: other_dtype(call.args[1])})
        bad("fit", "shared_y_sizes", call, {6: 1})

        (g,) = api._predict_groups(fxs, ys, xss)
        call = api._predict_marshal(g, 3)
        head("predict", call, 15)
        test_points("predict", call, (("mean", 12), ("var", 13)))
        for what in (0, 4):
            bad("predict", f"what{what}", call, {11: what})
        bad("predict", "mean", call, {12: None})
        bad("predict", "var", call, {13: None})

        call = api._predict_grad_marshal(g, 3)
        head("predict_grad", call, 17)
        test_points("predict_grad", call, (("mean", 12), ("var", 13), ("dmean", 14), ("dvar", 15)))
        bad("predict_grad", "what0", call, {11: 0})
        bad("predict_grad", "mean_and_dmean", call, {12: None, 14: None})
        bad("predict_grad", "var_and_dvar", call, {13: None, 15: None})

        call = api._joint_marshal(g, 29, *joint_inputs(fxs, xss))
        head("joint", call, 21)
        test_points("joint", call, (("mean", 13), ("cov", 14), ("ys", 15), ("xi", 18), ("samples", 19)))
        for what in (0, 2):
            bad("joint", f"what{what}", call, {12: what})
        for out, at in (("mean", 13), ("cov", 14), ("ys", 15), ("hlogpdf", 16), ("xi", 18), ("samples", 19)):
            bad("joint", out, call, {at: None})
        bad("joint", "nsamp", call, {17: -1})

        (g,) = api._batch_groups(fxs, ys)
        first = 10 if g.composite else 11  # dtheta, or dscale behind dvariance
        for fam, call in (("grad", api._grad_batch_marshal(g)), ("gradx", api._grad_batch_marshal(g, wrt_x=True)),
                          ("loo_grad", api._loo_grad_batch_marshal(g, True))):
            head(fam, call, 9, 8)
            for out, at in zip(("dtheta" if g.composite else "dscale", "dnoise", "dy", "dx"), range(first, len(call.args))):
                bad(fam, f"{out}_elem", call, {at: null_at(call.args[at])})
        call = api._loo_batch_marshal(g)
        head("loo", call, 9, 8)
        for out, at in (("lp", 10), ("mean", 11), ("var", 12)):
            bad("loo", f"{out}_elem", call, {at: null_at(call.args[at])})

    def points(fxs, seed, first):
        """ns cycles over POINTS from POINTS[first] on, shifted so that every size of the set meets several of them"""
        rng = np.random.default_rng(seed)
        return [agp.RowVecs(rng.uniform(0, 4, size=(POINTS[(first + b + b // 6) % 6], fx.x.X.shape[1]))) for b, fx in enumerate(fxs)]

    sets = {}
    for name, probs in (("single", single_kind_problems(agp)), ("composite", composite_problems(agp))):
        fxs, ys = [p[0] for p in probs], [p[1] for p in probs]
        info = fit(f"fit/{name}", fxs, ys)
        assert np.count_nonzero(info) == (1 if name == "single" else 0), info
        xss = points(fxs, 500, 0 if name == "single" else 4)
        predict(f"predict/{name}", fxs, ys, xss)
        grad(f"grad/{name}", fxs, ys)
        predict_grad(f"predict_grad/{name}", fxs, ys, xss)
        gradx(f"gradx/{name}", fxs, ys)
        joint(f"joint/{name}", fxs, ys, xss)
        loo(f"loo/{name}", fxs, ys)
        loo_grad(f"loo_grad/{name}", fxs, ys)
        sets[name] = (fxs, ys, xss)
    fxs, y, xs = shared_problems(agp)
    fit("fit/shared", fxs, y)
    predict("predict/shared", fxs, y, xs)
    grad("grad/shared", fxs, y)
    predict_grad("predict_grad/shared", fxs, y, xs)
    gradx("gradx/shared", fxs, y)
    joint("joint/shared", fxs, y, xs)
    loo("loo/shared", fxs, y)
    loo_grad("loo_grad/shared", fxs, y)

    # one bad call per argument check: problems 2..4 of the single-kind set (n = 1, 63, 63: sizes that one shared y cannot serve; every kernel has scales)
    # with five test points each, and the composite set
    for name, (fxs, ys, _) in sets.items():
        sub = slice(2, 5) if name == "single" else slice(None)
        fxs, ys = fxs[sub], ys[sub]
        rng = np.random.default_rng(600)
        errors(name, fxs, ys, [agp.RowVecs(rng.uniform(0, 4, size=(5, fx.x.X.shape[1]))) for fx in fxs])

    for v in LIMITS:
        os.environ[v] = "0"
    ctx.set_param("deterministic", 1)
    served, runs = dict(digests), []
    for _ in range(2):  # twice: what the single path does not reproduce itself cannot be compared by digest
        digests, values = {}, {}
        for name, (fxs, ys, xss) in sets.items():
            routed(fxs, ys, xss, name)
        runs.append((digests, values))
    unstable = sorted(k for k in runs[0][0] if runs[0][0][k] != runs[1][0][k])
    print(f"routed: {len(runs[0][0])} outputs, {len(unstable)} differ between two runs of this library: {unstable[:20]}")
    digests = {**served, **runs[0][0]}
    if a.routed_values:
        Path(a.routed_values).parent.mkdir(parents=True, exist_ok=True)
        np.savez_compressed(a.routed_values, unstable=np.array(unstable, dtype=str), **{f"run{r}/{k}": v for r in (0, 1) for k, v in runs[r][1].items()})

    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(digests, indent=0, sort_keys=True) + "\n")
    print(f"{len(digests)} digests -> {a.out}")


if __name__ == "__main__":
    main()
