"""Scenarios of tests/test_gpu_threads.py: the C ABI called from several host threads at once.  `python -m tests.thread_cases <group>` (group: AB, CDE, FG, HI)
runs the scenarios of the group in THIS process — every context is created here, the pytest process holds none of them — and prints one JSON line per
scenario: name, ok, the compared quantities (largest error of each), the worst ratio of an error to its bound, the number of pairs of calls from different
threads whose host intervals [start, end] overlap, seconds, and the failures in words.

What is promised (include/gpmi355.h "Conventions", INTEGRATION.md §2, csrc/engine.hpp Guard): any entry point from any OS thread; calls on one ctx serialised by
its mutex; gp_last_error() thread-local; a call on a handle cannot race a *_free / gp_ctx_destroy of it from another thread — it either completes or is refused
with −1 "not a live ...".

References: oracle/gp_oracle.py for values, and — wherever the path is bitwise repeatable ("deterministic" = 1, "gemm_streamk" = 0: the fp64 exact path and the
batch kernel) — a SERIAL pass of the same list of (inputs, call) items made in this process before any thread starts.  Every ctx is set to deterministic = 1,
gemm_streamk = 0, nb = 512, lookahead_min_n = 0: both ctx streams and the look-ahead are in play at N = 1 537 / 2 049 (four / five panels, neither a multiple of
128).  The bounds are the suite's own; each names the test it comes from.  Threads are threading.Thread objects released together by a threading.Barrier; the
library is a ctypes.CDLL, so the GIL is released during every call.

Non-vacuity: a scenario of A–E, G, I whose threaded pass shows no overlapping pair of calls fails."""
import ctypes as C
import json
import math
import queue
import sys
import threading
import time
import traceback

import numpy as np

import abstractgps_jl_amd as agp
from oracle import gp_oracle as o
from tests import batch_cases as bc
from tests.composite_ref import ml_kernel, dense_data, ref_kernelmatrix

api = agp.api
CTX_PARAMS = {"deterministic": 1, "gemm_streamk": 0, "nb": 512, "lookahead_min_n": 0}
N_SMALL, N_LARGE, D, NS = 1537, 2049, 3, 64
LOOPS = 30                      # iterations of every fit / predict / free loop: enough for 67 or more overlapping call pairs in every scenario (profiles/r14/threads.log)
NEEDS_OVERLAP = set("ABCDEGI")
# fp64 exact path against the oracle: tests/test_gpu_parity.py (module docstring; test_mid_size_parity)
LP_REL, ALPHA_REL, MEAN_ABS, VAR_ABS = 1e-10, 1e-8, 1e-8, 1e-9
# fp32 exact path against the fp64 oracle ("1e-4 … 5e-3", tests/test_gpu_units_f32.py docstring): logpdf tests/test_gpu_parity.py
# test_float32_type_stability_and_accuracy (N = 1 500, σ² = 0.1, unit Matern52 — the kernel and noise of scenario B's fp32 thread), α test_float32_gradient_update_and_rand, predictive mean
# tests/test_gpu_composite.py test_fp32_composite_fit (relative 2-norm); the logpdf of the fp32 gradient call: test_float32_gradient_update_and_rand (2e-4)
F32_LP_REL, F32_ALPHA_REL, F32_MEAN_REL, F32_GRAD_LP_REL, F32_GRAD_REL = 1e-4, 5e-3, 5e-3, 2e-4, 5e-3
# fp64 VFE against the oracle: tests/test_gpu_parity.py test_vfe_schedule_variants (objective rel 1e-8, mean / var abs 1e-6), test_vfe_grad_vs_golden (every
# gradient block to 1e-5 of max(1, its largest component))
VFE_OBJ_REL, VFE_PRED_ABS, VFE_GRAD_REL = 1e-8, 1e-6, 1e-5
# composite kernels against a host Cholesky: tests/test_gpu_composite.py test_logpdf_and_alpha_against_a_host_cholesky
SUM_LP_REL, SUM_ALPHA_REL = 1e-10, 1e-8
# gp_kernelmatrix: tests/test_gpu_parity.py test_kernelmatrix_vs_oracle (abs <= 1e-14·σ², exactly symmetric)
KMAT_ABS = 1e-14
# the batch entry points: tests/test_gpu_batch.py LP_TOL / A_TOL (logpdf relative to max(|ref|, 1), tests/batch_cases.py lp_err)
BATCH_LP, BATCH_ALPHA = 1e-10, 1e-8


# ---- bookkeeping ----------------------------------------------------------------------------------------------------------------------------
class Log:
    """[thread, start, end] of every library call (time.perf_counter around it); list.append is atomic under the GIL"""

    def __init__(self):
        self.iv = []

    def call(self, tid, fn, *a, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*a, **kw)
        finally:
            self.iv.append((tid, t0, time.perf_counter()))

    def overlapping_pairs(self) -> int:
        iv = sorted(self.iv, key=lambda r: r[1])
        n = 0
        for i, (ti, _, ei) in enumerate(iv):
            for tj, sj, _ in iv[i + 1:]:
                if sj > ei:
                    break
                n += ti != tj
        return n


class Report:
    def __init__(self, name):
        self.name, self.q, self.worst, self.fail, self.t0 = name, {}, 0.0, [], time.perf_counter()
        self.pairs, self.extra = None, {}

    def bound(self, what, err, bound):
        err = float(err)
        r = err / bound if math.isfinite(err) else math.inf
        self.q[what] = max(self.q.get(what, 0.0), err) if math.isfinite(err) else math.inf
        self.worst = max(self.worst, r)
        if not r <= 1.0:
            self._fail(f"{what}: {err:.3e} > {bound:.1e}")

    def bits(self, what, a, b):
        a, b = np.asarray(a), np.asarray(b)
        same = a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        self.q.setdefault("bitwise_mismatches", 0)
        if not same:
            self.q["bitwise_mismatches"] += 1
            self.worst = math.inf
            nd = int(np.sum(a != b)) if a.shape == b.shape else -1
            self._fail(f"{what}: not the bits of the serial pass ({nd} of {a.size} entries differ)")

    def require(self, what, cond, detail=""):
        if not cond:
            self.worst = math.inf
            self._fail(f"{what}: {detail}")

    def _fail(self, msg):
        if len(self.fail) < 12:
            self.fail.append(msg)
        elif len(self.fail) == 12:
            self.fail.append("... (more)")

    def line(self) -> str:
        if self.pairs is not None and self.name in NEEDS_OVERLAP and self.pairs == 0:
            self._fail("no two calls of different threads overlapped: the scenario tested nothing")
        fin = lambda v: v if not isinstance(v, float) or math.isfinite(v) else repr(v)
        return json.dumps({"name": self.name, "ok": not self.fail, "quantities": {k: fin(v) for k, v in self.q.items()}, "worst_ratio": fin(self.worst),
                           "overlap_pairs": self.pairs, "seconds": round(time.perf_counter() - self.t0, 3), "failures": self.fail, **self.extra})


def run_threads(fns):
    """every fn on a thread of its own, released together; returns their results, raises the first traceback"""
    bar = threading.Barrier(len(fns))
    res, err = [None] * len(fns), [None] * len(fns)

    def wrap(i):
        try:
            bar.wait()
            res[i] = fns[i]()
        except BaseException:
            err[i] = traceback.format_exc()

    ts = [threading.Thread(target=wrap, args=(i,), name=f"case-thread-{i}") for i in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    bad = [e for e in err if e]
    if bad:
        raise RuntimeError("a thread raised:\n" + "\n".join(bad))
    return res


def new_ctx(extra=None, **kw):
    c = agp.Context(**kw) if kw else agp.Context(0)
    for k, v in {**CTX_PARAMS, **(extra or {})}.items():
        c.set_param(k, v)
    return c


def relnorm(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


# ---- the kinds of work: call(ctx, inputs, log, tid) -> outputs; against_serial / against_oracle compare them ------------------------------------
def exact_inputs(n, kind, seed, s2=0.01, dtype=np.float64, var=1.2, scale=0.7):
    X, y = o.synth_inputs(n, D, seed)
    X, y = X.astype(dtype), y.astype(dtype)
    return {"n": n, "kind": kind, "X": X, "y": y, "xs": (X[:NS] + dtype(0.05)).astype(dtype), "s2": dtype(s2), "var": var, "scale": scale, "dtype": dtype,
            "tag": f"n{n}k{kind}{'f32' if dtype == np.float32 else ''}"}


def _kernel(inp):
    return inp["var"] * agp.Kernel(inp["kind"]) @ agp.ScaleTransform(inp["scale"])


_ORACLE = {}


def exact_oracle(inp):
    key = ("exact", inp["tag"], id(inp["X"]))
    if key not in _ORACLE:
        X, y, xs = (np.asarray(inp[k], dtype=np.float64) for k in ("X", "y", "xs"))
        lp, post = o.logpdf_and_posterior(o.FiniteGP(o.GP(o.Kernel(inp["kind"], inp["var"], inp["scale"])), X, float(inp["s2"])), y)
        m, v = post.mean_and_var(xs)
        _ORACLE[key] = {"logpdf": float(lp), "alpha": np.asarray(post.alpha), "mean": m, "var": v}
    return _ORACLE[key]


class ExactWork:
    """gp_posterior_fit -> gp_posterior_predict (mean + var at 64 points) -> [gp_logpdf_grad] -> gp_posterior_free"""

    def __init__(self, grad=True):
        self.grad = grad

    def __call__(self, ctx, inp, log, tid):
        fx = agp.GP(_kernel(inp), ctx=ctx)(agp.RowVecs(inp["X"]), inp["s2"])
        post = log.call(tid, agp.posterior, fx, inp["y"])
        try:
            m, v = log.call(tid, post.mean_and_var, agp.RowVecs(inp["xs"]))
            out = {"logpdf": np.asarray(post.logpdf_value), "alpha": post.data.alpha, "mean": m, "var": v}
            if self.grad:
                lp, g = log.call(tid, agp.logpdf_and_grad, fx, inp["y"])
                out["grad"] = {"logpdf": np.asarray(lp), "variance": g["variance"], "scale": g["scale"], "noise": np.asarray(g["noise"]), "y": g["y"]}
        finally:
            log.call(tid, post.data.C.free)
        return out

    def against_serial(self, rep, tag, inp, got, ref):
        f32 = inp["dtype"] == np.float32
        if not f32:
            for k in ("logpdf", "alpha", "mean", "var"):
                rep.bits(f"{tag} {k}", got[k], ref[k])
        if self.grad:  # the gradient keeps its floating-point atomics (tests/test_gpu_poisoned_blocks.py:16): the bounds of tests/test_gpu_parity.py test_logpdf_grad_vs_oracle
            g, r = got["grad"], ref["grad"]
            if f32:    # ... and of test_float32_gradient_update_and_rand for an fp32 call
                for k in ("variance", "scale", "noise"):
                    rep.bound(f"f32 grad.{k} vs serial (rel)", abs(float(g[k]) - float(r[k])) / max(abs(float(r[k])), 1e-300), F32_GRAD_REL)
                return
            rep.bound("grad.logpdf vs serial (rel)", abs(float(g["logpdf"]) - float(r["logpdf"])) / abs(float(r["logpdf"])), LP_REL)
            rep.bound("grad.variance vs serial", abs(g["variance"] - r["variance"]) / max(abs(r["variance"]), 1.0), 1e-8)
            rep.bound("grad.scale vs serial", abs(g["scale"] - r["scale"]) / (max(1.0, abs(r["scale"])) + abs(r["scale"])), 1e-8)
            rep.bound("grad.noise vs serial", abs(float(g["noise"]) - float(r["noise"])) / (max(1.0, abs(float(r["noise"]))) + abs(float(r["noise"]))), 1e-7)
            rep.bound("grad.y vs serial", maxabs(g["y"], r["y"]) / float(np.max(np.abs(r["y"]))), 1e-8)

    def against_oracle(self, rep, tag, inp, got):
        ref = exact_oracle(inp)
        if inp["dtype"] == np.float32:
            rep.require("f32 dtypes", got["alpha"].dtype == np.float32 and got["mean"].dtype == np.float32, "Float32 in must give Float32 out")
            rep.bound("f32 logpdf vs oracle (rel)", abs(float(got["logpdf"]) - ref["logpdf"]) / abs(ref["logpdf"]), F32_LP_REL)
            rep.bound("f32 alpha vs oracle (rel 2-norm)", relnorm(got["alpha"], ref["alpha"]), F32_ALPHA_REL)
            rep.bound("f32 mean vs oracle (rel 2-norm)", relnorm(got["mean"], ref["mean"]), F32_MEAN_REL)
            rep.require("f32 var finite", bool(np.all(np.isfinite(got["var"]))), "predictive variance not finite")
            if self.grad:
                rep.bound("f32 grad.logpdf vs oracle (rel)", abs(float(got["grad"]["logpdf"]) - ref["logpdf"]) / abs(ref["logpdf"]), F32_GRAD_LP_REL)
            return
        rep.bound("logpdf vs oracle (rel)", abs(float(got["logpdf"]) - ref["logpdf"]) / abs(ref["logpdf"]), LP_REL)
        rep.bound("alpha vs oracle (rel 2-norm)", relnorm(got["alpha"], ref["alpha"]), ALPHA_REL)
        rep.bound("mean vs oracle (abs)", maxabs(got["mean"], ref["mean"]), MEAN_ABS)
        rep.bound("var vs oracle (abs)", maxabs(got["var"], ref["var"]), VAR_ABS)
        if self.grad:
            rep.bound("grad.logpdf vs oracle (rel)", abs(float(got["grad"]["logpdf"]) - ref["logpdf"]) / abs(ref["logpdf"]), LP_REL)


def vfe_inputs(n=3000, m=200, seed=55):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 4, (n, D))
    y = np.sin(X.sum(1)) + 0.3 * rng.standard_normal(n)
    return {"X": X, "y": y, "z": X[rng.permutation(n)[:m]].copy(), "xs": rng.uniform(0, 4, (NS, D)), "s2": 0.1, "jitter": 1e-4, "tag": f"vfe n{n} m{m}"}


def vfe_oracle(inp):
    key = ("vfe", id(inp["X"]))
    if key not in _ORACLE:
        of = o.GP(o.Kernel(o.SE))
        ofx = o.FiniteGP(of, inp["X"], inp["s2"])
        op = o.vfe_posterior(of, inp["z"], inp["jitter"], ofx, inp["y"])
        m, v = op.mean_and_var(inp["xs"])
        _ORACLE[key] = {"objective": o.objective_from_posterior(op, ofx, inp["y"], vfe=True), "mean": m, "var": v,
                        "grad": o.elbo_grad(of, inp["z"], inp["jitter"], ofx, inp["y"], vfe=True)}
    return _ORACLE[key]


class VfeWork:
    """gp_vfe_fit -> gp_vfe_predict -> gp_vfe_grad -> gp_vfe_free; the VFE path keeps its atomics under "deterministic": bounds, not bits"""

    def __call__(self, ctx, inp, log, tid):
        f = agp.GP(agp.SqExponentialKernel(), ctx=ctx)
        ap = log.call(tid, agp.posterior, agp.VFE(f(agp.RowVecs(inp["z"]), inp["jitter"])), f(agp.RowVecs(inp["X"]), inp["s2"]), inp["y"])
        try:
            m, v = log.call(tid, ap.mean_and_var, agp.RowVecs(inp["xs"]))
            g = log.call(tid, ap.objective_grad, True)
        finally:
            log.call(tid, ap._state._fin)
        return {"objective": float(ap.objective), "mean": m, "var": v, "grad": g}

    def against_serial(self, rep, tag, inp, got, ref):
        rep.bound("vfe objective vs serial (rel)", abs(got["objective"] - ref["objective"]) / abs(ref["objective"]), VFE_OBJ_REL)

    def against_oracle(self, rep, tag, inp, got):
        ref = vfe_oracle(inp)
        rep.bound("vfe objective vs oracle (rel)", abs(got["objective"] - ref["objective"]) / abs(ref["objective"]), VFE_OBJ_REL)
        rep.bound("vfe mean vs oracle (abs)", maxabs(got["mean"], ref["mean"]), VFE_PRED_ABS)
        rep.bound("vfe var vs oracle (abs)", maxabs(got["var"], ref["var"]), VFE_PRED_ABS)
        for k in ("variance", "noise", "y", "z", "x"):
            r = np.asarray(ref["grad"][k], dtype=np.float64)
            g = np.asarray(got["grad"][k], dtype=np.float64).reshape(r.shape)
            rep.bound(f"vfe grad.{k} vs oracle", float(np.max(np.abs(g - r))) / max(1.0, float(np.max(np.abs(r)))), VFE_GRAD_REL)


def sum_inputs(n=N_SMALL):
    x, y = dense_data(n, seed=n)
    return {"x": x, "y": y, "xs": x[:NS] + 0.01, "s2": 0.1, "tag": f"sum n{n}"}


def sum_oracle(inp):
    key = ("sum", id(inp["x"]))
    if key not in _ORACLE:
        lp, a = bc.host_fit(ref_kernelmatrix(ml_kernel(), inp["x"]) + inp["s2"] * np.eye(len(inp["x"])), inp["y"])
        _ORACLE[key] = {"logpdf": float(lp), "alpha": a}
    return _ORACLE[key]


class SumWork:
    """gp_posterior_fit_sum -> gp_posterior_predict -> gp_logpdf_grad_sum -> gp_posterior_free with the Mauna Loa form (tests/composite_ref.py ml_kernel)"""

    def __call__(self, ctx, inp, log, tid):
        fx = agp.GP(ml_kernel(), ctx=ctx)(inp["x"], inp["s2"])
        post = log.call(tid, agp.posterior, fx, inp["y"])
        try:
            m, v = log.call(tid, post.mean_and_var, inp["xs"])
            lp, g = log.call(tid, agp.logpdf_and_grad, fx, inp["y"])
        finally:
            log.call(tid, post.data.C.free)
        return {"logpdf": np.asarray(post.logpdf_value), "alpha": post.data.alpha, "mean": m, "var": v, "grad_logpdf": float(lp), "theta": g["theta"]}

    def against_serial(self, rep, tag, inp, got, ref):
        rep.bound("sum logpdf vs serial (rel)", abs(float(got["logpdf"]) - float(ref["logpdf"])) / abs(float(ref["logpdf"])), SUM_LP_REL)

    def against_oracle(self, rep, tag, inp, got):
        ref = sum_oracle(inp)
        rep.bound("sum logpdf vs host Cholesky (rel)", abs(float(got["logpdf"]) - ref["logpdf"]) / abs(ref["logpdf"]), SUM_LP_REL)
        rep.bound("sum alpha vs host Cholesky (rel 2-norm)", relnorm(got["alpha"], ref["alpha"]), SUM_ALPHA_REL)
        rep.bound("sum grad.logpdf vs host Cholesky (rel)", abs(got["grad_logpdf"] - ref["logpdf"]) / abs(ref["logpdf"]), SUM_LP_REL)
        rep.require("sum outputs finite", all(bool(np.all(np.isfinite(got[k]))) for k in ("mean", "var", "theta")), "non-finite output")


def serial_then_threads(rep, lanes):
    """lanes: one (ctx, [(inputs, work), ...]) per thread.  The serial pass of every lane, then all lanes at once; every threaded output against its serial twin
    and against the oracle."""
    serial = [[work(ctx, inp, Log(), t) for inp, work in items] for t, (ctx, items) in enumerate(lanes)]
    log = Log()
    threaded = run_threads([(lambda t=t, ctx=ctx, items=items: [work(ctx, inp, log, t) for inp, work in items]) for t, (ctx, items) in enumerate(lanes)])
    rep.pairs = log.overlapping_pairs()
    for t, (ctx, items) in enumerate(lanes):
        for i, (inp, work) in enumerate(items):
            tag = f"thread {t} item {i} ({inp['tag']})"
            work.against_serial(rep, tag, inp, threaded[t][i], serial[t][i])
            work.against_oracle(rep, tag, inp, threaded[t][i])
            if i < 2:
                work.against_oracle(rep, tag + " serial", inp, serial[t][i])
    return serial, threaded


# ---- A, B: one context per thread ------------------------------------------------------------------------------------------------------------
def scenario_A(rep):
    a, b, c, d = exact_inputs(N_SMALL, 0, 101), exact_inputs(N_LARGE, 2, 102), exact_inputs(N_LARGE, 0, 103), exact_inputs(N_SMALL, 2, 104)
    ctxs = [new_ctx(), new_ctx()]
    try:
        w = ExactWork(grad=True)
        serial_then_threads(rep, [(ctxs[0], [((a, b)[i % 2], w) for i in range(LOOPS)]), (ctxs[1], [((c, d)[i % 2], w) for i in range(LOOPS)])])
    finally:
        for c_ in ctxs:
            c_.close()


def scenario_B(rep):
    e64 = (exact_inputs(N_SMALL, 2, 111), exact_inputs(N_LARGE, 0, 112))
    # fp32: the kernel and noise of tests/test_gpu_parity.py test_float32_type_stability_and_accuracy, whose bound is used; composite: N = 2 049, where |logpdf| (64)
    # is no smaller against N than in the test the bound comes from (31 at N = 1 000) — at N = 1 537 the terms of this data set's logpdf happen to cancel to 12
    e32 = exact_inputs(N_SMALL, 3, 113, s2=0.1, dtype=np.float32, var=1.0, scale=1.0)
    vf, sm = vfe_inputs(), sum_inputs(N_LARGE)
    ctxs = [new_ctx(), new_ctx(), new_ctx({"vfe_chunk": 2048}), new_ctx()]  # vfe_chunk: the smallest legal value, so N = 3 000 streams as two chunks
    try:
        rep.require("vfe_chunk", ctxs[2].get_param("vfe_chunk") == 2048, "vfe_chunk did not take the smallest legal value")
        w, w32, wv, ws = ExactWork(grad=True), ExactWork(grad=True), VfeWork(), SumWork()
        serial_then_threads(rep, [(ctxs[0], [(e64[i % 2], w) for i in range(LOOPS)]), (ctxs[1], [(e32, w32)] * LOOPS), (ctxs[2], [(vf, wv)] * LOOPS),
                                  (ctxs[3], [(sm, ws)] * LOOPS)])
    finally:
        for c_ in ctxs:
            c_.close()


# ---- C: two threads on ONE context -----------------------------------------------------------------------------------------------------------
def scenario_C(rep):
    a, b = exact_inputs(N_SMALL, 0, 121), exact_inputs(N_LARGE, 2, 122)
    ctx = new_ctx()
    try:
        w = ExactWork(grad=False)
        first = w(ctx, a, Log(), 0)  # the very first call of a fresh ctx
        serial_then_threads(rep, [(ctx, [(a, w)] * LOOPS), (ctx, [(b, w)] * LOOPS)])
        blocks, mb = ctx.get_param("pool_blocks"), ctx.get_param("pool_cached_mb")
        rep.extra["pool_before_trim"] = {"blocks": blocks, "cached_mb": mb}
        rep.require("pool after the loops", blocks > 0 and mb > 0, f"every handle was freed, so the cache holds their blocks: pool_blocks {blocks}, pool_cached_mb {mb}")
        rep.require("gp_ctx_trim", ctx.lib.gp_ctx_trim(ctx.handle) == 0, "status != 0")
        rep.require("pool_blocks after trim", ctx.get_param("pool_blocks") == 0 and ctx.get_param("pool_cached_mb") == 0, f"{ctx.get_param('pool_blocks')} blocks left")
        again = w(ctx, a, Log(), 0)  # the stream-K scope counter and every workspace back at rest: the first fit's bits
        for k in ("logpdf", "alpha", "mean", "var"):
            rep.bits(f"one more serial fit against the very first, {k}", again[k], first[k])
    finally:
        ctx.close()


# ---- D: handles made on one thread, used and freed on another ---------------------------------------------------------------------------------
def _timings_ok(t: dict) -> bool:
    return all(math.isfinite(float(v)) and float(v) >= 0 for v in t.values())


def scenario_D(rep):
    cases = (exact_inputs(N_SMALL, 0, 131), exact_inputs(N_SMALL, 2, 132))
    rng = np.random.default_rng(133)
    X2 = rng.standard_normal((256, D))
    y2 = np.sin(X2.sum(1)) + 0.1 * rng.standard_normal(256)
    ctx = new_ctx({"time_kernels": 1})
    items = [cases[i % 2] for i in range(LOOPS)]
    status = []

    def fit(inp, log, tid):
        return log.call(tid, agp.posterior, agp.GP(_kernel(inp), ctx=ctx)(agp.RowVecs(inp["X"]), inp["s2"]), inp["y"])

    def between(log, tid):
        status.append(log.call(tid, ctx.lib.gpd_sync, ctx.handle))
        t = log.call(tid, ctx.timings)
        status.append(0 if _timings_ok(t) else ("timings", t))

    def consume(i, post, log, tid):
        out = {}
        out["mean"], out["var"] = log.call(tid, post.mean_and_var, agp.RowVecs(items[i]["xs"]))
        between(log, tid)
        if i % 2 == 0:
            p2 = log.call(tid, agp.posterior, post(agp.RowVecs(X2), 0.02), y2)
            out["alpha2"], out["logpdf2"] = p2.data.alpha, np.asarray(p2.logpdf_value)
            between(log, tid)
            status.append(log.call(tid, ctx.lib.gp_posterior_free, p2.data.C.handle))
            p2.data.C._fin.detach()
        status.append(log.call(tid, ctx.lib.gp_posterior_free, post.data.C.handle))
        post.data.C._fin.detach()
        return out

    try:
        slog = Log()
        serial = [consume(i, fit(inp, slog, 0), slog, 0) for i, inp in enumerate(items)]
        log, q = Log(), queue.Queue()

        def producer():
            for i, inp in enumerate(items):
                q.put((i, fit(inp, log, 0)))
            q.put(None)

        def consumer():
            out = {}
            while True:
                it = q.get()
                if it is None:
                    return out
                out[it[0]] = consume(it[0], it[1], log, 1)

        _, got = run_threads([producer, consumer])
        rep.pairs = log.overlapping_pairs()
        for i in range(len(items)):
            for k in serial[i]:
                rep.bits(f"item {i} {k}", got[i][k], serial[i][k])
        bad = [s for s in status if s != 0]
        rep.require("every status 0, every gp_get_timings field finite and non-negative", not bad, f"{bad[:3]}")
        t = ctx.timings()
        rep.require("time_kernels", t["gemm_launches"] > 0 and t["gemm_ms"] > 0, f"time_kernels = 1 recorded nothing: {t}")
        # the updated α against the oracle's update_chol path (tests/test_gpu_parity.py test_sequential_conditioning_matches_batch: 1e-8 of max |α|)
        inp = items[0]
        of = o.GP(o.Kernel(inp["kind"], inp["var"], inp["scale"]))
        op12 = o.posterior(o.FiniteGP(o.posterior(o.FiniteGP(of, inp["X"], float(inp["s2"])), inp["y"]), X2, 0.02), y2)
        rep.bound("updated alpha vs oracle (abs / max |alpha|)", maxabs(got[0]["alpha2"], op12.alpha) / float(np.abs(op12.alpha).max()), 1e-8)
        m, v = exact_oracle(inp)["mean"], exact_oracle(inp)["var"]
        rep.bound("mean vs oracle (abs)", maxabs(got[0]["mean"], m), MEAN_ABS)
        rep.bound("var vs oracle (abs)", maxabs(got[0]["var"], v), VAR_ABS)
    finally:
        ctx.close()


# ---- E: batches and single calls on one context ----------------------------------------------------------------------------------------------
def _rebind(case, ctx):
    """the FiniteGP of a tests/batch_cases.py problem on `ctx` instead of the default context"""
    f = case["fx"].f
    g = agp.GP(f.kernel, ctx=ctx) if f.mean_fn is None else agp.GP(f.mean_fn, f.kernel, ctx=ctx)
    return dict(case, fx=agp.FiniteGP(g, case["fx"].x, case["fx"].sigma2))


def _batch(ctx, fxs, ys, want_alpha, log, tid):
    (g,) = api._batch_groups(fxs, ys)
    call = api._batch_marshal(g, want_alpha)
    rc = log.call(tid, getattr(ctx.lib, call.entry), ctx.handle, *call.args)
    return {"rc": rc, "logpdf": call.out, "info": call.info, "alphas": call.alphas}


def scenario_E(rep):
    ctx = new_ctx()
    big = agp._lib.batch_max_n()
    reps = 12

    def make(seed, bad_at=None):
        cs = bc.small_cases(12, seed=seed, lo=24, hi=200)
        cs += [bc.make_case(big + 128, 3, "ard", 3, "colvecs", "vector", "zero", seed=seed + 50), bc.make_case(big + 257, 0, "scale", 3, "rowvecs", "scalar", "const", seed=seed + 51)]
        if bad_at is not None:  # one problem that is not positive definite, as tests/test_gpu_batch.py test_failures_are_per_problem builds it
            c = cs[bad_at]
            s2 = np.array(np.broadcast_to(c["s2"], (c["n"],)), dtype=np.float64)
            s2[int(0.4 * (c["n"] - 1))] = -10.0
            cs[bad_at] = dict(c, fx=agp.FiniteGP(c["fx"].f, c["fx"].x, s2), minor=int(0.4 * (c["n"] - 1)) + 1)
        return [_rebind(c, ctx) for c in cs]

    batches = [make(41, bad_at=3), make(42)]
    xm, ym = bc.mauna_loa_data(240)
    sums = [[agp.GP(k, ctx=ctx)(xm, 1e-2 * api._prior_variance(k)) for k in bc.perturbed_kernels(ml_kernel(), 6, seed=5 + t)] for t in range(2)]
    single = exact_inputs(N_SMALL, 2, 141)

    def lane(t):  # [(inputs, call)]: `reps` batch calls alternating with / without α, then one composite batch
        items = [((batches[t], i % 2 == 0), lambda inp, log, tid: _batch(ctx, [c["fx"] for c in inp[0]], [c["y"] for c in inp[0]], inp[1], log, tid)) for i in range(reps)]
        return items + [((sums[t], True), lambda inp, log, tid: _batch(ctx, inp[0], ym, inp[1], log, tid))]

    def single_lane():
        fx = agp.GP(_kernel(single), ctx=ctx)(agp.RowVecs(single["X"]), single["s2"])
        return [(single, lambda inp, log, tid: np.asarray(log.call(tid, agp.logpdf, fx, inp["y"])))] * (2 * reps)

    try:
        lanes = [lane(0), lane(1), single_lane()]
        serial = [[call(inp, Log(), t) for inp, call in items] for t, items in enumerate(lanes)]
        log = Log()
        got = run_threads([(lambda t=t, items=items: [call(inp, log, t) for inp, call in items]) for t, items in enumerate(lanes)])
        rep.pairs = log.overlapping_pairs()
        for t in range(2):
            for i, ((cases, want_alpha), _) in enumerate(lanes[t]):
                g, s = got[t][i], serial[t][i]
                rep.require(f"thread {t} call {i} status", g["rc"] == 0 and s["rc"] == 0, f"{g['rc']} / {s['rc']}")
                rep.bits(f"thread {t} call {i} logpdf", g["logpdf"], s["logpdf"])  # NaN of the failing problem included: same bits
                rep.bits(f"thread {t} call {i} info", g["info"], s["info"])
                if want_alpha:
                    for b in range(len(cases)):
                        rep.bits(f"thread {t} call {i} alpha[{b}]", g["alphas"][b], s["alphas"][b])
                if i >= reps:  # the composite batch against a host Cholesky (tests/test_gpu_batch.py test_composite_batch_and_a_mixed_call_against_a_host_cholesky)
                    for b, fx in enumerate(cases):
                        lp_h, a_h = bc.host_fit(ref_kernelmatrix(fx.f.kernel, xm) + float(fx.sigma2) * np.eye(len(xm)), ym)
                        rep.bound("composite batch logpdf vs host Cholesky", bc.lp_err(g["logpdf"][b], lp_h), BATCH_LP)
                        rep.bound("composite batch alpha vs host Cholesky", bc.vec_err(g["alphas"][b], a_h), BATCH_ALPHA)
                    continue
                for b, c in enumerate(cases):
                    if "minor" in c:
                        rep.require("the failing problem", int(g["info"][b]) == c["minor"] and math.isnan(float(g["logpdf"][b]))
                                    and (not want_alpha or bool(np.isnan(g["alphas"][b]).all())), f"info {int(g['info'][b])}, expected minor {c['minor']}, logpdf {g['logpdf'][b]}")
                        continue
                    rep.require("info of a good problem", int(g["info"][b]) == 0, f"thread {t} call {i} problem {b}: info {int(g['info'][b])}")
                    if i < 2:  # (the later calls carry the same bits as these)
                        lp_o, a_o = bc.oracle_fit(c)
                        rep.bound("batch logpdf vs oracle", bc.lp_err(g["logpdf"][b], lp_o), BATCH_LP)
                        if want_alpha:
                            rep.bound("batch alpha vs oracle", bc.vec_err(g["alphas"][b], a_o), BATCH_ALPHA)
        for i, v in enumerate(got[2]):
            rep.bits(f"single gp_logpdf {i}", v, serial[2][i])
        rep.bound("single logpdf vs oracle (rel)", abs(float(got[2][0]) - exact_oracle(single)["logpdf"]) / abs(exact_oracle(single)["logpdf"]), LP_REL)
    finally:
        ctx.close()


# ---- F: gp_last_error() is thread-local -------------------------------------------------------------------------------------------------------
def _raw_fit(lib, h, inp, y_null=False):
    """gp_posterior_fit straight through ctypes: (status, handle, α, logpdf)"""
    m = api._Marshal(np.float64)
    px = m.points(agp.RowVecs(inp["X"]))
    kk, nz, y = m.kernel(_kernel(inp), px.d), m.noise(inp["s2"], px.n), m.arr(inp["y"])
    alpha, lp, post = np.empty(px.n), np.empty(1), C.c_void_p()
    rc = lib.gp_posterior_fit(h, C.byref(kk), C.byref(px), C.byref(nz), None, None if y_null else y.ctypes.data, C.byref(post), alpha.ctypes.data, lp.ctypes.data)
    return rc, post, alpha, lp


def _raw_predict(lib, post, xs):
    m = api._Marshal(np.float64)
    px = m.points(agp.RowVecs(xs))
    mean, var = np.empty(px.n), np.empty(px.n)
    rc = lib.gp_posterior_predict(post, C.byref(px), None, 3, mean.ctypes.data, var.ctypes.data, None)
    return rc, mean, var


def scenario_F(rep):
    ctx = new_ctx()
    lib, h = ctx.lib, ctx.handle
    inp = exact_inputs(300, 0, 151)
    T1 = "invalid argument 2: multi-device parameter on a single-device ctx"   # tests/test_gpu_abi_errors.py:220
    T2 = "invalid argument 6: y is NULL"
    err = lambda: lib.gp_last_error().decode()
    log = Log()
    started, done1 = threading.Event(), threading.Event()

    def failing():
        seen = []
        for i in range(400):
            rc = log.call(0, lib.gp_ctx_set_param, h, b"lookahead_depth", 0)
            seen.append((rc, err()))
            started.set()
        done1.set()
        return seen

    def succeeding():
        seen = [("fresh", 0, err())]
        started.wait()
        n = 0
        while n < 20 or (not done1.is_set() and n < 200):
            rc, post, _, _ = log.call(1, _raw_fit, lib, h, inp)
            seen.append(("fit", rc, err()))
            seen.append(("free", log.call(1, lib.gp_posterior_free, post), err()))
            n += 1
        rc, post, _, _ = log.call(1, _raw_fit, lib, h, inp, True)
        seen.append(("null y", rc, err()))
        return seen

    def bystander():
        started.wait()
        v = C.c_int64()
        out = []
        for _ in range(50):
            out.append((log.call(2, lib.gp_ctx_get_param, h, b"nb", C.byref(v)), err()))
        return out

    try:
        before = err()
        s0, s1, s2 = run_threads([failing, succeeding, bystander])
        rep.pairs = log.overlapping_pairs()
        rep.require("thread 1 keeps its own text", all(rc == -2 and t == T1 for rc, t in s0), f"{[x for x in s0 if x != (-2, T1)][:3]}")
        ok_part = s1[:-1]
        rep.require("thread 2 succeeds with an empty text", all(rc == 0 and t == "" for _, rc, t in ok_part), f"{[x for x in ok_part if x[1] != 0 or x[2] != ''][:3]}")
        rep.require("thread 2's own failure", s1[-1][1:] == (-6, T2), f"{s1[-1]}")
        rep.require("a thread that never failed reads an empty string", all(rc == 0 and t == "" for rc, t in s2), f"{[x for x in s2 if x != (0, '')][:3]}")
        rep.require("the main thread's text is untouched", err() == before, f"{before!r} -> {err()!r}")
        rep.extra["calls"] = {"failing": len(s0), "fits": (len(s1) - 2) // 2}
    finally:
        ctx.close()


# ---- G: the process-wide "kmat_rows" ------------------------------------------------------------------------------------------------------------
def scenario_G(rep):
    A, B = new_ctx(), new_ctx()
    n_k = 700
    Xk, _ = o.synth_inputs(n_k, D, 161)
    inp = exact_inputs(N_SMALL, 0, 162)
    ok = o.Kernel(0, 1.3, 0.7)
    kern = 1.3 * agp.Kernel(0) @ agp.ScaleTransform(0.7)
    Ko = o.kernelmatrix(ok, Xk)
    default = A.get_param("kmat_rows")
    log, stop, seen = Log(), threading.Event(), []
    fx = agp.GP(_kernel(inp), ctx=A)(agp.RowVecs(inp["X"]), inp["s2"])

    def work():
        out = []
        try:
            for _ in range(LOOPS):
                out.append((log.call(0, agp.kernelmatrix, kern, agp.RowVecs(Xk), None, A), float(log.call(0, agp.logpdf, fx, inp["y"]))))
        finally:
            stop.set()
        return out

    def toggle():
        v, n = 0, 0
        while not stop.is_set() or n < 20:
            log.call(1, B.set_param, "kmat_rows", v)
            seen.append((v, log.call(1, A.get_param, "kmat_rows"), B.get_param("kmat_rows")))
            v, n = 1 - v, n + 1
        return n

    try:
        out, ntog = run_threads([work, toggle])
        rep.pairs = log.overlapping_pairs()
        rep.extra["toggles"] = ntog
        rep.require("kmat_rows is process-wide", all(a == v and b == v for v, a, b in seen), f"{[s for s in seen if s[1] != s[0] or s[2] != s[0]][:3]}")
        lp_o = exact_oracle(inp)["logpdf"]
        for K, lp in out:
            rep.bound("K vs oracle (abs / variance)", maxabs(K, Ko) / ok.variance, KMAT_ABS)
            rep.require("K exactly symmetric", bool(np.array_equal(K, K.T)), "K != K.T")
            rep.bound("logpdf vs oracle (rel)", abs(lp - lp_o) / abs(lp_o), LP_REL)
    finally:
        try:
            A.set_param("kmat_rows", default)
        finally:
            A.close()
            B.close()


# ---- H: a handle released under a thread that is using it (each ONCE) ---------------------------------------------------------------------------
def _raw_ctx(lib):
    h = C.c_void_p()
    agp.check(lib.gp_ctx_create(C.byref(h), 0, None))
    for k, v in CTX_PARAMS.items():
        agp.check(lib.gp_ctx_set_param(h, k.encode(), v))
    return h


def _chain(rep, what, text, step, release, serial_bits, limit):
    """One thread calls step() up to `limit` times; after its first call has returned the main thread calls release() once.  Every call: 0 with the serial bits, or
    −1 with `text`; −1 is final (three more calls after the first one).  release() returns 0, a second one −1."""
    lib = agp._lib.load()
    first, seen = threading.Event(), []

    def user():
        after = 0
        for _ in range(limit):
            rc, outs = step()
            seen.append((rc, lib.gp_last_error().decode() if rc != 0 else "", outs))
            first.set()
            if rc != 0:
                after += 1
                if after > 3:
                    break
        first.set()

    t = threading.Thread(target=user, name=f"case-thread-{what}")
    t.start()
    first.wait()
    r1 = release()
    t.join()
    r2 = release()
    rep.require(f"{what}: release returns 0 exactly once", (r1, r2) == (0, -1), f"first {r1}, second {r2}")
    rcs = [s[0] for s in seen]
    rep.require(f"{what}: only 0 and -1", set(rcs) <= {0, -1}, f"statuses {sorted(set(rcs))}; text {[s[1] for s in seen if s[0] not in (0, -1)][:2]}")
    k = rcs.index(-1) if -1 in rcs else len(rcs)
    rep.require(f"{what}: -1 is final", all(r == -1 for r in rcs[k:]), f"{rcs}")
    rep.require(f"{what}: the refusal's text", all(s[1] == f"invalid argument 1: {text}" for s in seen[k:]), f"{[s[1] for s in seen[k:]][:2]}")
    rep.require(f"{what}: the release was seen by the user thread", k < len(rcs), f"all {len(rcs)} calls finished before the release: nothing raced")
    for i, (rc, _, outs) in enumerate(seen[:k]):
        for name, a in outs.items():
            rep.bits(f"{what}: call {i} {name}", a, serial_bits[name])
    rep.extra[what] = {"calls_ok": k, "calls_refused": len(rcs) - k}


def scenario_H(rep):
    lib = agp._lib.load()
    inp = exact_inputs(N_SMALL, 0, 171)
    vf = vfe_inputs(seed=172)
    rep.pairs = None
    # (i) gp_ctx_destroy under a chain of fits
    ref_ctx = _raw_ctx(lib)
    rc, post, a0, lp0 = _raw_fit(lib, ref_ctx, inp)
    rep.require("serial fit", rc == 0, f"status {rc}")
    rc, m0, v0 = _raw_predict(lib, post, inp["xs"])
    rep.require("serial predict", rc == 0, f"status {rc}")
    X = _raw_ctx(lib)
    leftovers = []

    def fit_step():
        rc, p, a, lp = _raw_fit(lib, X, inp)
        if rc != 0:
            return rc, {}
        leftovers.append(lib.gp_posterior_free(p))  # a handle of a destroyed ctx is still freed with 0
        return 0, {"alpha": a, "logpdf": lp}

    _chain(rep, "ctx_destroy", "not a live gp_ctx", fit_step, lambda: lib.gp_ctx_destroy(X), {"alpha": a0, "logpdf": lp0}, 300)
    rep.require("ctx_destroy: every posterior of the chain was freed with 0", all(r == 0 for r in leftovers), f"{leftovers}")

    # (ii) gp_posterior_free under a loop of predictions
    def predict_step():
        rc, m, v = _raw_predict(lib, post, inp["xs"])
        return rc, ({"mean": m, "var": v} if rc == 0 else {})

    _chain(rep, "posterior_free", "not a live gp_post", predict_step, lambda: lib.gp_posterior_free(post), {"mean": m0, "var": v0}, 3000)

    # (iii) gp_vfe_free under a loop of predictions (the VFE path keeps its atomics: a returned prediction is held to the serial one at the VFE bound, not to its bits)
    ctxv = agp.Context(0)
    for k, v in {**CTX_PARAMS, "vfe_chunk": 2048}.items():
        ctxv.set_param(k, v)
    f = agp.GP(agp.SqExponentialKernel(), ctx=ctxv)
    ap = agp.posterior(agp.VFE(f(agp.RowVecs(vf["z"]), vf["jitter"])), f(agp.RowVecs(vf["X"]), vf["s2"]), vf["y"])
    ap._state._fin.detach()
    hv = ap._state.handle
    mv0, vv0 = ap.mean_and_var(agp.RowVecs(vf["xs"]))
    vfe_out = []

    def vfe_step():
        m = api._Marshal(np.float64)
        px = m.points(agp.RowVecs(vf["xs"]))
        mean, var = np.empty(px.n), np.empty(px.n)
        rc = lib.gp_vfe_predict(hv, C.byref(px), None, 3, mean.ctypes.data, var.ctypes.data, None)
        if rc == 0:
            vfe_out.append((mean, var))
        return rc, {}

    _chain(rep, "vfe_free", "not a live gp_vfe", vfe_step, lambda: lib.gp_vfe_free(hv), {}, 3000)
    for mean, var in vfe_out:
        rep.bound("vfe_free: mean of a served call vs serial (abs)", maxabs(mean, mv0), VFE_PRED_ABS)
        rep.bound("vfe_free: var of a served call vs serial (abs)", maxabs(var, vv0), VFE_PRED_ABS)
    ctxv.close()

    # (iv) a posterior whose ctx has been destroyed
    rc, q, _, _ = _raw_fit(lib, ref_ctx, inp)
    rep.require("(iv) fit", rc == 0, f"status {rc}")
    rep.require("(iv) destroy", lib.gp_ctx_destroy(ref_ctx) == 0, "gp_ctx_destroy != 0")
    rc, _, _ = _raw_predict(lib, q, inp["xs"])
    rep.require("(iv) predict on a posterior of a destroyed ctx", rc == -1 and lib.gp_last_error().decode() == "invalid argument 1: not a live gp_post",
                f"status {rc}, text {lib.gp_last_error().decode()!r}")
    rep.require("(iv) its free", lib.gp_posterior_free(q) == 0, "gp_posterior_free != 0")
    rep.require("(iv) second free / destroy", lib.gp_posterior_free(q) == -1 and lib.gp_ctx_destroy(ref_ctx) == -1, "a dead handle was accepted")


# ---- I: a multi-device context created and used off the main thread ------------------------------------------------------------------------------
def scenario_I(rep):
    inp, inp1 = exact_inputs(N_SMALL, 0, 181), exact_inputs(N_SMALL, 2, 182)
    reps = 8
    w = ExactWork(grad=False)

    def multi_ctx():
        return new_ctx(devices=[0, 0], nb=256)

    m0 = multi_ctx()
    one = new_ctx()
    made = []
    try:
        serial_multi = w(m0, inp, Log(), 0)                       # the same call, serially, from the main thread
        serial_one = w(one, inp1, Log(), 0)
        log, done = Log(), threading.Event()

        def multi_thread():
            try:
                c = multi_ctx()                                   # created AND used on this thread
                made.append(c)
                return [w(c, inp, log, 0) for _ in range(reps)], c.multi_info(), c.multi_stats()
            finally:
                done.set()

        res = {}
        t = threading.Thread(target=lambda: res.update(out=run_threads([multi_thread])[0]), name="case-thread-multi")
        t.start()
        mine, n = [], 0
        while not done.is_set() or n < reps:                       # the main thread itself is the second caller
            mine.append(w(one, inp1, log, 1))
            n += 1
        t.join()
        rep.require("the multi thread finished", "out" in res, "no result")
        outs, info, stats = res["out"]
        rep.pairs = log.overlapping_pairs()
        rep.extra["multi"] = {"info": info, "stats": stats, "single_fits_beside": n}
        rep.require("two ranks", info["P"] * info["Q"] == 2, f"{info}")
        for i, g in enumerate(outs):
            w.against_oracle(rep, f"multi fit {i}", inp, g)
            # threaded against serial multi-device fit: tests/test_gpu_multi.py holds every grid to the oracle at logpdf 1e-10 / α 1e-8 / mean 1e-8 / var 1e-9 and has no
            # grid-against-grid bound of its own; two results inside those bounds differ by at most twice them — the bounds themselves are used here, which asks more
            rep.bound("multi logpdf vs serial multi (rel)", abs(float(g["logpdf"]) - float(serial_multi["logpdf"])) / abs(float(serial_multi["logpdf"])), LP_REL)
            rep.bound("multi alpha vs serial multi (rel 2-norm)", relnorm(g["alpha"], serial_multi["alpha"]), ALPHA_REL)
            rep.bound("multi mean vs serial multi (abs)", maxabs(g["mean"], serial_multi["mean"]), MEAN_ABS)
            rep.bound("multi var vs serial multi (abs)", maxabs(g["var"], serial_multi["var"]), VAR_ABS)
        w.against_oracle(rep, "serial multi", inp, serial_multi)
        for i, g in enumerate(mine):
            w.against_oracle(rep, f"single fit {i}", inp1, g)
            w.against_serial(rep, f"single fit {i}", inp1, g, serial_one)
    finally:
        for c in made + [m0, one]:
            c.close()


GROUPS = {"AB": "AB", "CDE": "CDE", "FG": "FG", "HI": "HI"}


def main(group):
    for name in GROUPS[group]:
        rep = Report(name)
        try:
            globals()["scenario_" + name](rep)
        except BaseException:
            rep.worst = math.inf
            rep._fail("exception: " + traceback.format_exc()[-1500:])
        print(rep.line(), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
