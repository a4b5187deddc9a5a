"""Host-side mirror of the AbstractGPs.jl API surface for the accelerated path.

Line-for-line Python counterpart of the Julia shim (julia/HipGPs.jl): same names, argument meaning
and error behaviour as the reference (file:line cited per function, relative to the upstream repo),
every numeric step a call through the C ABI (include/gpmi355.h) into the HIP library.  Nothing here
computes Gram matrices, factorisations or solves on the host (held-out logpdf and posterior sampling included:
gp_posterior_logpdf / gp_posterior_rand / gp_vfe_logpdf / gp_vfe_rand).

    f   = GP(SqExponentialKernel())                    # src/base_gp.jl:57-64
    fx  = f(x, 0.01)                                   # src/finite_gp_projection.jl:32
    lp  = logpdf(fx, y)                                # src/finite_gp_projection.jl:306
    fp  = posterior(fx, y)                             # src/exact_gpr_posterior.jl:29
    m, v = mean_and_var(fp(xs))                        # src/exact_gpr_posterior.jl:85
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Mapping
import math
import threading
import weakref
from dataclasses import dataclass, field
from typing import Callable, Optional, Union

import numpy as np

from . import _lib
from ._lib import PosDefException, check, gp_kernel, gp_kfactor, gp_ksum, gp_kterm, gp_noise, gp_points, gp_timings

default_sigma2 = 1e-18  # src/finite_gp_projection.jl:17


# --------------------------------------------------------------------------------------------
# Kernels and transforms (KernelFunctions.jl surface used by the path)
# --------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ScaleTransform:
    s: float


@dataclass(frozen=True)
class ARDTransform:
    v: tuple

    def __init__(self, v):
        object.__setattr__(self, "v", tuple(float(t) for t in np.asarray(v).ravel()))


class _KernelOps:
    """KernelFunctions' composition operators: k1 + k2 (KernelSum), k1 * k2 (KernelProduct), a * k (ScaledKernel)."""

    def __add__(self, other):
        if not isinstance(other, _KernelOps):
            return NotImplemented
        return KernelSum(_flat(self, KernelSum) + _flat(other, KernelSum))

    def _times(self, other):  # a kernel times a kernel: KernelProduct
        return KernelProduct(_flat(self, KernelProduct) + _flat(other, KernelProduct))


def _flat(k, cls) -> tuple:
    return k.kernels if isinstance(k, cls) else (k,)


@dataclass(frozen=True)
class Kernel(_KernelOps):
    """variance · base(kind) ∘ transform.  kind 0..3 SqExponential / Matern12 / Matern32 / Matern52 (the single-kind path, gp_kernel);
    4 Periodic (param = r), 5 RationalQuadratic (param = (α,)), 6 White (composite path, gp_ksum — include/gpmi355.h)."""

    kind: int
    variance: float = 1.0
    transform: Union[None, ScaleTransform, ARDTransform] = None
    param: tuple = ()

    def __matmul__(self, t):  # k ∘ ScaleTransform(s)  /  k ∘ ARDTransform(v)
        if not isinstance(t, (ScaleTransform, ARDTransform)):
            raise TypeError("only ScaleTransform / ARDTransform are accelerated")
        if self.transform is not None:
            raise TypeError("nested transforms are not accelerated")
        if self.kind == 6:  # δ(x, x') does not change under a (nonzero) scale, and the transform's tangent is zero: dropped
            return self
        return Kernel(self.kind, self.variance, t, self.param)

    def __rmul__(self, a):  # α * k  (ScaledKernel)
        return Kernel(self.kind, self.variance * float(a), self.transform, self.param)

    def __mul__(self, a):  # k * k2 (KernelProduct) or k * α
        if isinstance(a, _KernelOps):
            return self._times(a)
        return self.__rmul__(a)


@dataclass(frozen=True)
class KernelSum(_KernelOps):
    kernels: tuple

    def __matmul__(self, t):
        raise TypeError("a transform around a sum of kernels is not accelerated: put it on each base kernel")

    def __mul__(self, a):
        return self._times(a) if isinstance(a, _KernelOps) else ScaledKernel(self, float(a))

    def __rmul__(self, a):
        return ScaledKernel(self, float(a))


@dataclass(frozen=True)
class KernelProduct(_KernelOps):
    kernels: tuple

    def __matmul__(self, t):
        raise TypeError("a transform around a product of kernels is not accelerated: put it on each base kernel")

    def __mul__(self, a):
        return self._times(a) if isinstance(a, _KernelOps) else ScaledKernel(self, float(a))

    def __rmul__(self, a):
        return ScaledKernel(self, float(a))


@dataclass(frozen=True)
class ScaledKernel(_KernelOps):
    """σ² · k for a composite k (a base kernel folds its ScaledKernel factor into Kernel.variance)."""

    kernel: object
    variance: float

    def __matmul__(self, t):
        raise TypeError("a transform around a scaled sum or product of kernels is not accelerated")

    def __mul__(self, a):
        return self._times(a) if isinstance(a, _KernelOps) else ScaledKernel(self.kernel, self.variance * float(a))

    def __rmul__(self, a):
        return ScaledKernel(self.kernel, self.variance * float(a))


def SqExponentialKernel():
    return Kernel(0)


SEKernel = RBFKernel = GaussianKernel = SqExponentialKernel


def Matern12Kernel():
    return Kernel(1)


ExponentialKernel = Matern12Kernel


def Matern32Kernel():
    return Kernel(2)


def Matern52Kernel():
    return Kernel(3)


def PeriodicKernel(r=(1.0,)):
    """PeriodicKernel(; r): exp(−½ Σ_p (sinpi(u_p) / r_p)²), one r_p > 0 per input dimension (KernelFunctions' default r = [1.0])."""
    r = tuple(float(v) for v in np.asarray(r, dtype=np.float64).ravel())
    if not r or not all(v > 0 for v in r):
        raise ValueError("PeriodicKernel: every r must be > 0")
    return Kernel(4, 1.0, None, r)


def RationalQuadraticKernel(alpha=2.0):
    """RationalQuadraticKernel(; α): (1 + d²/(2α))^(−α), α > 0 (KernelFunctions' default α = 2)."""
    if not float(alpha) > 0:
        raise ValueError("RationalQuadraticKernel: alpha must be > 0")
    return Kernel(5, 1.0, None, (float(alpha),))


def WhiteKernel():
    """WhiteKernel(): 1 where x and x' are equal in every coordinate, else 0."""
    return Kernel(6)


# Limits of the composite path (include/gpmi355.h gp_ksum)
KSUM_MAX_TERMS, KSUM_MAX_FACTORS_PER_TERM, KSUM_MAX_FACTORS, KSUM_MAX_THETA, KSUM_MAX_D = 8, 4, 16, 64, 16


def _is_composite(k) -> bool:
    """True for what goes through the *_sum entry points: a sum, a product, a scaled composite or a base kernel of kind 4..6."""
    return not (isinstance(k, Kernel) and k.kind <= 3)


class _NormalForm:
    """Σ_t σ_t² Π_f κ_f of a kernel tree.  `params` holds the tree's own parameters depth-first, left to right — a node's before its children's;
    a base kernel: its variance (the ScaledKernel factor), then Periodic r / RQ α, then its transform's s or v — and every term refers to them by
    index, so that products distributed over sums share their parameters.  `theta` is the flat vector of the C ABI (term by term σ_t², then per
    factor scale, then param); `chain` maps ∂/∂theta back to ∂/∂params."""

    def __init__(self, k):
        self.params = []
        self.terms = self._walk(k)  # [(variance indices, [(kind, scale indices, param indices)])]

    def _new(self, v) -> int:
        self.params.append(float(v))
        return len(self.params) - 1

    def _walk(self, k):
        if isinstance(k, Kernel):
            vi = self._new(k.variance)
            pi = [self._new(v) for v in k.param]
            t = k.transform
            si = [self._new(t.s)] if isinstance(t, ScaleTransform) else ([self._new(v) for v in t.v] if isinstance(t, ARDTransform) else [])
            return [([vi], [(k.kind, si, pi)])]
        if isinstance(k, ScaledKernel):
            vi = self._new(k.variance)
            return [([vi] + v, f) for v, f in self._walk(k.kernel)]
        if isinstance(k, KernelSum):
            return [t for c in k.kernels for t in self._walk(c)]
        if isinstance(k, KernelProduct):
            terms = [([], [])]
            for c in k.kernels:
                ct = self._walk(c)
                terms = [(v1 + v2, f1 + f2) for v1, f1 in terms for v2, f2 in ct]
            return terms
        raise TypeError(f"not an accelerated kernel: {k!r}")

    def check(self, d: int) -> None:
        """The limits of include/gpmi355.h gp_ksum (TypeError) and the per-dimension parameter counts (ValueError, as ARDTransform's)."""
        nt, nf = len(self.terms), sum(len(f) for _, f in self.terms)
        if nt > KSUM_MAX_TERMS:
            raise TypeError(f"composite kernel: {nt} terms in the normal form, at most {KSUM_MAX_TERMS} are accelerated")
        if any(len(f) > KSUM_MAX_FACTORS_PER_TERM for _, f in self.terms):
            raise TypeError(f"composite kernel: a term with more than {KSUM_MAX_FACTORS_PER_TERM} factors is not accelerated")
        if nf > KSUM_MAX_FACTORS:
            raise TypeError(f"composite kernel: {nf} factors in all, at most {KSUM_MAX_FACTORS} are accelerated")
        if len(self.theta()) > KSUM_MAX_THETA:
            raise TypeError(f"composite kernel: {len(self.theta())} entries in theta, at most {KSUM_MAX_THETA} are accelerated")
        if d > KSUM_MAX_D:
            raise TypeError(f"composite kernel: D = {d}, at most {KSUM_MAX_D} is accelerated")
        for _, fs in self.terms:
            for kind, si, pi in fs:
                if len(si) > 1 and len(si) != d:
                    raise ValueError(f"DimensionMismatch: ARDTransform has {len(si)} scales, inputs have D={d}")
                if kind == 4 and len(pi) != d:
                    raise ValueError(f"DimensionMismatch: PeriodicKernel has {len(pi)} entries in r, inputs have D={d}")

    def theta(self) -> list:
        p, th = self.params, []
        for vi, fs in self.terms:
            th.append(math.prod(p[i] for i in vi))
            for _, si, pi in fs:
                th += [p[i] for i in si] + [p[i] for i in pi]
        return th

    def chain(self, g_theta) -> np.ndarray:
        """∂/∂params from ∂/∂theta: ∂σ_t²/∂v = Π of the term's other variances (no division), scales and parameters one to one; a parameter
        in several terms sums its contributions."""
        p, g, j = self.params, np.zeros(len(self.params)), 0
        for vi, fs in self.terms:
            for a in range(len(vi)):
                g[vi[a]] += g_theta[j] * math.prod(p[vi[b]] for b in range(len(vi)) if b != a)
            j += 1
            for _, si, pi in fs:
                for i in si + pi:
                    g[i] += g_theta[j]
                    j += 1
        return g


def params(k) -> np.ndarray:
    """The kernel tree's own parameters in a fixed order — depth-first, left to right: ScaledKernel σ², and per base kernel its variance, Periodic r /
    RationalQuadratic α, then ScaleTransform s / ARDTransform v — the order of logpdf_and_grad's g["kernel"]."""
    return np.array(_NormalForm(k).params)


def with_params(k, theta):
    """The same tree with the parameters `theta` (the order of params(k))."""
    it = iter(np.asarray(theta, dtype=np.float64).ravel().tolist())

    def rebuild(k):
        if isinstance(k, Kernel):
            v = next(it)
            par = tuple(next(it) for _ in k.param)
            t = k.transform
            if isinstance(t, ScaleTransform):
                t = ScaleTransform(next(it))
            elif isinstance(t, ARDTransform):
                t = ARDTransform([next(it) for _ in t.v])
            return Kernel(k.kind, v, t, par)
        if isinstance(k, ScaledKernel):
            v = next(it)
            return ScaledKernel(rebuild(k.kernel), v)
        if isinstance(k, (KernelSum, KernelProduct)):
            return type(k)(tuple(rebuild(c) for c in k.kernels))
        raise TypeError(f"not an accelerated kernel: {k!r}")

    out = rebuild(k)
    if next(it, None) is not None:
        raise ValueError("with_params: more values than the kernel has parameters")
    return out


def _prior_variance(k) -> float:
    """k(x, x) = Σ_t σ_t² (every base κ(x, x) = 1)."""
    if isinstance(k, Kernel) and k.kind <= 3:
        return k.variance
    nf = _NormalForm(k)
    return float(sum(math.prod(nf.params[i] for i in vi) for vi, _ in nf.terms))


def compose(k: Kernel, t) -> Kernel:
    return k @ t


def with_lengthscale(k: Kernel, l) -> Kernel:
    """with_lengthscale(k, ℓ) ≡ k ∘ ScaleTransform(1/ℓ) (scalar) or k ∘ ARDTransform(1 ./ ℓ)."""
    l = np.asarray(l, dtype=np.float64)
    return k @ (ScaleTransform(1.0 / float(l)) if l.ndim == 0 else ARDTransform(1.0 / l))


# --------------------------------------------------------------------------------------------
# Input containers (KernelFunctions ColVecs / RowVecs; src/finite_gp_projection.jl:32-37)
# --------------------------------------------------------------------------------------------
@dataclass
class ColVecs:
    X: np.ndarray  # D × N, points are columns

    def __len__(self):
        return self.X.shape[1]


@dataclass
class RowVecs:
    X: np.ndarray  # N × D, points are rows

    def __len__(self):
        return self.X.shape[0]


def _as_input(x):
    if isinstance(x, (ColVecs, RowVecs)):
        return x
    x = np.asarray(x)
    if x.ndim == 1:
        return x
    if x.ndim == 2:
        return RowVecs(x)  # a bare matrix is taken as N × D
    raise TypeError("inputs must be a vector, RowVecs or ColVecs")


def _npoints(x) -> int:
    return len(x)


class _Marshal:
    """Keeps the numpy buffers behind the ctypes structs alive for the duration of a call."""

    def __init__(self, dtype):
        self.dtype = np.dtype(dtype)
        self.keep = []

    def arr(self, a, order="C"):
        a = np.ascontiguousarray(a, dtype=self.dtype) if order == "C" else np.asfortranarray(a, dtype=self.dtype)
        self.keep.append(a)
        return a

    def ptr(self, a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    def points(self, x) -> gp_points:
        """gp_points of an input container WITHOUT a host copy when the array already lies in one of the two ABI layouts (round 6: the transposing copy of
        RowVecs(X) with a C-ordered X cost 0.6–1.9 ms per call at N = 262 144 — inside every timed sparse fit — and has no counterpart in the Julia shim, where
        RowVecs(X) is column-major N×D = layout 2 as it lies).  layout 1 = element (dimension dd, point i) at data[dd + i·D] — a C-ordered (N, D) array, or a
        Fortran-ordered (D, N) one; layout 2 = data[i + dd·N] — a C-ordered (D, N) array, or a Fortran-ordered (N, D) one."""
        x = _as_input(x)
        if isinstance(x, (ColVecs, RowVecs)):
            A = np.asarray(x.X)
            n, d = (A.shape[1], A.shape[0]) if isinstance(x, ColVecs) else (A.shape[0], A.shape[1])
            point_major = A.flags.c_contiguous if isinstance(x, RowVecs) else A.flags.f_contiguous      # memory order [point][dimension]
            dim_major = A.flags.f_contiguous if isinstance(x, RowVecs) else A.flags.c_contiguous        # memory order [dimension][point]
            if A.dtype == self.dtype and (point_major or dim_major) and A.size:
                self.keep.append(A)
                return gp_points(A.ctypes.data, n, d, 1 if point_major else 2)
            if isinstance(x, ColVecs):  # D×N column-major  == (N, D) C-contiguous
                X = self.arr(A.T)
                return gp_points(X.ctypes.data, X.shape[0], X.shape[1], 1)
            X = self.arr(A.T)           # N×D column-major == (D, N) C-contiguous
            return gp_points(X.ctypes.data, X.shape[1], X.shape[0], 2)
        v = self.arr(x)
        return gp_points(v.ctypes.data, v.shape[0], 1, 0)

    def kernel(self, k: Kernel, d: int) -> gp_kernel:
        dt = 0 if self.dtype == np.float64 else 1
        if k.transform is None:
            return gp_kernel(k.kind, dt, k.variance, 0, None)
        if isinstance(k.transform, ScaleTransform):
            s = np.array([k.transform.s], dtype=np.float64)
        else:
            s = np.array(k.transform.v, dtype=np.float64)
            if s.shape[0] != d:
                raise ValueError(f"DimensionMismatch: ARDTransform has {s.shape[0]} scales, inputs have D={d}")
        self.keep.append(s)
        return gp_kernel(k.kind, dt, k.variance, s.shape[0], s.ctypes.data_as(C.POINTER(C.c_double)))

    def ksum(self, k, d: int):
        """gp_ksum of a composite kernel (normal form on the host) and its _NormalForm (for the chain rule of the gradient)."""
        nf = _NormalForm(k)
        nf.check(d)
        dt = 0 if self.dtype == np.float64 else 1
        p = nf.params
        terms = (gp_kterm * len(nf.terms))()
        for t, (vi, fs) in enumerate(nf.terms):
            facs = (gp_kfactor * len(fs))()
            for j, (kind, si, pi) in enumerate(fs):
                sv = np.array([p[i] for i in si], dtype=np.float64)
                pv = np.array([p[i] for i in pi], dtype=np.float64)
                self.keep += [sv, pv]
                dp = C.POINTER(C.c_double)
                facs[j] = gp_kfactor(kind, len(si), sv.ctypes.data_as(dp) if len(si) else None, len(pi), pv.ctypes.data_as(dp) if len(pi) else None)
            self.keep.append(facs)
            terms[t] = gp_kterm(math.prod(p[i] for i in vi), len(fs), facs)
        self.keep.append(terms)
        return gp_ksum(dt, len(nf.terms), terms), nf

    def any_kernel(self, k, d: int):
        """(entry-point suffix, descriptor): "" and a gp_kernel for kinds 0..3, "_sum" and a gp_ksum for everything composite."""
        if _is_composite(k):
            return "_sum", self.ksum(k, d)[0]
        return "", self.kernel(k, d)

    def noise(self, sigma2, n: int) -> gp_noise:
        s = np.asarray(sigma2)
        if s.ndim == 0:
            return gp_noise(0, float(s), None)
        if s.ndim == 1:
            if s.shape[0] != n:
                raise ValueError("DimensionMismatch: noise vector length != number of points")
            v = self.arr(s)
            return gp_noise(1, 0.0, v.ctypes.data)
        # dense Σy: the engine reads ONE triangle of an n×n column-major array (include/gpmi355.h gp_noise: kind 2 upper, kind 3 lower).  The mirror always
        # means the UPPER triangle of the array the user passed, as Symmetric(Σy) does (src/util/common_covmat_ops.jl:5): a C-ordered array is the column-major
        # array of its transpose — its upper triangle is that one's lower (kind 3, zero-copy); a Fortran-ordered array is column-major as it lies (kind 2,
        # zero-copy); anything else (strided, another dtype) is copied once into C order.
        if s.ndim != 2 or s.shape != (n, n):
            raise ValueError(f"DimensionMismatch: noise covariance has shape {s.shape}, expected ({n},) or ({n}, {n})")
        if s.dtype == self.dtype and s.flags.c_contiguous:
            self.keep.append(s)
            return gp_noise(3, 0.0, s.ctypes.data)
        if s.dtype == self.dtype and s.flags.f_contiguous:
            self.keep.append(s)
            return gp_noise(2, 0.0, s.ctypes.data)
        v = self.arr(s)
        return gp_noise(3, 0.0, v.ctypes.data)


def _input_dim(x) -> int:
    x = _as_input(x)
    if isinstance(x, ColVecs):
        return x.X.shape[0]
    if isinstance(x, RowVecs):
        return x.X.shape[1]
    return 1


def _input_dtype(x):
    x = _as_input(x)
    a = x.X if isinstance(x, (ColVecs, RowVecs)) else x
    return np.float32 if np.asarray(a).dtype == np.float32 else np.float64


# --------------------------------------------------------------------------------------------
# Engine context (one per device)
# --------------------------------------------------------------------------------------------
class Context:
    """gp_ctx wrapper.  `stream` = a raw hipStream_t (int) to issue main-stream work on, or None.
    `devices=[d0, d1, ...]` builds a multi-device context (gp_ctx_create_multi): fp64 logpdf / posterior fits are then
    partitioned 2D block-cyclically over those devices inside the library (grid P×Q, 0 = chosen for the fabric; block nb);
    listing one device several times gives virtual ranks (the whole schedule on one GPU)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None, devices=None, P: int = 0, Q: int = 0, nb: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        if devices is not None:
            devs = (C.c_int32 * len(devices))(*[int(v) for v in devices])
            check(self.lib.gp_ctx_create_multi(C.byref(h), devs, len(devices), int(P), int(Q), int(nb)))
            device = int(devices[0])
        else:
            check(self.lib.gp_ctx_create(C.byref(h), int(device), C.c_void_p(stream) if stream else None))
        self.handle = h
        self.device = device
        self._fin = weakref.finalize(self, self.lib.gp_ctx_destroy, h)

    def multi_info(self) -> dict:
        v = [C.c_int32() for _ in range(5)]
        check(self.lib.gp_ctx_multi_info(self.handle, *[C.byref(t) for t in v]))
        P, Q, nb, comm, depth = (t.value for t in v)
        return {"P": P, "Q": Q, "nb": nb, "comm": {0: "none", 1: "rccl", 2: "copies"}.get(comm, str(comm)), "lookahead_depth": depth}

    def multi_stats(self) -> dict:
        """fit attempts of the multi-device driver and how many were repetitions after a failed self-check (gp_ctx_multi_stats)"""
        f, r, sv = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.gp_ctx_multi_stats(self.handle, C.byref(f), C.byref(r), C.byref(sv)))
        return {"fits": f.value, "retries": r.value, "solves": sv.value}

    def set_param(self, name: str, value: int) -> None:
        check(self.lib.gp_ctx_set_param(self.handle, name.encode(), int(value)))

    def get_param(self, name: str) -> int:
        v = C.c_int64()
        check(self.lib.gp_ctx_get_param(self.handle, name.encode(), C.byref(v)))
        return int(v.value)

    def timings(self) -> dict:
        t = gp_timings()
        check(self.lib.gp_get_timings(self.handle, C.byref(t)))
        return {f: getattr(t, f) for f, _ in gp_timings._fields_}

    def trim(self) -> None:
        """Hand the ctx's cached free device blocks back to the HIP allocator (e.g. after freeing a 34 GB posterior)."""
        check(self.lib.gp_ctx_trim(self.handle))

    def close(self):
        self._fin()


_default_ctx = {}
_ctx_lock = threading.Lock()


def default_context(device: int = 0) -> Context:
    with _ctx_lock:
        if device not in _default_ctx:
            _default_ctx[device] = Context(device)
        return _default_ctx[device]


# --------------------------------------------------------------------------------------------
# GP types
# --------------------------------------------------------------------------------------------
Mean = Union[None, float, Callable]


def _mean_vector(mean: Mean, x, dtype) -> Optional[np.ndarray]:
    """mean_vector — src/mean_function.jl:27,40,52-55.  None = ZeroMean (stays lazy)."""
    if mean is None:
        return None
    n = _npoints(x)
    if isinstance(mean, (int, float, np.floating)):
        return np.full(n, mean, dtype=dtype)
    x = _as_input(x)
    if isinstance(x, ColVecs):
        return np.asarray([mean(c) for c in x.X.T], dtype=dtype)
    if isinstance(x, RowVecs):
        return np.asarray([mean(r) for r in x.X], dtype=dtype)
    return np.asarray([mean(v) for v in x], dtype=dtype)


class AbstractGP:
    def __call__(self, x, sigma2=default_sigma2) -> "FiniteGP":  # src/finite_gp_projection.jl:32
        return FiniteGP(self, _as_input(x), sigma2)

    def mean(self, x=None):  # src/abstract_gp.jl:66-87
        if x is None:
            raise TypeError("`mean(f)` for an AbstractGP requires inputs: use `mean(f(x))` or `mean(f, x)`")
        raise NotImplementedError


@dataclass(eq=False)
class GP(AbstractGP):
    """HipGP: GP(mean, kernel) whose FiniteGP methods run on the MI355X (src/base_gp.jl:57-64)."""

    kernel: Kernel
    mean_fn: Mean = None
    ctx: Optional[Context] = None

    def __init__(self, *args, ctx: Optional[Context] = None):
        if len(args) == 1:
            self.mean_fn, self.kernel = None, args[0]  # GP(kernel) -> ZeroMean  base_gp.jl:64
        elif len(args) == 2:
            self.mean_fn, self.kernel = args  # GP(c::Real, k) / GP(f, k)  base_gp.jl:62-63
        else:
            raise TypeError("GP(kernel) or GP(mean, kernel)")
        if not isinstance(self.kernel, _KernelOps):
            raise TypeError("kernel must be one of the accelerated kernels")
        self.ctx = ctx

    def context(self) -> Context:
        return self.ctx or default_context()

    # internal AbstractGP API (src/base_gp.jl:68-74)
    def mean(self, x=None):
        if x is None:
            return super().mean()
        m = _mean_vector(self.mean_fn, x, _input_dtype(x))
        return np.zeros(_npoints(x), dtype=_input_dtype(x)) if m is None else m

    def cov(self, x, z=None):
        return kernelmatrix(self.kernel, x, z, ctx=self.context())

    def var(self, x):
        return np.full(_npoints(x), _prior_variance(self.kernel), dtype=_input_dtype(x))  # kernelmatrix_diag

    def mean_and_var(self, x):
        return self.mean(x), self.var(x)


@dataclass(eq=False)
class FiniteGP:
    """src/finite_gp_projection.jl:7-21."""

    f: AbstractGP
    x: object
    sigma2: object = default_sigma2

    def __len__(self):
        return _npoints(self.x)

    def noise_vector(self):
        """diag(Σy): what var / mean_and_var / marginals add (src/finite_gp_projection.jl:115-116, 156-157)."""
        s = np.asarray(self.sigma2)
        if s.ndim == 2:
            return np.diagonal(s).copy()
        return np.full(len(self), float(s)) if s.ndim == 0 else s

    def noise_matrix_or_none(self):
        """Symmetric(Σy) for a dense Σy (the upper triangle of the array, mirrored), None for a scalar / vector one."""
        s = np.asarray(self.sigma2)
        if s.ndim != 2:
            return None
        u = np.triu(s)
        return u + np.triu(s, 1).T

    def _prior_factor(self):
        """Device-resident factor of cov(fx) = K + Σy for a GP prior, computed once per FiniteGP object and reused by
        rand (the reference refactors on every call, src/finite_gp_projection.jl:235)."""
        fac = getattr(self, "_fac", None)
        if fac is None:
            fac = _posterior_exact(self, np.zeros(len(self), dtype=_input_dtype(self.x)), zero_mean=True).data.C
            object.__setattr__(self, "_fac", fac)
        return fac


def kernelmatrix(k: Kernel, x, z=None, ctx: Optional[Context] = None) -> np.ndarray:
    """KernelFunctions.kernelmatrix(k, x[, z]) on the device (src/base_gp.jl:70,74)."""
    ctx = ctx or default_context()
    dt = _input_dtype(x)
    m = _Marshal(dt)
    px = m.points(x)
    sfx, kk = m.any_kernel(k, px.d)
    fn = getattr(ctx.lib, "gp_kernelmatrix" + sfx)
    n = px.n
    if z is None:
        out = np.empty((n, n), dtype=dt, order="F")
        check(fn(ctx.handle, C.byref(kk), C.byref(px), None, out.ctypes.data))
    else:
        pz = m.points(z)
        out = np.empty((n, pz.n), dtype=dt, order="F")
        check(fn(ctx.handle, C.byref(kk), C.byref(px), C.byref(pz), out.ctypes.data))
    return out


# --------------------------------------------------------------------------------------------
# FiniteGP API on GP priors: logpdf / posterior
# --------------------------------------------------------------------------------------------
def _check_y(fx: FiniteGP, y):
    y = np.asarray(y)
    if y.shape[0] != len(fx):
        raise ValueError(f"DimensionMismatch: length(fx) = {len(fx)} but y has {y.shape[0]} rows")
    return y


def logpdf(fx: FiniteGP, y):
    """logpdf(f::FiniteGP, Y) — src/finite_gp_projection.jl:306-311.  Vector -> scalar of the input
    eltype; matrix (N×S) -> length-S vector."""
    y = _check_y(fx, y)
    f = fx.f
    if isinstance(f, (PosteriorGP, ApproxPosteriorGP)):
        return _logpdf_posterior(fx, y)
    if not isinstance(f, GP):
        raise TypeError("logpdf: unsupported GP type")
    ctx = f.context()
    dt = np.result_type(_input_dtype(fx.x), np.float32 if y.dtype == np.float32 else np.float64).type
    m = _Marshal(dt)
    px = m.points(fx.x)
    sfx, kk = m.any_kernel(f.kernel, px.d)
    nz = m.noise(fx.sigma2, px.n)
    mean = _mean_vector(f.mean_fn, fx.x, dt)
    mean = None if mean is None else m.arr(mean)
    Y = m.arr(y if y.ndim == 2 else y[:, None], order="F")
    out = np.empty(Y.shape[1], dtype=dt)
    check(getattr(ctx.lib, "gp_logpdf" + sfx)(ctx.handle, C.byref(kk), C.byref(px), C.byref(nz), m.ptr(mean), Y.ctypes.data,
                                              Y.shape[0], Y.shape[1], out.ctypes.data))
    return out[0] if y.ndim == 1 else out


# --------------------------------------------------------------------------------------------
# many small problems in one call: gp_logpdf_batch / gp_logpdf_batch_sum
# --------------------------------------------------------------------------------------------
@dataclass(eq=False)
class _BatchGroup:
    """The problems of a logpdf_batch call that travel in ONE ABI call: one ctx, one dtype, single-kind or composite descriptors."""

    ctx: Optional[Context]  # None: the default context
    dtype: type
    composite: bool
    index: list             # positions in the caller's sequence, ascending
    fxs: list
    ys: list
    nx: int = 0             # 1: every problem holds the SAME x object (sent once), else len(index)
    ny: int = 0
    xss: Optional[list] = None  # mean_and_var_batch: the test points of every problem
    nxs: int = 0


def _batch_groups(fxs, ys) -> list:
    """Grouping of a logpdf_batch call — needs no context and no device.  ys: a sequence of vectors, or ONE vector shared by all."""
    fxs = list(fxs)
    if isinstance(ys, np.ndarray) and ys.ndim == 1 or (len(ys) > 0 and np.ndim(ys[0]) == 0):
        ys = [ys] * len(fxs)  # one vector for every problem: the same object in every entry
    ys = list(ys)
    if len(ys) != len(fxs):
        raise ValueError(f"DimensionMismatch: {len(fxs)} problems but {len(ys)} observation vectors")
    groups = {}
    for i, (fx, y) in enumerate(zip(fxs, ys)):
        if not isinstance(fx, FiniteGP) or not isinstance(fx.f, GP):
            raise TypeError("logpdf_batch: every entry must be a FiniteGP over a GP prior")
        yv = y if isinstance(y, np.ndarray) else np.asarray(y)
        if yv.ndim != 1 or yv.shape[0] != len(fx):
            raise ValueError(f"DimensionMismatch: problem {i}: length(fx) = {len(fx)} but y has shape {yv.shape}")
        dt = np.result_type(_input_dtype(fx.x), np.float32 if yv.dtype == np.float32 else np.float64).type
        key = (id(fx.f.ctx) if fx.f.ctx is not None else None, dt, _is_composite(fx.f.kernel))
        g = groups.get(key)
        if g is None:
            g = groups[key] = _BatchGroup(fx.f.ctx, dt, key[2], [], [], [])
        g.index.append(i)
        g.fxs.append(fx)
        g.ys.append(y)
    out = list(groups.values())
    for g in out:
        g.nx = 1 if all(fx.x is g.fxs[0].x for fx in g.fxs) else len(g.index)
        g.ny = 1 if all(y is g.ys[0] for y in g.ys) else len(g.index)
    return out


@dataclass(eq=False)
class _BatchCall:
    """The marshalled arguments of one gp_logpdf_batch[_sum] call (everything after the ctx) and the buffers behind them."""

    entry: str
    nb: int
    nx: int
    ny: int
    args: tuple
    out: np.ndarray
    info: np.ndarray
    alphas: Optional[list]
    keep: object


def _batch_marshal(g: _BatchGroup, return_alpha: bool) -> _BatchCall:
    """ctypes arguments of one group — needs no context."""
    m = _Marshal(g.dtype)
    nb = len(g.index)
    pts = (gp_points * g.nx)(*[m.points(fx.x) for fx in g.fxs[:g.nx]])
    dims = [pts[0 if g.nx == 1 else b].d for b in range(nb)]
    kerns = [m.ksum(fx.f.kernel, d)[0] if g.composite else m.kernel(fx.f.kernel, d) for fx, d in zip(g.fxs, dims)]
    karr = ((gp_ksum if g.composite else gp_kernel) * nb)(*kerns)
    narr = (gp_noise * nb)(*[m.noise(fx.sigma2, len(fx)) for fx in g.fxs])
    means = [_mean_vector(fx.f.mean_fn, fx.x, g.dtype) for fx in g.fxs]
    means = [None if v is None else m.arr(v) for v in means]
    marr = None if all(v is None for v in means) else (C.c_void_p * nb)(*[None if v is None else v.ctypes.data for v in means])
    yarr = (C.c_void_p * g.ny)(*[m.arr(y).ctypes.data for y in g.ys[:g.ny]])
    out = np.empty(nb, dtype=g.dtype)
    info = np.zeros(nb, dtype=np.int32)
    alphas = [np.empty(len(fx), dtype=g.dtype) for fx in g.fxs] if return_alpha else None
    aarr = (C.c_void_p * nb)(*[a.ctypes.data for a in alphas]) if return_alpha else None
    m.keep += [pts, karr, narr, marr, yarr, aarr]
    args = (nb, karr, g.nx, pts, narr, marr, g.ny, yarr, out.ctypes.data, info.ctypes.data_as(C.POINTER(C.c_int32)), aarr)
    return _BatchCall("gp_logpdf_batch" + ("_sum" if g.composite else ""), nb, g.nx, g.ny, args, out, info, alphas, m)


def _batch_merge(n: int, parts: list, return_alpha: bool, on_error: str):
    """Results of the groups back in the caller's order.  parts: (index, logpdf, info, alphas or None) per group."""
    dt = np.float64 if any(p[1].dtype == np.float64 for p in parts) else np.float32
    lp = np.empty(n, dtype=dt)
    info = np.zeros(n, dtype=np.int32)
    alphas = [None] * n
    for index, out, inf, al in parts:
        lp[index] = out
        info[index] = inf
        if al is not None:
            for i, a in zip(index, al):
                alphas[i] = a
    bad = np.flatnonzero(info)
    if on_error == "raise" and bad.size:
        raise PosDefException(int(info[bad[0]]), index=int(bad[0]))
    return (lp, alphas) if return_alpha else lp


def logpdf_batch(fxs, ys, *, return_alpha: bool = False, on_error: str = "raise"):
    """logpdf(fx_b, y_b) of many independent exact GPs in one library call per (ctx, dtype, single-kind / composite) group
    (src/finite_gp_projection.jl:306-311 once per problem; with return_alpha also α_b = C_b \\ (y_b − m_b), src/exact_gpr_posterior.jl:29-35).
    fxs: FiniteGPs over GP priors — any mix of kernels, sizes, containers, means and noise forms; ys: a sequence of vectors, or ONE vector shared by
    all.  The same x object / y object in every entry is sent once.  on_error = "raise": the PosDefException of the first failing problem (.info,
    .index); "nan": NaN in its place.  Returns an array of the promoted dtype (and the list of α vectors)."""
    if on_error not in ("raise", "nan"):
        raise ValueError('on_error must be "raise" or "nan"')
    fxs = list(fxs)
    if not fxs:
        return (np.empty(0), []) if return_alpha else np.empty(0)
    parts = []
    for g in _batch_groups(fxs, ys):
        call = _batch_marshal(g, return_alpha)
        ctx = g.ctx or default_context()
        check(getattr(ctx.lib, call.entry)(ctx.handle, *call.args))
        parts.append((g.index, call.out, call.info, call.alphas))
    return _batch_merge(len(fxs), parts, return_alpha, on_error)


# --------------------------------------------------------------------------------------------
# the predictive half: gp_predict_batch / gp_predict_batch_sum
# --------------------------------------------------------------------------------------------
def _predict_groups(fxs, ys, xs) -> list:
    """Grouping of a mean_and_var_batch call — needs no context and no device.  The groups are those of _batch_groups (ctx, dtype, single-kind or
    composite); each also carries its problems' test points (`xss`) and nxs = 1 when every problem holds the SAME xs object.  xs: a sequence of input
    containers, one per problem, or ONE container (an array, ColVecs, RowVecs) shared by all."""
    fxs = list(fxs)
    if isinstance(xs, (np.ndarray, ColVecs, RowVecs)):
        xs = [xs] * len(fxs)  # one set of test points for every problem: the same object in every entry
    xs = list(xs)
    if len(xs) != len(fxs):
        raise ValueError(f"DimensionMismatch: {len(fxs)} problems but {len(xs)} sets of test points")
    groups = _batch_groups(fxs, ys)
    for g in groups:
        g.xss = [xs[i] for i in g.index]
        g.nxs = 1 if all(v is g.xss[0] for v in g.xss) else len(g.index)
    return groups


@dataclass(eq=False)
class _PredictCall:
    """The marshalled arguments of one gp_predict_batch[_sum] call (everything after the ctx) and the buffers behind them."""

    entry: str
    nb: int
    nx: int
    ny: int
    nxs: int
    args: tuple
    out: np.ndarray
    info: np.ndarray
    means: Optional[list]
    vars: Optional[list]
    keep: object


def _predict_marshal(g: _BatchGroup, what: int) -> _PredictCall:
    """ctypes arguments of one group — needs no context.  The leading arguments are those of _batch_marshal."""
    fit = _batch_marshal(g, False)
    m = fit.keep
    nb = fit.nb
    nbk, karr, nx, pts, narr, marr, ny, yarr, out, info, _ = fit.args
    xpts = (gp_points * g.nxs)(*[m.points(v) for v in g.xss[:g.nxs]])
    ns = [int(xpts[0 if g.nxs == 1 else b].n) for b in range(nb)]
    pms = [_mean_vector(fx.f.mean_fn, v, g.dtype) for fx, v in zip(g.fxs, g.xss)]  # m(x*) on the host; None = ZeroMean
    pms = [None if v is None else m.arr(v) for v in pms]
    pmarr = None if all(v is None for v in pms) else (C.c_void_p * nb)(*[None if v is None else v.ctypes.data for v in pms])
    means = [np.empty(k, dtype=g.dtype) for k in ns] if what & 1 else None
    vars_ = [np.empty(k, dtype=g.dtype) for k in ns] if what & 2 else None
    moarr = (C.c_void_p * nb)(*[a.ctypes.data for a in means]) if means is not None else None
    voarr = (C.c_void_p * nb)(*[a.ctypes.data for a in vars_]) if vars_ is not None else None
    m.keep += [xpts, pmarr, moarr, voarr]
    args = (nbk, karr, nx, pts, narr, marr, ny, yarr, g.nxs, xpts, pmarr, what, moarr, voarr, out, info)
    return _PredictCall("gp_predict_batch" + ("_sum" if g.composite else ""), nb, g.nx, g.ny, g.nxs, args, fit.out, fit.info, means, vars_, m)


def mean_and_var_batch(fxs, ys, xs, *, what: int = 3, return_logpdf: bool = False, on_error: str = "raise"):
    """mean_and_var(posterior(fx_b, y_b), xs_b) of many independent exact GPs (src/exact_gpr_posterior.jl:29-35, 60-70, once per problem) in one library
    call per (ctx, dtype, single-kind / composite) group: what cross-validation folds, grids, multi-start optimisers and independent outputs sharing one
    x ask after logpdf_batch.  fxs, ys as in logpdf_batch; xs: a sequence of input containers, one per problem (each with its own number of test points,
    0 included), or ONE container shared by all.  The same x / y / xs object in every entry is sent once.  what: 1 the mean, 2 the variance, 3 both.
    Returns the list of (mean, var) pairs in the caller's order, None in place of a side that was not asked for (with return_logpdf: that list and the
    array of logpdf(fx_b, y_b)).  on_error = "raise": the PosDefException of the first failing problem (.info, .index); "nan": NaN in its outputs."""
    if on_error not in ("raise", "nan"):
        raise ValueError('on_error must be "raise" or "nan"')
    if what not in (1, 2, 3):
        raise ValueError("what must be 1 (mean), 2 (var) or 3 (both)")
    fxs = list(fxs)
    if not fxs:
        return ([], np.empty(0)) if return_logpdf else []
    n = len(fxs)
    pairs = [None] * n
    parts = []
    for g in _predict_groups(fxs, ys, xs):
        call = _predict_marshal(g, what)
        ctx = g.ctx or default_context()
        check(getattr(ctx.lib, call.entry)(ctx.handle, *call.args))
        parts.append((g.index, call.out, call.info, None))
        for j, i in enumerate(g.index):
            pairs[i] = (call.means[j] if call.means is not None else None, call.vars[j] if call.vars is not None else None)
    lp = _batch_merge(n, parts, False, on_error)
    return (pairs, lp) if return_logpdf else pairs


# --------------------------------------------------------------------------------------------
# gradients of the batched predictions w.r.t. the test inputs: gp_predict_grad_batch / gp_predict_grad_batch_sum
# --------------------------------------------------------------------------------------------
@dataclass(eq=False)
class _PredictGradCall:
    """The marshalled arguments of one gp_predict_grad_batch[_sum] call (everything after the ctx) and the buffers behind them."""

    entry: str
    nb: int
    args: tuple
    out: np.ndarray
    info: np.ndarray
    means: Optional[list]
    vars: Optional[list]
    dmeans: Optional[list]   # in the ABI layout of each xs_b (_dx_buffer)
    dvars: Optional[list]
    xpts: object             # the gp_points of the test points (nxs entries)
    keep: object


def _predict_grad_marshal(g: _BatchGroup, what: int) -> _PredictGradCall:
    """ctypes arguments of one group — needs no context.  The arguments up to `what` are those of _predict_marshal; all four outputs of the sides in `what`."""
    pc = _predict_marshal(g, what)
    m = pc.keep
    nbk, karr, nx, pts, narr, marr, ny, yarr, nxs, xpts, pmarr, _, moarr, voarr, out, info = pc.args
    pxs = [xpts[0 if g.nxs == 1 else b] for b in range(pc.nb)]
    dmeans = [_dx_buffer(px, g.dtype) for px in pxs] if what & 1 else None
    dvars = [_dx_buffer(px, g.dtype) for px in pxs] if what & 2 else None
    dmarr = (C.c_void_p * pc.nb)(*[a.ctypes.data for a in dmeans]) if dmeans is not None else None
    dvarr = (C.c_void_p * pc.nb)(*[a.ctypes.data for a in dvars]) if dvars is not None else None
    m.keep += [dmarr, dvarr]
    args = (nbk, karr, nx, pts, narr, marr, ny, yarr, nxs, xpts, pmarr, what, moarr, voarr, dmarr, dvarr, out, info)
    return _PredictGradCall("gp_predict_grad_batch" + ("_sum" if g.composite else ""), pc.nb, args, pc.out, pc.info, pc.means, pc.vars, dmeans, dvars, pxs, m)


def mean_and_var_grad_batch(fxs, ys, xs, *, what: int = 3, mean_grads=None, return_logpdf: bool = False, on_error: str = "raise"):
    """mean_and_var_grad(posterior(fx_b, y_b), xs_b) of many independent exact GPs in one library call per (ctx, dtype, single-kind / composite) group:
    the predictions of mean_and_var_batch AND their gradients w.r.t. the test inputs — what a gradient-based acquisition step over many surrogates
    (multi-start UCB / EI, one local GP per trust region, independent outputs sharing one x) evaluates.  fxs, ys, xs, what, on_error as in
    mean_and_var_batch.  Returns the list of (mean, var, dmean, dvar) in the caller's order, None for whatever was not asked for; the gradients have the
    shape of each xs_b's array, as mean_and_var_grad shapes them (with return_logpdf: that list and the array of logpdf(fx_b, y_b)).
    The device treats the prior mean as constant in x*: a problem with a CustomMean and the mean side needs its entry of `mean_grads` (a sequence with one
    entry per problem, None where not needed): a callable x -> the (ns × d) derivative of the mean function, which is added to dmean (TypeError without it)."""
    if on_error not in ("raise", "nan"):
        raise ValueError('on_error must be "raise" or "nan"')
    if what not in (1, 2, 3):
        raise ValueError("what must be 1 (mean), 2 (var) or 3 (both)")
    fxs = list(fxs)
    if not fxs:
        return ([], np.empty(0)) if return_logpdf else []
    n = len(fxs)
    mean_grads = [None] * n if mean_grads is None else list(mean_grads)
    if len(mean_grads) != n:
        raise ValueError(f"DimensionMismatch: {n} problems but {len(mean_grads)} entries of mean_grads")
    groups = _predict_groups(fxs, ys, xs)
    for i, fx in enumerate(fxs):
        if callable(fx.f.mean_fn) and (what & 1) and mean_grads[i] is None:
            raise TypeError(f"problem {i}: the prior mean is a CustomMean: pass mean_grads[{i}] = callable returning its (ns × d) derivative at xs")
    quads = [None] * n
    parts = []
    for g in groups:
        call = _predict_grad_marshal(g, what)
        ctx = g.ctx or default_context()
        check(getattr(ctx.lib, call.entry)(ctx.handle, *call.args))
        parts.append((g.index, call.out, call.info, None))
        for j, i in enumerate(g.index):
            px, x = call.xpts[j], g.xss[j]
            dmean = _dx_shaped(call.dmeans[j], px, x) if call.dmeans is not None else None
            dvar = _dx_shaped(call.dvars[j], px, x) if call.dvars is not None else None
            if dmean is not None and callable(g.fxs[j].f.mean_fn):
                gm = np.asarray(mean_grads[i](x), dtype=g.dtype).reshape(px.n, px.d)  # (ns × d)
                dmean = dmean + (gm[:, 0] if px.layout == 0 else (gm.T if isinstance(_as_input(x), ColVecs) else gm))
            quads[i] = (call.means[j] if call.means is not None else None, call.vars[j] if call.vars is not None else None, dmean, dvar)
    lp = _batch_merge(n, parts, False, on_error)
    return (quads, lp) if return_logpdf else quads


# --------------------------------------------------------------------------------------------
# the joint predictive distribution of many small problems: gp_joint_batch / gp_joint_batch_sum
# --------------------------------------------------------------------------------------------
JOINT_MEAN, JOINT_COV, JOINT_LOGPDF, JOINT_RAND = 1, 4, 8, 16  # the bits of gp_joint_batch's `what`


@dataclass(eq=False)
class _JointCall:
    """The marshalled arguments of one gp_joint_batch[_sum] call (everything after the ctx) and the buffers behind them."""

    entry: str
    nb: int
    nx: int
    ny: int
    nxs: int
    args: tuple
    out: np.ndarray                # logpdf(fx_b, y_b)
    info: np.ndarray
    info_joint: np.ndarray
    means: Optional[list]
    covs: Optional[list]           # ns_b × ns_b, Fortran order
    heldout: Optional[np.ndarray]
    samples: Optional[list]        # ns_b × nsamp, Fortran order
    keep: object


def _joint_marshal(g: _BatchGroup, what: int, noises, ys_heldout, xis) -> _JointCall:
    """ctypes arguments of one group — needs no context.  The leading arguments are those of _predict_marshal; noises / ys_heldout / xis: one entry per
    problem of the group (Σy*_b or None = zero; y*_b; the standard normals of problem b, ns_b × nsamp), or None."""
    pc = _predict_marshal(g, what & 1)
    m, nb = pc.keep, pc.nb
    nbk, karr, nx, pts, narr, marr, ny, yarr, nxs, xpts, pmarr, _, moarr, _, out, info = pc.args
    ns = [int(xpts[0 if g.nxs == 1 else b].n) for b in range(nb)]
    nzarr = None
    if noises is not None and any(v is not None for v in noises):
        nzarr = (gp_noise * nb)(*[m.noise(0.0 if v is None else v, k) for v, k in zip(noises, ns)])
    covs = [np.empty((k, k), dtype=g.dtype, order="F") for k in ns] if what & JOINT_COV else None
    coarr = (C.c_void_p * nb)(*[a.ctypes.data for a in covs]) if covs is not None else None
    ysarr = heldout = None
    if what & JOINT_LOGPDF:
        ysv = []
        for b, (v, k) in enumerate(zip(ys_heldout, ns)):
            v = m.arr(np.asarray(v))
            if v.shape != (k,):
                raise ValueError(f"DimensionMismatch: problem {g.index[b]}: {k} test points but ys_heldout has shape {v.shape}")
            ysv.append(v)
        ysarr = (C.c_void_p * nb)(*[v.ctypes.data for v in ysv])
        heldout = np.zeros(nb, dtype=g.dtype)  # logpdf of no observations: 0
    nsamp, xiarr, samples, soarr = 0, None, None, None
    if what & JOINT_RAND:
        xiv = []
        for b, (v, k) in enumerate(zip(xis, ns)):
            v = np.asarray(v, dtype=g.dtype)
            v = v.reshape(k, -1) if v.ndim != 2 else v
            if v.shape[0] != k or (xiv and v.shape[1] != xiv[0].shape[1]):
                raise ValueError(f"DimensionMismatch: problem {g.index[b]}: xi must be ({k}, nsamp) with one nsamp per call, got {v.shape}")
            xiv.append(m.arr(v, order="F"))
        nsamp = xiv[0].shape[1]
        xiarr = (C.c_void_p * nb)(*[v.ctypes.data for v in xiv])
        samples = [np.empty((k, nsamp), dtype=g.dtype, order="F") for k in ns]
        soarr = (C.c_void_p * nb)(*[a.ctypes.data for a in samples])
    info_joint = np.zeros(nb, dtype=np.int32)
    m.keep += [nzarr, coarr, ysarr, xiarr, soarr]
    args = (nbk, karr, nx, pts, narr, marr, ny, yarr, nxs, xpts, pmarr, nzarr, what, moarr, coarr, ysarr, None if heldout is None else heldout.ctypes.data, nsamp,
            xiarr, soarr, out, info, info_joint.ctypes.data_as(C.POINTER(C.c_int32)))
    return _JointCall("gp_joint_batch" + ("_sum" if g.composite else ""), nb, g.nx, g.ny, g.nxs, args, pc.out, pc.info, info_joint, pc.means, covs, heldout, samples, m)


def _per_problem(v, n: int, name: str):
    """None, or one entry per problem: a sequence of n entries, or ONE entry (a scalar) for all of them"""
    if v is None:
        return None
    if not isinstance(v, (list, tuple)) and np.ndim(v) == 0:
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f"DimensionMismatch: {n} problems but {len(v)} entries of {name}")
    return v


def joint_batch(fxs, ys, xs, *, noise=None, ys_heldout=None, xi=None, what: Optional[int] = None, return_logpdf: bool = False, on_error: str = "raise"):
    """The joint predictive distribution of many independent exact GPs at their test points, in one library call per (ctx, dtype, single-kind / composite)
    group — per problem what posterior(fx_b, y_b)(xs_b, noise_b) answers (src/exact_gpr_posterior.jl:78-83, src/finite_gp_projection.jl:133-136, 233-237,
    306-311): mean and latent covariance (no Σy* added, as mean_and_cov(post, xs_b)), the held-out logpdf(post_b(xs_b, noise_b), ys_heldout_b) and joint samples
    mean + chol(cov + noise_b).L @ xi_b.  fxs, ys, xs as in mean_and_var_batch.  noise: None (zero), one scalar for all, or one entry per problem (None, a
    scalar, a vector or a dense matrix over the ns_b test points).  ys_heldout: one vector per problem; xi: one (ns_b × nsamp) array of standard normals per
    problem, one nsamp per call.  what: bits 1 mean | 4 covariance | 8 held-out logpdf | 16 samples; default: mean and covariance, plus whatever ys_heldout /
    xi ask for.  Returns the list of (mean, cov, heldout_logpdf, samples) in the caller's order, None for what was not asked for (with return_logpdf: that
    list and the array of logpdf(fx_b, y_b)).  on_error = "raise": the PosDefException of the first failing problem — its fit, or its joint covariance (.info,
    .index); "nan": NaN in the outputs the failure reaches (a joint covariance that is not positive definite leaves mean and cov valid)."""
    if on_error not in ("raise", "nan"):
        raise ValueError('on_error must be "raise" or "nan"')
    if what is None:
        what = JOINT_MEAN | JOINT_COV | (JOINT_LOGPDF if ys_heldout is not None else 0) | (JOINT_RAND if xi is not None else 0)
    if what <= 0 or what & ~(JOINT_MEAN | JOINT_COV | JOINT_LOGPDF | JOINT_RAND):
        raise ValueError("what must be a combination of 1 (mean), 4 (cov), 8 (held-out logpdf) and 16 (samples)")
    if what & JOINT_LOGPDF and ys_heldout is None:
        raise ValueError("the held-out logpdf needs ys_heldout")
    if what & JOINT_RAND and xi is None:
        raise ValueError("samples need xi, the standard normals of every problem")
    fxs = list(fxs)
    if not fxs:
        return ([], np.empty(0)) if return_logpdf else []
    n = len(fxs)
    noise, ys_heldout, xi = _per_problem(noise, n, "noise"), _per_problem(ys_heldout, n, "ys_heldout"), _per_problem(xi, n, "xi")
    quads = [None] * n
    parts, joint_bad = [], []
    for g in _predict_groups(fxs, ys, xs):
        pick = lambda v: None if v is None else [v[i] for i in g.index]
        call = _joint_marshal(g, what, pick(noise), pick(ys_heldout), pick(xi))
        ctx = g.ctx or default_context()
        check(getattr(ctx.lib, call.entry)(ctx.handle, *call.args))
        parts.append((g.index, call.out, call.info, None))
        for j, i in enumerate(g.index):
            quads[i] = (call.means[j] if call.means is not None else None, call.covs[j] if call.covs is not None else None,
                        call.heldout[j] if call.heldout is not None else None, call.samples[j] if call.samples is not None else None)
            if call.info_joint[j]:
                joint_bad.append((i, int(call.info_joint[j])))
    lp = _batch_merge(n, parts, False, on_error)
    if on_error == "raise" and joint_bad:
        i, info = min(joint_bad)
        raise PosDefException(info, index=i)
    return (quads, lp) if return_logpdf else quads


def mean_and_cov_batch(fxs, ys, xs, **kw):
    """mean_and_cov(posterior(fx_b, y_b), xs_b) of every problem: the (mean, cov) pairs of joint_batch(what = 1 | 4)."""
    res = joint_batch(fxs, ys, xs, what=JOINT_MEAN | JOINT_COV, **kw)
    pairs = [(q[0], q[1]) for q in (res[0] if kw.get("return_logpdf") else res)]
    return (pairs, res[1]) if kw.get("return_logpdf") else pairs


def logpdf_heldout_batch(fxs, ys, xs, ys_heldout, *, noise=None, **kw):
    """logpdf(posterior(fx_b, y_b)(xs_b, noise_b), ys_heldout_b) of every problem — the score of a cross-validation fold: joint_batch(what = 8) as one array."""
    res = joint_batch(fxs, ys, xs, noise=noise, ys_heldout=ys_heldout, what=JOINT_LOGPDF, **kw)
    quads = res[0] if kw.get("return_logpdf") else res
    hl = np.array([q[2] for q in quads], dtype=np.result_type(*[np.asarray(q[2]).dtype for q in quads]) if quads else np.float64)
    return (hl, res[1]) if kw.get("return_logpdf") else hl


def rand_batch(fxs, ys, xs, xi, *, noise=None, **kw):
    """rand(posterior(fx_b, y_b)(xs_b, noise_b), nsamp) of every problem with the caller's standard normals xi_b (ns_b × nsamp): joint_batch(what = 16), the list of
    (ns_b × nsamp) arrays."""
    res = joint_batch(fxs, ys, xs, noise=noise, xi=xi, what=JOINT_RAND, **kw)
    draws = [q[3] for q in (res[0] if kw.get("return_logpdf") else res)]
    return (draws, res[1]) if kw.get("return_logpdf") else draws


def _terms(fx: FiniteGP, y, want_logdet: bool, want_sqmahal: bool):
    """gp_logpdf_terms (gp_logpdf_terms_sum for a composite kernel): logdet(cov(fx)) and / or sqmahal(fx, y) from ONE factorisation on the device."""
    f = fx.f
    if not isinstance(f, GP):
        raise TypeError("only GP priors are accelerated here (the shim falls back to the stock methods otherwise)")
    ctx = f.context()
    dt = _input_dtype(fx.x) if y is None else np.result_type(_input_dtype(fx.x), np.float32 if np.asarray(y).dtype == np.float32 else np.float64).type
    m = _Marshal(dt)
    px = m.points(fx.x)
    composite = _is_composite(f.kernel)
    kk = m.ksum(f.kernel, px.d)[0] if composite else m.kernel(f.kernel, px.d)
    nz = m.noise(fx.sigma2, px.n)
    mean = _mean_vector(f.mean_fn, fx.x, dt)
    mean = None if mean is None else m.arr(mean)
    Y = None if y is None else m.arr(y if y.ndim == 2 else y[:, None], order="F")
    ld = np.empty(1, dtype=dt)
    sq = np.empty(1 if Y is None else Y.shape[1], dtype=dt)
    terms = ctx.lib.gp_logpdf_terms_sum if composite else ctx.lib.gp_logpdf_terms
    check(terms(ctx.handle, C.byref(kk), C.byref(px), C.byref(nz), m.ptr(mean), m.ptr(Y), px.n, 0 if Y is None else Y.shape[1],
                ld.ctypes.data if want_logdet else None, sq.ctypes.data if want_sqmahal else None))
    return ld[0], sq


def sqmahal(fx: FiniteGP, y):
    """Distributions.sqmahal(f::FiniteGP, x) — src/finite_gp_projection.jl:315-326: (y − m)ᵀ C⁻¹ (y − m); one value per column."""
    y = _check_y(fx, y)
    sq = _terms(fx, y, False, True)[1]
    return sq[0] if y.ndim == 1 else sq


def logdetcov(fx: FiniteGP):
    """Distributions.logdetcov(f::FiniteGP) = logdet(cov(f)) — src/finite_gp_projection.jl:313."""
    return _terms(fx, None, True, False)[0]


def gradlogpdf(fx: FiniteGP, y):
    """Distributions.gradlogpdf(f::FiniteGP, x) = C \\ (m .- x) — src/finite_gp_projection.jl:328-337: −α for a vector; for a matrix
    the factor of the first column's fit is reused for all columns (gp_posterior_solve)."""
    y = _check_y(fx, y)
    f = fx.f
    if not isinstance(f, GP):
        raise TypeError("only GP priors are accelerated here")
    post = _posterior_exact(fx, y if y.ndim == 1 else y[:, 0])
    try:
        if y.ndim == 1:
            return -post.data.alpha
        dt = post.data.alpha.dtype
        mean = _mean_vector(f.mean_fn, fx.x, dt)
        D = np.asfortranarray((np.asarray(y, dtype=dt) - (0 if mean is None else np.asarray(mean, dtype=dt)[:, None])))
        out = np.empty_like(D, order="F")
        check(post.data.C.ctx.lib.gp_posterior_solve(post.data.C.handle, D.ctypes.data, D.shape[1], out.ctypes.data))
        return -out
    finally:
        post.data.C.free()


def _dnoise_shape(nz: gp_noise, n: int):
    """dnoise_out of gp_logpdf_grad: 1 entry (scalar Σy), n (Diagonal), n×n (dense: symmetric, so column-major == row-major)."""
    return 1 if nz.kind == 0 else (n if nz.kind == 1 else (n, n))


def _dx_buffer(px: gp_points, dt) -> np.ndarray:
    """dx_out of gp_logpdf_grad / gp_logpdf_grad_sum_x, in the ABI layout of the inputs: (n,) vector; ColVecs (N, D) C-order = D×N column-major; RowVecs (D, N)."""
    return np.empty((px.n,) if px.layout == 0 else ((px.n, px.d) if px.layout == 1 else (px.d, px.n)), dtype=dt)


def _dx_shaped(dxb: np.ndarray, px: gp_points, x) -> np.ndarray:
    """The buffer comes back in the ABI layout the inputs were passed in: (n, d) for layout 1, (d, n) for layout 2; the result has the shape of x.X."""
    if px.layout == 0:
        return dxb
    nd = dxb if px.layout == 1 else dxb.T                       # (N, D) view
    return np.ascontiguousarray(nd.T if isinstance(_as_input(x), ColVecs) else nd)


def logpdf_and_grad(fx: FiniteGP, y, wrt_x: bool = False) -> tuple:
    """Value and gradient of logpdf(fx, y) for the rrule of the accelerated path (the reference differentiates the same
    expression by AD — test/finite_gp_projection.jl:152-178).  Returns (logpdf, grads) with grads =
    {"variance": ∂/∂σ_k², "scale": ∂/∂s (ScaleTransform) or ∂/∂v (ARDTransform) or None, "noise": ∂/∂σ² (scalar Σy), the
    vector ∂/∂Σy_ii, or for a dense Σy the (n, n) symmetric matrix G = ½(ααᵀ − C⁻¹) with d logpdf = ⟨G, dΣy⟩ for symmetric dΣy (a parametric Σy(φ) chains
    as ⟨G, ∂Σy/∂φ⟩), "y": −α, "mean": +α} and, with wrt_x, "x": ∂/∂x in the shape of the input container's array.
    A composite kernel (sums, products, Periodic / RationalQuadratic / White) returns "kernel": ∂/∂params(k) in the order of params(k), and "theta":
    the gradient against the flat θ of include/gpmi355.h (gp_logpdf_grad_sum; gp_logpdf_grad_sum_x with wrt_x), in place of "variance" / "scale"."""
    return _objective_and_grad(fx, y, wrt_x, "logpdf_and_grad", "gp_logpdf_grad")


def _objective_and_grad(fx: FiniteGP, y, wrt_x: bool, who: str, call: str) -> tuple:
    """The body logpdf_and_grad (call = "gp_logpdf_grad") and loo_logpdf_and_grad ("gp_loo_grad") share: the two families take the same arguments and
    return the same outputs, except that gp_logpdf_grad_sum has no dx_out (gp_logpdf_grad_sum_x has it) where gp_loo_grad_sum always has one."""
    y = _check_y(fx, y)
    if y.ndim != 1:
        raise TypeError(f"{who} expects a vector of observations")
    f = fx.f
    if not isinstance(f, GP):
        raise TypeError(f"{who}: unsupported GP type")
    ctx = f.context()
    dt = np.result_type(_input_dtype(fx.x), np.float32 if y.dtype == np.float32 else np.float64).type
    m = _Marshal(dt)
    px = m.points(fx.x)
    kk = None if _is_composite(f.kernel) else m.kernel(f.kernel, px.d)
    nz = m.noise(fx.sigma2, px.n)
    mean = _mean_vector(f.mean_fn, fx.x, dt)
    mean = None if mean is None else m.arr(mean)
    yv = m.arr(y)
    lp = np.empty(1, dtype=dt)
    if _is_composite(f.kernel):
        ks, nf = m.ksum(f.kernel, px.d)
        dth = (C.c_double * max(len(nf.theta()), 1))()
        dnoise = np.empty(_dnoise_shape(nz, px.n), dtype=dt)
        dy = np.empty(px.n, dtype=dt)
        head = (ctx.handle, C.byref(ks), C.byref(px), C.byref(nz), m.ptr(mean), yv.ctypes.data, lp.ctypes.data, dth, dnoise.ctypes.data, dy.ctypes.data)
        dxb = _dx_buffer(px, dt) if wrt_x else None
        if wrt_x or call != "gp_logpdf_grad":
            check(getattr(ctx.lib, call + ("_sum_x" if call == "gp_logpdf_grad" else "_sum"))(*head, m.ptr(dxb)))
        else:
            check(ctx.lib.gp_logpdf_grad_sum(*head))
        gth = np.array(dth[:len(nf.theta())])
        g = {"kernel": nf.chain(gth), "theta": gth, "noise": dnoise[0] if nz.kind == 0 else dnoise, "y": dy, "mean": -dy}
        if wrt_x:
            g["x"] = _dx_shaped(dxb, px, fx.x)
        return lp[0], g
    dvar = C.c_double()
    dscale = (C.c_double * max(kk.nscale, 1))()
    dnoise = np.empty(_dnoise_shape(nz, px.n), dtype=dt)
    dy = np.empty(px.n, dtype=dt)
    dxb = _dx_buffer(px, dt) if wrt_x else None
    check(getattr(ctx.lib, call)(ctx.handle, C.byref(kk), C.byref(px), C.byref(nz), m.ptr(mean), yv.ctypes.data,
                                 lp.ctypes.data, C.byref(dvar), dscale, dnoise.ctypes.data, dy.ctypes.data, m.ptr(dxb)))
    sc = None
    if kk.nscale == 1:
        sc = float(dscale[0])
    elif kk.nscale > 1:
        sc = np.array([dscale[i] for i in range(kk.nscale)])
    g = {"variance": dvar.value, "scale": sc, "noise": dnoise[0] if nz.kind == 0 else dnoise, "y": dy, "mean": -dy}
    if wrt_x:
        g["x"] = _dx_shaped(dxb, px, fx.x)
    return lp[0], g


# --------------------------------------------------------------------------------------------
# leave-one-out cross-validation: gp_loo / gp_loo_grad and their *_sum forms
# --------------------------------------------------------------------------------------------
def _loo(fx: FiniteGP, y, who: str):
    """(L, ℓ, μ, v) of gp_loo / gp_loo_sum for a GP prior and a vector of observations."""
    y = _check_y(fx, y)
    if y.ndim != 1:
        raise TypeError(f"{who} expects a vector of observations")
    f = fx.f
    if not isinstance(f, GP):
        raise TypeError(f"{who}: only GP priors are accelerated here (condition on the data with one fit instead of a PosteriorGP prior)")
    ctx = f.context()
    dt = np.result_type(_input_dtype(fx.x), np.float32 if y.dtype == np.float32 else np.float64).type
    m = _Marshal(dt)
    px = m.points(fx.x)
    sfx, kk = m.any_kernel(f.kernel, px.d)
    nz = m.noise(fx.sigma2, px.n)
    mean = _mean_vector(f.mean_fn, fx.x, dt)
    mean = None if mean is None else m.arr(mean)
    yv = m.arr(y)
    val = np.empty(1, dtype=dt)
    lp, mu, var = (np.empty(px.n, dtype=dt) for _ in range(3))
    check(getattr(ctx.lib, "gp_loo" + sfx)(ctx.handle, C.byref(kk), C.byref(px), C.byref(nz), m.ptr(mean), yv.ctypes.data, val.ctypes.data,
                                           lp.ctypes.data, mu.ctypes.data, var.ctypes.data))
    return val[0], lp, mu, var


def loo_mean_and_var(fx: FiniteGP, y) -> tuple:
    """Leave-one-out predictions (Rasmussen & Williams §5.4.2): (μ, v) with μ_i, v_i the predictive mean and variance of y_i — its own observation noise
    included — given every other observation, from ONE fit (gp_loo): μ_i = y_i − α_i / [C⁻¹]_ii, v_i = 1 / [C⁻¹]_ii."""
    _, _, mu, var = _loo(fx, y, "loo_mean_and_var")
    return mu, var


def loo_logpdf(fx: FiniteGP, y, pointwise: bool = False):
    """The leave-one-out log predictive density L = Σ_i log p(y_i | y_−i) of fx at y (gp_loo); with pointwise, the n terms log p(y_i | y_−i) instead."""
    val, lp, _, _ = _loo(fx, y, "loo_logpdf")
    return lp if pointwise else val


def loo_logpdf_and_grad(fx: FiniteGP, y, wrt_x: bool = False) -> tuple:
    """Value and gradient of loo_logpdf(fx, y) as a training objective (gp_loo_grad / gp_loo_grad_sum): (L, grads) with the keys of logpdf_and_grad —
    "variance" / "scale" (or "kernel" / "theta" for a composite kernel), "noise" (scalar, vector, or for a dense Σy the symmetric (n, n) matrix G with
    dL = ⟨G, dΣy⟩), "y", "mean" and, with wrt_x, "x"."""
    return _objective_and_grad(fx, y, wrt_x, "loo_logpdf_and_grad", "gp_loo_grad")


# --------------------------------------------------------------------------------------------
# the training half of the batch calls: gp_logpdf_grad_batch / gp_logpdf_grad_batch_sum
# --------------------------------------------------------------------------------------------
@dataclass(eq=False)
class _GradBatchCall:
    """The marshalled arguments of one gp_logpdf_grad_batch[_sum] call (everything after the ctx) and the buffers behind them."""

    entry: str
    nb: int
    nx: int
    ny: int
    args: tuple
    out: np.ndarray
    info: np.ndarray
    dvar: Optional[np.ndarray]   # single-kind: nb entries
    dscale: Optional[list]       # single-kind: per problem an array of nscale entries, None where the kernel has no transform
    dtheta: Optional[list]       # composite: per problem an array over θ
    nfs: Optional[list]          # composite: the _NormalForm of every problem (the chain rule back to params(k))
    dnoise: list                 # per problem: 1 entry, n entries or (n, n)
    dy: list
    noise_kind: list
    keep: object
    dx: Optional[list] = None    # wrt_x: per problem the buffer in the ABI layout of its inputs (_dx_buffer)
    pts: object = None           # the gp_points array of the call (nx entries)


def _grad_batch_marshal(g: _BatchGroup, wrt_x: bool = False) -> _GradBatchCall:
    """ctypes arguments of one group — needs no context.  The leading arguments are those of _batch_marshal; with wrt_x the entry point is the one with
    `_x` behind its name and the dx array behind the others (every problem its own buffer, also where all share one x)."""
    call = _grad_batch_marshal_plain(g)
    if not wrt_x:
        return call
    pts = call.args[3]
    call.pts = pts
    call.dx = [_dx_buffer(pts[0 if g.nx == 1 else b], g.dtype) for b in range(call.nb)]
    dxarr = (C.c_void_p * call.nb)(*[a.ctypes.data for a in call.dx])
    call.keep.keep.append(dxarr)
    call.entry += "_x"
    call.args = call.args + (dxarr,)
    return call


def _grad_batch_marshal_plain(g: _BatchGroup) -> _GradBatchCall:
    fit = _batch_marshal(g, False)
    m = fit.keep
    nb = fit.nb
    nbk, karr, nx, pts, narr, marr, ny, yarr, out, info, _ = fit.args
    ns = [len(fx) for fx in g.fxs]
    kinds = [int(narr[b].kind) for b in range(nb)]
    dnoise = [np.empty(_dnoise_shape(narr[b], ns[b]), dtype=g.dtype) for b in range(nb)]
    dy = [np.empty(n, dtype=g.dtype) for n in ns]
    dnarr = (C.c_void_p * nb)(*[a.ctypes.data for a in dnoise])
    dyarr = (C.c_void_p * nb)(*[a.ctypes.data for a in dy])
    m.keep += [dnarr, dyarr]
    if g.composite:
        nfs = [_NormalForm(fx.f.kernel) for fx in g.fxs]
        dtheta = [np.empty(len(nf.theta()), dtype=np.float64) for nf in nfs]
        dtarr = (C.c_void_p * nb)(*[a.ctypes.data for a in dtheta])
        m.keep.append(dtarr)
        args = (nbk, karr, nx, pts, narr, marr, ny, yarr, out, info, dtarr, dnarr, dyarr)
        return _GradBatchCall("gp_logpdf_grad_batch_sum", nb, g.nx, g.ny, args, fit.out, fit.info, None, None, dtheta, nfs, dnoise, dy, kinds, m)
    dvar = np.empty(nb, dtype=np.float64)
    dscale = [np.empty(karr[b].nscale, dtype=np.float64) if karr[b].nscale > 0 else None for b in range(nb)]
    dsarr = (C.c_void_p * nb)(*[None if a is None else a.ctypes.data for a in dscale])  # NULL where nscale = 0
    m.keep.append(dsarr)
    args = (nbk, karr, nx, pts, narr, marr, ny, yarr, out, info, dvar.ctypes.data_as(C.POINTER(C.c_double)), dsarr, dnarr, dyarr)
    return _GradBatchCall("gp_logpdf_grad_batch", nb, g.nx, g.ny, args, fit.out, fit.info, dvar, dscale, None, None, dnoise, dy, kinds, m)


def logpdf_and_grad_batch(fxs, ys, *, wrt_x: bool = False, on_error: str = "raise"):
    """Value and gradient of logpdf(fx_b, y_b) of many independent exact GPs in one library call per (ctx, dtype, single-kind / composite) group —
    what multi-start hyper-parameter optimisation, gradient-based samplers over hyper-parameters and per-fold training evaluate at every step.  fxs, ys
    as in logpdf_batch (the same x / y object in every entry is sent once).  Returns (array of logpdf, list of dicts in the caller's order); each dict
    is that of logpdf_and_grad: {"variance", "scale", "noise", "y", "mean"} for a single-kind kernel, {"kernel", "theta", "noise", "y", "mean"} for a
    composite one and, with wrt_x (gp_logpdf_grad_batch_x / _sum_x), "x": ∂/∂x in the shape and dtype of that problem's input array, as
    logpdf_and_grad(wrt_x=True) returns it — what a deep-kernel model behind many small GPs back-propagates into its feature map; problems that share one x
    object each get their own gradient w.r.t. it.  on_error = "raise": the PosDefException of the first failing problem (.info, .index); "nan": NaN in its
    logpdf and in every entry of its gradient."""
    return _objective_and_grad_batch(fxs, ys, wrt_x, on_error, _grad_batch_marshal)


def _objective_and_grad_batch(fxs, ys, wrt_x, on_error: str, marshal):
    """The body logpdf_and_grad_batch (marshal = _grad_batch_marshal) and loo_logpdf_and_grad_batch (_loo_grad_batch_marshal) share: the two families
    take the same arguments and return the same outputs."""
    if on_error not in ("raise", "nan"):
        raise ValueError('on_error must be "raise" or "nan"')
    if not isinstance(wrt_x, (bool, np.bool_)):
        raise TypeError("wrt_x must be a bool")
    fxs = list(fxs)
    if not fxs:
        return np.empty(0), []
    grads = [None] * len(fxs)
    parts = []
    for g in _batch_groups(fxs, ys):
        call = marshal(g, bool(wrt_x))
        ctx = g.ctx or default_context()
        check(getattr(ctx.lib, call.entry)(ctx.handle, *call.args))
        parts.append((g.index, call.out, call.info, None))
        for j, i in enumerate(g.index):
            dn = call.dnoise[j][0] if call.noise_kind[j] == 0 else call.dnoise[j]
            tail = {"noise": dn, "y": call.dy[j], "mean": -call.dy[j]}
            if g.composite:
                grads[i] = {"kernel": call.nfs[j].chain(call.dtheta[j]), "theta": call.dtheta[j], **tail}
            else:
                sc = call.dscale[j]
                grads[i] = {"variance": float(call.dvar[j]), "scale": None if sc is None else (float(sc[0]) if sc.shape[0] == 1 else sc), **tail}
            if wrt_x:
                grads[i]["x"] = _dx_shaped(call.dx[j], call.pts[0 if g.nx == 1 else j], g.fxs[j].x)
    return _batch_merge(len(fxs), parts, False, on_error), grads


# --------------------------------------------------------------------------------------------
# leave-one-out cross-validation of many small problems in one call: gp_loo_batch / gp_loo_grad_batch and their *_sum forms
# --------------------------------------------------------------------------------------------
@dataclass(eq=False)
class _LooBatchCall:
    """The marshalled arguments of one gp_loo_batch[_sum] call (everything after the ctx) and the buffers behind them."""

    entry: str
    nb: int
    nx: int
    ny: int
    args: tuple
    out: np.ndarray           # L of every problem
    info: np.ndarray
    lp: Optional[list]        # per problem n entries, or None where the call does not ask for them
    mean: Optional[list]
    var: Optional[list]
    keep: object


def _loo_batch_marshal(g: _BatchGroup, want_lp: bool = True, want_pred: bool = True) -> _LooBatchCall:
    """ctypes arguments of one group — needs no context.  The leading arguments are those of _batch_marshal; behind value_out and info_out the arrays of
    ℓ (want_lp), μ and v (want_pred) pointers, NULL for what is not asked for."""
    fit = _batch_marshal(g, False)
    m, nb = fit.keep, fit.nb
    ns = [len(fx) for fx in g.fxs]

    def outs(want):
        if not want:
            return None, None
        bufs = [np.empty(n, dtype=g.dtype) for n in ns]
        arr = (C.c_void_p * nb)(*[a.ctypes.data for a in bufs])
        m.keep.append(arr)
        return bufs, arr

    (lp, lparr), (mu, muarr), (var, vararr) = outs(want_lp), outs(want_pred), outs(want_pred)
    return _LooBatchCall("gp_loo_batch" + ("_sum" if g.composite else ""), nb, g.nx, g.ny, fit.args[:-1] + (lparr, muarr, vararr), fit.out, fit.info,
                         lp, mu, var, m)


def _loo_grad_batch_marshal(g: _BatchGroup, wrt_x: bool = False) -> _GradBatchCall:
    """ctypes arguments of one group — needs no context: those of _grad_batch_marshal for gp_loo_grad_batch[_sum], whose dx array is always part of the
    prototype (NULL without wrt_x)."""
    call = _grad_batch_marshal(g, wrt_x)
    call.entry = "gp_loo_grad_batch" + ("_sum" if g.composite else "")
    if not wrt_x:
        call.args = call.args + (None,)
    return call


def _loo_batch(fxs, ys, on_error: str, want_lp: bool, want_pred: bool):
    """(L in the caller's order, per-problem ℓ, μ, v lists) of one gp_loo_batch[_sum] call per group"""
    if on_error not in ("raise", "nan"):
        raise ValueError('on_error must be "raise" or "nan"')
    fxs = list(fxs)
    n = len(fxs)
    lp, mu, var = [None] * n, [None] * n, [None] * n
    if not fxs:
        return np.empty(0), lp, mu, var
    parts = []
    for g in _batch_groups(fxs, ys):
        call = _loo_batch_marshal(g, want_lp, want_pred)
        ctx = g.ctx or default_context()
        check(getattr(ctx.lib, call.entry)(ctx.handle, *call.args))
        parts.append((g.index, call.out, call.info, None))
        for j, i in enumerate(g.index):
            if want_lp:
                lp[i] = call.lp[j]
            if want_pred:
                mu[i], var[i] = call.mean[j], call.var[j]
    return _batch_merge(n, parts, False, on_error), lp, mu, var


def loo_logpdf_batch(fxs, ys, *, pointwise: bool = False, on_error: str = "raise"):
    """loo_logpdf(fx_b, y_b) of many independent exact GPs in one library call per (ctx, dtype, single-kind / composite) group (gp_loo_batch) — what a grid
    of hyper-parameters scored by its leave-one-out log predictive density evaluates again and again.  fxs, ys as in logpdf_batch (the same x / y object
    in every entry is sent once).  Returns the array of L_b; with pointwise, (that array, the list of the vectors log p(y_i | y_−i) in the caller's
    order).  on_error = "raise": the PosDefException of the first failing problem (.info, .index); "nan": NaN in every output of that problem."""
    L, lp, _, _ = _loo_batch(fxs, ys, on_error, bool(pointwise), False)
    return (L, lp) if pointwise else L


def loo_mean_and_var_batch(fxs, ys, *, on_error: str = "raise"):
    """loo_mean_and_var(fx_b, y_b) of many independent exact GPs in one library call per group (gp_loo_batch): (list of μ vectors, list of v vectors) in
    the caller's order.  fxs, ys and on_error as in loo_logpdf_batch."""
    _, _, mu, var = _loo_batch(fxs, ys, on_error, False, True)
    return mu, var


def loo_logpdf_and_grad_batch(fxs, ys, *, wrt_x: bool = False, on_error: str = "raise"):
    """Value and gradient of loo_logpdf(fx_b, y_b) of many independent exact GPs in one library call per group (gp_loo_grad_batch) — restarts or folds
    trained on the leave-one-out objective.  Arguments and result as logpdf_and_grad_batch: (array of L_b, list of the dicts of loo_logpdf_and_grad in the
    caller's order).  With wrt_x every problem of the call runs on the single path inside the library (the batch kernels have no ∂/∂x yet)."""
    return _objective_and_grad_batch(fxs, ys, wrt_x, on_error, _loo_grad_batch_marshal)


def loglikelihood(fx: FiniteGP, Y):  # src/finite_gp_projection.jl:304
    return np.sum(logpdf(fx, Y))


class _Factor:
    """Device-resident Cholesky factor handle (PosteriorGP.data.C)."""

    def __init__(self, ctx: Context, handle: C.c_void_p, n: int, dtype):
        self.ctx, self.handle, self.n, self.dtype = ctx, handle, n, dtype
        self._fin = weakref.finalize(self, ctx.lib.gp_posterior_free, handle)

    @property
    def U(self) -> np.ndarray:
        """C.U on the host (parity/debug; N×N copy)."""
        out = np.empty((self.n, self.n), dtype=self.dtype, order="F")
        check(self.ctx.lib.gp_posterior_get_factor(self.handle, out.ctypes.data))
        return out

    def solve(self, B) -> np.ndarray:
        """`C \\ B` by forward + backward sweeps over the resident factor (gp_posterior_solve) — on the block-cyclic pieces when the
        factor comes from a multi-device fit."""
        B = np.asarray(B, dtype=self.dtype)
        D = np.asfortranarray(B.reshape(self.n, -1))
        out = np.empty_like(D, order="F")
        check(self.ctx.lib.gp_posterior_solve(self.handle, D.ctypes.data, D.shape[1], out.ctypes.data))
        return np.ascontiguousarray(out).reshape(B.shape)

    def Ut_mul(self, xi) -> np.ndarray:
        """`C.U' * xi` (gp_posterior_factor_mul: the sampling transform of rand) — on the pieces for a multi-device factor."""
        xi = np.asarray(xi, dtype=self.dtype)
        D = np.asfortranarray(xi.reshape(self.n, -1))
        out = np.empty_like(D, order="F")
        check(self.ctx.lib.gp_posterior_factor_mul(self.handle, D.ctypes.data, D.shape[1], out.ctypes.data))
        return np.ascontiguousarray(out).reshape(xi.shape)

    def free(self):
        self._fin()


@dataclass
class _PostData:
    alpha: np.ndarray  # α
    C: _Factor
    x: object
    delta: np.ndarray  # δ


def _predict_grad(fn, handle, dt, mean_fn, x, what: int, mean_grad=None) -> tuple:
    """gp_posterior_predict_grad / gp_vfe_predict_grad: (mean, var, dmean, dvar) of the sides in `what` (bit 0 mean, bit 1 variance; the others None),
    values and gradients from one call.  The gradients have the shape of x's array: (n,) for a vector, the ColVecs / RowVecs array shape otherwise.
    The device treats the prior mean as constant in x — exact for ZeroMean / ConstMean; a CustomMean needs `mean_grad`, a callable x -> the (ns × d)
    derivative of the mean function, which is added to dmean (TypeError without it: never a silently incomplete gradient)."""
    custom = callable(mean_fn) and (what & 1)
    if custom and mean_grad is None:
        raise TypeError("the prior mean is a CustomMean: pass mean_grad=callable returning its (ns × d) derivative at x")
    m = _Marshal(dt)
    px = m.points(x)
    pm = _mean_vector(mean_fn, x, dt)
    pm = None if pm is None else m.arr(pm)
    mean = np.empty(px.n, dtype=dt) if what & 1 else None
    var = np.empty(px.n, dtype=dt) if what & 2 else None
    dmean = _dx_buffer(px, dt) if what & 1 else None
    dvar = _dx_buffer(px, dt) if what & 2 else None
    check(fn(handle, C.byref(px), m.ptr(pm), what, m.ptr(mean), m.ptr(var), m.ptr(dmean), m.ptr(dvar)))
    dmean = None if dmean is None else _dx_shaped(dmean, px, x)
    dvar = None if dvar is None else _dx_shaped(dvar, px, x)
    if custom:
        g = np.asarray(mean_grad(x), dtype=dt).reshape(px.n, px.d)  # (ns × d)
        dmean = dmean + (g[:, 0] if px.layout == 0 else (g.T if isinstance(_as_input(x), ColVecs) else g))
    return mean, var, dmean, dvar


class PosteriorGP(AbstractGP):
    """src/exact_gpr_posterior.jl:1-4, with data = (α, C, x, δ) (:34); C lives on the device."""

    def __init__(self, prior: GP, data: _PostData, logpdf_value):
        self.prior, self.data, self.logpdf_value = prior, data, logpdf_value

    def _predict(self, x, what):
        ctx = self.data.C.ctx
        dt = self.data.C.dtype
        m = _Marshal(dt)
        px = m.points(x)
        ns = px.n
        pm = _mean_vector(self.prior.mean_fn, x, dt)
        pm = None if pm is None else m.arr(pm)
        mean = np.empty(ns, dtype=dt) if what & 1 else None
        var = np.empty(ns, dtype=dt) if what & 2 else None
        cov = np.empty((ns, ns), dtype=dt, order="F") if what & 4 else None
        check(ctx.lib.gp_posterior_predict(self.data.C.handle, C.byref(px), m.ptr(pm), what, m.ptr(mean), m.ptr(var),
                                           m.ptr(cov)))
        return mean, var, cov

    def mean(self, x=None):  # :60-62
        if x is None:
            return super().mean()
        return self._predict(x, 1)[0]

    def var(self, x):  # :68-70
        return self._predict(x, 2)[1]

    def cov(self, x, z=None):  # :64-66, :72-76
        if z is None:
            return self._predict(x, 4)[2]
        # cov(f, x, z) = block of the joint covariance over [x; z]
        xa, za = _stack_inputs(x, z)
        nx = _npoints(x)
        return np.asfortranarray(self._predict(xa, 4)[2][:nx, nx:]) if za else None

    def mean_and_var(self, x):  # :85-90
        m, v, _ = self._predict(x, 3)
        return m, v

    def mean_and_cov(self, x):  # :78-83
        m, _, c = self._predict(x, 5)
        return m, c

    def mean_and_var_grad(self, x, mean_grad=None):
        """(mean, var, ∂mean/∂x, ∂var/∂x) at x in one device call (_predict_grad): what AD through mean_and_var(f_post, x) yields in the reference."""
        return _predict_grad(self.data.C.ctx.lib.gp_posterior_predict_grad, self.data.C.handle, self.data.C.dtype, self.prior.mean_fn, x, 3, mean_grad)

    def mean_grad(self, x, mean_grad=None):
        """(mean, ∂mean/∂x): the α-weighted kernel only, no solve."""
        r = _predict_grad(self.data.C.ctx.lib.gp_posterior_predict_grad, self.data.C.handle, self.data.C.dtype, self.prior.mean_fn, x, 1, mean_grad)
        return r[0], r[2]

    def var_grad(self, x):
        """(var, ∂var/∂x)."""
        r = _predict_grad(self.data.C.ctx.lib.gp_posterior_predict_grad, self.data.C.handle, self.data.C.dtype, self.prior.mean_fn, x, 2)
        return r[1], r[3]


def _stack_inputs(x, z):
    x, z = _as_input(x), _as_input(z)
    if isinstance(x, ColVecs):
        return ColVecs(np.concatenate([x.X, (z.X if isinstance(z, ColVecs) else z.X.T)], axis=1)), True
    if isinstance(x, RowVecs):
        return RowVecs(np.concatenate([x.X, (z.X if isinstance(z, RowVecs) else z.X.T)], axis=0)), True
    return np.concatenate([x, z]), True


def _posterior_exact(fx: FiniteGP, y, zero_mean: bool = False) -> PosteriorGP:
    """posterior(fx::FiniteGP, y) — src/exact_gpr_posterior.jl:29-35.  One device call: Gram, Cholesky,
    α and logpdf(fx, y) (kept as .logpdf_value) from a single factorisation."""
    y = _check_y(fx, y)
    if y.ndim != 1:
        raise TypeError("posterior expects a vector of observations")
    f = fx.f
    if isinstance(f, PosteriorGP):
        return _posterior_sequential(fx, y)
    if not isinstance(f, GP):
        raise TypeError("posterior: unsupported GP type")
    ctx = f.context()
    dt = np.result_type(_input_dtype(fx.x), np.float32 if y.dtype == np.float32 else np.float64).type
    m = _Marshal(dt)
    px = m.points(fx.x)
    sfx, kk = m.any_kernel(f.kernel, px.d)
    nz = m.noise(fx.sigma2, px.n)
    mean = None if zero_mean else _mean_vector(f.mean_fn, fx.x, dt)
    yv = m.arr(y)
    delta = yv - mean if mean is not None else yv.copy()  # δ = y - m  (:32)
    mean = None if mean is None else m.arr(mean)
    alpha = np.empty(px.n, dtype=dt)
    lp = np.empty(1, dtype=dt)
    h = C.c_void_p()
    check(getattr(ctx.lib, "gp_posterior_fit" + sfx)(ctx.handle, C.byref(kk), C.byref(px), C.byref(nz), m.ptr(mean), yv.ctypes.data,
                                                     C.byref(h), alpha.ctypes.data, lp.ctypes.data))
    return PosteriorGP(f, _PostData(alpha, _Factor(ctx, h, px.n, dt), fx.x, delta), lp[0])


# --------------------------------------------------------------------------------------------
# one factorisation for a matrix of observations: gp_posterior_fit_cols / gp_posterior_predict_cols / gp_logpdf_grad_cols
# --------------------------------------------------------------------------------------------
@dataclass(eq=False)
class _ColsCall:
    """The arguments of a *_cols call, built without a context (tests/test_cols_cpu.py reads them)."""
    dt: type
    m: _Marshal
    px: gp_points
    sfx: str            # "" or "_sum"
    kk: object          # gp_kernel or gp_ksum
    nf: object          # _NormalForm of a composite kernel, else None
    nz: gp_noise
    mean: Optional[np.ndarray]  # the ONE prior-mean vector every column shares
    Y: np.ndarray       # (n, S), column-major
    ldy: int
    ncols: int


def _cols_marshal(fx: FiniteGP, Y, name: str) -> _ColsCall:
    Y = _check_y(fx, Y)
    if Y.ndim != 2:
        raise TypeError(f"{name} expects an (n, S) matrix of observations, one GP per column; a vector goes to its single-column counterpart")
    f = fx.f
    if not isinstance(f, GP):
        raise TypeError(f"{name}: the prior must be a GP (sequential conditioning of column posteriors is not offered)")
    if not 1 <= Y.shape[1] <= _lib.cols_max():
        raise ValueError(f"{name}: {Y.shape[1]} columns, 1..{_lib.cols_max()} (GPMI355_COLS_MAX) fit one call: split them into groups")
    dt = np.result_type(_input_dtype(fx.x), np.float32 if Y.dtype == np.float32 else np.float64).type
    m = _Marshal(dt)
    px = m.points(fx.x)
    nf = None
    if _is_composite(f.kernel):
        sfx = "_sum"
        kk, nf = m.ksum(f.kernel, px.d)
    else:
        sfx, kk = "", m.kernel(f.kernel, px.d)
    nz = m.noise(fx.sigma2, px.n)
    mean = _mean_vector(f.mean_fn, fx.x, dt)
    mean = None if mean is None else m.arr(mean)
    # a column-major array of the right dtype goes as it lies — the leading rows of a taller column-major array included (ldy = its column stride)
    it = Y.itemsize
    if Y.dtype == dt and Y.strides[0] == it and Y.strides[1] % it == 0 and Y.strides[1] // it >= max(Y.shape[0], 1) and Y.shape[1] > 1:
        Yf, ldy = Y, Y.strides[1] // it
    else:
        Yf = m.arr(Y, order="F")
        ldy = Yf.shape[0]
    m.keep.append(Yf)
    return _ColsCall(dt, m, px, sfx, kk, nf, nz, mean, Yf, ldy, Yf.shape[1])


@dataclass
class _ColsData:
    alpha: np.ndarray  # (n, S): α_s = C \ (Y[:, s] − m)
    C: _Factor
    x: object
    delta: np.ndarray  # (n, S)


class ColumnsPosteriorGP(AbstractGP):
    """S posteriors that share x, kernel, Σy and the prior mean and differ in y (the columns of Y): ONE device-resident factor, α for every column.
    mean(x) is (ns, S); var / cov do not depend on y and are those of every column."""

    def __init__(self, prior: GP, data: _ColsData, logpdf_values):
        self.prior, self.data, self.logpdf_values = prior, data, logpdf_values

    @property
    def ncols(self) -> int:
        out = C.c_int32()
        check(self.data.C.ctx.lib.gp_posterior_ncols(self.data.C.handle, C.byref(out)))
        return out.value

    def _predict(self, x, what):
        ctx, dt = self.data.C.ctx, self.data.C.dtype
        m = _Marshal(dt)
        px = m.points(x)
        ns, S = px.n, self.data.alpha.shape[1]
        pm = _mean_vector(self.prior.mean_fn, x, dt)
        pm = None if pm is None else m.arr(pm)
        mean = np.empty((ns, S), dtype=dt, order="F") if what & 1 else None
        var = np.empty(ns, dtype=dt) if what & 2 else None
        cov = np.empty((ns, ns), dtype=dt, order="F") if what & 4 else None
        check(ctx.lib.gp_posterior_predict_cols(self.data.C.handle, C.byref(px), m.ptr(pm), what, m.ptr(mean), m.ptr(var), m.ptr(cov)))
        return mean, var, cov

    def mean(self, x=None):
        if x is None:
            return super().mean()
        return self._predict(x, 1)[0]

    def var(self, x):
        return self._predict(x, 2)[1]

    def cov(self, x, z=None):
        if z is not None:
            raise TypeError("cov(f, x, z) is not offered for a column posterior: take the block of cov(f, [x; z])")
        return self._predict(x, 4)[2]

    def mean_and_var(self, x):
        m, v, _ = self._predict(x, 3)
        return m, v

    def mean_and_cov(self, x):
        m, _, c = self._predict(x, 5)
        return m, c

    def _one_column_only(self, *a, **k):
        raise TypeError("a column posterior holds one mean per column: this method needs a single-column posterior (posterior(fx, Y[:, s]))")

    mean_and_var_grad = mean_grad = _one_column_only

    def var_grad(self, x):
        """(var, ∂var/∂x): the variance side uses no α."""
        r = _predict_grad(self.data.C.ctx.lib.gp_posterior_predict_grad, self.data.C.handle, self.data.C.dtype, self.prior.mean_fn, x, 2)
        return r[1], r[3]

    def __call__(self, x, sigma2=default_sigma2):
        raise TypeError("a FiniteGP over a column posterior (held-out logpdf, samples, sequential conditioning) is not offered: use posterior(fx, Y[:, s])")


def posterior_columns(fx, Y, *rest):
    """posterior_columns(fx, Y): posterior(fx, Y[:, s]) for every column s of the (n, S) matrix Y from ONE Gram assembly and ONE factorisation
    (gp_posterior_fit_cols; S <= 128).  .data.alpha is (n, S), .logpdf_values (S,) = logpdf(fx, Y).
    posterior_columns(VFE(fz)|DTC(fz), fx, Y): the sparse posteriors of every column from ONE streamed pass (gp_vfe_fit_cols) — an
    ApproxColumnsPosteriorGP."""
    if len(rest) == 1:  # (approx, fx, Y): the positional names of the two-argument form shift by one
        return _vfe_posterior_columns(fx, Y, rest[0])
    if rest:
        raise TypeError("posterior_columns(fx, Y) or posterior_columns(approx, fx, Y)")
    a = _cols_marshal(fx, Y, "posterior_columns")
    f = fx.f
    ctx = f.context()
    delta = np.asfortranarray(a.Y - a.mean[:, None] if a.mean is not None else a.Y.copy(order="F"))
    alpha = np.empty((a.px.n, a.ncols), dtype=a.dt, order="F")
    lp = np.empty(a.ncols, dtype=a.dt)
    h = C.c_void_p()
    check(getattr(ctx.lib, "gp_posterior_fit_cols" + a.sfx)(ctx.handle, C.byref(a.kk), C.byref(a.px), C.byref(a.nz), a.m.ptr(a.mean), a.Y.ctypes.data, a.ldy,
                                                            a.ncols, C.byref(h), alpha.ctypes.data, lp.ctypes.data))
    return ColumnsPosteriorGP(f, _ColsData(alpha, _Factor(ctx, h, a.px.n, a.dt), fx.x, delta), lp)


def logpdf_and_grad_columns(fx: FiniteGP, Y, wrt_x: bool = False) -> tuple:
    """(logpdf(fx, Y[:, s]) for every s, gradient of their SUM) from one factorisation and one C⁻¹ (gp_logpdf_grad_cols / _sum; S <= 128).  The keys of
    the gradient are those of logpdf_and_grad; "y" and "mean" are (n, S) — column s is −α_s / +α_s; sum "mean" over the columns for the shared mean vector."""
    a = _cols_marshal(fx, Y, "logpdf_and_grad_columns")
    ctx = fx.f.context()
    n, S, dt, m = a.px.n, a.ncols, a.dt, a.m
    lp = np.empty(S, dtype=dt)
    dnoise = np.empty(_dnoise_shape(a.nz, n), dtype=dt)
    dY = np.empty((n, S), dtype=dt, order="F")
    dxb = _dx_buffer(a.px, dt) if wrt_x else None
    head = (ctx.handle, C.byref(a.kk), C.byref(a.px), C.byref(a.nz), m.ptr(a.mean), a.Y.ctypes.data, a.ldy, S, lp.ctypes.data)
    if a.nf is not None:
        dth = (C.c_double * max(len(a.nf.theta()), 1))()
        check(ctx.lib.gp_logpdf_grad_cols_sum(*head, dth, dnoise.ctypes.data, dY.ctypes.data, m.ptr(dxb)))
        gth = np.array(dth[:len(a.nf.theta())])
        g = {"kernel": a.nf.chain(gth), "theta": gth}
    else:
        dvar = C.c_double()
        dscale = (C.c_double * max(a.kk.nscale, 1))()
        check(ctx.lib.gp_logpdf_grad_cols(*head, C.byref(dvar), dscale, dnoise.ctypes.data, dY.ctypes.data, m.ptr(dxb)))
        sc = None if a.kk.nscale == 0 else (float(dscale[0]) if a.kk.nscale == 1 else np.array(dscale[:a.kk.nscale]))
        g = {"variance": dvar.value, "scale": sc}
    g.update({"noise": dnoise[0] if a.nz.kind == 0 else dnoise, "y": dY, "mean": -dY})
    if wrt_x:
        g["x"] = _dx_shaped(dxb, a.px, fx.x)
    return lp, g


def _posterior_sequential(fx: FiniteGP, y) -> PosteriorGP:
    """posterior(fx::FiniteGP{<:PosteriorGP}, y) — src/exact_gpr_posterior.jl:46-56: the device-resident factor is
    extended by update_chol (src/util/common_covmat_ops.jl:38-42) instead of being recomputed."""
    post = fx.f
    prior = post.prior
    fac = post.data.C
    dt = fac.dtype
    m = _Marshal(dt)
    px = m.points(fx.x)
    nz = m.noise(fx.sigma2, px.n)
    m2 = _mean_vector(prior.mean_fn, fx.x, dt)
    d2 = m.arr(y) - m2 if m2 is not None else m.arr(y).copy()          # δ2 = y - m2           (:48-49)
    delta = m.arr(np.concatenate([post.data.delta, d2]))                # δ = vcat(δ_old, δ2)  (:52)
    n = delta.shape[0]
    alpha = np.empty(n, dtype=dt)
    lp = np.empty(1, dtype=dt)
    h = C.c_void_p()
    check(fac.ctx.lib.gp_posterior_update(fac.handle, C.byref(px), C.byref(nz), delta.ctypes.data, C.byref(h),
                                          alpha.ctypes.data, lp.ctypes.data))
    x_all, _ = _stack_inputs(post.data.x, fx.x)                         # x = vcat(x_old, x2)  (:54)
    return PosteriorGP(prior, _PostData(alpha, _Factor(fac.ctx, h, n, dt), x_all, delta), lp[0])


def _joint_call(fx: FiniteGP, name: str, payload: np.ndarray):
    """Shared marshalling of gp_{posterior,vfe}_{logpdf,rand}: payload is ns × ncols (y* columns or standard normals)."""
    f = fx.f
    if isinstance(f, PosteriorGP):
        ctx, h, dt, prior, fn = f.data.C.ctx, f.data.C.handle, f.data.C.dtype, f.prior, "gp_posterior_" + name
    elif isinstance(f, ApproxPosteriorGP):
        ctx, h, dt, prior, fn = f._state.ctx, f._state.handle, f._dtype, f.prior, "gp_vfe_" + name
    else:
        raise TypeError(f"{name}: unsupported GP type")
    m = _Marshal(dt)
    px = m.points(fx.x)
    nz = m.noise(fx.sigma2, px.n)
    pm = _mean_vector(prior.mean_fn, fx.x, dt)
    pm = None if pm is None else m.arr(pm)
    P = m.arr(payload, order="F")
    ncols = P.shape[1]
    if name == "logpdf":
        out = np.empty(ncols, dtype=dt)
        check(getattr(ctx.lib, fn)(h, C.byref(px), m.ptr(pm), C.byref(nz), P.ctypes.data, P.shape[0], ncols, out.ctypes.data))
    else:
        out = np.empty((px.n, ncols), dtype=dt, order="F")
        check(getattr(ctx.lib, fn)(h, C.byref(px), m.ptr(pm), C.byref(nz), P.ctypes.data, ncols, out.ctypes.data))
    return out


def rand(fx: FiniteGP, N: Optional[int] = None, rng=None, xi=None):
    """rand([rng,] fx[, N]) — src/finite_gp_projection.jl:233-240: m .+ C.U' * randn(rng, n, N).  Factor and triangular
    product run on the device for priors AND posteriors (exact / VFE: the N*×N* predictive covariance is built and
    factored in HBM against the resident factor — nothing is refitted); the standard normals are drawn on the host
    (`rng`: numpy Generator) or passed in as `xi` (n × N) for reproducible parity checks."""
    f = fx.f
    n = len(fx)
    ncols = 1 if N is None else int(N)
    if isinstance(f, GP):
        fac = fx._prior_factor()
        dt = fac.dtype
    elif isinstance(f, (PosteriorGP, ApproxPosteriorGP)):
        dt = f.data.C.dtype if isinstance(f, PosteriorGP) else f._dtype
    else:
        raise TypeError("rand: unsupported GP type")
    if xi is None:
        xi = (rng or np.random.default_rng()).standard_normal((n, ncols))
    xi = np.asfortranarray(np.asarray(xi, dtype=dt).reshape(n, ncols))
    if isinstance(f, GP):
        out = np.empty((n, ncols), dtype=dt, order="F")
        check(fac.ctx.lib.gp_posterior_factor_mul(fac.handle, xi.ctypes.data, ncols, out.ctypes.data))
        out += np.asarray(f.mean(fx.x), dtype=dt)[:, None]
    else:
        out = _joint_call(fx, "rand", xi)
    return out[:, 0] if N is None else out


def rand_(fx: FiniteGP, out: np.ndarray, rng=None, xi=None) -> np.ndarray:
    """rand!(rng, fx, y) — src/finite_gp_projection.jl:271-277 (via _rand!): fills the vector (n) or matrix (n × N) `out`
    in place and returns it."""
    out_arr = np.asarray(out)
    if out_arr.shape[0] != len(fx):
        raise ValueError(f"DimensionMismatch: length(fx) = {len(fx)} but the output has {out_arr.shape[0]} rows")
    res = rand(fx, None if out_arr.ndim == 1 else out_arr.shape[1], rng=rng, xi=xi)
    out[...] = res
    return out


def _logpdf_posterior(fx: FiniteGP, y):
    """logpdf(post(x*, Σy*), y*) — the generic FiniteGP path of the reference (src/finite_gp_projection.jl:306-311 over the
    posterior's mean_and_cov, src/exact_gpr_posterior.jl:78-83 / src/sparse_approximations.jl:205-210) as ONE device call."""
    out = _joint_call(fx, "logpdf", y if y.ndim == 2 else y[:, None])
    return out[0] if y.ndim == 1 else out


# Distribution-style accessors on FiniteGP (src/finite_gp_projection.jl:53,96,114,133,154,203)
def mean(fx_or_f, x=None):
    if isinstance(fx_or_f, FiniteGP):
        return fx_or_f.f.mean(fx_or_f.x)
    return fx_or_f.mean(x)


def var(fx_or_f, x=None):
    if isinstance(fx_or_f, FiniteGP):
        return fx_or_f.f.var(fx_or_f.x) + fx_or_f.noise_vector()
    return fx_or_f.var(x)


def cov(fx_or_f, x=None, z=None):
    if isinstance(fx_or_f, FiniteGP):
        fx = fx_or_f
        if isinstance(x, FiniteGP):  # cov(fx, gx)  :177-180
            assert fx.f is x.f
            return fx.f.cov(fx.x, x.x)
        Cm = np.array(fx.f.cov(fx.x))
        S = fx.noise_matrix_or_none()
        if S is not None:  # cov(f, x) + Σy with a dense Σy  :96, :135
            return Cm + S.astype(Cm.dtype, copy=False)
        Cm[np.diag_indices_from(Cm)] += fx.noise_vector()
        return Cm
    return fx_or_f.cov(x, z)


def mean_and_var(fx_or_f, x=None):
    if isinstance(fx_or_f, FiniteGP):
        m, v = fx_or_f.f.mean_and_var(fx_or_f.x)
        return m, v + fx_or_f.noise_vector()
    return fx_or_f.mean_and_var(x)


def mean_and_cov(fx_or_f, x=None):
    if isinstance(fx_or_f, FiniteGP):
        return mean(fx_or_f), cov(fx_or_f)
    return fx_or_f.mean_and_cov(x)


def marginals(fx: FiniteGP):
    """marginals(fx) = Normal.(m, sqrt.(c)) -> (mean, std) arrays (src/finite_gp_projection.jl:203-206)."""
    m, c = mean_and_var(fx)
    return m, np.sqrt(c)


# --------------------------------------------------------------------------------------------
# Sparse approximations: VFE / DTC (src/sparse_approximations.jl)
# --------------------------------------------------------------------------------------------
@dataclass(eq=False)
class VFE:
    """VFE(fz::FiniteGP) — src/sparse_approximations.jl:12-14."""

    fz: FiniteGP


@dataclass(eq=False)
class DTC:
    """DTC(fz::FiniteGP) — src/sparse_approximations.jl:21-23."""

    fz: FiniteGP


class ExactInference:  # src/exact_gpr_posterior.jl:6-12
    pass


class _VfeState:
    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle
        self._fin = weakref.finalize(self, ctx.lib.gp_vfe_free, handle)


def _refuse_dense_vfe(fx: FiniteGP):
    if np.ndim(fx.sigma2) == 2:
        raise NotImplementedError("VFE / DTC with a dense Σy are not accelerated: the reference factors Σy there (an N×N Cholesky that defeats the sparse cost, "
                                  "src/sparse_approximations.jl:61, :97) and its elbo has no method for a dense Σy (:307-313); the exact path takes a dense Σy")


def _vfe_call(approx, fx: FiniteGP, y, want_post: bool):
    y = _check_y(fx, y)
    if y.ndim != 1:
        raise TypeError("expected a vector of observations")
    f = fx.f
    if approx.fz.f is not f:  # @assert vfe.fz.f === fx.f  (:59, :249, :283)
        raise AssertionError("vfe.fz.f === fx.f")
    if not isinstance(f, GP):
        raise TypeError("VFE/DTC: unsupported prior type")
    if _is_composite(f.kernel):
        raise NotImplementedError("VFE / DTC with a composite kernel are not accelerated (the Julia shim falls back to stock AbstractGPs; "
                                  "the exact path takes composite kernels)")
    _refuse_dense_vfe(fx)
    ctx = f.context()
    dt = np.result_type(_input_dtype(fx.x), np.float32 if y.dtype == np.float32 else np.float64).type
    m = _Marshal(dt)
    px, pz = m.points(fx.x), m.points(approx.fz.x)
    kk = m.kernel(f.kernel, px.d)
    nz = m.noise(fx.sigma2, px.n)
    jit = np.asarray(approx.fz.sigma2)
    if jit.ndim != 0:
        raise NotImplementedError("inducing-point noise must be a scalar jitter")
    mean = _mean_vector(f.mean_fn, fx.x, dt)
    mean = None if mean is None else m.arr(mean)
    yv = m.arr(y)
    obj = np.empty(1, dtype=dt)
    h = C.c_void_p()
    check(ctx.lib.gp_vfe_fit(ctx.handle, C.byref(kk), C.byref(px), C.byref(pz), C.byref(nz), float(jit), m.ptr(mean),
                             yv.ctypes.data, 0 if isinstance(approx, VFE) else 1,
                             C.byref(h) if want_post else None, obj.ctypes.data))
    return (h if want_post else None), obj[0], ctx, dt, pz.n


class _VfeData(Mapping):
    """Lazy read-only Mapping over an ApproxPosteriorGP's device-resident cache (field names of src/sparse_approximations.jl:73, ASCII):
    iteration, len, keys / items / values / get behave like the plain dict this property once returned; every read of a field fetches it
    from the device (nothing is cached on the host)."""

    _FIELDS = ("alpha", "m_eps", "U", "Lam_U", "b_y")

    def __init__(self, post):
        self._post = post

    def __iter__(self):
        return iter(self._FIELDS)

    def __len__(self):
        return len(self._FIELDS)

    def __contains__(self, k):
        return k in self._FIELDS

    def __getattr__(self, k):
        if k.startswith("_") or k not in self._FIELDS:
            raise AttributeError(k)
        return self[k]

    def __getitem__(self, k):
        p = self._post
        st, dt, m = p._state, p._dtype, p._m
        lib = st.ctx.lib
        if k in ("alpha", "m_eps"):
            a = np.empty(m, dtype=dt)
            check(lib.gp_vfe_get(st.handle, a.ctypes.data if k == "alpha" else None, a.ctypes.data if k == "m_eps" else None))
            return a
        if k in ("U", "Lam_U"):
            out = np.empty((m, m), dtype=dt, order="F")
            check(lib.gp_vfe_get_factors(st.handle, out.ctypes.data if k == "U" else None, out.ctypes.data if k == "Lam_U" else None))
            return out
        if k == "b_y":
            n = int(lib.gp_vfe_n(st.handle))
            out = np.empty(max(n, 0), dtype=dt)
            check(lib.gp_vfe_get_by(st.handle, out.ctypes.data))
            return out
        raise KeyError(k)


class ApproxPosteriorGP(AbstractGP):
    """src/sparse_approximations.jl:25-29; the cache (:73) lives on the device."""

    def __init__(self, approx, prior: GP, state: _VfeState, dtype, m: int, objective):
        self.approx, self.prior, self._state, self._dtype, self._m = approx, prior, state, dtype, m
        self.objective = objective

    @property
    def data(self):
        """The cache of src/sparse_approximations.jl:73 — (m_ε, Λ_ε, U, α, b_y, …) — read from the device on demand: `alpha`, `m_eps`
        (M-vectors), `U` = cholesky(cov(fz)).U and `Lam_U` = Λ_ε.U (M×M upper, column-major), `b_y` (N-vector).  Mapping access
        (`data["alpha"]`) and attribute access (`data.alpha`) both work; B_εf is never materialised (it is N×M)."""
        return _VfeData(self)

    def _predict(self, x, what):
        st = self._state
        mm = _Marshal(self._dtype)
        px = mm.points(x)
        pm = _mean_vector(self.prior.mean_fn, x, self._dtype)
        pm = None if pm is None else mm.arr(pm)
        mean = np.empty(px.n, dtype=self._dtype) if what & 1 else None
        var = np.empty(px.n, dtype=self._dtype) if what & 2 else None
        cov = np.empty((px.n, px.n), dtype=self._dtype, order="F") if what & 4 else None
        check(st.ctx.lib.gp_vfe_predict(st.handle, C.byref(px), mm.ptr(pm), what, mm.ptr(mean), mm.ptr(var), mm.ptr(cov)))
        return mean, var, cov

    def mean(self, x=None):  # :183-185
        if x is None:
            return super().mean()
        return self._predict(x, 1)[0]

    def var(self, x):  # :192-195
        return self._predict(x, 2)[1]

    def cov(self, x, z=None):  # :187-190, :197-203
        if z is None:
            return self._predict(x, 4)[2]
        xa, _ = _stack_inputs(x, z)  # cov(f, x, z) = off-diagonal block of the joint covariance over [x; z]
        nx = _npoints(x)
        return np.asfortranarray(self._predict(xa, 4)[2][:nx, nx:])

    def mean_and_var(self, x):  # :212-217
        return self._predict(x, 3)[:2]

    def mean_and_cov(self, x):  # :205-210
        m, _, c = self._predict(x, 5)
        return m, c

    def mean_and_var_grad(self, x, mean_grad=None):
        """(mean, var, ∂mean/∂x, ∂var/∂x) at x in one device call (_predict_grad)."""
        st = self._state
        return _predict_grad(st.ctx.lib.gp_vfe_predict_grad, st.handle, self._dtype, self.prior.mean_fn, x, 3, mean_grad)

    def mean_grad(self, x, mean_grad=None):
        st = self._state
        r = _predict_grad(st.ctx.lib.gp_vfe_predict_grad, st.handle, self._dtype, self.prior.mean_fn, x, 1, mean_grad)
        return r[0], r[2]

    def var_grad(self, x):
        st = self._state
        r = _predict_grad(st.ctx.lib.gp_vfe_predict_grad, st.handle, self._dtype, self.prior.mean_fn, x, 2)
        return r[1], r[3]


    def objective_grad(self, wrt_x: bool = False) -> dict:
        """Gradient of the objective this posterior was fitted with (`self.objective`: elbo for VFE, approx_log_evidence for DTC —
        src/sparse_approximations.jl:248-254, :282-286) at its own parameters, from the state resident on the device (gp_vfe_grad): what an AD backend
        computes for examples/0-intro-1d/script.jl:385-394.  Keys as `logpdf_and_grad`: "variance", "scale" (None / float / vector), "noise" (the sum
        Σ_i ∂/∂Σy_ii — the gradient for a scalar σ²) and "noise_diag" (the vector), "y", "mean" (= −"y"), "z" in the shape of the pseudo-input
        container's array (fp64 posteriors only), and with wrt_x "x" in the shape of the observations' container (all observations seen so far, arrival order, as a
        RowVecs-shaped (N, D) array when the posterior has been updated)."""
        st = self._state
        dt = self._dtype
        n = int(st.ctx.lib.gp_vfe_n(st.handle))
        zin = _as_input(self.approx.fz.x)
        mm = _Marshal(dt)
        pz = mm.points(self.approx.fz.x)
        nscale = mm.kernel(self.prior.kernel, pz.d).nscale
        dvar, dns = C.c_double(), C.c_double()
        dscale = (C.c_double * max(nscale, 1))()
        dnoise = np.empty(n, dtype=dt)
        dy = np.empty(n, dtype=dt)
        dz = None   # fp64 posteriors only: an fp32 fit's streamed B Bᵀ does not carry ∂/∂z (the C ABI refuses it, include/gpmi355.h)
        if np.dtype(dt) == np.float64:
            dz = np.empty((pz.n,) if pz.layout == 0 else ((pz.n, pz.d) if pz.layout == 1 else (pz.d, pz.n)), dtype=np.float64)
        dxb = np.empty((n, pz.d), dtype=dt) if wrt_x else None          # layout 1: point-contiguous (N, D)
        check(st.ctx.lib.gp_vfe_grad(st.handle, C.byref(dvar), dscale, C.byref(dns), dnoise.ctypes.data, dy.ctypes.data, None if dz is None else dz.ctypes.data, pz.layout,
                                     None if dxb is None else dxb.ctypes.data, 1))
        sc = None if nscale == 0 else (float(dscale[0]) if nscale == 1 else np.array([dscale[i] for i in range(nscale)]))
        g = {"variance": dvar.value, "scale": sc, "noise": dns.value, "noise_diag": dnoise, "y": dy, "mean": -dy}
        if dz is not None:
            if pz.layout == 0:
                g["z"] = dz
            else:
                nd = dz if pz.layout == 1 else dz.T
                g["z"] = np.ascontiguousarray(nd.T if isinstance(zin, ColVecs) else nd)
        if wrt_x:
            g["x"] = dxb[:, 0] if pz.d == 1 and pz.layout == 0 else dxb
        return g


def elbo_and_grad(a, fx: FiniteGP, y, wrt_x: bool = False) -> tuple:
    """(approx_log_evidence(a, fx, y), its gradient) in one fit + one backward pass on the device — the value / pullback pair an rrule of
    `elbo(VFE(f(z, jitter)), f(x, Σy), y)` needs (the reference differentiates the same expression by AD: examples/0-intro-1d/script.jl:385-394).
    "x" comes back in the shape of fx.x's array."""
    if not isinstance(a, (VFE, DTC)):
        raise TypeError("elbo_and_grad: VFE or DTC")
    post = posterior(a, fx, y)
    g = post.objective_grad(wrt_x)
    if wrt_x and "x" in g and np.ndim(g["x"]) == 2 and isinstance(_as_input(fx.x), ColVecs):
        g["x"] = np.ascontiguousarray(g["x"].T)
    return post.objective, g


def inducing_points(f: ApproxPosteriorGP):  # :219
    return f.approx.fz.x


def update_posterior(f_post_approx: ApproxPosteriorGP, fx: FiniteGP, y=None):
    """update_posterior(f_post_approx, fx, y)  — new observations, same pseudo-points (src/sparse_approximations.jl:87-121):
    the device continues its streamed reductions with the new points and re-finalises the M×M side.
    update_posterior(f_post_approx, fz)      — append pseudo-points (:131-176): bordered Cholesky of K_zz on the resident
    factor (update_chol), then the observations retained on the device are streamed once more for the NEW block rows of
    B Bᵀ / B b_y only (gp_vfe_append)."""
    if f_post_approx.prior is not fx.f:
        raise AssertionError("f_post_approx.prior === fx.f")
    if isinstance(f_post_approx, ApproxColumnsPosteriorGP):
        return _vfe_cols_update(f_post_approx, fx, y)
    st = f_post_approx._state
    dt = f_post_approx._dtype
    mm = _Marshal(dt)
    obj = np.empty(1, dtype=dt)
    h = C.c_void_p()
    if y is None:  # new pseudo-points: fx is fz
        pz = mm.points(fx.x)
        check(st.ctx.lib.gp_vfe_append(st.handle, C.byref(pz), C.byref(h), obj.ctypes.data))
        z_all, _ = _stack_inputs(f_post_approx.approx.fz.x, fx.x)                                     # z_new = vcat(z_old, z)  (:160)
        approx = type(f_post_approx.approx)(f_post_approx.prior(z_all, f_post_approx.approx.fz.sigma2))  # _update_approx (:178-179)
        return ApproxPosteriorGP(approx, f_post_approx.prior, _VfeState(st.ctx, h), dt, f_post_approx._m + pz.n, obj[0])
    y = _check_y(fx, y)
    _refuse_dense_vfe(fx)
    px = mm.points(fx.x)
    nz = mm.noise(fx.sigma2, px.n)
    mean = _mean_vector(f_post_approx.prior.mean_fn, fx.x, dt)
    mean = None if mean is None else mm.arr(mean)
    yv = mm.arr(y)
    check(st.ctx.lib.gp_vfe_update(st.handle, C.byref(px), C.byref(nz), mm.ptr(mean), yv.ctypes.data, C.byref(h), obj.ctypes.data))
    return ApproxPosteriorGP(f_post_approx.approx, f_post_approx.prior, _VfeState(st.ctx, h), dt, f_post_approx._m, obj[0])


def posterior(*args):
    """posterior(fx, y)                      — src/exact_gpr_posterior.jl:29-35
    posterior(VFE(fz)|DTC(fz), fx, y)     — src/sparse_approximations.jl:58-75
    posterior(ExactInference(), fx, y)    — src/exact_gpr_posterior.jl:8"""
    if len(args) == 2:
        return _posterior_exact(*args)
    if len(args) == 3:
        a, fx, y = args
        if isinstance(a, ExactInference):
            return _posterior_exact(fx, y)
        if isinstance(a, (VFE, DTC)):
            h, obj, ctx, dt, m = _vfe_call(a, fx, y, True)
            return ApproxPosteriorGP(a, fx.f, _VfeState(ctx, h), dt, m, obj)
    raise TypeError("posterior(fx, y) or posterior(approx, fx, y)")


def approx_log_evidence(a, fx: FiniteGP, y):
    """src/sparse_approximations.jl:248-252 (VFE), :282-286 (DTC); src/exact_gpr_posterior.jl:10-12."""
    if isinstance(a, ExactInference):
        return logpdf(fx, y)
    if not isinstance(a, (VFE, DTC)):
        raise TypeError("approx_log_evidence: unsupported approximation")
    return _vfe_call(a, fx, y, False)[1]


def elbo(a, fx: FiniteGP, y):
    """elbo(vfe, fx, y) = approx_log_evidence(vfe, fx, y) (:254); elbo(::DTC) is deprecated upstream."""
    if not isinstance(a, VFE):
        raise TypeError("elbo is defined for VFE")
    return approx_log_evidence(a, fx, y)


# --------------------------------------------------------------------------------------------
# VFE / DTC for a matrix of observations: gp_vfe_fit_cols / _update_cols / _append_cols / _predict_cols / _get_cols / _get_by_cols / _grad_cols
# --------------------------------------------------------------------------------------------
@dataclass(eq=False)
class _VfeColsCall:
    """The arguments of a gp_vfe_fit_cols call, built without a context (tests/test_vfe_cols_cpu.py reads them)."""
    dt: type
    m: _Marshal
    px: gp_points
    pz: gp_points
    kk: gp_kernel
    nz: gp_noise
    jitter: float
    mean: Optional[np.ndarray]  # the ONE prior-mean vector every column shares
    Y: np.ndarray               # (n, S), column-major
    ldy: int
    ncols: int
    approx: int


def _cols_matrix(fx: FiniteGP, Y, name: str, ncols: Optional[int] = None) -> np.ndarray:
    Y = np.asarray(Y)
    if Y.ndim != 2:
        raise TypeError(f"{name} expects an (n, S) matrix of observations, one sparse GP per column; a vector goes to its single-column counterpart")
    if Y.shape[0] != len(fx):
        raise ValueError(f"DimensionMismatch: length(fx) = {len(fx)} but Y has {Y.shape[0]} rows")
    if not 1 <= Y.shape[1] <= _lib.cols_max():
        raise ValueError(f"{name}: {Y.shape[1]} columns, 1..{_lib.cols_max()} (GPMI355_COLS_MAX) fit one call: split them into groups")
    if ncols is not None and Y.shape[1] != ncols:
        raise ValueError(f"{name}: Y has {Y.shape[1]} columns but the posterior holds {ncols}")
    return Y


def _vfe_cols_marshal(approx, fx: FiniteGP, Y, name: str) -> _VfeColsCall:
    if not isinstance(approx, (VFE, DTC)):
        raise TypeError(f"{name}: VFE or DTC")
    Y = _cols_matrix(fx, Y, name)
    f = fx.f
    if approx.fz.f is not f:
        raise AssertionError("vfe.fz.f === fx.f")
    if not isinstance(f, GP):
        raise TypeError("VFE/DTC: unsupported prior type")
    if _is_composite(f.kernel):
        raise NotImplementedError("VFE / DTC with a composite kernel are not accelerated (the exact path takes composite kernels)")
    _refuse_dense_vfe(fx)
    jit = np.asarray(approx.fz.sigma2)
    if jit.ndim != 0:
        raise NotImplementedError("inducing-point noise must be a scalar jitter")
    dt = np.result_type(_input_dtype(fx.x), np.float32 if Y.dtype == np.float32 else np.float64).type
    m = _Marshal(dt)
    px, pz = m.points(fx.x), m.points(approx.fz.x)
    kk = m.kernel(f.kernel, px.d)
    nz = m.noise(fx.sigma2, px.n)
    mean = _mean_vector(f.mean_fn, fx.x, dt)
    mean = None if mean is None else m.arr(mean)
    Yf = m.arr(Y, order="F")
    return _VfeColsCall(dt, m, px, pz, kk, nz, float(jit), mean, Yf, max(Yf.shape[0], 1), Yf.shape[1], 0 if isinstance(approx, VFE) else 1)


def _vfe_cols_call(approx, fx: FiniteGP, Y, want_post: bool, name: str):
    a = _vfe_cols_marshal(approx, fx, Y, name)
    ctx = fx.f.context()
    obj = np.empty(a.ncols, dtype=a.dt)
    h = C.c_void_p()
    check(ctx.lib.gp_vfe_fit_cols(ctx.handle, C.byref(a.kk), C.byref(a.px), C.byref(a.pz), C.byref(a.nz), a.jitter, a.m.ptr(a.mean), a.Y.ctypes.data, a.ldy,
                                  a.ncols, a.approx, C.byref(h) if want_post else None, obj.ctypes.data))
    return (h if want_post else None), obj, ctx, a


class _VfeColsData(_VfeData):
    """_VfeData of a column posterior: `alpha`, `m_eps` are (M, S), `b_y` is (n, S); `U`, `Lam_U` do not depend on y."""

    def __getitem__(self, k):
        p = self._post
        st, dt, m, S = p._state, p._dtype, p._m, p.ncols
        lib = st.ctx.lib
        if k in ("alpha", "m_eps"):
            a = np.empty((m, S), dtype=dt, order="F")
            check(lib.gp_vfe_get_cols(st.handle, a.ctypes.data if k == "alpha" else None, a.ctypes.data if k == "m_eps" else None))
            return a
        if k == "b_y":
            n = int(lib.gp_vfe_n(st.handle))
            out = np.empty((max(n, 0), S), dtype=dt, order="F")
            check(lib.gp_vfe_get_by_cols(st.handle, out.ctypes.data))
            return out
        return super().__getitem__(k)


class ApproxColumnsPosteriorGP(AbstractGP):
    """S sparse posteriors that share x, z, kernel, jitter, Σy and the prior mean and differ in y (the columns of Y): ONE streamed pass, ONE pair of M×M
    factors, α for every column.  `objective` is (S,); mean(x) is (ns, S); var / cov do not depend on y and are those of every column."""

    def __init__(self, approx, prior: GP, state: _VfeState, dtype, m: int, ncols: int, objective):
        self.approx, self.prior, self._state, self._dtype, self._m, self._ncols = approx, prior, state, dtype, m, ncols
        self.objective = objective

    @property
    def ncols(self) -> int:
        return self._ncols

    @property
    def data(self):
        return _VfeColsData(self)

    def _predict(self, x, what):
        st, dt = self._state, self._dtype
        mm = _Marshal(dt)
        px = mm.points(x)
        pm = _mean_vector(self.prior.mean_fn, x, dt)
        pm = None if pm is None else mm.arr(pm)
        mean = np.empty((px.n, self._ncols), dtype=dt, order="F") if what & 1 else None
        var = np.empty(px.n, dtype=dt) if what & 2 else None
        cov = np.empty((px.n, px.n), dtype=dt, order="F") if what & 4 else None
        check(st.ctx.lib.gp_vfe_predict_cols(st.handle, C.byref(px), mm.ptr(pm), what, mm.ptr(mean), mm.ptr(var), mm.ptr(cov)))
        return mean, var, cov

    def mean(self, x=None):
        if x is None:
            return super().mean()
        return self._predict(x, 1)[0]

    def var(self, x):
        return self._predict(x, 2)[1]

    def cov(self, x, z=None):
        if z is not None:
            raise TypeError("cov(f, x, z) is not offered for a column posterior: take the block of cov(f, [x; z])")
        return self._predict(x, 4)[2]

    def mean_and_var(self, x):
        return self._predict(x, 3)[:2]

    def mean_and_cov(self, x):
        m, _, c = self._predict(x, 5)
        return m, c

    def _one_column_only(self, *a, **k):
        raise TypeError("a column posterior holds one mean per column: this method needs a single-column posterior (posterior(approx, fx, Y[:, s]))")

    mean_and_var_grad = mean_grad = _one_column_only

    def var_grad(self, x):
        """(var, ∂var/∂x): the variance side uses no α."""
        st = self._state
        r = _predict_grad(st.ctx.lib.gp_vfe_predict_grad, st.handle, self._dtype, self.prior.mean_fn, x, 2)
        return r[1], r[3]

    def __call__(self, x, sigma2=default_sigma2):
        raise TypeError("a FiniteGP over a column posterior (held-out logpdf, samples) is not offered: use posterior(approx, fx, Y[:, s])")

    def objective_grad(self, wrt_x: bool = False) -> dict:
        """Gradient of the SUM over the columns of the objective this posterior was fitted with, at its own parameters (gp_vfe_grad_cols).  Keys as
        ApproxPosteriorGP.objective_grad; "y" and "mean" (= −"y") are (n, S) — sum "mean" over the columns for the shared mean vector."""
        st, dt, S = self._state, self._dtype, self._ncols
        n = int(st.ctx.lib.gp_vfe_n(st.handle))
        zin = _as_input(self.approx.fz.x)
        mm = _Marshal(dt)
        pz = mm.points(self.approx.fz.x)
        nscale = mm.kernel(self.prior.kernel, pz.d).nscale
        dvar, dns = C.c_double(), C.c_double()
        dscale = (C.c_double * max(nscale, 1))()
        dnoise = np.empty(n, dtype=dt)
        dY = np.empty((n, S), dtype=dt, order="F")
        dz = None
        if np.dtype(dt) == np.float64:
            dz = np.empty((pz.n,) if pz.layout == 0 else ((pz.n, pz.d) if pz.layout == 1 else (pz.d, pz.n)), dtype=np.float64)
        dxb = np.empty((n, pz.d), dtype=dt) if wrt_x else None          # layout 1: point-contiguous (N, D)
        check(st.ctx.lib.gp_vfe_grad_cols(st.handle, C.byref(dvar), dscale, C.byref(dns), dnoise.ctypes.data, dY.ctypes.data, None if dz is None else dz.ctypes.data,
                                          pz.layout, None if dxb is None else dxb.ctypes.data, 1))
        sc = None if nscale == 0 else (float(dscale[0]) if nscale == 1 else np.array([dscale[i] for i in range(nscale)]))
        g = {"variance": dvar.value, "scale": sc, "noise": dns.value, "noise_diag": dnoise, "y": dY, "mean": -dY}
        if dz is not None:
            if pz.layout == 0:
                g["z"] = dz
            else:
                nd = dz if pz.layout == 1 else dz.T
                g["z"] = np.ascontiguousarray(nd.T if isinstance(zin, ColVecs) else nd)
        if wrt_x:
            g["x"] = dxb[:, 0] if pz.d == 1 and pz.layout == 0 else dxb
        return g


def _vfe_posterior_columns(approx, fx: FiniteGP, Y) -> ApproxColumnsPosteriorGP:
    h, obj, ctx, a = _vfe_cols_call(approx, fx, Y, True, "posterior_columns")
    return ApproxColumnsPosteriorGP(approx, fx.f, _VfeState(ctx, h), a.dt, a.pz.n, a.ncols, obj)


def _vfe_cols_update(post: ApproxColumnsPosteriorGP, fx: FiniteGP, Y2=None) -> ApproxColumnsPosteriorGP:
    st, dt, S = post._state, post._dtype, post._ncols
    mm = _Marshal(dt)
    obj = np.empty(S, dtype=dt)
    h = C.c_void_p()
    if Y2 is None:  # new pseudo-points: fx is fz
        pz = mm.points(fx.x)
        check(st.ctx.lib.gp_vfe_append_cols(st.handle, C.byref(pz), C.byref(h), obj.ctypes.data))
        z_all, _ = _stack_inputs(post.approx.fz.x, fx.x)
        approx = type(post.approx)(post.prior(z_all, post.approx.fz.sigma2))
        return ApproxColumnsPosteriorGP(approx, post.prior, _VfeState(st.ctx, h), dt, post._m + pz.n, S, obj)
    Y2 = _cols_matrix(fx, Y2, "update_posterior", S)
    _refuse_dense_vfe(fx)
    px = mm.points(fx.x)
    nz = mm.noise(fx.sigma2, px.n)
    mean = _mean_vector(post.prior.mean_fn, fx.x, dt)
    mean = None if mean is None else mm.arr(mean)
    Yf = mm.arr(Y2, order="F")
    check(st.ctx.lib.gp_vfe_update_cols(st.handle, C.byref(px), C.byref(nz), mm.ptr(mean), Yf.ctypes.data, max(Yf.shape[0], 1), C.byref(h), obj.ctypes.data))
    return ApproxColumnsPosteriorGP(post.approx, post.prior, _VfeState(st.ctx, h), dt, post._m, S, obj)


def approx_log_evidence_columns(a, fx: FiniteGP, Y) -> np.ndarray:
    """approx_log_evidence(a, fx, Y[:, s]) for every column s, shape (S,), from one streamed pass (gp_vfe_fit_cols without a handle)."""
    return _vfe_cols_call(a, fx, Y, False, "approx_log_evidence_columns")[1]


def elbo_columns(a, fx: FiniteGP, Y) -> np.ndarray:
    """elbo(vfe, fx, Y[:, s]) for every column s, shape (S,)."""
    if not isinstance(a, VFE):
        raise TypeError("elbo is defined for VFE")
    return approx_log_evidence_columns(a, fx, Y)


def elbo_and_grad_columns(a, fx: FiniteGP, Y, wrt_x: bool = False) -> tuple:
    """(objectives (S,), gradient of their SUM): one column fit + one backward pass (gp_vfe_fit_cols + gp_vfe_grad_cols).  "x" comes back in the shape
    of fx.x's array."""
    post = _vfe_posterior_columns(a, fx, Y)
    g = post.objective_grad(wrt_x)
    if wrt_x and "x" in g and np.ndim(g["x"]) == 2 and isinstance(_as_input(fx.x), ColVecs):
        g["x"] = np.ascontiguousarray(g["x"].T)
    return post.objective, g
