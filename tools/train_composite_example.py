"""The reference's Mauna Loa example on the device: examples/1-mauna-loa/script.jl:102-116 builds SE(θ₁) + Per(θ₂)·SE(θ₃) + RQ(θ₄) + (SE(θ₅) + σₙ²·White)
and trains its hyperparameters by LBFGS on the gradient of logpdf (:201-240).  Here every LBFGS evaluation is one `logpdf_and_grad` call
(gp_logpdf_grad_sum), in log-parameter space, on seeded synthetic monthly data (trend + seasonal + noise; x in years since 1958).
    python tools/train_composite_example.py [n=545] [iters=30]        (n = 545 is the example's size; n = 65536 the large case)"""
import json
import sys
import time
from pathlib import Path

import numpy as np
from scipy.optimize import minimize

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import abstractgps_jl_amd as agp  # noqa: E402


def initial_kernel():
    se, per, rq = agp.SqExponentialKernel(), agp.PeriodicKernel(r=[1.0]), agp.RationalQuadraticKernel(alpha=1.0)
    return (4.0 * agp.with_lengthscale(se, 30.0) + 1.0 * (agp.with_lengthscale(per, 1.0) * agp.with_lengthscale(se, 60.0))
            + 0.3 * agp.with_lengthscale(rq, 1.0) + (0.1 * agp.with_lengthscale(se, 0.2) + 0.05 * agp.WhiteKernel()))


def main():
    opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
    n, iters = int(opt.get("n", 545)), int(opt.get("iters", 30))
    rng = np.random.default_rng(0)
    x = np.arange(n) / 12.0 * (545 / max(n, 545))  # monthly from 1958 at the example's size; denser sampling of the same 45 years beyond it
    y = 0.012 * x**2 + 1.4 * x + 2.8 * np.sin(2 * np.pi * x) + 0.6 * np.cos(4 * np.pi * x) + 0.25 * rng.standard_normal(n)
    y = (y - y.mean()) / y.std()
    k0 = initial_kernel()
    p0 = np.log(np.concatenate([agp.params(k0), [0.01]]))  # kernel parameters and the observation noise, in log space
    calls = []

    def fun(lp):
        p = np.exp(lp)
        val, g = agp.logpdf_and_grad(agp.GP(agp.with_params(k0, p[:-1]))(x, p[-1]), y)
        calls.append(float(val))
        return -float(val), -np.concatenate([g["kernel"], [g["noise"]]]) * p

    t0 = time.perf_counter()
    v0 = -fun(p0)[0]
    res = minimize(fun, p0, jac=True, method="L-BFGS-B", options={"maxiter": iters})
    dt = time.perf_counter() - t0
    print(json.dumps({"n": n, "logpdf_start": v0, "logpdf_end": -float(res.fun), "evaluations": len(calls), "s_total": dt,
                      "ms_per_evaluation": dt / len(calls) * 1e3, "params": np.exp(res.x).round(5).tolist(),
                      "status": res.message if isinstance(res.message, str) else res.message.decode()}))


if __name__ == "__main__":
    main()
