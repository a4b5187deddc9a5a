"""Bayesian optimisation with the device's predictive value AND gradient: the use the reference's users make of Zygote / ForwardDiff through
mean(f_post, x) and var(f_post, x) (src/exact_gpr_posterior.jl:60-90).

A GP (Matern52 behind an ARD transform, fixed hyper-parameters) on a 2-D (Branin) or 3-D (Hartmann-3) test function, minimised.  Every round maximises the
upper confidence bound of the NEGATED function, a(x) = mean(x) + beta·sqrt(var(x)), by SciPy L-BFGS-B from `starts` random starting points: the starts are
independent, so they are optimised as ONE separable problem and every evaluation of the objective is ONE gp_posterior_predict_grad call for all of them
(value and gradient from the same pass; ∂a/∂x = ∂mean/∂x + beta/(2·sqrt(var)) · ∂var/∂x).  The best point is evaluated and the posterior is extended by
sequential conditioning (gp_posterior_update), not refitted.  Printed per round: the acquisition value at the best start before and after the optimisation
(it must rise), the number of device calls and the ms per acquisition evaluation.

    python tools/bayesopt_example.py [d=2] [rounds=4] [n0=40] [starts=32] [beta=2.0] [seed=0]"""
import sys
import time
from pathlib import Path

import numpy as np
from scipy.optimize import minimize

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def branin(X):  # on [0, 1]², scaled to O(1); minimum ≈ −1.047 (three minimisers)
    x1, x2 = 15 * X[:, 0] - 5, 15 * X[:, 1]
    v = (x2 - 5.1 / (4 * np.pi**2) * x1**2 + 5 / np.pi * x1 - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x1) + 10
    return (v - 54.8) / 51.9


def hartmann3(X):  # on [0, 1]³; minimum −3.8628
    A = np.array([[3.0, 10, 30], [0.1, 10, 35], [3.0, 10, 30], [0.1, 10, 35]])
    P = 1e-4 * np.array([[3689, 1170, 2673], [4699, 4387, 7470], [1091, 8732, 5547], [381, 5743, 8828]])
    al = np.array([1.0, 1.2, 3.0, 3.2])
    return -np.sum(al * np.exp(-np.sum(A[None] * (X[:, None, :] - P[None]) ** 2, axis=2)), axis=1)


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    d, rounds, n0, starts = int(kv.get("d", 2)), int(kv.get("rounds", 4)), int(kv.get("n0", 40)), int(kv.get("starts", 32))
    beta, seed = float(kv.get("beta", 2.0)), int(kv.get("seed", 0))
    import abstractgps_jl_amd as agp

    fun = branin if d == 2 else hartmann3
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n0, d))
    y = -fun(X)                                   # maximise the negated function
    s2 = 1e-4
    f = agp.GP(float(np.mean(y)), float(np.var(y)) * agp.Matern52Kernel() @ agp.ARDTransform(np.full(d, 4.0)))
    post = agp.posterior(f(agp.RowVecs(X), s2), y)
    best = float(y.max())
    print(f"d={d}: {n0} initial points, best f = {-best:.4f}")
    for r in range(rounds):
        calls, t_dev = [0], [0.0]

        def neg_acq(flat):
            P = np.ascontiguousarray(flat.reshape(starts, d))
            t0 = time.perf_counter()
            m, v, dm, dv = post.mean_and_var_grad(agp.RowVecs(P))
            t_dev[0] += time.perf_counter() - t0
            calls[0] += 1
            sd = np.sqrt(np.maximum(v, 1e-300))
            return -float(np.sum(m + beta * sd)), -(dm + (beta / (2 * sd))[:, None] * dv).ravel()

        P0 = rng.uniform(0, 1, size=(starts, d))
        m0, v0 = post.mean_and_var(agp.RowVecs(P0))
        a0 = m0 + beta * np.sqrt(v0)
        res = minimize(neg_acq, P0.ravel(), jac=True, method="L-BFGS-B", bounds=[(0.0, 1.0)] * (starts * d), options={"maxiter": 60})
        P1 = res.x.reshape(starts, d)
        m1, v1 = post.mean_and_var(agp.RowVecs(P1))
        a1 = m1 + beta * np.sqrt(v1)
        assert a1.sum() >= a0.sum(), "L-BFGS-B lowered the summed acquisition: value and gradient disagree"  # (the line search acts on the SUM over the starts)
        j = int(np.argmax(a1))
        xn = P1[j:j + 1]
        yn = -fun(xn)
        post = agp.posterior(post(agp.RowVecs(xn), s2), yn)      # sequential conditioning on the device
        best = max(best, float(yn[0]))
        print(f"round {r + 1}: acquisition max over the starts {a0.max():.4f} -> {a1.max():.4f} (mean {a0.mean():.4f} -> {a1.mean():.4f}); "
              f"{calls[0]} device calls of {starts} points, {1e3 * t_dev[0] / calls[0]:.3f} ms per acquisition evaluation; "
              f"f(x_new) = {-float(yn[0]):.4f}, best f = {-best:.4f}, n = {n0 + r + 1}")
    print("BAYESOPT_OK")


if __name__ == "__main__":
    main()
