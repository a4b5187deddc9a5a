"""The reference's deep-kernel example on the device: examples/2-deep-kernel-learning/script.jl puts a small MLP (1 -> 20 -> 30 -> 5) in front of a
SqExponentialKernel and trains the network by Adam(0.005) for 200 steps on −logpdf of N = 150 noisy samples of sinc(|x|^|x|) (noise 0.01²).  Here the MLP is a
torch module, and one `logpdf_and_grad(..., wrt_x=True)` call per step returns the value and ∂logpdf/∂(features), which `NegLogpdf` — a
torch.autograd.Function — hands back to autograd as the gradient of the feature matrix.  `kernel=composite` swaps the SE for SE + 0.5·Matern52 (both
untransformed): the same training through gp_logpdf_grad_sum_x / kgradx_sum_kernel.  The script's Dense layers carry no activation (its feature map is affine);
`act=tanh`, the default here, makes the map non-linear, `act=identity` is the script's literal network.
    python tools/train_deep_kernel_example.py [kernel=se|composite] [n=150] [iters=200] [dtype=float64|float32] [device=cpu|cuda] [act=tanh|identity]
A demonstration, not a benchmark: it prints the loss every 10 steps and one JSON line (first loss, last loss, ms per step)."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import abstractgps_jl_amd as agp  # noqa: E402


class NegLogpdf(torch.autograd.Function):
    """−logpdf(GP(kernel)(RowVecs(features), sigma2), y) with ∂/∂features from the library (the observations and Σy are constants)."""

    @staticmethod
    def forward(ctx, features, y, kernel, sigma2):
        lp, g = agp.logpdf_and_grad(agp.GP(kernel)(agp.RowVecs(features.detach().cpu().numpy()), sigma2), y, wrt_x=True)
        ctx.gx = torch.from_numpy(np.ascontiguousarray(-g["x"])).to(device=features.device, dtype=features.dtype)
        return features.new_tensor(-float(lp))

    @staticmethod
    def backward(ctx, grad_out):
        return grad_out * ctx.gx, None, None, None


def make_kernel(name: str):
    if name == "se":
        return agp.SqExponentialKernel()
    if name == "composite":
        return agp.SqExponentialKernel() + 0.5 * agp.Matern52Kernel()
    raise ValueError("kernel must be se or composite")


def make_data(n: int, seed: int = 42, noise_std: float = 0.01):
    """script.jl:31-38: x ~ U(−3, 3), y = sinc(|x|^|x|) + noise_std·ε (sinc(t) = sin(πt)/(πt))."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.0, 3.0, n)
    return x, np.sinc(np.abs(x) ** np.abs(x)) + noise_std * rng.standard_normal(n)


def make_mlp(sizes=(1, 20, 30, 5), act: str = "tanh", dtype=torch.float64, seed: int = 0) -> torch.nn.Sequential:
    torch.manual_seed(seed)
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if act == "tanh" and i < len(sizes) - 2:
            layers.append(torch.nn.Tanh())
    return torch.nn.Sequential(*layers).to(dtype)


def loss_fn(net, x_t, y, kernel, sigma2):
    return NegLogpdf.apply(net(x_t), y, kernel, sigma2)


def train(net, x_t, y, kernel, sigma2, iters: int, lr: float = 0.005, log_every: int = 10) -> list:
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    losses = []
    for i in range(1, iters + 1):
        opt.zero_grad()
        loss = loss_fn(net, x_t, y, kernel, sigma2)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if log_every and i % log_every == 0:
            print(f"iteration {i}/{iters}: loss = {losses[-1]:.6f}", flush=True)
    return losses


def main():
    opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
    n, iters = int(opt.get("n", 150)), int(opt.get("iters", 200))
    npdt = np.dtype(opt.get("dtype", "float64")).type
    tdt = torch.float32 if npdt is np.float32 else torch.float64
    dev = opt.get("device", "cpu")
    kernel = make_kernel(opt.get("kernel", "se"))
    x, y = make_data(n)
    y = y.astype(npdt)
    net = make_mlp(act=opt.get("act", "tanh"), dtype=tdt).to(dev)
    x_t = torch.from_numpy(x.astype(npdt))[:, None].to(dev)
    sigma2 = npdt(0.01**2)
    t0 = time.perf_counter()
    losses = train(net, x_t, y, kernel, sigma2, iters)
    dt = time.perf_counter() - t0
    print(json.dumps({"kernel": opt.get("kernel", "se"), "n": n, "iters": iters, "dtype": np.dtype(npdt).name, "loss_first": losses[0], "loss_last": losses[-1],
                      "ms_per_step": dt / max(iters, 1) * 1e3}))


if __name__ == "__main__":
    main()
