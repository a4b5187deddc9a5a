"""Is the dual-target epilogue of the Strassen products exposed?  One off-diagonal block of the trailing update through gpd_gemm_nt (default: the first
panel's block at N = 65 536, 30 720 x 30 720 x 2 048), classical (strassen_min_rows = 0: one launch) against one level of Strassen (seven half-size products in
four launches after two launches of strassen_sums_kernel).

With time_kernels = 1 the library records an event pair around every tile-GEMM launch and around nothing else, so gpd_gemm_time's total IS the products' time
with the sums taken out; the wall time of the call (host clock around the call and gpd_sync) is printed beside it, the difference being the sums and the launch gaps.
Median of --reps after one warm-up per form.  The flops say products / classical = 7/8 = 0.875; what the ratio lies above that is what the products' epilogue
(twelve quadrant read-modify-writes instead of the classical prologue loads and plain stores) and their shorter k loops cost on such a block.

GPMI355_LIB selects the library, so that two builds can be compared process by process."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import abstractgps_jl_amd as agp  # noqa: E402
from abstractgps_jl_amd._lib import check  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30720x30720x2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--strassen-min-rows", type=int, default=8192)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    m, n, k = [int(v) for v in args.shape.split("x")]
    ctx = agp.Context(0)
    ctx.set_param("time_kernels", 1)
    lib, h = ctx.lib, ctx.handle
    ld = k + 32
    g = torch.Generator(device="cuda").manual_seed(1)
    A = torch.randn(m + 128, ld, dtype=torch.float64, device="cuda", generator=g)
    B = torch.randn(n + 128, ld, dtype=torch.float64, device="cuda", generator=g)
    Cm = torch.zeros(m, n + 32, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()

    def once():
        t0 = time.perf_counter()
        check(lib.gpd_gemm_nt(h, P(Cm), n + 32, P(A), ld, P(B), ld, m, n, k, None, 0, 0))
        check(lib.gpd_sync(h))
        wall = (time.perf_counter() - t0) * 1e3
        ms, nl = C.c_double(), C.c_int64()
        check(lib.gpd_gemm_time(h, C.byref(ms), C.byref(nl)))
        return wall, ms.value, nl.value

    out = {"label": args.label, "m": m, "n": n, "k": k, "reps": args.reps}
    for name, v in (("classical", 0), ("strassen", args.strassen_min_rows)):
        ctx.set_param("strassen_min_rows", v)
        once()  # warm-up
        runs = [once() for _ in range(args.reps)]
        out[name] = {"launches": runs[0][2], "gemm_ms_median": round(statistics.median(r[1] for r in runs), 3),
                     "gemm_ms_min": round(min(r[1] for r in runs), 3), "gemm_ms_max": round(max(r[1] for r in runs), 3),
                     "wall_ms_median": round(statistics.median(r[0] for r in runs), 3)}
    c, s = out["classical"], out["strassen"]
    out["sums_and_gaps_ms"] = round(s["wall_ms_median"] - s["gemm_ms_median"], 3)
    out["products_over_classical"] = round(s["gemm_ms_median"] / c["gemm_ms_median"], 4)
    out["products_over_classical_range"] = [round(s["gemm_ms_min"] / c["gemm_ms_max"], 4), round(s["gemm_ms_max"] / c["gemm_ms_min"], 4)]
    out["flops_ratio"] = 0.875
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
