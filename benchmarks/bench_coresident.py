#!/usr/bin/env python3
"""Kernel benchmark beside other kernels: the Cholesky DAG's mix at one tile
size, on four non-blocking streams at once (_core.bench_coresident).

Two streams loop rocblas_dgemm NT nb^3 (C -= A B^T), one the hand tile SYRK
(n = k = nb), one the hand TRSM product (m = n = nb), at the DAG's 5:1:1
launch ratio: --per-round P gives 5P GEMM, P SYRK and P TRMM launches per
call. --kernel picks the hand kinds' full-tile kernel (3 or 4; 0 is
PARSEC_MCA_dgemm_nt_kernel). A solo figure says what a kernel does with the
GPU to itself; in the DAG 3 to 4 kernels share it, and this is the figure
that goes with that.

The value is the median wall time of the whole mix over --calls calls, with
(max - min) / median as its spread; the per-stream times (first to last
event of each stream) come from the median call. Run it under a time limit
of its own, e.g. `timeout -k 10 300 python benchmarks/bench_coresident.py`.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=4096)
    ap.add_argument("--per-round", type=int, default=8)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--kernel", type=int, default=0, choices=[0, 3, 4])
    args = ap.parse_args()

    import parsec_amd as pm
    from parsec_amd import _core

    if pm.hip_device_count() == 0:
        sys.exit("bench_coresident: no GPU")
    _core.bench_coresident(args.nb, args.per_round, args.kernel)  # warm-up
    calls = sorted((_core.bench_coresident(args.nb, args.per_round,
                                           args.kernel)
                    for _ in range(args.calls)), key=lambda r: r["wall_ms"])
    med = calls[len(calls) // 2]
    walls = [r["wall_ms"] for r in calls]
    # the flops the mix needs: dense GEMMs, half-tiles for SYRK and TRMM
    flops = (5 * 2.0 + 1.0 + 1.0) * args.per_round * float(args.nb) ** 3
    print(json.dumps({
        "metric": "ms, Cholesky kernel mix side by side",
        "value": round(med["wall_ms"], 3),
        "unit": "ms",
        "spread": round((walls[-1] - walls[0]) / med["wall_ms"], 4),
        "wall_ms_all_calls": [round(w, 3) for w in walls],
        "tflops": round(flops / med["wall_ms"] / 1e9, 2),
        "gemm_stream_ms": [round(t, 3) for t in med["gemm_ms"]],
        "syrk_stream_ms": round(med["syrk_ms"], 3),
        "trmm_stream_ms": round(med["trmm_ms"], 3),
        "higher_is_better": False,
        "dtype": "fp64",
        "data": "synthetic",
        "config": {"nb": args.nb, "gemm_launches": 5 * args.per_round,
                   "syrk_launches": args.per_round,
                   "trmm_launches": args.per_round,
                   "dgemm_nt_kernel": args.kernel or os.environ.get(
                       "PARSEC_MCA_dgemm_nt_kernel", "default")},
    }), flush=True)


if __name__ == "__main__":
    main()
