#!/usr/bin/env python3
"""FP8 (E4M3 / E5M2) MFMA tile-GEMM benchmark.

C (fp32) = A^T B over one-byte tiles, both operands K-major; whole-job
TFLOP/s on the DTD engine. --fmt-a / --fmt-b pick each operand's format (see
docs/API.md). --kernel times the tile kernel alone on one size x size x kdim
problem instead.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--kdim", type=int, default=65536)
    ap.add_argument("--tile", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fmt-a", default="e4m3", choices=["e4m3", "e5m2"])
    ap.add_argument("--fmt-b", default="e4m3", choices=["e4m3", "e5m2"])
    ap.add_argument("--kernel", action="store_true",
                    help="kernel-only rate (no DAG, --steps launches)")
    args = ap.parse_args()

    import parsec_amd as pm

    dtype = f"{args.fmt_a}x{args.fmt_b}(fp32 acc)"
    if args.kernel:
        from parsec_amd import _core
        for _ in range(args.warmup):
            _core.bench_gemm_fp8(args.size, args.size, args.kdim, 2,
                                 args.fmt_a, args.fmt_b)
        tf = _core.bench_gemm_fp8(args.size, args.size, args.kdim,
                                  args.steps, args.fmt_a, args.fmt_b)
        print(json.dumps({
            "metric": "TFLOP/s fp8 tile-GEMM kernel", "value": round(tf, 1),
            "M": args.size, "N": args.size, "K": args.kdim,
            "launches": args.steps, "dtype": dtype, "data": "synthetic",
        }), flush=True)
        return

    ctx = pm.init_distributed(nworkers=4)
    world = ctx.world
    p, q = (1, world)
    M = N = args.size
    K = args.kdim
    kb = mb = args.tile
    At = pm.TiledMatrix(ctx, K, M, kb, mb, p, q, elem_size=1)
    B = pm.TiledMatrix(ctx, K, N, kb, mb, p, q, elem_size=1)
    C = pm.TiledMatrix(ctx, M, N, mb, mb, p, q, elem_size=4)

    def step(n):
        tp = pm.Dtd(ctx)
        for _ in range(n):
            pm.insert_fill_fp8(tp, At, 1)
            pm.insert_fill_fp8(tp, B, 2)
            pm.insert_gemm_fp8(tp, At, B, C, fmt_a=args.fmt_a,
                               fmt_b=args.fmt_b)
        tp.wait()

    step(args.warmup)
    ctx.gpu_sync()
    ctx.barrier()
    t0 = time.perf_counter()
    step(args.steps)
    ctx.gpu_sync()
    ctx.barrier()
    dt = time.perf_counter() - t0
    tf = args.steps * 2.0 * M * N * K / dt / 1e12
    if ctx.rank == 0:
        print(json.dumps({
            "metric": "TFLOP/s fp8 tile-GEMM DAG", "value": round(tf, 1),
            "n_gpus": world, "M": M, "N": N, "K": K, "tile": args.tile,
            "dtype": dtype, "data": "synthetic",
        }), flush=True)
    del At, B, C, ctx


if __name__ == "__main__":
    main()
