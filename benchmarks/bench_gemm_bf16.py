#!/usr/bin/env python3
"""bf16 MFMA tile-GEMM DAG benchmark (BASELINE.json config 5).

C (fp32) = op(A) op(B) over bf16 tiles; whole-job TFLOP/s on the DTD engine.
--layout picks the operand storage (TN: both K-major, the default; first
letter N: A is M x K column-major; second letter T: B is N x K column-major;
see docs/API.md). --kernel
times the tile kernel alone on one size x size x kdim problem instead.
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
    ap.add_argument("--layout", default="TN", choices=["TN", "NN", "NT", "TT"])
    ap.add_argument("--kernel", action="store_true",
                    help="kernel-only rate (no DAG, --steps launches)")
    args = ap.parse_args()

    import parsec_amd as pm

    if args.kernel:
        from parsec_amd import _core
        for _ in range(args.warmup):
            _core.bench_gemm_bf16(args.size, args.size, args.kdim, 2,
                                  args.layout)
        tf = _core.bench_gemm_bf16(args.size, args.size, args.kdim,
                                   args.steps, args.layout)
        print(json.dumps({
            "metric": "TFLOP/s bf16 tile-GEMM kernel", "value": round(tf, 1),
            "layout": args.layout, "M": args.size, "N": args.size,
            "K": args.kdim, "launches": args.steps,
            "dtype": "bf16(fp32 acc)", "data": "synthetic",
        }), flush=True)
        return

    ta, tb = args.layout
    ctx = pm.init_distributed(nworkers=4)
    world = ctx.world
    p, q = (1, world)
    M = N = args.size
    K = args.kdim
    kb = mb = args.tile
    At = (pm.TiledMatrix(ctx, K, M, kb, mb, p, q, elem_size=2) if ta == "T"
          else pm.TiledMatrix(ctx, M, K, mb, kb, p, q, elem_size=2))
    B = (pm.TiledMatrix(ctx, K, N, kb, mb, p, q, elem_size=2) if tb == "N"
         else pm.TiledMatrix(ctx, N, K, mb, kb, p, q, elem_size=2))
    C = pm.TiledMatrix(ctx, M, N, mb, mb, p, q, elem_size=4)

    def step(n):
        tp = pm.Dtd(ctx)
        for _ in range(n):
            pm.insert_fill_bf16(tp, At, 1)
            pm.insert_fill_bf16(tp, B, 2)
            pm.insert_gemm_bf16(tp, At, B, C, transa=ta, transb=tb)
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
            "metric": "TFLOP/s bf16 tile-GEMM DAG", "value": round(tf, 1),
            "n_gpus": world, "M": M, "N": N, "K": K, "tile": args.tile,
            "layout": args.layout, "dtype": "bf16(fp32 acc)", "data": "synthetic",
        }), flush=True)
    del At, B, C, ctx


if __name__ == "__main__":
    main()
