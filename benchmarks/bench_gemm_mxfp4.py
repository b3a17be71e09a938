#!/usr/bin/env python3
"""MXFP4 (E2M1 two to a byte with E8M0 block scales) MFMA tile-GEMM benchmark.

C (fp32) = A^T B over packed tiles with one scale byte per column and 32 K
elements; whole-job TFLOP/s on the DTD engine. The operands are quantised
once from synthetic fp32 tiles; with --quantize both are quantised again in
every timed step. --kernel times the tile kernel alone on one size x size x
kdim problem (synthetic bytes, scale bytes in 120..134), and --kernel
--quantize the quantiser kernel alone on a size x kdim fp32 matrix (GB/s
over the bytes it reads and writes).
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
    ap.add_argument("--kernel", action="store_true",
                    help="kernel-only rate (no DAG, --steps launches)")
    ap.add_argument("--quantize", action="store_true",
                    help="quantise both fp32 operands inside the timed step")
    args = ap.parse_args()

    import parsec_amd as pm

    dtype = "mx e2m1xe2m1(fp32 acc)"
    if args.kernel:
        from parsec_amd import _core
        if args.quantize:
            def run(n):
                return _core.bench_quantize_mxfp4(args.size, args.kdim, n)
            metric = "GB/s mxfp4 quantiser kernel"
        else:
            def run(n):
                return _core.bench_gemm_mxfp4(args.size, args.size, args.kdim,
                                              n)
            metric = "TFLOP/s mxfp4 tile-GEMM kernel"
        for _ in range(args.warmup):
            run(2)
        print(json.dumps({
            "metric": metric, "value": round(run(args.steps), 1),
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

    def operand(rows):  # fp32 source, packed elements, scales
        return (pm.TiledMatrix(ctx, K, rows, kb, mb, p, q, elem_size=4),
                pm.TiledMatrix(ctx, K // 2, rows, kb // 2, mb, p, q,
                               elem_size=1),
                pm.TiledMatrix(ctx, K // 32, rows, kb // 32, mb, p, q,
                               elem_size=1))

    Xa, Qa, Sa = operand(M)
    Xb, Qb, Sb = operand(N)
    C = pm.TiledMatrix(ctx, M, N, mb, mb, p, q, elem_size=4)

    def quantise(tp):
        pm.insert_quantize_mxfp4(tp, Xa, Qa, Sa)
        pm.insert_quantize_mxfp4(tp, Xb, Qb, Sb)

    tp = pm.Dtd(ctx)
    pm.insert_fill_f32(tp, Xa, 1)
    pm.insert_fill_f32(tp, Xb, 2)
    quantise(tp)
    tp.wait()

    def step(n):
        tp = pm.Dtd(ctx)
        for _ in range(n):
            if args.quantize:
                quantise(tp)
            pm.insert_gemm_mxfp4(tp, Qa, Sa, Qb, Sb, C)
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
            "metric": "TFLOP/s mxfp4 tile-GEMM DAG", "value": round(tf, 1),
            "n_gpus": world, "M": M, "N": N, "K": K, "tile": args.tile,
            "quantize": args.quantize, "dtype": dtype, "data": "synthetic",
        }), flush=True)
    del Xa, Qa, Sa, Xb, Qb, Sb, C, ctx


if __name__ == "__main__":
    main()
