#!/usr/bin/env python3
"""MXFP6 (E2M3 / E3M2, four elements to three bytes, E8M0 block scales) MFMA
tile-GEMM benchmark, with MXFP4 and MXFP8 timed beside it.

C (fp32) = A^T B over packed tiles with one scale byte per column and 32 K
elements; whole-job TFLOP/s on the DTD engine. The operands are quantised
once from synthetic fp32 tiles; with --quantize both are quantised again in
every timed step. --kernel times the tile kernel alone on one size x size x
kdim problem (synthetic bytes, scale bytes in 120..134), and --kernel
--quantize the quantiser kernel alone on a size x kdim fp32 matrix (GB/s
over the bytes it reads and writes).

Every figure is taken --passes times, the three formats alternating within
a pass, in this one process; the JSON line carries each pass in order.
--only-mxfp6 leaves MXFP4 and MXFP8 out.
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
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--fmt-a", default="e2m3", choices=["e2m3", "e3m2"])
    ap.add_argument("--fmt-b", default="e2m3", choices=["e2m3", "e3m2"])
    ap.add_argument("--only-mxfp6", action="store_true")
    ap.add_argument("--kernel", action="store_true",
                    help="kernel-only rate (no DAG, --steps launches)")
    ap.add_argument("--quantize", action="store_true",
                    help="quantise both fp32 operands inside the timed step")
    args = ap.parse_args()

    import parsec_amd as pm

    names = ["mxfp6"] if args.only_mxfp6 else ["mxfp6", "mxfp4", "mxfp8"]
    dtype = "mx %sx%s(fp32 acc)" % (args.fmt_a, args.fmt_b)
    if args.kernel:
        from parsec_amd import _core
        m, k = args.size, args.kdim
        if args.quantize:
            run = {"mxfp6": lambda n: _core.bench_quantize_mxfp6(m, k, n, args.fmt_a),
                   "mxfp4": lambda n: _core.bench_quantize_mxfp4(m, k, n),
                   "mxfp8": lambda n: _core.bench_quantize_mxfp8(m, k, n)}
            metric = "GB/s quantiser kernel"
        else:
            run = {"mxfp6": lambda n: _core.bench_gemm_mxfp6(m, m, k, n, args.fmt_a,
                                                             args.fmt_b),
                   "mxfp4": lambda n: _core.bench_gemm_mxfp4(m, m, k, n),
                   "mxfp8": lambda n: _core.bench_gemm_mxfp8(m, m, k, n)}
            metric = "TFLOP/s tile-GEMM kernel"
        for name in names:
            for _ in range(args.warmup):
                run[name](2)
        out = {name: [] for name in names}
        for _ in range(args.passes):
            for name in names:
                out[name].append(round(run[name](args.steps), 1))
        print(json.dumps({
            "metric": metric, "value": out["mxfp6"][-1], "passes": out,
            "M": m, "N": m, "K": k, "launches": args.steps, "dtype": dtype,
            "data": "synthetic",
        }), flush=True)
        return

    ctx = pm.init_distributed(nworkers=4)
    world = ctx.world
    p, q = (1, world)
    M = N = args.size
    K = args.kdim
    kb = mb = args.tile
    # packed bytes per K element as a fraction, quantiser, GEMM
    kinds = {
        "mxfp6": (3, 4,
                  lambda tp, X, Q, S, f: pm.insert_quantize_mxfp6(tp, X, Q, S, format=f),
                  lambda tp, a, b, C: pm.insert_gemm_mxfp6(
                      tp, a[0], a[1], b[0], b[1], C, a_format=args.fmt_a,
                      b_format=args.fmt_b)),
        "mxfp4": (1, 2,
                  lambda tp, X, Q, S, f: pm.insert_quantize_mxfp4(tp, X, Q, S),
                  lambda tp, a, b, C: pm.insert_gemm_mxfp4(tp, a[0], a[1], b[0],
                                                           b[1], C)),
        "mxfp8": (1, 1,
                  lambda tp, X, Q, S, f: pm.insert_quantize_mxfp8(tp, X, Q, S),
                  lambda tp, a, b, C: pm.insert_gemm_mxfp8(tp, a[0], a[1], b[0],
                                                           b[1], C)),
    }

    Xa = pm.TiledMatrix(ctx, K, M, kb, mb, p, q, elem_size=4)
    Xb = pm.TiledMatrix(ctx, K, N, kb, mb, p, q, elem_size=4)
    C = pm.TiledMatrix(ctx, M, N, mb, mb, p, q, elem_size=4)

    def packed(name, rows):  # packed elements, scales
        num, den = kinds[name][:2]
        return (pm.TiledMatrix(ctx, K * num // den, rows, kb * num // den, mb,
                               p, q, elem_size=1),
                pm.TiledMatrix(ctx, K // 32, rows, kb // 32, mb, p, q,
                               elem_size=1))

    ops = {name: (packed(name, M), packed(name, N)) for name in names}

    def quantise(tp, name):
        a, b = ops[name]
        kinds[name][2](tp, Xa, a[0], a[1], args.fmt_a)
        kinds[name][2](tp, Xb, b[0], b[1], args.fmt_b)

    tp = pm.Dtd(ctx)
    pm.insert_fill_f32(tp, Xa, 1)
    pm.insert_fill_f32(tp, Xb, 2)
    for name in names:
        quantise(tp, name)
    tp.wait()

    def step(name, n):
        tp = pm.Dtd(ctx)
        for _ in range(n):
            if args.quantize:
                quantise(tp, name)
            kinds[name][3](tp, ops[name][0], ops[name][1], C)
        tp.wait()

    def timed(name):
        ctx.gpu_sync()
        ctx.barrier()
        t0 = time.perf_counter()
        step(name, args.steps)
        ctx.gpu_sync()
        ctx.barrier()
        dt = time.perf_counter() - t0
        return round(args.steps * 2.0 * M * N * K / dt / 1e12, 1)

    for name in names:
        step(name, args.warmup)
    out = {name: [] for name in names}
    for _ in range(args.passes):
        for name in names:
            out[name].append(timed(name))
    if ctx.rank == 0:
        print(json.dumps({
            "metric": "TFLOP/s tile-GEMM DAG", "value": out["mxfp6"][-1],
            "passes": out, "n_gpus": world, "M": M, "N": N, "K": K,
            "tile": args.tile, "quantize": args.quantize, "dtype": dtype,
            "data": "synthetic",
        }), flush=True)
    del Xa, Xb, C, ops, ctx


if __name__ == "__main__":
    main()
