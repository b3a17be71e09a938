#!/usr/bin/env python3
"""Householder least squares / solve (insert_gels) benchmark, and the A/B of
the hand NN kernel against rocblas_dgemm NN.

Without --step this is the driver: it runs every step below in a process of
its own (chores are chosen once per process) under `timeout -k 10`, prints
each step's JSON line, and stops at the first step that fails:

  - insert_gels at N x N (default 16384, tile 1024) with nrhs = nb and with
    nrhs = N, under PARSEC_MCA_chore_gemm_nn=rocblas and =hip;
  - C -= A B at 2048^3 and 4096^3, hand kernel and library.

Only insert_gels is timed; the fills happen before the clock starts. Flop
count (M = N): 4N^3/3 for the QR of A, 2 N^2 nrhs for Q^T B, N^2 nrhs for
the backward sweep. The driver itself never touches the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def step_gels(args):
    import parsec_amd as pm

    has_gpu = pm.hip_device_count() > 0
    n, nb = (args.n, args.nb) if has_gpu else (512, 128)
    nrhs = n if args.nrhs == "n" else nb
    ctx = pm.init_distributed(nworkers=4)
    A = pm.TiledMatrix(ctx, n, n, nb, nb, 1, 1)
    B = pm.TiledMatrix(ctx, n, nrhs, nb, nb, 1, 1)

    def step():
        tp = pm.Dtd(ctx)
        pm.insert_full_fill(tp, A, 3)
        pm.insert_full_fill(tp, B, 5)
        tp.wait()
        ctx.gpu_sync()
        t0 = time.perf_counter()
        tp = pm.Dtd(ctx)
        pm.insert_gels(tp, A, B)
        tp.wait()
        ctx.gpu_sync()
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        step()
    times = sorted(step() for _ in range(args.steps))
    med = times[len(times) // 2]
    flops = 4.0 / 3.0 * float(n) ** 3 + 3.0 * float(n) ** 2 * nrhs
    print(json.dumps({
        "metric": "TFLOP/s Householder least squares (dgels)",
        "value": round(flops / med / 1e12, 2),
        "unit": "TFLOP/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(med * 1e3, 2),
        "ms_all_steps": [round(t * 1e3, 2) for t in times],
        "higher_is_better": True,
        "dtype": "fp64",
        "data": "synthetic",
        "config": {"model": "tile_dgels", "N": n, "tile": nb, "nrhs": nrhs,
                   "chore_gemm_nn": os.environ.get("PARSEC_MCA_chore_gemm_nn",
                                                   "default")},
    }), flush=True)
    del A, B, ctx


def step_kernel(args):
    from parsec_amd import _core

    s = args.size
    iters = max(3, int(20 * (2048.0 / s) ** 3))
    tf = _core.bench_dgemm_nn_hip(s, s, s, iters, args.impl)
    print(json.dumps({
        "metric": "TFLOP/s fp64 C -= A B (NN)",
        "value": round(tf, 2),
        "unit": "TFLOP/s",
        "higher_is_better": True,
        "dtype": "fp64",
        "config": {"m": s, "n": s, "k": s, "iters": iters,
                   "impl": args.impl},
    }), flush=True)


def drive(args):
    me = os.path.abspath(__file__)
    common = ["--n", str(args.n), "--nb", str(args.nb), "--steps",
              str(args.steps), "--warmup", str(args.warmup)]
    steps = []
    for size in (2048, 4096):
        for impl in ("rocblas", "hip"):
            steps.append((60, None, ["--step", "kernel", "--size", str(size),
                                     "--impl", impl]))
    for nrhs in ("nb", "n"):
        for chore in ("rocblas", "hip"):
            steps.append((300, chore, ["--step", "gels", "--nrhs", nrhs,
                                       *common]))
    for limit, chore, argv in steps:
        env = dict(os.environ)
        if chore:
            env["PARSEC_MCA_chore_gemm_nn"] = chore
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable,
                            me, *argv], env=env)
        if r.returncode != 0:
            print(f"bench_gels: step {argv} (chore_gemm_nn={chore}) ended "
                  f"with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--nb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step", choices=["gels", "kernel"])
    ap.add_argument("--nrhs", choices=["nb", "n"], default="nb")
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--impl", choices=["hip", "rocblas"], default="hip")
    args = ap.parse_args()
    if args.step == "gels":
        step_gels(args)
    elif args.step == "kernel":
        step_kernel(args)
    else:
        sys.exit(drive(args))


if __name__ == "__main__":
    main()
