#!/usr/bin/env python3
"""Single-precision tile Cholesky benchmark: whole-job TFLOP/s of
insert_potrf_f32 beside the fp64 insert_potrf, same process, same matrix.

Each step fills the fp64 SPD matrix, converts it to fp32 (insert_convert),
then times the two factorizations one after the other, fp32 first on even
steps and fp64 first on odd ones. The fill and the conversion are outside the
clock. Both count N^3/3 flops. PARSEC_MCA_chore_sgemm / chore_ssyrk /
chore_strsm_inv select the fp32 chores (read once per process: compare
settings across runs of this script)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SELECTORS = ("chore_sgemm", "chore_ssyrk", "chore_strsm_inv")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--nb", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import parsec_amd as pm

    has_gpu = pm.hip_device_count() > 0
    n, nb = (args.n, args.nb) if has_gpu else (512, 128)
    ctx = pm.init_distributed(nworkers=4)
    A64 = pm.TiledMatrix(ctx, n, n, nb, nb, 1, 1)
    A32 = pm.TiledMatrix(ctx, n, n, nb, nb, 1, 1, elem_size=4)

    def timed(insert, A):
        ctx.gpu_sync()
        t0 = time.perf_counter()
        tp = pm.Dtd(ctx)
        insert(tp, A)
        tp.wait()
        ctx.gpu_sync()
        return time.perf_counter() - t0

    def step(i):
        tp = pm.Dtd(ctx)
        pm.insert_spd_fill(tp, A64, 11)
        pm.insert_convert(tp, A64, A32)
        tp.wait()
        runs = [("fp32", pm.insert_potrf_f32, A32), ("fp64", pm.insert_potrf, A64)]
        return {name: timed(ins, A) for name, ins, A in runs[::1 - 2 * (i % 2)]}

    for i in range(args.warmup):
        step(i)
    steps = [step(i) for i in range(args.steps)]
    flops = float(n) ** 3 / 3
    med = {k: sorted(s[k] for s in steps)[len(steps) // 2] for k in ("fp32", "fp64")}
    print(json.dumps({
        "metric": "TFLOP/s Cholesky fp32 (insert_potrf_f32)",
        "value": round(flops / med["fp32"] / 1e12, 2),
        "unit": "TFLOP/s",
        "fp64_same_run": round(flops / med["fp64"] / 1e12, 2),
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": {k: round(v * 1e3, 2) for k, v in med.items()},
        "ms_all_steps": {k: [round(s[k] * 1e3, 2) for s in steps] for k in med},
        "higher_is_better": True,
        "dtype": "fp32",
        "data": "synthetic",
        "config": {"model": "cholesky_f32", "N": n, "tile": nb,
                   **{s: os.environ.get("PARSEC_MCA_" + s, "default")
                      for s in SELECTORS}},
    }), flush=True)
    del A64, A32, ctx


if __name__ == "__main__":
    main()
