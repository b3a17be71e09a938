#!/usr/bin/env python3
"""SPD inverse benchmark: whole-job TFLOP/s of insert_poinv (potrf + trtri +
lauum in one taskpool) or of one of its parts on the DTD engine.

Only the chosen operation is timed; what it needs as input (the factor for
potri and trtri, W = L^-1 for lauum) is prepared before the clock starts.
Flop counts: N^3 poinv, 2N^3/3 potri, N^3/3 trtri or lauum. `--op posv` is
there for scale: insert_posv against a dense N x N right-hand side, the only
route to A^-1 without these builders, counted as the same N^3 useful flops
(it executes 7N^3/3). PARSEC_MCA_chore_lauum / chore_gemm_tn select the
LAUUM-phase chores."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOPS = {"poinv": 1.0, "potri": 2.0 / 3.0, "trtri": 1.0 / 3.0,
         "lauum": 1.0 / 3.0, "posv": 1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--nb", type=int, default=2048)
    ap.add_argument("--op", choices=sorted(FLOPS), default="poinv")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import parsec_amd as pm

    has_gpu = pm.hip_device_count() > 0
    n, nb = (args.n, args.nb) if has_gpu else (512, 128)
    ctx = pm.init_distributed(nworkers=4)
    A = pm.TiledMatrix(ctx, n, n, nb, nb, 1, 1, sym=True)
    B = pm.TiledMatrix(ctx, n, n, nb, nb, 1, 1) if args.op == "posv" else None

    def step():
        """One prepared, then timed, run of the operation; returns seconds."""
        tp = pm.Dtd(ctx)
        pm.insert_spd_fill(tp, A, 11)
        if B is not None:
            pm.insert_full_fill(tp, B, 5)
        if args.op in ("potri", "trtri", "lauum"):
            pm.insert_potrf(tp, A)
        if args.op == "lauum":
            pm.insert_trtri(tp, A)
        tp.wait()
        ctx.gpu_sync()
        t0 = time.perf_counter()
        tp = pm.Dtd(ctx)
        if args.op == "posv":
            pm.insert_posv(tp, A, B)
        else:
            getattr(pm, "insert_" + args.op)(tp, A)
        tp.wait()
        ctx.gpu_sync()
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        step()
    times = sorted(step() for _ in range(args.steps))
    med = times[len(times) // 2]
    flops = FLOPS[args.op] * float(n) ** 3
    print(json.dumps({
        "metric": f"TFLOP/s SPD inverse ({args.op})",
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
        "config": {"model": "spd_inverse_" + args.op, "N": n, "tile": nb,
                   "chore_lauum": os.environ.get("PARSEC_MCA_chore_lauum",
                                                 "default"),
                   "chore_gemm_tn": os.environ.get("PARSEC_MCA_chore_gemm_tn",
                                                   "default")},
    }), flush=True)
    del A, B, ctx


if __name__ == "__main__":
    main()
