#!/usr/bin/env python3
"""Flagship benchmark: whole-node tiled Cholesky fp64 (BASELINE.json metric).

One step = one full tiled Cholesky factorization (DTD DAG: POTRF/TRSM/SYRK/
GEMM tile tasks on the HIP engine) of a synthetic SPD fp64 matrix of order
--matrix-size, preceded by its on-GPU re-fill (the factorization is in
place; the fill is part of the timed step and costs <1% of it).

Launched by the driver as:
  python bench.py --gpus 1 ...                      (single rank)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N ... (one rank per GPU, RCCL)

Rank 0 prints one JSON line with the whole-job aggregate GFLOP/s.

A plain run sets up, warms up, times --steps steps and prints that line.
--dump-outputs DIR also writes a fixed sample of the factor the last timed
step produced, for comparing two builds output for output (the inputs are
the same seeded fill on every run). --full is where measurements beyond
the headline figure belong; there are none at present.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def pick_grid(world):
    return {1: (1, 1), 2: (2, 1), 4: (2, 2), 8: (2, 4)}.get(
        world, (1, world))


def sample_plan(n, nb):
    """The fixed, seeded sample of the factor that --dump-outputs keeps:
    (bi, bj, rows, cols) for every diagonal nb x nb block and for up to 12
    seeded off-diagonal blocks of the lower triangle, with up to 256 seeded
    row and column indices inside each block."""
    import numpy as np

    rng = np.random.default_rng(20240607)
    nblk = (n + nb - 1) // nb
    off = [(i, j) for i in range(nblk) for j in range(i)]
    picks = rng.permutation(len(off))[:12]
    blocks = [(b, b) for b in range(nblk)] + sorted(off[k] for k in picks)
    plan = []
    for bi, bj in blocks:
        ri = np.sort(rng.permutation(min(nb, n - bi * nb))[:256])
        ci = np.sort(rng.permutation(min(nb, n - bj * nb))[:256])
        plan.append((bi, bj, ri, ci))
    return plan


def dump_outputs(A, n, nb, algo, outdir):
    """Write what the last timed step left in A (the Cholesky factor L) as
    float64 .npy files. The factor is far larger than a dump may be, so
    only sample_plan()'s entries are kept (L_block_<bi>_<bj>.npy), plus the
    whole diagonal of L (L_diag_<bi>.npy): ~12 MB in all at the default
    size. Entries above the diagonal are not part of L and are written as
    zero. Each rank writes the blocks it owns."""
    import numpy as np

    os.makedirs(outdir, exist_ok=True)
    for bi, bj, ri, ci in sample_plan(n, nb):
        # panel storage keeps block column bj as one n x nb tile
        tm, r0 = (0, bi * nb) if algo == "panel" else (bi, 0)
        if not A.is_local(tm, bj):
            continue
        t = A.tile_numpy(tm, bj)
        s = t[np.ix_(r0 + ri, ci)]
        if bi == bj:
            s = np.where(ri[:, None] >= ci[None, :], s, 0.0)
            rows = min(nb, n - bi * nb)
            d = np.ascontiguousarray(np.diagonal(t[r0:r0 + rows]))
            np.save(os.path.join(outdir, f"L_diag_{bi:03d}.npy"), d)
        np.save(os.path.join(outdir, f"L_block_{bi:03d}_{bj:03d}.npy"),
                np.ascontiguousarray(s, dtype=np.float64))
        del t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--matrix-size", type=int, default=80000)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--chore-gemm", type=str, default=os.environ.get(
        "PARSEC_MCA_chore_gemm", "rocblas"), choices=["rocblas", "hip"])
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--algo", type=str, default="auto",
                    choices=["auto", "tile", "panel"])
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write a fixed sample of the "
                         "last step's factor L to DIR/<name>.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure (none yet: the plain run is the whole "
                         "benchmark)")
    args = ap.parse_args()

    import parsec_amd as pm

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    has_gpu = pm.hip_device_count() > 0
    n, nb = args.matrix_size, args.tile
    if not has_gpu:
        # debug-only path for CPU containers; GPU boxes run the real config
        n, nb = 1024, 128
    pm.param_set("chore_gemm", args.chore_gemm)

    ctx = pm.init_distributed(nworkers=args.workers)
    assert ctx.world == world
    # panel granularity (one tall dgemm per update) maximizes per-kernel
    # efficiency on one GPU; tile granularity exposes the parallelism the
    # multi-GPU strong-scaling run needs.
    # measured: tile granularity wins at every world size (panel's tall
    # dgemms run below the square-tile rate and its critical path idles
    # the GPU ~40%; see profiles/ and docs/DESIGN.md)
    algo = args.algo
    if algo == "auto":
        algo = "tile"
    if algo == "panel":
        # big kernels keep the chip full from one bulk stream; extra
        # streams only co-schedule kernels below their solo rate
        pm.param_set("gpu_exec_streams", "2")
    p, q = pick_grid(world)
    if algo == "panel":
        p, q = 1, world
        A = pm.TiledMatrix(ctx, n, n, n, nb, p, q)
    else:
        A = pm.TiledMatrix(ctx, n, n, nb, nb, p, q)

    use_torch_dist = world > 1
    if use_torch_dist:
        import torch
        import torch.distributed as dist
        if has_gpu and torch.cuda.is_available():
            torch.cuda.set_device(
                int(os.environ.get("LOCAL_RANK", rank))
                % torch.cuda.device_count())

    def barrier_sync():
        ctx.gpu_sync()
        if has_gpu:
            try:
                import torch
                if torch.cuda.is_available():
                    torch.cuda.synchronize()
            except Exception:
                pass
        if use_torch_dist:
            dist.barrier()
        else:
            ctx.barrier()

    def run_steps(nsteps):
        # All steps share one taskpool: the DTD chaining orders step i+1's
        # re-fill after step i's last reads (WAR), so the tail of one
        # factorization overlaps the head of the next — each step still
        # executes in full.
        tp = pm.Dtd(ctx)
        for _ in range(nsteps):
            if algo == "panel":
                pm.insert_panel_fill(tp, A, 42)
                pm.insert_potrf_panel(tp, A)
            else:
                pm.insert_spd_fill(tp, A, 42)
                pm.insert_potrf(tp, A)
        tp.wait()

    if args.warmup:
        run_steps(args.warmup)
    barrier_sync()
    t0 = time.perf_counter()
    run_steps(args.steps)
    barrier_sync()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if use_torch_dist:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs:
        dump_outputs(A, n, nb, algo, args.dump_outputs)

    flops_per_step = n**3 / 3.0 + n**2 / 2.0 + n / 6.0
    value = args.steps * flops_per_step / elapsed / 1e9  # GFLOP/s whole job
    if rank == 0:
        nlabel = f"N={n//1000}k" if n % 1000 == 0 else f"N={n}"
        out = {
            "metric": f"GFLOP/s (whole node) tiled Cholesky {nlabel}",
            "value": round(value, 1),
            "unit": "GFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 2),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "fp64",
            "data": "synthetic",
            "config": {
                "model": "tiled_cholesky_dpotrf",
                "N": n,
                "tile": nb,
                "parallelism": f"dtd-{algo}-p{p}q{q}",
                "chore_gemm": args.chore_gemm,
                "gpu": has_gpu,
            },
        }
        print(json.dumps(out), flush=True)
    if use_torch_dist:
        import torch.distributed as dist2
        dist2.destroy_process_group()
    del A
    del ctx


if __name__ == "__main__":
    main()
