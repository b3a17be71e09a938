"""Inputs and the solve step of test_gels.py, and its subprocess worker.

test_gels.py imports make_input/solve_tiles/assemble; run as a script it
solves the named cases in a context of its own (another QR tree, another
chore setting, or one rank of several) and writes its local tiles to an .npz
for the parent to assemble and check:

    _gels_worker.py OUT.npz CASE[,CASE...] [gesv]

Environment: GELS_GPU=1 for a GPU context, GELS_TREE=binary for the binary
QR tree, RANK/WORLD_SIZE/PORT for a P x 1 grid over the TCP engine.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import parsec_amd as pm  # noqa: E402

# m, n, nrhs, tile size of A (and of B's columns), kind of A
CASES = {
    # one full and one 32-wide column tile of B
    "tall_cpu": (320, 192, 96, 64, "gauss"),
    "square_cpu": (256, 256, 96, 64, "gauss"),
    "illcond": (256, 256, 96, 64, "logspace"),
    "zeroblock": (256, 256, 96, 64, "zeroblock"),
    # the tile no multiple of 128; one full and one 64-wide column tile of B
    "tall_gpu": (768, 576, 256, 192, "gauss"),
    "square_gpu": (576, 576, 256, 192, "gauss"),
    # the input of test_qr.py's DAG tests
    "qr_dag": (576, 576, 64, 192, "qr_dag"),
}


def make_input(case):
    m, n, nrhs, nb, kind = CASES[case]
    rng = np.random.default_rng(17)
    if kind == "logspace":
        # singular values from 1 down to 1e-10
        U, _ = np.linalg.qr(rng.standard_normal((m, n)))
        V, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A0 = (U * np.logspace(0, -10, n)) @ V.T
    elif kind == "qr_dag":
        A0 = np.random.default_rng(11).standard_normal((m, n))
    else:
        A0 = rng.standard_normal((m, n))
        if kind == "zeroblock":
            A0[:nb, :nb] = 0.0  # a zero pivot for LU without pivoting
    B0 = rng.standard_normal((m, nrhs))
    return A0, B0


def _scatter(M, M0):
    for i in range(M.mt):
        for j in range(M.nt):
            if M.is_local(i, j):
                M.tile_numpy_set(i, j, M0[i * M.mb:i * M.mb + M.tile_rows(i),
                                          j * M.nb:j * M.nb + M.tile_cols(j)])


def _local_tiles(M, name):
    return {f"{name}_{i}_{j}": M.tile_numpy(i, j)
            for i in range(M.mt) for j in range(M.nt) if M.is_local(i, j)}


def solve_tiles(ctx, case, p=1, q=1, factor_only=False):
    """insert_gels (or insert_geqrf alone) on the case's input over a p x q
    grid; this rank's tiles of A and B afterwards, keyed A_i_j / B_i_j."""
    m, n, nrhs, nb, _ = CASES[case]
    A0, B0 = make_input(case)
    A = pm.TiledMatrix(ctx, m, n, nb, nb, p, q)
    B = pm.TiledMatrix(ctx, m, nrhs, nb, nb, p, q)
    _scatter(A, A0)
    _scatter(B, B0)
    tp = pm.Dtd(ctx, "gels")
    if factor_only:
        pm.insert_geqrf(tp, A)
    else:
        pm.insert_gels(tp, A, B)
    tp.flush_all(A)
    tp.flush_all(B)
    tp.wait()
    if p * q > 1:
        ctx.barrier()
    out = {**_local_tiles(A, "A"), **_local_tiles(B, "B")}
    del A, B
    return out


def assemble(case, tiles):
    """(A, B) after the solve from every rank's tiles together."""
    m, n, nrhs, nb, _ = CASES[case]
    full = {"A": np.full((m, n), np.nan), "B": np.full((m, nrhs), np.nan)}
    for key, t in tiles.items():
        name, i, j = key.split("_")
        i, j = int(i) * nb, int(j) * nb
        full[name][i:i + t.shape[0], j:j + t.shape[1]] = t
    return full["A"], full["B"]


def gesv_nopiv_err(ctx):
    """The diagonally dominant problem and the error measure of
    test_lu.py::test_gesv_nopiv_vs_numpy."""
    n, nb, nrhs = 320, 64, 96
    A = pm.TiledMatrix(ctx, n, n, nb, nb, 1, 1)
    B = pm.TiledMatrix(ctx, n, nrhs, nb, nb, 1, 1)
    tp = pm.Dtd(ctx)
    pm.insert_full_fill(tp, A, 9)
    pm.insert_full_fill(tp, B, 5)
    pm.insert_apply_scale(tp, A, 0.01, 0)
    tp.wait()
    for i in range(A.mt):
        t = A.tile_numpy(i, i)
        t += np.eye(A.tile_rows(i)) * 50.0
        A.tile_numpy_set(i, i, t)

    def full(M):
        out = np.zeros((M.m, M.n))
        for i in range(M.mt):
            for j in range(M.nt):
                out[i * M.mb:i * M.mb + M.tile_rows(i),
                    j * M.nb:j * M.nb + M.tile_cols(j)] = M.tile_numpy(i, j)
        return out

    Af, Bf = full(A), full(B)
    tp2 = pm.Dtd(ctx)
    pm.insert_gesv_nopiv(tp2, A, B)
    tp2.wait()
    ref = np.linalg.solve(Af, Bf)
    err = abs(full(B) - ref).max() / abs(ref).max()
    del A, B
    return err


def main():
    out, cases = sys.argv[1], sys.argv[2].split(",")
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    use_gpu = os.environ.get("GELS_GPU") == "1"
    if os.environ.get("GELS_TREE"):
        pm.param_set("qr_tree", os.environ["GELS_TREE"])
    if world > 1:
        pm.param_set("comm_base_port", os.environ["PORT"])
        ctx = pm.Context(nworkers=2, rank=rank, world=world, comm="tcp",
                         gpu=-2)
    else:
        ctx = pm.Context(nworkers=2, rank=0, world=1,
                         gpu=(-1 if use_gpu else -2))
    assert ctx.has_gpu == use_gpu
    res = {}
    for case in cases:
        tiles = solve_tiles(ctx, case, p=world, q=1)
        res.update({f"{case}:{k}": v for k, v in tiles.items()})
    if "gesv" in sys.argv[3:]:
        res["gesv_err"] = np.array(gesv_nopiv_err(ctx))
    if use_gpu:
        res["gpu_tasks"] = np.array(ctx.gpu_stats()["tasks"])
        # asked after the DAGs ran: what their C -= A B tasks took
        res["chore_gemm_nn"] = np.array(pm._core.chore_gemm_nn())
    np.savez(out, **res)
    if world > 1:
        ctx.barrier()
    print("GELS_WORKER_OK", rank)
    del ctx


if __name__ == "__main__":
    main()
