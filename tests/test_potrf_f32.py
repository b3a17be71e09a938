"""insert_potrf_f32 (single-precision tile Cholesky) and insert_convert.

3 x 3 tiles of 256 at n = 768, 640 (a 128-row edge tile) and 386 (a 130-row
edge tile: the bounds-checked kernel and the library fallback of the TRSM
product). A = n I + S with S symmetric, entries uniform in [-0.5, 0.5],
rounded to float32, so cond(A) < 2.

Measured in float64 over the lower triangle:
    r(L) = max_ij |A - L L^T| / ((n+1) eps (|L| |L|^T))
The TRSM goes through an explicit inverse, so Higham's constant 1 cannot be
derived; the bound comes from a reference instead: r_ref of np.linalg.cholesky
on the same float32 matrix (LAPACK spotrf), and r(L) <= 4 max(r_ref, 1/(n+1)).
The 4 covers another summation order and the kappa(L)^2 < 2 term of the
product with the inverse.

The round trip fp64 fill -> convert -> potrf_f32 -> convert is held to
|L32 - L64|_F / |L64|_F <= 4 r_ref (n+1) eps against the fp64 insert_potrf.

The CPU cases run the float CPU chores in this process. The GPU cases run
this file as a script in one fresh process per selector setting (the
selectors are read once per process): all hip, and all rocblas.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float32).eps
NB = 256
SIZES = (768, 640, 386)
N_TRIP = 640


def _matrix(n):
    R = np.random.default_rng(1000 + n).uniform(-0.5, 0.5, (n, n))
    return (n * np.eye(n) + np.tril(R) + np.tril(R, -1).T).astype(np.float32)


def _tiles(n):
    mt = (n + NB - 1) // NB
    return [(i, j) for i in range(mt) for j in range(i + 1)]


def _get(M, n, dtype):
    """The lower tiles of M as an n x n array, through tile_bytes."""
    out = np.zeros((n, n), dtype=dtype)
    for i, j in _tiles(n):
        t = np.frombuffer(M.tile_bytes(i, j), dtype=dtype)
        t = t.reshape((NB, NB), order="F")
        out[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB] = \
            t[:M.tile_rows(i), :M.tile_cols(j)]
    return out


def _factor(pm, ctx, A):
    n = A.shape[0]
    M = pm.TiledMatrix(ctx, n, n, NB, NB, 1, 1, elem_size=4)
    for i, j in _tiles(n):
        t = np.zeros((NB, NB), dtype=np.float32)
        blk = A[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB]
        t[:blk.shape[0], :blk.shape[1]] = blk
        M.tile_bytes_set(i, j, t.tobytes(order="F"))
    tp = pm.Dtd(ctx)
    pm.insert_potrf_f32(tp, M)
    tp.wait()
    return _get(M, n, np.float32)


def _round_trip(pm, ctx, n):
    """(the fp64 fill, L through fp32 and back, the fp64 L)"""
    A64, B64 = (pm.TiledMatrix(ctx, n, n, NB, NB, 1, 1) for _ in range(2))
    A32 = pm.TiledMatrix(ctx, n, n, NB, NB, 1, 1, elem_size=4)
    tp = pm.Dtd(ctx)
    pm.insert_spd_fill(tp, A64, 42)
    tp.wait()
    fill = _get(A64, n, np.float64)
    tp = pm.Dtd(ctx)
    pm.insert_convert(tp, A64, A32)
    pm.insert_potrf_f32(tp, A32)
    pm.insert_convert(tp, A32, B64)
    pm.insert_potrf(tp, A64)
    tp.wait()
    return fill, _get(B64, n, np.float64), _get(A64, n, np.float64)


def _run_all(pm, ctx):
    out = {f"L{n}": _factor(pm, ctx, _matrix(n)) for n in SIZES}
    out["fill"], out["L32"], out["L64"] = _round_trip(pm, ctx, N_TRIP)
    return out


def _ratio(A, L):
    A, L = A.astype(np.float64), np.tril(L).astype(np.float64)
    n = A.shape[0]
    q = np.abs(A - L @ L.T) / ((n + 1) * EPS * (np.abs(L) @ np.abs(L).T))
    return np.tril(q).max()


def _check_factor(L, n, what):
    A = _matrix(n)
    assert np.linalg.cond(A.astype(np.float64)) < 2
    assert np.all(np.isfinite(np.tril(L))) and np.all(np.diag(L) > 0)
    r_ref, r = _ratio(A, np.linalg.cholesky(A)), _ratio(A, L)
    print(f"{what} n={n}: r = {r:.4f}, r_ref = {r_ref:.4f}")
    assert r <= 4 * max(r_ref, 1 / (n + 1))


def _check_round_trip(fill, L32, L64, what):
    n = fill.shape[0]
    A = (np.tril(fill) + np.tril(fill, -1).T).astype(np.float32)
    r_ref = _ratio(A, np.linalg.cholesky(A))
    L32, L64 = np.tril(L32), np.tril(L64)
    err = np.linalg.norm(L32 - L64) / np.linalg.norm(L64)
    print(f"{what} round trip n={n}: err = {err:.3e}, r_ref = {r_ref:.4f}")
    assert err <= 4 * r_ref * (n + 1) * EPS


@pytest.fixture(scope="module")
def cpu_results():
    import parsec_amd as pm
    ctx = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)  # CPU chores
    return _run_all(pm, ctx)


@pytest.mark.parametrize("n", SIZES)
def test_potrf_f32_cpu(cpu_results, n):
    _check_factor(cpu_results[f"L{n}"], n, "cpu")


def test_round_trip_cpu(cpu_results):
    _check_round_trip(cpu_results["fill"], cpu_results["L32"],
                      cpu_results["L64"], "cpu")


@pytest.fixture(scope="module")
def gpu_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("potrf_f32")
    procs = {}
    for impl in ("hip", "rocblas"):
        env = dict(os.environ)
        for sel in ("chore_ssyrk", "chore_strsm_inv", "chore_sgemm"):
            env["PARSEC_MCA_" + sel] = impl
        procs[impl] = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), str(d / impl)],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
            text=True)
    logs = {}
    for impl, proc in procs.items():  # reap both before judging either
        try:
            logs[impl], _ = proc.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            proc.kill()
            logs[impl], _ = proc.communicate()
    for impl, proc in procs.items():
        assert proc.returncode == 0, f"{impl}: {logs[impl]}"
    return {impl: np.load(str(d / impl) + ".npz") for impl in procs}


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("impl", ["hip", "rocblas"])
def test_potrf_f32_gpu(gpu_results, impl, n):
    _check_factor(gpu_results[impl][f"L{n}"], n, impl)


@pytest.mark.gpu
@pytest.mark.parametrize("impl", ["hip", "rocblas"])
def test_round_trip_gpu(gpu_results, impl):
    res = gpu_results[impl]
    _check_round_trip(res["fill"], res["L32"], res["L64"], impl)


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    import parsec_amd as pm
    ctx = pm.Context(nworkers=2, rank=0, world=1)
    assert ctx.has_gpu
    res = _run_all(pm, ctx)
    assert ctx.gpu_stats()["tasks"] > 0
    np.savez(sys.argv[1], **res)
    del ctx
