"""SPD inverse (insert_trtri / insert_lauum / insert_potri / insert_poinv)
vs NumPy on the CPU chores, the numerics oracle of the family: the context
is created without a device wherever the tests run (test_poinv_gpu.py
covers the GPU chores).

Tolerance: relative max error < 1e-11, that of test_posv_vs_numpy. The fill
is diagonally dominant (cond ~ 1), and a NumPy emulation of the same tile
algorithm stays near 1e-15 on these sizes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import parsec_amd as pm
from conftest import port_base

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-11
SHAPES = [(320, 64), (200, 64), (192, 48)]


@pytest.fixture(scope="module")
def ctx():
    c = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)
    assert not c.has_gpu
    yield c
    del c


def _lower(A):
    """The lower tiles of A as a dense matrix (zeros above the diagonal)."""
    M = np.zeros((A.m, A.n))
    for i in range(A.mt):
        for j in range(i + 1):
            M[i * A.mb:i * A.mb + A.tile_rows(i),
              j * A.nb:j * A.nb + A.tile_cols(j)] = A.tile_numpy(i, j)
    return np.tril(M)


def _sym(Lo):
    return Lo + np.tril(Lo, -1).T


def _set_lower(A, M):
    """Write the lower tiles of A from M; diagonal tiles get NaN above their
    diagonal, which nothing may read."""
    for i in range(A.mt):
        for j in range(i + 1):
            t = M[i * A.mb:i * A.mb + A.tile_rows(i),
                  j * A.nb:j * A.nb + A.tile_cols(j)].copy()
            if i == j:
                t[np.triu_indices_from(t, 1)] = np.nan
            A.tile_numpy_set(i, j, t)


def _filled(ctx, n, nb, sym):
    A = pm.TiledMatrix(ctx, n, n, nb, nb, 1, 1, sym=sym)
    tp = pm.Dtd(ctx)
    pm.insert_spd_fill(tp, A, 11)
    tp.wait()
    return A, _sym(_lower(A))


def _relerr(X, ref):
    return np.abs(X - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_poinv_vs_numpy(ctx, n, nb, sym):
    A, Af = _filled(ctx, n, nb, sym)
    tp = pm.Dtd(ctx)
    pm.insert_poinv(tp, A)
    tp.wait()
    ref = np.linalg.inv(Af)
    err = _relerr(_sym(_lower(A)), ref)
    print(f"poinv n={n} nb={nb} sym={sym}: rel err {err:.3e}")
    assert err < TOL, err


@pytest.mark.parametrize("n,nb", SHAPES)
def test_potri_matches_poinv(ctx, n, nb):
    A, Af = _filled(ctx, n, nb, True)
    B, _ = _filled(ctx, n, nb, True)
    tp = pm.Dtd(ctx)
    pm.insert_potrf(tp, A)
    tp.wait()
    tp = pm.Dtd(ctx)
    pm.insert_potri(tp, A)
    pm.insert_poinv(tp, B)
    tp.wait()
    ref = np.linalg.inv(Af)
    X, Y = _sym(_lower(A)), _sym(_lower(B))
    print(f"potri n={n} nb={nb}: rel err {_relerr(X, ref):.3e}, "
          f"vs poinv {_relerr(X, Y):.3e}")
    assert _relerr(X, ref) < TOL
    assert _relerr(X, Y) < TOL


@pytest.mark.parametrize("n,nb", SHAPES)
def test_trtri_vs_numpy(ctx, n, nb):
    A, Af = _filled(ctx, n, nb, True)
    L = np.linalg.cholesky(Af)
    _set_lower(A, L)
    tp = pm.Dtd(ctx)
    pm.insert_trtri(tp, A)
    tp.wait()
    ref = np.linalg.inv(L)
    err = _relerr(_lower(A), ref)
    print(f"trtri n={n} nb={nb}: rel err {err:.3e}")
    assert err < TOL, err


@pytest.mark.parametrize("n,nb", SHAPES)
def test_lauum_vs_numpy(ctx, n, nb):
    A, Af = _filled(ctx, n, nb, True)
    W = np.linalg.inv(np.linalg.cholesky(Af))
    _set_lower(A, np.tril(W))
    tp = pm.Dtd(ctx)
    pm.insert_lauum(tp, A)
    tp.wait()
    ref = np.tril(W).T @ np.tril(W)
    err = _relerr(_sym(_lower(A)), ref)
    print(f"lauum n={n} nb={nb}: rel err {err:.3e}")
    assert err < TOL, err


@pytest.mark.parametrize("n,nb", SHAPES)
def test_potri_diagonal_tile_rule(ctx, n, nb):
    """The strict upper triangle of a diagonal tile is junk on entry: NaN
    there reaches neither the result nor what potri leaves in its place,
    which is zero or the symmetric value."""
    A, Af = _filled(ctx, n, nb, True)
    tp = pm.Dtd(ctx)
    pm.insert_potrf(tp, A)
    tp.wait()
    for i in range(A.mt):
        t = A.tile_numpy(i, i)
        t[np.triu_indices_from(t, 1)] = np.nan
        A.tile_numpy_set(i, i, t)
    tp = pm.Dtd(ctx)
    pm.insert_potri(tp, A)
    tp.wait()
    Lo = _lower(A)
    assert np.isfinite(Lo).all()
    err = _relerr(_sym(Lo), np.linalg.inv(Af))
    print(f"potri with NaN above the diagonal n={n} nb={nb}: rel err {err:.3e}")
    assert err < TOL, err
    for i in range(A.mt):
        t = A.tile_numpy(i, i)
        iu = np.triu_indices_from(t, 1)
        up, mirror = t[iu], t.T[iu]
        assert np.isfinite(up).all(), f"tile {i}: NaN above the diagonal"
        assert np.all((up == 0.0) | (up == mirror)), f"tile {i}"


def test_params_registered(ctx):
    A, _ = _filled(ctx, 128, 64, True)
    tp = pm.Dtd(ctx)
    pm.insert_poinv(tp, A)
    tp.wait()
    dump = pm.param_dump()
    assert "chore_lauum" in dump and "chore_gemm_tn" in dump


_WORLD2 = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["PARSEC_REPO"])
import parsec_amd as pm
rank = int(os.environ["RANK"])
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=2, comm="tcp", gpu=-2)
n, nb = 256, 64
A = pm.TiledMatrix(ctx, n, n, nb, nb, 2, 1, sym=True)
tp = pm.Dtd(ctx)
pm.insert_spd_fill(tp, A, 11)
tp.wait()
out = {}
for i in range(A.mt):
    for j in range(i + 1):
        if A.is_local(i, j):
            out[f"a_{i}_{j}"] = A.tile_numpy(i, j)
tp2 = pm.Dtd(ctx)
pm.insert_poinv(tp2, A)
tp2.wait()
tp2.flush_all(A)
for i in range(A.mt):
    for j in range(i + 1):
        if A.is_local(i, j):
            out[f"x_{i}_{j}"] = A.tile_numpy(i, j)
np.savez(os.path.join(os.environ["OUT"], f"poinv{rank}.npz"), **out)
ctx.barrier()
del A, tp, tp2, ctx
print("POINV_RANK_OK", rank)
"""


def test_distributed_poinv(tmp_path):
    """World-2 insert_poinv over the TCP engine on a 2x1 grid: the inverse
    assembled from both ranks matches numpy."""
    world, n, nb = 2, 256, 64
    port = port_base(39)
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world), PORT=str(port),
                   OUT=str(tmp_path), PARSEC_REPO=os.path.dirname(HERE))
        procs.append(subprocess.Popen([sys.executable, "-c", _WORLD2], env=env,
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=180)[0])
    finally:
        for pr in procs:  # a dead rank leaves its peer blocked on it
            if pr.poll() is None:
                pr.kill()
                pr.communicate()
    for pr, out in zip(procs, outs):
        assert pr.returncode == 0 and b"POINV_RANK_OK" in out, out.decode()
    Af = np.zeros((n, n))
    X = np.zeros((n, n))
    for r in range(world):
        z = np.load(os.path.join(tmp_path, f"poinv{r}.npz"))
        for key in z.files:
            kind, i, j = key.split("_")
            i, j = int(i), int(j)
            dst = Af if kind == "a" else X
            dst[i * nb:(i + 1) * nb, j * nb:(j + 1) * nb] = z[key]
    Af, X = _sym(np.tril(Af)), _sym(np.tril(X))
    err = _relerr(X, np.linalg.inv(Af))
    print(f"distributed poinv: rel err {err:.3e}")
    assert err < TOL, err
