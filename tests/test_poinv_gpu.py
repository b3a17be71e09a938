"""insert_poinv on the GPU engine with each chore of its LAUUM phase.

  (n, nb) = (1024, 256)  full tiles, two 128-blocks a side
  (n, nb) = (1000, 192)  edge tiles of 40 rows, and 192 is no multiple of 128

chore_lauum and chore_gemm_tn are read once per process, so each setting
gets a fresh subprocess that inverts both sizes: chore_lauum=hip,
chore_lauum=rocblas, and chore_gemm_tn=hip (GEMM-TN on the hand kernel's
plain kind). The three run side by side. Each also runs insert_potri on a
factor whose diagonal tiles carry NaN above their diagonal. Every result
must match numpy.linalg.inv of the same fill to the tolerance of
test_gpu.py::test_gpu_posv_numerics (relative max error < 1e-10), and the two
chore_lauum values must agree with each other to the same tolerance.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1024, 256), (1000, 192))
TOL = 1e-10
RUNS = {
    "lauum_hip": {"PARSEC_MCA_chore_lauum": "hip"},
    "lauum_rocblas": {"PARSEC_MCA_chore_lauum": "rocblas"},
    "gemm_tn_hip": {"PARSEC_MCA_chore_gemm_tn": "hip"},
}

pytestmark = pytest.mark.gpu

_CODE = """
import sys
import numpy as np
sys.path.insert(0, {repo!r})
import parsec_amd as pm
ctx = pm.Context(nworkers=2, rank=0, world=1)
assert ctx.has_gpu
def lower(A):
    M = np.zeros((A.m, A.n))
    for i in range(A.mt):
        for j in range(i + 1):
            M[i * A.mb:i * A.mb + A.tile_rows(i),
              j * A.nb:j * A.nb + A.tile_cols(j)] = A.tile_numpy(i, j)
    return np.tril(M)
out = {{}}
for n, nb in {shapes!r}:
    A = pm.TiledMatrix(ctx, n, n, nb, nb, 1, 1, sym=True)
    tp = pm.Dtd(ctx); pm.insert_spd_fill(tp, A, 11); tp.wait()
    out["A%d" % n] = lower(A)
    tp = pm.Dtd(ctx); pm.insert_poinv(tp, A); tp.wait()
    out["X%d" % n] = lower(A)
    # potri on a factor whose diagonal tiles hold NaN above their diagonal
    tp = pm.Dtd(ctx); pm.insert_spd_fill(tp, A, 11); pm.insert_potrf(tp, A)
    tp.wait()
    for i in range(A.mt):
        t = A.tile_numpy(i, i)
        t[np.triu_indices_from(t, 1)] = np.nan
        A.tile_numpy_set(i, i, t)
    tp = pm.Dtd(ctx); pm.insert_potri(tp, A); tp.wait()
    out["P%d" % n] = lower(A)
    for i in range(A.mt):
        out["D%d_%d" % (n, i)] = A.tile_numpy(i, i)
    del A, tp
assert ctx.gpu_stats()["tasks"] > 0
np.savez({path!r}, **out)
del ctx
"""


def _start(env_extra, path):
    env = dict(os.environ)
    for name in ("PARSEC_MCA_chore_lauum", "PARSEC_MCA_chore_gemm_tn"):
        env.pop(name, None)
    env.update(env_extra)
    # a context reserves 85% of the free device memory by default, which
    # leaves the third of three concurrent ones nothing for its library
    # handles; these matrices take a few MB
    env["PARSEC_MCA_gpu_mem_limit_mb"] = "2048"
    code = _CODE.format(repo=REPO, shapes=SHAPES, path=path)
    return subprocess.Popen([sys.executable, "-c", code], env=env,
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                            text=True)


def _sym(Lo):
    return Lo + np.tril(Lo, -1).T


@pytest.fixture(scope="module")
def inverses(tmp_path_factory):
    """Every setting inverts both sizes once, the three processes side by
    side (most of a run is context start-up); every test reads these."""
    d = tmp_path_factory.mktemp("poinv_gpu")
    paths = {run: str(d / f"{run}.npz") for run in RUNS}
    procs = {run: _start(RUNS[run], p) for run, p in paths.items()}
    logs = {}
    for run, proc in procs.items():  # reap all before judging any
        try:
            logs[run], _ = proc.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            proc.kill()
            logs[run], _ = proc.communicate()
    for run, proc in procs.items():
        assert proc.returncode == 0, f"{run}: {logs[run]}"
    return {run: np.load(p) for run, p in paths.items()}


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("n,nb", SHAPES)
def test_gpu_poinv_vs_numpy(inverses, n, nb, run):
    Af = _sym(inverses[run][f"A{n}"])
    X = _sym(inverses[run][f"X{n}"])
    ref = np.linalg.inv(Af)
    err = np.abs(X - ref).max() / np.abs(ref).max()
    print(f"n={n} nb={nb} {run}: rel err {err:.3e}")
    assert err < TOL, err


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("n,nb", SHAPES)
def test_gpu_potri_diagonal_tile_rule(inverses, n, nb, run):
    """NaN above the diagonal of the factor's diagonal tiles reaches neither
    the inverse nor what the GPU chores leave in its place: zero or the
    symmetric value."""
    z = inverses[run]
    P = z[f"P{n}"]
    assert np.isfinite(P).all()
    ref = np.linalg.inv(_sym(z[f"A{n}"]))
    err = np.abs(_sym(P) - ref).max() / np.abs(ref).max()
    print(f"n={n} nb={nb} {run}: potri over NaN, rel err {err:.3e}")
    assert err < TOL, err
    for i in range(-(-n // nb)):
        t = z[f"D{n}_{i}"]
        iu = np.triu_indices_from(t, 1)
        up, mirror = t[iu], t.T[iu]
        assert np.isfinite(up).all(), f"tile {i}: NaN above the diagonal"
        assert np.all((up == 0.0) | (up == mirror)), f"tile {i}"


@pytest.mark.parametrize("n,nb", SHAPES)
def test_gpu_poinv_chores_agree(inverses, n, nb):
    Xh = inverses["lauum_hip"][f"X{n}"]
    Xr = inverses["lauum_rocblas"][f"X{n}"]
    err = np.abs(Xh - Xr).max() / np.abs(Xr).max()
    print(f"n={n} nb={nb}: hip vs rocblas rel diff {err:.3e}")
    assert err < TOL, err
