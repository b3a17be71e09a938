"""Blocked tile POTRF with the hand triangular SYRK as its trailing update.

A single tile goes through the normal DTD path (insert_spd_fill, then
insert_potrf) on the GPU:
  n = 384  every trailing size is a multiple of 128: the glds (v3) update
  n = 328  trailing sizes 200 and 72, last panel 72: the bounds-checked path
Each size runs with chore_potrf_syrk=hip and =rocblas. The parameter is read
once per process, so each value gets a fresh subprocess (which factors both
sizes). tril(L) must match numpy.linalg.cholesky of the same fill to the
tolerance of test_gpu.py::test_gpu_cholesky_numerics (max abs error < 1e-8),
and the two chores must agree with each other to the same tolerance.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (384, 328)
TOL = 1e-8

pytestmark = pytest.mark.gpu

_CODE = """
import sys
import numpy as np
sys.path.insert(0, {repo!r})
import parsec_amd as pm
ctx = pm.Context(nworkers=2, rank=0, world=1)
assert ctx.has_gpu
out = {{}}
for n in {sizes!r}:
    A = pm.TiledMatrix(ctx, n, n, n, n, 1, 1)
    assert A.mt == 1 and A.nt == 1
    tp = pm.Dtd(ctx); pm.insert_spd_fill(tp, A, 42); tp.wait()
    out["M%d" % n] = np.array(A.tile_numpy(0, 0))
    tp = pm.Dtd(ctx); pm.insert_potrf(tp, A); tp.wait()
    out["L%d" % n] = np.array(A.tile_numpy(0, 0))
    del A
assert ctx.gpu_stats()["tasks"] > 0
np.savez({path!r}, **out)
del ctx
"""


def _start(chore, path):
    env = dict(os.environ)
    env["PARSEC_MCA_chore_potrf_syrk"] = chore
    code = _CODE.format(repo=REPO, sizes=SIZES, path=path)
    return subprocess.Popen([sys.executable, "-c", code], env=env,
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                            text=True)


@pytest.fixture(scope="module")
def factors(tmp_path_factory):
    """Both chores factor both sizes once, side by side in two processes
    (most of a run is context start-up); every test reads these results."""
    d = tmp_path_factory.mktemp("potrf_tile")
    paths = {chore: str(d / f"{chore}.npz") for chore in ("hip", "rocblas")}
    procs = {chore: _start(chore, p) for chore, p in paths.items()}
    logs = {}
    for chore, proc in procs.items():  # reap both before judging either
        try:
            logs[chore], _ = proc.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            proc.kill()
            logs[chore], _ = proc.communicate()
    for chore, proc in procs.items():
        assert proc.returncode == 0, f"{chore}: {logs[chore]}"
    return {chore: np.load(p) for chore, p in paths.items()}


@pytest.mark.parametrize("chore", ["hip", "rocblas"])
@pytest.mark.parametrize("n", SIZES)
def test_tile_potrf_vs_numpy(factors, n, chore):
    M = factors[chore][f"M{n}"]
    assert M.shape == (n, n)
    M = np.tril(M) + np.tril(M, -1).T
    L0 = np.linalg.cholesky(M)
    L = np.tril(factors[chore][f"L{n}"])
    err = np.abs(L - L0).max()
    print(f"n={n} chore_potrf_syrk={chore}: max err {err:.3e}")
    assert err < TOL, f"max err {err}"


@pytest.mark.parametrize("n", SIZES)
def test_tile_potrf_chores_agree(factors, n):
    Lh = np.tril(factors["hip"][f"L{n}"])
    Lr = np.tril(factors["rocblas"][f"L{n}"])
    err = np.abs(Lh - Lr).max()
    print(f"n={n}: hip vs rocblas max diff {err:.3e}")
    assert err < TOL, f"max diff {err}"
