"""k_dgemm_nt_v4 (the ring-pipelined full-tile kernel) against k_dgemm_nt_v3
and NumPy, for its three kinds: GEMM, SYRK and the TRSM product.

v4 keeps v3's block shape, fragment map and ascending-k accumulation and
changes only how K-tiles are staged, so v4 against v3 from the same build is
np.array_equal on the whole buffer, padding rows included: any difference is
a bug. v4 is also held to the componentwise bounds of test_dgemm_kernel.py
(2 (k+1) eps (|C| + |A| |B|^T)) and test_trmm_kernel.py
(2 n eps (|B| |W|^T)) against float64 NumPy.

S and BKD are the ring's slot count and K-tile depth (V4_S and V4_BK in
src/kernels_hip.cpp). The K sizes BKD * {1, 2, S-1, S, S+1, 2S+1} cover
fewer tiles than the prefetch distance, exactly one ring, a wrap and the
drain; k must also be a multiple of 16 to reach a full-tile kernel at all,
which every one of these is at BKD = 16.

The DAG-level cases factor 3 x 3 tiles of 256, 640 = 256 + 256 + 128 (a
128-row edge tile) and 386 = 256 + 130, in one fresh process per kernel:
the parameter is read once per process. Every tile must be byte-equal.
n = 386 is also the TRSM product's non-qualifying case: launch_dtrmm_rlt has
no bounds-checked kernel behind it and refuses such a shape outright, so the
place where a 130-row product is sent elsewhere (to the library dgemm) is the
TRSM tile task, and that must not depend on the selector.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from parsec_amd import _core

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
BLK = 128
SENTINEL = -3.0
S, BKD = 3, 16
KS = sorted({BKD * t for t in (1, 2, S - 1, S, S + 1, 2 * S + 1)})


def _padded(M, ld, fill=SENTINEL):
    """Column-major buffer with leading dimension ld >= rows, flattened."""
    rows, cols = M.shape
    buf = np.full((ld, cols), fill, dtype=np.float64, order="F")
    buf[:rows, :] = M
    return buf.ravel(order="F")


def _gemm_bound_ok(out, C, A, B, k, mask, what):
    ref = C - A @ B.T
    bound = 2 * (k + 1) * EPS * (np.abs(C) + np.abs(A) @ np.abs(B).T)
    diff = np.abs(out - ref)
    print(f"{what}: max |C-ref| = {diff[mask].max():.3e}, "
          f"max diff/bound = {(diff[mask] / bound[mask]).max():.3e}")
    assert np.all(np.isfinite(out[mask]))
    assert np.all(diff[mask] <= bound[mask])


def _gemm(m, n, k, kernel, lda=None, ldb=None, ldc=None, seed=11):
    lda, ldb, ldc = lda or m, ldb or n, ldc or m
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, k))
    B = rng.standard_normal((n, k))
    C = rng.standard_normal((m, n))
    cbuf = _padded(C, ldc)
    _core.dgemm_nt_hip(_padded(A, lda), _padded(B, ldb), cbuf, m, n, k,
                       lda, ldb, ldc, kernel=kernel)
    return cbuf.reshape((ldc, n), order="F"), (A, B, C)


def _check_gemm(m, n, k, **ld):
    out4, (A, B, C) = _gemm(m, n, k, 4, **ld)
    out3, _ = _gemm(m, n, k, 3, **ld)
    assert np.array_equal(out4, out3)
    _gemm_bound_ok(out4[:m, :], C, A, B, k, np.ones((m, n), dtype=bool),
                   f"gemm v4 m={m} n={n} k={k} {ld}")
    assert np.all(out4[m:, :] == SENTINEL)
    return out4


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m,n", [(128, 128), (256, 384)])
def test_gemm_v4(m, n, k):
    _check_gemm(m, n, k)


def test_gemm_v4_padded_ld():
    m, n = 256, 384
    _check_gemm(m, n, BKD * (2 * S + 1), lda=m + 2, ldb=n + 2, ldc=m + 2)


def test_gemm_v4_non_qualifying_takes_v2():
    """m = 130 is no whole number of blocks: the bounds-checked kernel runs
    whatever the selector says, and gives what it gives without one."""
    m, n, k = 130, 128, 32
    out4, (A, B, C) = _gemm(m, n, k, 4)
    out0, _ = _gemm(m, n, k, 0)
    out3, _ = _gemm(m, n, k, 3)
    assert np.array_equal(out4, out0) and np.array_equal(out4, out3)
    _gemm_bound_ok(out4, C, A, B, k, np.ones((m, n), dtype=bool),
                   "gemm m=130 kernel=4")


def _syrk(n, k, kernel, lda=None, ldc=None, seed=13):
    lda, ldc = lda or n, ldc or n
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, k))
    C = rng.standard_normal((n, n))
    cbuf = _padded(C, ldc)
    _core.dsyrk_ln_hip(_padded(A, lda), cbuf, n, k, lda, ldc, kernel=kernel)
    return cbuf.reshape((ldc, n), order="F"), (A, C)


def _check_syrk(n, k, **ld):
    out4, (A, C) = _syrk(n, k, 4, **ld)
    out3, _ = _syrk(n, k, 3, **ld)
    assert np.array_equal(out4, out3)
    blk = np.arange(n) // BLK
    # every block on or below the block diagonal, computed whole
    on_or_below = blk[:, None] >= blk[None, :]
    _gemm_bound_ok(out4[:n, :], C, A, A, k, on_or_below,
                   f"syrk v4 n={n} k={k} {ld}")
    # blocks above the diagonal blocks are left as they came in
    assert np.array_equal(out4[:n, :][~on_or_below], C[~on_or_below])
    assert np.all(out4[n:, :] == SENTINEL)


@pytest.mark.parametrize("k", sorted({BKD, 128, BKD * (2 * S + 1)}))
@pytest.mark.parametrize("n", [128, 384, 1152])
def test_syrk_v4(n, k):
    _check_syrk(n, k)


def test_syrk_v4_padded_ld():
    n = 384
    _check_syrk(n, BKD * (2 * S + 1), lda=n + 2, ldc=n + 2)


def test_syrk_v4_non_qualifying_takes_v2():
    n, k = 130, 32
    out4, (A, C) = _syrk(n, k, 4)
    out0, _ = _syrk(n, k, 0)
    assert np.array_equal(out4, out0)
    _gemm_bound_ok(out4, C, A, A, k, np.tril(np.ones((n, n), dtype=bool)),
                   "syrk n=130 kernel=4")


def _trmm(m, n, kernel, ldb=None, ldw=None, ldx=None, seed=7):
    ldb, ldw, ldx = ldb or m, ldw or n, ldx or m
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((m, n))
    W = np.tril(rng.standard_normal((n, n)))
    W[np.diag_indices(n)] += 4.0  # boosted diagonal, like an inverse factor
    assert not np.triu(W, 1).any()   # stored zeros above the diagonal
    xbuf = np.full(ldx * n, np.nan)  # beta = 0: never read
    _core.dtrmm_rlt_hip(_padded(B, ldb, 0.0), _padded(W, ldw, 0.0), xbuf, m,
                        n, ldb, ldw, ldx, kernel=kernel)
    return xbuf.reshape((ldx, n), order="F"), (B, W)


def _check_trmm(m, n, **ld):
    out4, (B, W) = _trmm(m, n, 4, **ld)
    out3, _ = _trmm(m, n, 3, **ld)
    X = out4[:m, :]
    assert not np.isnan(X).any()
    assert np.array_equal(X, out3[:m, :])
    assert np.all(np.isnan(out4[m:, :]))  # rows past m are not written
    ref = B @ W.T
    bound = 2 * n * EPS * (np.abs(B) @ np.abs(W).T)
    diff = np.abs(X - ref)
    print(f"trmm v4 m={m} n={n} {ld}: max |X-ref| = {diff.max():.3e}, "
          f"max diff/bound = {(diff / bound).max():.3e}")
    assert np.all(diff <= bound)


# n = 1152: 9 block columns, a second snake round with 7 padding columns
@pytest.mark.parametrize("n", [128, 1152])
@pytest.mark.parametrize("m", [128, 256])
def test_trmm_v4(m, n):
    _check_trmm(m, n)


def test_trmm_v4_padded_ld():
    m, n = 256, 1152
    _check_trmm(m, n, ldb=m + 2, ldw=n + 2, ldx=m + 2)


_DAG_CODE = """
import sys
import numpy as np
sys.path.insert(0, {repo!r})
import parsec_amd as pm
ctx = pm.Context(nworkers=2, rank=0, world=1)
assert ctx.has_gpu
out = {{}}
for n in {sizes!r}:
    A = pm.TiledMatrix(ctx, n, n, 256, 256, 1, 1)
    assert A.mt == A.nt == (n + 255) // 256
    tp = pm.Dtd(ctx); pm.insert_spd_fill(tp, A, 42); pm.insert_potrf(tp, A)
    tp.wait()
    for i in range(A.mt):
        for j in range(i + 1):
            out["L%d_%d_%d" % (n, i, j)] = np.array(A.tile_numpy(i, j))
    del A
assert ctx.gpu_stats()["tasks"] > 0
np.savez({path!r}, **out)
del ctx
"""


DAG_SIZES = (768, 640, 386)


@pytest.fixture(scope="module")
def dag_factors(tmp_path_factory):
    """Both kernels factor both matrices once, side by side in two
    processes."""
    d = tmp_path_factory.mktemp("potrf_v4")
    paths = {kern: str(d / f"v{kern}.npz") for kern in (3, 4)}
    procs = {}
    for kern, path in paths.items():
        env = dict(os.environ)
        env["PARSEC_MCA_dgemm_nt_kernel"] = str(kern)
        # the trailing GEMM tiles take the hand kernel too
        env["PARSEC_MCA_chore_gemm"] = "hip"
        procs[kern] = subprocess.Popen(
            [sys.executable, "-c", _DAG_CODE.format(repo=REPO, path=path, sizes=DAG_SIZES)],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
            text=True)
    logs = {}
    for kern, proc in procs.items():  # reap both before judging either
        try:
            logs[kern], _ = proc.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            proc.kill()
            logs[kern], _ = proc.communicate()
    for kern, proc in procs.items():
        assert proc.returncode == 0, f"kernel {kern}: {logs[kern]}"
    return {kern: np.load(p) for kern, p in paths.items()}


@pytest.mark.parametrize("n", DAG_SIZES)
def test_potrf_dag_v4_equals_v3(dag_factors, n):
    mt = (n + 255) // 256
    for i in range(mt):
        for j in range(i + 1):
            name = f"L{n}_{i}_{j}"
            t3, t4 = dag_factors[3][name], dag_factors[4][name]
            assert t3.shape == t4.shape
            assert np.all(np.isfinite(np.tril(t4) if i == j else t4)), name
            assert t3.tobytes() == t4.tobytes(), name
    # and it is a Cholesky factor at all: a positive diagonal to the end
    last = dag_factors[4][f"L{n}_{mt - 1}_{mt - 1}"]
    assert np.all(np.diag(last)[:n - 256 * (mt - 1)] > 0)
