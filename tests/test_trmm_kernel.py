"""Triangular-aware X = B * W^T kernel (the TRSM-by-inverse product) vs NumPy.

W is lower triangular with stored zeros above its diagonal, as gpu_trtri
leaves it; the kernel cuts each output block column's K range at its
diagonal block and stores X without reading it (beta = 0).

Acceptance is the componentwise GEMM bound for a length-n inner product,
|X - ref| <= 2 n eps (|B| |W|^T): n*eps/(1 - n*eps) for the kernel's own
summation in any order plus the same for the NumPy reference.
"""
import numpy as np
import pytest

from parsec_amd import _core

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _operands(m, n, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((m, n))
    W = np.tril(rng.standard_normal((n, n)))
    W[np.diag_indices(n)] += 4.0  # boosted diagonal, like an inverse factor
    assert not np.triu(W, 1).any()
    return B, W


def _padded(M, ld, fill):
    """Column-major buffer with leading dimension ld >= rows, flattened."""
    rows, cols = M.shape
    buf = np.full((ld, cols), fill, dtype=np.float64, order="F")
    buf[:rows, :] = M
    return buf.ravel(order="F")


def _run(m, n, ldb, ldx, xfill, seed=7):
    B, W = _operands(m, n, seed)
    bbuf = _padded(B, ldb, 0.0)
    wbuf = _padded(W, n, 0.0)
    xbuf = np.full(ldx * n, xfill, dtype=np.float64)
    _core.dtrmm_rlt_hip(bbuf, wbuf, xbuf, m, n, ldb, n, ldx)
    Xfull = xbuf.reshape((ldx, n), order="F")
    X = Xfull[:m, :]
    ref = B @ W.T
    bound = 2 * n * EPS * (np.abs(B) @ np.abs(W).T)
    diff = np.abs(X - ref)
    print(f"m={m} n={n} ldb={ldb} ldx={ldx}: max |X-ref| = {diff.max():.3e}, "
          f"max diff/bound = {(diff / bound).max():.3e}")
    assert np.all(np.isfinite(X))
    assert np.all(diff <= bound)
    return Xfull


@pytest.mark.parametrize("m,n", [(128, 128), (256, 384), (384, 256)])
def test_dtrmm_rlt_vs_numpy(m, n):
    _run(m, n, ldb=m, ldx=m, xfill=0.0)


def test_dtrmm_rlt_padded_ld():
    """Tiles in the edge row of a matrix have ld > rows: rows past m of B
    are not read into the result and rows past m of X are not written."""
    m, n, ldb, ldx = 256, 384, 256 + 64, 256 + 192
    Xfull = _run(m, n, ldb=ldb, ldx=ldx, xfill=-3.0)
    assert np.all(Xfull[m:, :] == -3.0)


def test_dtrmm_rlt_ignores_output_buffer():
    """beta = 0 must not read X: the swapped-in pool buffer is
    uninitialized in real use, so NaNs in it may not reach the result."""
    _run(256, 384, ldb=256, ldx=256, xfill=np.nan)
