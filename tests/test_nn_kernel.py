"""The NN hand kernel, C -= A B with A contiguous along M and B contiguous
along K, vs NumPy.

Acceptance is the componentwise bound test_trmm_kernel.py derives, in its
form for an accumulating kind (as in test_tn_kernel.py): K eps / (1 - K eps)
for the kernel's summation in any order plus the same for the NumPy
reference, one more operation for the subtraction and C's entry value:
|C - ref| <= 2 (K + 1) eps (|C0| + |A| |B|).
"""
import numpy as np
import pytest

from parsec_amd import _core

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _padded(M, ld, fill):
    """Column-major buffer with leading dimension ld >= rows, flattened."""
    rows, cols = M.shape
    buf = np.full((ld, cols), fill, dtype=np.float64, order="F")
    buf[:rows, :] = M
    return buf.ravel(order="F")


def _unpad(buf, ld, cols):
    return buf.reshape((ld, cols), order="F")


def _check(what, got, ref, bound):
    diff = np.abs(got - ref)
    assert np.all(np.isfinite(got)), what
    print(f"{what}: max |C-ref| = {diff.max():.3e}, "
          f"max diff/bound = {(diff / bound).max():.3e}")
    assert np.all(diff <= bound), what


def _gemm(m, n, k, lda, ldb, ldc, seed=3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, k))
    B = rng.standard_normal((k, n))
    C0 = rng.standard_normal((m, n))
    cbuf = _padded(C0, ldc, -3.0)
    _core.dgemm_nn_hip(_padded(A, lda, np.nan), _padded(B, ldb, np.nan), cbuf,
                       m, n, k, lda, ldb, ldc)
    Cfull = _unpad(cbuf, ldc, n)
    ref = C0 - A @ B
    bound = 2 * (k + 1) * EPS * (np.abs(C0) + np.abs(A) @ np.abs(B))
    _check(f"gemm_nn m={m} n={n} k={k} ld={lda},{ldb},{ldc}", Cfull[:m], ref,
           bound)
    return Cfull


@pytest.mark.parametrize("m,n,k", [(128, 128, 128), (256, 384, 144),
                                   (200, 72, 328)])
def test_dgemm_nn_vs_numpy(m, n, k):
    """One full block; several blocks in both directions with K no multiple
    of 128; ragged edges in all three dimensions, with a block narrower than
    one wave's 64 columns."""
    _gemm(m, n, k, m, k, m)


def test_dgemm_nn_padded_ld():
    """Odd leading dimensions, as no tile of the DAG has but a caller may:
    rows past m of A and past k of B are not read (they hold NaN, so the
    result is finite only if they stayed out of it) and rows past m of C
    come back bit-identical."""
    m, n, k = 200, 72, 328
    Cfull = _gemm(m, n, k, lda=m + 3, ldb=k + 5, ldc=m + 3)
    assert np.all(Cfull[m:, :] == -3.0)
