"""The TN hand kernel, C (+)= A^T B with both operands contiguous along K,
in its four kinds (GEMM, SYRK, TRMM, LAUUM) vs NumPy.

Acceptance is the componentwise bound test_trmm_kernel.py derives: for the
storing kinds |C - ref| <= 2 K eps (|A|^T |B|), K the longest inner product
(K eps / (1 - K eps) for the kernel's summation in any order plus the same
for the NumPy reference); the accumulating kinds add one more operation and
C's entry value: 2 (K + 1) eps (|C0| + |A|^T |B|). The triangular kinds are
bounded with their masked operands, and are given NaN where the mask hides
an element, so a result that is finite proves the mask.
"""
import numpy as np
import pytest

from parsec_amd import _core

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
BLK = 128


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


def _lower_w(n, rng):
    """Lower triangular with a boosted diagonal, like an inverse factor, and
    NaN above the diagonal: what a diagonal tile may hold there is junk."""
    W = np.tril(rng.standard_normal((n, n)))
    W[np.diag_indices(n)] += 4.0
    Wjunk = W.copy()
    Wjunk[np.triu_indices(n, 1)] = np.nan
    return W, Wjunk


def _block_lower_mask(n):
    """True on the lower-triangular set of 128-blocks, diagonal blocks whole."""
    b = np.arange(n) // BLK
    return b[:, None] >= b[None, :]


def _gemm(m, n, k, lda, ldb, ldc, seed=3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((k, m))
    B = rng.standard_normal((k, n))
    C0 = rng.standard_normal((m, n))
    cbuf = _padded(C0, ldc, -3.0)
    _core.dgemm_tn_hip(_padded(A, lda, np.nan), _padded(B, ldb, np.nan), cbuf,
                       m, n, k, lda, ldb, ldc)
    Cfull = _unpad(cbuf, ldc, n)
    ref = C0 + A.T @ B
    bound = 2 * (k + 1) * EPS * (np.abs(C0) + np.abs(A).T @ np.abs(B))
    _check(f"gemm m={m} n={n} k={k} ld={lda},{ldb},{ldc}", Cfull[:m], ref,
           bound)
    return Cfull


@pytest.mark.parametrize("m,n,k", [(128, 128, 128), (256, 384, 144),
                                   (200, 72, 328)])
def test_dgemm_tn_vs_numpy(m, n, k):
    _gemm(m, n, k, k, k, m)


def test_dgemm_tn_padded_ld():
    """Odd leading dimensions, as no tile of the DAG has but a caller may:
    rows past k of the operands are not read (they hold NaN) and rows past
    m of C are not written."""
    m, n, k = 200, 72, 328
    Cfull = _gemm(m, n, k, lda=k + 3, ldb=k + 5, ldc=m + 3)
    assert np.all(Cfull[m:, :] == -3.0)


@pytest.mark.parametrize("n,k", [(384, 256), (328, 200)])
def test_dsyrk_lt_vs_numpy(n, k):
    rng = np.random.default_rng(5)
    A = rng.standard_normal((k, n))
    C0 = rng.standard_normal((n, n))
    cbuf = _padded(C0, n, 0.0)
    _core.dsyrk_lt_hip(_padded(A, k, 0.0), cbuf, n, k, k, n)
    C = _unpad(cbuf, n, n)
    ref = C0 + A.T @ A
    bound = 2 * (k + 1) * EPS * (np.abs(C0) + np.abs(A).T @ np.abs(A))
    low = _block_lower_mask(n)
    _check(f"syrk n={n} k={k}", C[low], ref[low], bound[low])
    assert np.array_equal(C[~low], C0[~low]), "strict upper blocks changed"


@pytest.mark.parametrize("m,n", [(384, 256), (328, 72)])
def test_dtrmm_llt_vs_numpy(m, n):
    """Three block rows at m = 384, so the K start differs per row. W holds
    NaN above its diagonal and the output buffer is NaN: a finite result
    proves both the mask and beta = 0."""
    rng = np.random.default_rng(7)
    W, Wjunk = _lower_w(m, rng)
    B = rng.standard_normal((m, n))
    xbuf = np.full(m * n, np.nan)
    _core.dtrmm_llt_hip(_padded(Wjunk, m, 0.0), _padded(B, m, 0.0), xbuf, m, n,
                        m, m, m)
    X = _unpad(xbuf, m, n)
    bound = 2 * m * EPS * (np.abs(W).T @ np.abs(B))
    _check(f"trmm m={m} n={n}", X, W.T @ B, bound)


@pytest.mark.parametrize("n", [384, 328])
def test_dlauum_l_vs_numpy(n):
    rng = np.random.default_rng(9)
    W, Wjunk = _lower_w(n, rng)
    xbuf = np.full(n * n, np.nan)
    _core.dlauum_l_hip(_padded(Wjunk, n, 0.0), xbuf, n, n, n)
    X = _unpad(xbuf, n, n)
    ref = W.T @ W
    bound = 2 * n * EPS * (np.abs(W).T @ np.abs(W))
    low = _block_lower_mask(n)
    # the lower result, and with it the whole (symmetric) diagonal blocks
    _check(f"lauum n={n}", X[low], ref[low], bound[low])
    # blocks above the diagonal blocks are the caller's to clear
    assert np.all(np.isnan(X[~low]))
