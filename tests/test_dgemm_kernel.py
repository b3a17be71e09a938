"""Hand fp64 MFMA kernels (GEMM, SYRK, potf2) vs NumPy, one launch each.

Shapes are the smallest that reach each kernel and each index calculation:
the glds full-tile kernel (128-multiples, k % 16 == 0, even leading
dimensions) and the bounds-checked kernel that takes everything else.

Acceptance is componentwise, derived as in test_trmm_kernel.py.
GEMM / SYRK: |C_out - (C - A B^T)| <= 2 (k+1) eps (|C| + |A| |B|^T), a
length-k inner product in any order plus the subtraction, for the kernel
and for NumPy. potf2: |A - L L^T| <= 2 (n+2) eps (|L| |L|^T) on the lower
triangle, Higham's gamma_{n+1} bound for Cholesky with one more rounding
for the reciprocal multiply, doubled; numpy.linalg.cholesky has to meet the
same bound on the same input.
"""
import numpy as np
import pytest

from parsec_amd import _core

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
BLK = 128
SENTINEL = -3.0


def _padded(M, ld, fill=SENTINEL):
    """Column-major buffer with leading dimension ld >= rows, flattened."""
    rows, cols = M.shape
    buf = np.full((ld, cols), fill, dtype=np.float64, order="F")
    buf[:rows, :] = M
    return buf.ravel(order="F")


def _check(out, C, A, B, k, mask, what):
    ref = C - A @ B.T
    bound = 2 * (k + 1) * EPS * (np.abs(C) + np.abs(A) @ np.abs(B).T)
    diff = np.abs(out - ref)
    print(f"{what}: max |C-ref| = {diff[mask].max():.3e}, "
          f"max diff/bound = {(diff[mask] / bound[mask]).max():.3e}")
    assert np.all(np.isfinite(out[mask]))
    assert np.all(diff[mask] <= bound[mask])


def _run_gemm(m, n, k, lda=None, ldb=None, ldc=None, seed=11):
    lda, ldb, ldc = lda or m, ldb or n, ldc or m
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, k))
    B = rng.standard_normal((n, k))
    C = rng.standard_normal((m, n))
    cbuf = _padded(C, ldc)
    _core.dgemm_nt_hip(_padded(A, lda), _padded(B, ldb), cbuf, m, n, k,
                       lda, ldb, ldc)
    full = cbuf.reshape((ldc, n), order="F")
    _check(full[:m, :], C, A, B, k, np.ones((m, n), dtype=bool),
           f"gemm m={m} n={n} k={k} lda={lda} ldb={ldb} ldc={ldc}")
    assert np.all(full[m:, :] == SENTINEL)


# full tiles: one block; non-square with three K-tiles (a swapped bx/by
# shows, both LDS buffers and an odd tile count); 9 blocks (the XCD remap
# has a remainder)
@pytest.mark.parametrize("m,n,k", [(128, 128, 16), (256, 384, 48),
                                   (384, 384, 32)])
def test_dgemm_full_tiles(m, n, k):
    _run_gemm(m, n, k)


# edges in m, n and k; full blocks with k % 16 != 0
@pytest.mark.parametrize("m,n,k", [(100, 70, 20), (129, 127, 17),
                                   (128, 128, 24)])
def test_dgemm_bounds_checked(m, n, k):
    _run_gemm(m, n, k)


def test_dgemm_default_ld():
    """The leading dimensions default to the row counts."""
    m, n, k = 100, 70, 20
    rng = np.random.default_rng(5)
    A = rng.standard_normal((m, k))
    B = rng.standard_normal((n, k))
    C = rng.standard_normal((m, n))
    cbuf = C.ravel(order="F").copy()
    _core.dgemm_nt_hip(A.ravel(order="F"), B.ravel(order="F"), cbuf, m, n, k)
    _check(cbuf.reshape((m, n), order="F"), C, A, B, k,
           np.ones((m, n), dtype=bool), "gemm default ld")


def test_dgemm_padded_even_ld():
    """Edge-row tiles have ld > rows: rows past m are neither read into the
    result nor written."""
    _run_gemm(256, 128, 32, lda=256 + 64, ldc=256 + 64)


def test_dgemm_odd_ld():
    """Columns of an odd-ld tile are not 16-byte aligned, so full blocks
    still have to take the bounds-checked kernel."""
    _run_gemm(128, 128, 16, lda=129, ldb=129, ldc=129)


def test_dgemm_rejects_short_buffers():
    a = np.zeros(128 * 16)
    with pytest.raises(ValueError):
        _core.dgemm_nt_hip(a, a, np.zeros(128 * 128 - 1), 128, 128, 16)
    with pytest.raises(ValueError):
        _core.dgemm_nt_hip(a, a, np.zeros(128 * 128), 128, 128, 16, 127)


def _run_syrk(n, k, lda=None, ldc=None, seed=13):
    lda, ldc = lda or n, ldc or n
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, k))
    C = rng.standard_normal((n, n))
    blk = np.arange(n) // BLK
    above = blk[:, None] < blk[None, :]   # blocks strictly above the diagonal
    C[above] = SENTINEL
    cbuf = _padded(C, ldc)
    _core.dsyrk_ln_hip(_padded(A, lda), cbuf, n, k, lda, ldc)
    full = cbuf.reshape((ldc, n), order="F")
    out = full[:n, :]
    _check(out, C, A, A, k, np.tril(np.ones((n, n), dtype=bool)),
           f"syrk n={n} k={k} lda={lda} ldc={ldc}")
    # the upper half of a diagonal block is unspecified
    assert np.all(out[above] == SENTINEL)
    assert np.all(full[n:, :] == SENTINEL)


# one block; 6 blocks (fewer than the 8 XCDs); 45 blocks (the remap has a
# quotient and a remainder)
@pytest.mark.parametrize("n,k", [(128, 16), (384, 128), (1152, 16)])
def test_dsyrk_full_tiles(n, k):
    _run_syrk(n, k)


@pytest.mark.parametrize("n,k", [(200, 20), (256, 24)])
def test_dsyrk_bounds_checked(n, k):
    _run_syrk(n, k)


def test_dsyrk_odd_ld():
    _run_syrk(128, 16, lda=129)


def _spd(n, seed=17):
    G = np.random.default_rng(seed).standard_normal((n, n))
    return G @ G.T + n * np.eye(n)


def _chol_ok(A, L, what):
    """|A - L L^T| <= 2 (n+2) eps |L| |L|^T on the lower triangle; the
    residual is evaluated in extended precision so that it adds no rounding
    of its own."""
    n = A.shape[0]
    Lx = L.astype(np.longdouble)
    diff = np.abs(A.astype(np.longdouble) - Lx @ Lx.T)
    bound = 2 * (n + 2) * EPS * (np.abs(L) @ np.abs(L).T)
    low = np.tril(np.ones((n, n), dtype=bool))
    print(f"{what} n={n}: max |A-LL^T| = {float(diff[low].max()):.3e}, "
          f"max diff/bound = {float((diff[low] / bound[low]).max()):.3e}")
    return bool(np.all(diff[low] <= bound[low]))


@pytest.mark.parametrize("n", [16, 17, 100, 128])
def test_potf2(n):
    A = _spd(n)
    assert _chol_ok(A, np.linalg.cholesky(A), "numpy")
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    buf = A.copy()
    buf[up] = SENTINEL
    flat = buf.ravel(order="F").copy()
    _core.potf2_hip(flat, n)
    out = flat.reshape((n, n), order="F")
    assert np.all(np.isfinite(out))
    assert np.all(out[up] == SENTINEL)
    assert _chol_ok(A, np.tril(out), "potf2")
