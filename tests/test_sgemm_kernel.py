"""The fp32 hand kernels (src/kernels_f32.cpp) against float64 NumPy on the
float32 inputs: k_sgemm_nt's three kinds (GEMM, SYRK, the TRSM product), the
bounds-checked k_sgemm_nt_edge behind the first two, and k_convert.

The bounds are those of the fp64 kernel tests with float32's eps, and hold
for any summation order: 2 (k+1) eps (|C| + |A| |B|^T) componentwise for GEMM
and SYRK, 2 n eps (|B| |W|^T) for the product. They are what proves the
32x32x2 accumulator map of the epilogue: a misplaced element is off by O(1).

S and BK are the ring's slot count and K-tile depth (SG_S and SG_BK). The K
sizes BK * {1, 2, S-1, S, S+1, 2S+1} cover fewer tiles than the prefetch
distance, exactly one ring, a wrap and the drain.
"""
import numpy as np
import pytest

from parsec_amd import _core

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float32).eps
BLK = 128
SENTINEL = np.float32(-3.0)
S, BK = 4, 16
KS = sorted({BK * t for t in (1, 2, S - 1, S, S + 1, 2 * S + 1)})


def _rand(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def _padded(M, ld, fill=SENTINEL):
    """Column-major float32 buffer with leading dimension ld, flattened."""
    buf = np.full((ld, M.shape[1]), fill, dtype=np.float32, order="F")
    buf[:M.shape[0], :] = M
    return buf.ravel(order="F")


def _bound_ok(out, C, A, B, k, mask, what):
    A, B, C = (x.astype(np.float64) for x in (A, B, C))
    ref = C - A @ B.T
    bound = 2 * (k + 1) * EPS * (np.abs(C) + np.abs(A) @ np.abs(B).T)
    diff = np.abs(out.astype(np.float64) - ref)
    print(f"{what}: max diff/bound = {(diff[mask] / bound[mask]).max():.3e}")
    assert np.all(np.isfinite(out[mask]))
    assert np.all(diff[mask] <= bound[mask])


def _check_gemm(m, n, k, pad=0):
    rng = np.random.default_rng(11)
    A, B, C = _rand(rng, (m, k)), _rand(rng, (n, k)), _rand(rng, (m, n))
    lda, ldb, ldc = m + pad, n + pad, m + pad
    cbuf = _padded(C, ldc)
    _core.sgemm_nt_hip(_padded(A, lda), _padded(B, ldb), cbuf, m, n, k, lda,
                       ldb, ldc)
    out = cbuf.reshape((ldc, n), order="F")
    _bound_ok(out[:m], C, A, B, k, np.ones((m, n), dtype=bool),
              f"sgemm m={m} n={n} k={k} pad={pad}")
    assert np.all(out[m:] == SENTINEL)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m,n", [(128, 128), (256, 384)])
def test_sgemm(m, n, k):
    _check_gemm(m, n, k)


# +4 keeps 16-B aligned columns (full-tile kernel, sentinel rows past m);
# +2 breaks them and m = 130 is no whole block: both take the edge kernel
@pytest.mark.parametrize("m,pad", [(256, 4), (256, 2), (130, 0)])
def test_sgemm_ld_and_edge(m, pad):
    _check_gemm(m, 384, BK * (2 * S + 1), pad)


@pytest.mark.parametrize("k", sorted({BK, 128, BK * (2 * S + 1)}))
@pytest.mark.parametrize("n", [128, 384, 1152, 130])
def test_ssyrk(n, k):
    rng = np.random.default_rng(13)
    A, C = _rand(rng, (n, k)), _rand(rng, (n, n))
    cbuf = C.ravel(order="F").copy()
    _core.ssyrk_ln_hip(A.ravel(order="F"), cbuf, n, k, n, n)
    out = cbuf.reshape((n, n), order="F")
    blk = np.arange(n) // BLK
    on_or_below = blk[:, None] >= blk[None, :]  # diagonal blocks whole
    _bound_ok(out, C, A, A, k, on_or_below, f"ssyrk n={n} k={k}")
    # blocks above the block diagonal are left as they came in, bit for bit
    assert np.array_equal(out[~on_or_below], C[~on_or_below])


# n = 1152: 9 block columns, a second snake round with 7 padding columns
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("n", [128, 1152])
@pytest.mark.parametrize("m", [128, 256])
def test_strmm(m, n, pad):
    rng = np.random.default_rng(7)
    B = _rand(rng, (m, n))
    W = np.tril(_rand(rng, (n, n)))
    W[np.diag_indices(n)] += np.float32(4.0)
    assert not np.triu(W, 1).any()   # stored zeros above the diagonal
    ldb, ldw, ldx = m + pad, n + pad, m + pad
    xbuf = np.full(ldx * n, np.nan, dtype=np.float32)  # beta = 0: never read
    _core.strmm_rlt_hip(_padded(B, ldb, 0), _padded(W, ldw, 0), xbuf, m, n,
                        ldb, ldw, ldx)
    out = xbuf.reshape((ldx, n), order="F")
    X = out[:m].astype(np.float64)
    assert not np.isnan(X).any()
    assert np.all(np.isnan(out[m:]))  # rows past m are not written
    B, W = B.astype(np.float64), W.astype(np.float64)
    bound = 2 * n * EPS * (np.abs(B) @ np.abs(W).T)
    diff = np.abs(X - B @ W.T)
    print(f"strmm m={m} n={n}: max diff/bound = {(diff / bound).max():.3e}")
    assert np.all(diff <= bound)


def test_convert():
    """130 x 70 in ld 256, both ways, exact, padding untouched. The fp64
    input carries ties (1 + 2^-24 rounds to even, down; 1 + 3 * 2^-24 up)."""
    rows, cols, ld = 130, 70, 256
    rng = np.random.default_rng(5)
    src64 = np.full((ld, cols), 9.0, order="F")
    src64[:rows] = rng.standard_normal((rows, cols)) * 10.0 ** rng.integers(
        -6, 7, (rows, cols))
    src64[:4, 0] = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -1 - 2.0 ** -24, 1e-50]
    dst32 = np.full(ld * cols, SENTINEL, dtype=np.float32)
    _core.convert_d2s_hip(src64.ravel(order="F"), dst32, rows, cols, ld)
    dst32 = dst32.reshape((ld, cols), order="F")
    assert np.array_equal(dst32[:rows], src64[:rows].astype(np.float32))
    assert np.all(dst32[rows:] == SENTINEL)
    dst64 = np.full(ld * cols, -3.0)
    _core.convert_s2d_hip(dst32.ravel(order="F"), dst64, rows, cols, ld)
    dst64 = dst64.reshape((ld, cols), order="F")
    assert np.array_equal(dst64[:rows], dst32[:rows].astype(np.float64))
    assert np.all(dst64[rows:] == -3.0)
