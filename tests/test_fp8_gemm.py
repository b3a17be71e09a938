"""FP8 (E4M3 / E5M2) tile-GEMM: C = alpha A B^T, K-major byte operands.

Operands are integers in [-4, 4], exact in both formats and encoded by
different bytes in each, with k <= 1024: every partial sum is an integer
below 2^14, fp32 accumulation is exact in any order, and the check is bitwise
equality with a float64 product. alpha is a power of two, so it stays exact.
"""
import numpy as np
import pytest
import torch

import parsec_amd as pm
from parsec_amd import _core

DT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
PAIRS = [("e4m3", "e4m3"), ("e5m2", "e5m2"), ("e5m2", "e4m3")]
TILE = 256  # the fast kernel's block; it needs k % 128 == 0 and k >= 256


def pack(x, fmt, ld=0):
    """rows x k values -> fp8 bytes, rows ld apart (0: tight), flat."""
    b = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    b = b.to(DT[fmt]).view(torch.uint8).numpy()
    buf = np.zeros((x.shape[0], ld or x.shape[1]), dtype=np.uint8)
    buf[:, :x.shape[1]] = b
    return buf.ravel()


def operands(m, n, k, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(-4, 5, (m, k)).astype(np.float64),
            rng.integers(-4, 5, (n, k)).astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("m,n,k,pad", [
    (16, 16, 128, 0),            # one MFMA: the fragment layout
    (1, 1, 1, 0),                # everything guarded
    (TILE, TILE, 256, 0),        # fast path, minimum K depth
    (TILE, TILE, 384, 0),        # the ring wraps
    (2 * TILE, TILE, 256, 0),    # more than one block: swizzle, block origin
    (130, 67, 45, 0),            # odd tight ld
    (130, 67, 45, 3),            # padded ld
    (TILE, TILE, 200, 0),        # k no multiple of the step: edge kernel
])
def test_kernel_exact(fa, fb, m, n, k, pad):
    A, B = operands(m, n, k)
    ld = k + pad if pad else 0
    C = np.zeros((n, m), dtype=np.float32)  # col-major m x n
    _core.gemm_fp8_hip(pack(A, fa, ld), pack(B, fb, ld), C.ravel(), m, n, k,
                       fmt_a=fa, fmt_b=fb, lda=ld, ldb=ld)
    assert np.array_equal(C.T.astype(np.float64), A @ B.T)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("m,n,k", [(TILE, TILE, 256), (130, 67, 45)])
def test_kernel_alpha_accumulate(alpha, accum, m, n, k):
    A, B = operands(m, n, k, seed=1)
    C0 = np.random.default_rng(2).integers(-8, 9, (m, n)).astype(np.float64)
    C = np.ascontiguousarray(C0.T, dtype=np.float32)
    _core.gemm_fp8_hip(pack(A, "e4m3"), pack(B, "e4m3"), C.ravel(), m, n, k,
                       alpha=alpha, accum=accum)
    assert np.array_equal(C.T.astype(np.float64),
                          alpha * (A @ B.T) + (C0 if accum else 0))


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("fa,fb,finite", [("e4m3", "e5m2", 254),
                                          ("e5m2", "e4m3", 248)])
def test_every_code_decodes(fa, fb, finite, fast):
    """Row i of A holds byte i at column i % 128, B is a one-hot identity,
    so C[i, i % 128] is the value of code i alone, subnormals included. The
    edge kernel runs it as 256 x 128 x 128; the fast kernel needs n and k
    padded to 256 with zero bytes, which adds zero columns to C."""
    n = k = 256 if fast else 128
    value = torch.arange(256, dtype=torch.uint8).view(DT[fa]).float().numpy()
    ok = np.isfinite(value)
    assert ok.sum() == finite
    rows = np.arange(256)
    A = np.zeros((256, k), dtype=np.uint8)
    A[rows, rows % 128] = np.where(ok, rows, 0)
    eye = np.zeros((n, k))
    eye[np.arange(128), np.arange(128)] = 1.0
    want = np.zeros((256, n), dtype=np.float32)
    want[rows, rows % 128] = np.where(ok, value, 0)
    C = np.zeros((n, 256), dtype=np.float32)
    _core.gemm_fp8_hip(A.ravel(), pack(eye, fb), C.ravel(), 256, n, k,
                       fmt_a=fa, fmt_b=fb)
    assert np.array_equal(C.T, want)


def run_dag(ctx, A, B, tile, fa, fb, alpha):
    """alpha A B^T (A: M x K, B: N x K) through insert_gemm_fp8."""
    def tiled(X, fmt):  # K x rows in tile x tile tiles, each K-major
        T = pm.TiledMatrix(ctx, X.shape[1], X.shape[0], tile, tile, 1, 1,
                           elem_size=1)
        for i in range(T.mt):
            for j in range(T.nt):
                blk = X[j * tile:(j + 1) * tile, i * tile:(i + 1) * tile]
                T.tile_bytes_set(i, j, pack(blk, fmt).tobytes())
        return T

    At, Bt = tiled(A, fa), tiled(B, fb)
    C = pm.TiledMatrix(ctx, A.shape[0], B.shape[0], tile, tile, 1, 1,
                       elem_size=4)
    tp = pm.Dtd(ctx)
    pm.insert_gemm_fp8(tp, At, Bt, C, fmt_a=fa, fmt_b=fb, alpha=alpha)
    tp.wait()
    got = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    for i in range(C.mt):
        for j in range(C.nt):
            raw = np.frombuffer(C.tile_bytes(i, j), dtype=np.float32)
            got[i * tile:(i + 1) * tile, j * tile:(j + 1) * tile] = \
                raw.reshape((tile, tile)).T
    return got.astype(np.float64)


@pytest.mark.gpu
def test_dag_gpu():
    ctx = pm.Context(nworkers=2, rank=0, world=1)
    A, B = operands(2 * TILE, 2 * TILE, 2 * TILE, seed=3)
    got = run_dag(ctx, A, B, TILE, "e4m3", "e4m3", 2.0)
    assert ctx.gpu_stats()["tasks"] >= 8
    assert np.array_equal(got, 2 * (A @ B.T))
    del ctx


def test_dag_cpu_chores():
    ctx = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)  # CPU chores only
    A, B = operands(128, 128, 128, seed=4)
    for fa, fb in PAIRS:
        assert np.array_equal(run_dag(ctx, A, B, 64, fa, fb, 1.0),
                              A @ B.T), (fa, fb)
    del ctx
