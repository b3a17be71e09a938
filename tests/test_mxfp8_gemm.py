"""MXFP8 tile-GEMM and quantiser: E4M3 / E5M2 bytes with one E8M0 scale byte
per row and 32 K elements.

  C[i,j] = alpha sum_b 2^(SA[i,b] + SB[j,b] - 254) sum_{p in b} A[i,p] B[j,p]

Wherever sums occur the values are integers in [-2, 2] and the scale bytes in
{126, 127, 128} with k <= 1024: every partial sum is a multiple of 2^-2 below
2^14, exact in fp32 in any order, so every check is bitwise equality with the
float64 value of the formula.
"""
import numpy as np
import pytest
import torch

import parsec_amd as pm
from parsec_amd import _core

DT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
EMAX = {"e4m3": 8, "e5m2": 15}
LIM = {"e4m3": 448.0, "e5m2": 57344.0}
PAIRS = [("e4m3", "e4m3"), ("e5m2", "e4m3")]
FAST, EDGE = (256, 256, 256), (130, 67, 45)


def to_bytes(x, fmt):
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return x.to(DT[fmt]).view(torch.uint8).numpy()


def padded(b, pad):
    """rows of a byte matrix pad bytes further apart, flat."""
    out = np.zeros((b.shape[0], b.shape[1] + pad), dtype=np.uint8)
    out[:, :b.shape[1]] = b
    return out.ravel()


def reference(A, SA, B, SB):
    """The formula in float64; A, B are values, SA, SB scale bytes."""
    def scaled(X, S):
        s = np.where(S == 255, np.nan, np.exp2(S.astype(np.float64) - 127))
        return X * np.repeat(s, 32, axis=1)[:, :X.shape[1]]
    return scaled(A, SA) @ scaled(B, SB).T


def gemm(A, SA, B, SB, fa="e4m3", fb="e4m3", alpha=1.0, pad=0, spad=0, C0=None):
    m, k, n = A.shape[0], A.shape[1], B.shape[0]
    C = np.zeros((n, m), dtype=np.float32)  # col-major m x n
    if C0 is not None:
        C[:] = C0.T
    _core.gemm_mxfp8_hip(padded(to_bytes(A, fa), pad), padded(SA, spad),
                         padded(to_bytes(B, fb), pad), padded(SB, spad),
                         C.ravel(), m, n, k, fmt_a=fa, fmt_b=fb, alpha=alpha,
                         lda=k + pad, ldb=k + pad, ldsa=SA.shape[1] + spad,
                         ldsb=SB.shape[1] + spad, accum=C0 is not None)
    return C.T.astype(np.float64)


def operands(m, n, k, seed=0):
    rng = np.random.default_rng(seed)
    kb = (k + 31) // 32
    return (rng.integers(-2, 3, (m, k)).astype(np.float64),
            rng.integers(126, 129, (m, kb)).astype(np.uint8),
            rng.integers(-2, 3, (n, k)).astype(np.float64),
            rng.integers(126, 129, (n, kb)).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("role", ["A", "B"])
@pytest.mark.parametrize("m,n,k", [(16, 16, 128), (256, 256, 256)])
def test_scale_routing(m, n, k, role):
    """Row i of the tested operand is 1.0 at column i % 128 under scale byte
    1 + i % 254 (127 in its other blocks); the other operand is a one-hot
    identity under byte 127. C[i, i % 128] is that row's power of two alone:
    a byte from a wrong row, block or operand shows as a wrong power."""
    rows = np.arange(m)
    X = np.zeros((m, k))
    X[rows, rows % 128] = 1.0
    SX = np.full((m, k // 32), 127, dtype=np.uint8)
    SX[rows, (rows % 128) // 32] = 1 + rows % 254
    E = np.zeros((n, k))
    E[np.arange(min(n, 128)), np.arange(min(n, 128))] = 1.0
    SE = np.full((n, k // 32), 127, dtype=np.uint8)
    args = (X, SX, E, SE) if role == "A" else (E, SE, X, SX)
    want = reference(*args)
    assert np.count_nonzero(want) == m
    assert np.array_equal(gemm(*args), want)


@pytest.mark.gpu
@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("m,n,k,pad,spad,alpha,accum", [
    FAST + (0, 0, 1.0, False),             # fast path, minimum K depth
    (256, 256, 384, 0, 0, 1.0, False),     # ring wraps, scale slot alternates
    (512, 256, 256, 0, 0, 1.0, False),     # more than one block
    EDGE + (0, 0, 1.0, False),             # partial last block, tight
    EDGE + (3, 1, 1.0, False),             # ... and padded lda / ldsa
    (256, 256, 200, 0, 0, 1.0, False),     # k no multiple of the step: edge
    FAST + (0, 1, 1.0, False),             # unaligned scale stride: edge
    FAST + (0, 0, 0.5, True),
    EDGE + (0, 0, 0.5, True),
])
def test_exact_sums(fa, fb, m, n, k, pad, spad, alpha, accum):
    A, SA, B, SB = operands(m, n, k)
    C0 = np.random.default_rng(1).integers(-8, 9, (m, n)).astype(np.float64)
    got = gemm(A, SA, B, SB, fa, fb, alpha, pad, spad, C0 if accum else None)
    assert np.array_equal(got, alpha * reference(A, SA, B, SB)
                          + (C0 if accum else 0))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [FAST, EDGE])
def test_cancelling_scales(m, n, k):
    A, SA, B, SB = operands(m, n, k, seed=2)
    SA[:], SB[:] = 227, 27
    assert np.array_equal(gemm(A, SA, B, SB), A @ B.T)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [FAST, EDGE])
def test_nan_scale(m, n, k):
    A, SA, B, SB = operands(m, n, k, seed=3)
    SA[m - 3, 1] = 255
    want = reference(A, SA, B, SB)
    assert np.isnan(want[m - 3]).all() and np.isnan(want).sum() == n
    assert np.array_equal(gemm(A, SA, B, SB), want, equal_nan=True)


# ------------------------------------------------------------- quantiser
def quant_reference(x, fmt):
    """(Q bytes, S bytes) of x (rows x k, fp32) by the rule of the issue."""
    rows, k = x.shape
    kb = (k + 31) // 32
    blocks = np.zeros((rows, kb * 32))
    blocks[:, :k] = x
    blocks = blocks.reshape(rows, kb, 32)
    amax = np.abs(blocks).max(axis=2)
    X = np.clip(np.frexp(amax)[1] - 1 - EMAX[fmt], -127, 127)  # floor(log2)
    X[amax == 0] = 0
    y = np.clip(blocks * np.exp2(-X.astype(np.float64))[:, :, None],
                -LIM[fmt], LIM[fmt])
    return (to_bytes(y.reshape(rows, kb * 32)[:, :k], fmt),
            (X + 127).astype(np.uint8))


def quant_input(rows, k):
    rng = np.random.default_rng(5)
    kb = (k + 31) // 32
    mag = np.exp2(rng.uniform(-20, 20, (rows, kb)))
    x = rng.standard_normal((rows, k)) * np.repeat(mag, 32, axis=1)[:, :k]
    x[0, 0:32] = 0                                  # an all-zero block
    x[1, 32:64] = rng.uniform(-1, 1, 32)
    x[1, 40] = 32.0                                 # amax a power of two
    x[2, 64:min(k, 96)] = rng.uniform(-1, 1, min(k, 96) - 64)
    x[2, 70] = 1.9                                  # 1.9 * 2^emax: clamped
    return x.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("rows,k,pad", [(64, 256, 0), (5, 77, 0), (64, 256, 4)])
def test_quantiser(rows, k, pad, fmt):
    x = quant_input(rows, k)
    buf = np.zeros((rows, k + pad), dtype=np.float32)
    buf[:, :k] = x
    Q, S = _core.quantize_mxfp8_hip(buf.ravel(), rows, k, fmt=fmt, ldx=k + pad)
    wantQ, wantS = quant_reference(x, fmt)
    assert np.array_equal(S, wantS)
    assert np.array_equal(Q, wantQ)


# ------------------------------------------------------------------- DAG
def tiled(ctx, X, mb, nb, dtype):
    """X (rows x K) as a K x rows TiledMatrix of mb x nb K-major tiles."""
    T = pm.TiledMatrix(ctx, X.shape[1], X.shape[0], mb, nb, 1, 1,
                       elem_size=np.dtype(dtype).itemsize)
    for i in range(T.mt):
        for j in range(T.nt):
            blk = X[j * nb:(j + 1) * nb, i * mb:(i + 1) * mb]
            buf = np.zeros((nb, mb), dtype=dtype)
            buf[:blk.shape[0], :blk.shape[1]] = blk
            T.tile_bytes_set(i, j, buf.tobytes())
    return T


def untiled(T, dtype):
    """The rows x K (for C: N x M) array of a TiledMatrix."""
    out = np.zeros((T.nt * T.nb, T.mt * T.mb), dtype=dtype)
    for i in range(T.mt):
        for j in range(T.nt):
            raw = np.frombuffer(T.tile_bytes(i, j), dtype=dtype)
            out[j * T.nb:(j + 1) * T.nb, i * T.mb:(i + 1) * T.mb] = \
                raw.reshape(T.nb, T.mb)
    return out[:T.n, :T.m]


def quantise_dag(ctx, x, mb, nb, fmt, tp):
    X = tiled(ctx, x, mb, nb, np.float32)
    Q = tiled(ctx, np.zeros(x.shape, np.uint8), mb, nb, np.uint8)
    S = tiled(ctx, np.zeros((x.shape[0], (x.shape[1] + 31) // 32), np.uint8),
              mb // 32, nb, np.uint8)
    pm.insert_quantize_mxfp8(tp, X, Q, S, fmt=fmt)
    return X, Q, S


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("rows,k,mb,nb", [(64, 256, 128, 32), (5, 77, 64, 4)])
def test_quantiser_cpu_chore(rows, k, mb, nb, fmt):
    ctx = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)  # CPU chores only
    x = quant_input(rows, k)
    tp = pm.Dtd(ctx)
    X, Q, S = quantise_dag(ctx, x, mb, nb, fmt, tp)
    tp.wait()
    wantQ, wantS = quant_reference(x, fmt)
    assert np.array_equal(untiled(S, np.uint8), wantS)
    assert np.array_equal(untiled(Q, np.uint8), wantQ)
    del ctx


def check_dag(ctx, size, tile, fa, fb):
    """Quantise fp32 operands (the integer data above times known block
    scales, so the quantiser recovers it exactly), then multiply."""
    A, SA, B, SB = operands(size, size, size, seed=6)
    xa = A * np.repeat(np.exp2(SA.astype(np.float64) - 127), 32, axis=1)
    xb = B * np.repeat(np.exp2(SB.astype(np.float64) - 127), 32, axis=1)
    tp = pm.Dtd(ctx)
    Xa, Qa, Sa = quantise_dag(ctx, xa, tile, tile, fa, tp)  # all stay alive
    Xb, Qb, Sb = quantise_dag(ctx, xb, tile, tile, fb, tp)  # until the wait
    C = pm.TiledMatrix(ctx, size, size, tile, tile, 1, 1, elem_size=4)
    pm.insert_gemm_mxfp8(tp, Qa, Sa, Qb, Sb, C, fmt_a=fa, fmt_b=fb, alpha=2.0)
    tp.wait()
    for Q, S, x, fmt in ((Qa, Sa, xa, fa), (Qb, Sb, xb, fb)):
        wantQ, wantS = quant_reference(x, fmt)
        assert np.array_equal(untiled(S, np.uint8), wantS), (fa, fb)
        assert np.array_equal(untiled(Q, np.uint8), wantQ), (fa, fb)
    got = untiled(C, np.float32).T.astype(np.float64)
    assert np.array_equal(got, 2 * (xa @ xb.T)), (fa, fb)


@pytest.mark.gpu
def test_dag_gpu():
    ctx = pm.Context(nworkers=2, rank=0, world=1)
    check_dag(ctx, 512, 256, "e4m3", "e4m3")
    assert ctx.gpu_stats()["tasks"] >= 16
    del ctx


def test_dag_cpu_chores():
    ctx = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)
    for fa, fb in PAIRS + [("e5m2", "e5m2")]:
        check_dag(ctx, 128, 64, fa, fb)
    del ctx
