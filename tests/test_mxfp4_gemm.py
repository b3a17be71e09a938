"""MXFP4 tile-GEMM and quantiser: E2M1 elements two to a byte (element 2q in
the low nibble of byte q) with one E8M0 scale byte per row and 32 K elements.

  C[i,j] = alpha sum_b 2^(SA[i,b] + SB[j,b] - 254) sum_{p in b} A[i,p] B[j,p]

Wherever sums occur the elements are random draws over all 16 codes and the
scale bytes in {126, 127, 128} with k <= 1024: every product is a multiple of
2^-2, every scaled partial sum a multiple of 2^-4 below 1024 * 36 * 4 < 2^18,
22 bits, exact in fp32 in any order. So every check is bitwise equality with
the float64 value of the formula.
"""
import numpy as np
import pytest

import parsec_amd as pm
from parsec_amd import _core

VAL = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])
FAST, EDGE = (256, 256, 512), (130, 67, 45)


def pack(codes, pad=0):
    """rows x k codes as rows of ceil(k/2) + pad bytes, flat; the spare high
    nibble of an odd k holds code 15 (-6), which must be ignored."""
    rows, k = codes.shape
    c = np.full((rows, k + k % 2), 15, dtype=np.uint8)
    c[:, :k] = codes
    out = np.zeros((rows, c.shape[1] // 2 + pad), dtype=np.uint8)
    out[:, :c.shape[1] // 2] = c[:, 0::2] | (c[:, 1::2] << 4)
    return out.ravel()


def unpack(Q, k):
    return np.stack([Q & 15, Q >> 4], axis=-1).reshape(Q.shape[0], -1)[:, :k]


def padded(b, pad):
    out = np.zeros((b.shape[0], b.shape[1] + pad), dtype=np.uint8)
    out[:, :b.shape[1]] = b
    return out.ravel()


def reference(A, SA, B, SB):
    """The formula in float64; A, B are codes, SA, SB scale bytes."""
    def scaled(X, S):
        s = np.where(S == 255, np.nan, np.exp2(S.astype(np.float64) - 127))
        return VAL[X] * np.repeat(s, 32, axis=1)[:, :X.shape[1]]
    return scaled(A, SA) @ scaled(B, SB).T


def gemm(A, SA, B, SB, alpha=1.0, pad=0, spad=0, C0=None):
    m, k, n = A.shape[0], A.shape[1], B.shape[0]
    C = np.zeros((n, m), dtype=np.float32)  # col-major m x n
    if C0 is not None:
        C[:] = C0.T
    kbytes = (k + 1) // 2
    _core.gemm_mxfp4_hip(pack(A, pad), padded(SA, spad), pack(B, pad),
                         padded(SB, spad), C.ravel(), m, n, k, alpha=alpha,
                         lda=kbytes + pad, ldb=kbytes + pad,
                         ldsa=SA.shape[1] + spad, ldsb=SB.shape[1] + spad,
                         accum=C0 is not None)
    return C.T.astype(np.float64)


def operands(m, n, k, seed=0):
    rng = np.random.default_rng(seed)
    kb = (k + 31) // 32
    return (rng.integers(0, 16, (m, k)).astype(np.uint8),
            rng.integers(126, 129, (m, kb)).astype(np.uint8),
            rng.integers(0, 16, (n, k)).astype(np.uint8),
            rng.integers(126, 129, (n, kb)).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("role", ["A", "B"])
@pytest.mark.parametrize("m,n,k", [(16, 16, 256), FAST])
def test_routing(m, n, k, role):
    """Row i of the tested operand is 1.0 at element i % 256 under scale byte
    1 + i % 254 in that block (127 elsewhere); the other operand is a one-hot
    identity under byte 127. C[i, i % 256] is that row's power of two alone: a
    wrong nibble order, lane-K layout, scale block, op_sel byte or operand
    shows as a wrong power of two or a wrong column."""
    rows = np.arange(m)
    X = np.zeros((m, k), dtype=np.uint8)
    X[rows, rows % 256] = 2
    SX = np.full((m, k // 32), 127, dtype=np.uint8)
    SX[rows, (rows % 256) // 32] = 1 + rows % 254
    E = np.zeros((n, k), dtype=np.uint8)
    E[np.arange(min(n, 256)), np.arange(min(n, 256))] = 2
    SE = np.full((n, k // 32), 127, dtype=np.uint8)
    args = (X, SX, E, SE) if role == "A" else (E, SE, X, SX)
    want = reference(*args)
    assert np.count_nonzero(want) == m
    assert np.array_equal(gemm(*args), want)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,pad,spad,alpha,accum", [
    FAST + (0, 0, 1.0, False),             # fast path, minimum K depth
    (256, 256, 768, 0, 0, 1.0, False),     # ring wraps, scale slot alternates
    (512, 256, 512, 0, 0, 1.0, False),     # more than one block
    EDGE + (0, 0, 1.0, False),             # odd k, spare nibble set, tight
    EDGE + (3, 1, 1.0, False),             # ... and padded lda / ldsa
    (256, 256, 200, 0, 0, 1.0, False),     # k no multiple of the step: edge
    FAST + (0, 1, 1.0, False),             # unaligned scale stride: edge
    FAST + (0, 0, 0.5, True),
    EDGE + (0, 0, 0.5, True),
])
def test_exact_sums(m, n, k, pad, spad, alpha, accum):
    A, SA, B, SB = operands(m, n, k)
    C0 = np.random.default_rng(1).integers(-8, 9, (m, n)).astype(np.float64)
    got = gemm(A, SA, B, SB, alpha, pad, spad, C0 if accum else None)
    assert np.array_equal(got, alpha * reference(A, SA, B, SB)
                          + (C0 if accum else 0))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [FAST, EDGE])
def test_nan_scale(m, n, k):
    A, SA, B, SB = operands(m, n, k, seed=3)
    SA[m - 3, 1] = 255
    want = reference(A, SA, B, SB)
    assert np.isnan(want[m - 3]).all() and np.isnan(want).sum() == n
    assert np.array_equal(gemm(A, SA, B, SB), want, equal_nan=True)


# ------------------------------------------------------------- quantiser
def quant_reference(x):
    """(element values, S bytes) of x (rows x k, fp32): nearest table entry,
    ties to the even code."""
    rows, k = x.shape
    kb = (k + 31) // 32
    blocks = np.zeros((rows, kb * 32))
    blocks[:, :k] = x
    blocks = blocks.reshape(rows, kb, 32)
    amax = np.abs(blocks).max(axis=2)
    X = np.clip(np.frexp(amax)[1] - 1 - 2, -127, 127)  # floor(log2) - 2
    X[amax == 0] = 0
    y = np.clip(blocks * np.exp2(-X.astype(np.float64))[:, :, None], -6, 6)
    order = np.array([0, 2, 4, 6, 1, 3, 5, 7])  # argmin takes the first: even
    code = order[np.abs(np.abs(y)[..., None] - VAL[order]).argmin(axis=-1)]
    return ((np.sign(y) * VAL[code]).reshape(rows, kb * 32)[:, :k],
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
    x[2, 70] = 1.9                                  # 1.9 * 4 clamps to 6
    x[3, 0:32] = 0                                  # scale 1; the ties go to
    x[3, 0:8] = [6, 0.25, 0.75, 1.25, 2.5, 3.5, 5.0, -2.5]  # 0 1 1 2 4 4 -2
    return x.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,k,pad", [(64, 256, 0), (5, 77, 0), (64, 256, 4),
                                        (64, 256, 1)])
def test_quantiser(rows, k, pad):
    x = quant_input(rows, k)
    buf = np.zeros((rows, k + pad), dtype=np.float32)
    buf[:, :k] = x
    Q, S = _core.quantize_mxfp4_hip(buf.ravel(), rows, k, ldx=k + pad)
    want, wantS = quant_reference(x)
    assert list(want[3, :8]) == [6, 0, 1, 1, 2, 4, 4, -2]
    assert np.array_equal(S, wantS)
    assert np.array_equal(VAL[unpack(Q, k)], want)
    assert k % 2 == 0 or not (Q[:, -1] >> 4).any()  # the spare nibble is 0


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


def quantise_dag(ctx, x, mb, nb, tp):
    """x (rows x even K) in element tiles of mb x nb -> (X, Q, S)."""
    rows, k = x.shape
    X = tiled(ctx, x, mb, nb, np.float32)
    Q = tiled(ctx, np.zeros((rows, k // 2), np.uint8), mb // 2, nb, np.uint8)
    S = tiled(ctx, np.zeros((rows, (k + 31) // 32), np.uint8), mb // 32, nb,
              np.uint8)
    pm.insert_quantize_mxfp4(tp, X, Q, S)
    return X, Q, S


@pytest.mark.parametrize("rows,k,mb,nb", [(64, 256, 128, 32), (5, 78, 64, 4)])
def test_quantiser_cpu_chore(rows, k, mb, nb):
    ctx = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)  # CPU chores only
    x = quant_input(rows, k)
    tp = pm.Dtd(ctx)
    X, Q, S = quantise_dag(ctx, x, mb, nb, tp)
    tp.wait()
    want, wantS = quant_reference(x)
    assert np.array_equal(untiled(S, np.uint8), wantS)
    assert np.array_equal(VAL[unpack(untiled(Q, np.uint8), k)], want)
    del ctx


def check_dag(ctx, size, tile, alpha):
    """Quantise fp32 operands (the exact-sum data times its block scales, a
    6 in every block, so the quantiser recovers codes and scales exactly),
    then multiply. Returns the number of inserted tasks."""
    A, SA, B, SB = operands(size, size, size, seed=6)
    A[:, ::32] = B[:, ::32] = 7
    xa = VAL[A] * np.repeat(np.exp2(SA.astype(np.float64) - 127), 32, axis=1)
    xb = VAL[B] * np.repeat(np.exp2(SB.astype(np.float64) - 127), 32, axis=1)
    tp = pm.Dtd(ctx)
    Xa, Qa, Sa = quantise_dag(ctx, xa, tile, tile, tp)  # all stay alive
    Xb, Qb, Sb = quantise_dag(ctx, xb, tile, tile, tp)  # until the wait
    C = pm.TiledMatrix(ctx, size, size, tile, tile, 1, 1, elem_size=4)
    pm.insert_gemm_mxfp4(tp, Qa, Sa, Qb, Sb, C, alpha=alpha)
    tp.wait()
    for Q, S, codes, scales in ((Qa, Sa, A, SA), (Qb, Sb, B, SB)):
        assert np.array_equal(untiled(S, np.uint8), scales)
        assert np.array_equal(VAL[unpack(untiled(Q, np.uint8), size)],
                              VAL[codes])
    got = untiled(C, np.float32).T.astype(np.float64)
    assert np.array_equal(got, alpha * (xa @ xb.T))
    return 2 * Xa.mt * Xa.nt + C.mt * C.nt * Qa.mt


@pytest.mark.gpu
def test_dag_gpu():
    ctx = pm.Context(nworkers=2, rank=0, world=1)
    tasks = check_dag(ctx, 512, 256, 2.0)
    assert tasks == 16 and ctx.gpu_stats()["tasks"] >= tasks
    del ctx


def test_dag_cpu_chores():
    ctx = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)
    check_dag(ctx, 128, 64, 1.0)
    del ctx
