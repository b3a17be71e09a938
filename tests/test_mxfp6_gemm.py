"""MXFP6 tile-GEMM and quantiser: 6-bit E2M3 / E3M2 elements, element p in
bits [6p, 6p + 6) of the row read as a little-endian bit string, with one
E8M0 scale byte per row and 32 K elements.

  C[i,j] = alpha sum_b 2^(SA[i,b] + SB[j,b] - 254) sum_{p in b} A[i,p] B[j,p]

Every GPU check is bitwise equality with the float64 value of the formula,
because the inputs make every partial sum exact in fp32 in any order:

  E2M3   all 64 codes (multiples of 2^-3, at most 7.5), scale bytes in
         {127, 128}, k <= 1024: a product is a multiple of 2^-6 of at most
         56.25, a scaled partial sum a multiple of 2^-6 below
         1024 * 56.25 * 4 = 230400 < 2^18: 24 bits.
  E3M2   the codes with exponent field 2..4 (0.5 .. 3.5 in steps of 2^-3):
         products are multiples of 2^-6 of at most 12.25 (26.25 against
         E2M3), sums below 1024 * 26.25 * 4 < 2^17: 23 bits. The remaining
         codes are decoded by test_routing.
  alpha = 0.5 with an integer C0 in [-8, 8]: k <= 512 halves the bound, so
         alpha * sum is a multiple of 2^-7 below 2^16 + 8: 24 bits.
  DAG    one largest code (7.5 / 28) per block of 32 at size <= 512: at most
         16 products of 7.5 * 28 = 210 beside the above, below
         (16 * 210 + 512 * 26.25) * 4 < 2^17: 23 bits; alpha = 2 is exact.

test_routing has one product per result; it is compared with the float64
value rounded to fp32, which is exact except where 2^127 times a value above
2 overflows to an infinity on both sides.
"""
import numpy as np
import pytest

import parsec_amd as pm
from parsec_amd import _core

_c = np.arange(64)
_s = np.where(_c & 32, -1.0, 1.0)
VAL = {
    "e2m3": _s * np.where((_c >> 3) & 3, (8 + (_c & 7)) * np.exp2(((_c >> 3) & 3) - 4.0),
                          (_c & 7) / 8),
    "e3m2": _s * np.where((_c >> 2) & 7, (4 + (_c & 3)) * np.exp2(((_c >> 2) & 7) - 5.0),
                          (_c & 3) / 16),
}
ONE = {"e2m3": 8, "e3m2": 12}    # the code of 1.0
EMAX = {"e2m3": 2, "e3m2": 4}
FAST, EDGE = (256, 256, 256), (130, 67, 45)


def pack(codes, pad=0):
    """rows x k codes as rows of ceil(3k/4) + pad bytes, flat; the spare high
    bits of the last byte are ones, which must be ignored."""
    rows, k = codes.shape
    bits = np.ones((rows, (6 * k + 7) // 8 * 8), dtype=np.uint8)
    bits[:, :6 * k] = ((codes[:, :, None] >> np.arange(6)) & 1).reshape(rows, -1)
    out = np.zeros((rows, bits.shape[1] // 8 + pad), dtype=np.uint8)
    out[:, :bits.shape[1] // 8] = np.packbits(bits, axis=1, bitorder="little")
    return out.ravel()


def unpack(Q, k):
    bits = np.unpackbits(Q, axis=1, bitorder="little")[:, :6 * k]
    return bits.reshape(Q.shape[0], k, 6) @ (1 << np.arange(6))


def padded(b, pad):
    out = np.zeros((b.shape[0], b.shape[1] + pad), dtype=np.uint8)
    out[:, :b.shape[1]] = b
    return out.ravel()


def reference(A, SA, B, SB, fa, fb):
    """The formula in float64; A, B are codes, SA, SB scale bytes."""
    def scaled(X, S, f):
        s = np.where(S == 255, np.nan, np.exp2(S.astype(np.float64) - 127))
        return VAL[f][X] * np.repeat(s, 32, axis=1)[:, :X.shape[1]]
    return scaled(A, SA, fa) @ scaled(B, SB, fb).T


def gemm(A, SA, B, SB, fa, fb, alpha=1.0, pad=0, spad=0, C0=None):
    m, k, n = A.shape[0], A.shape[1], B.shape[0]
    C = np.zeros((n, m), dtype=np.float32)  # col-major m x n
    if C0 is not None:
        C[:] = C0.T
    kbytes = (3 * k + 3) // 4
    _core.gemm_mxfp6_hip(pack(A, pad), padded(SA, spad), pack(B, pad),
                         padded(SB, spad), C.ravel(), m, n, k, a_format=fa,
                         b_format=fb, alpha=alpha, lda=kbytes + pad,
                         ldb=kbytes + pad, ldsa=SA.shape[1] + spad,
                         ldsb=SB.shape[1] + spad, accum=C0 is not None)
    return C.T.astype(np.float64)


def codes(rng, rows, k, f):
    if f == "e2m3":
        return rng.integers(0, 64, (rows, k)).astype(np.uint8)
    return (rng.integers(8, 20, (rows, k)) + 32 * rng.integers(0, 2, (rows, k))
            ).astype(np.uint8)


def operands(m, n, k, fa, fb, seed=0):
    rng = np.random.default_rng(seed)
    kb = (k + 31) // 32
    return (codes(rng, m, k, fa), rng.integers(127, 129, (m, kb)).astype(np.uint8),
            codes(rng, n, k, fb), rng.integers(127, 129, (n, kb)).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["e2m3", "e3m2"])
@pytest.mark.parametrize("role", ["A", "B"])
@pytest.mark.parametrize("m,n,k", [(16, 16, 256), FAST])
def test_routing(m, n, k, role, fmt):
    """Row i of the tested operand holds code i % 64 at element i % 256 under
    scale byte 1 + i % 254 in that block (127 elsewhere); the other operand,
    in the other format, is a one-hot 1.0 identity under byte 127. C[i, i % 256]
    is one table value times one power of two: a wrong bit order inside the
    3-byte groups, lane-K layout, scale block, op_sel byte, operand order or
    decoding of any of the 64 codes shows as a wrong value or column."""
    other = "e3m2" if fmt == "e2m3" else "e2m3"
    rows = np.arange(m)
    X = np.zeros((m, k), dtype=np.uint8)
    X[rows, rows % 256] = rows % 64
    SX = np.full((m, k // 32), 127, dtype=np.uint8)
    SX[rows, (rows % 256) // 32] = 1 + rows % 254
    E = np.zeros((n, k), dtype=np.uint8)
    E[np.arange(min(n, 256)), np.arange(min(n, 256))] = ONE[other]
    SE = np.full((n, k // 32), 127, dtype=np.uint8)
    args = (X, SX, E, SE, fmt, other) if role == "A" else (E, SE, X, SX, other, fmt)
    with np.errstate(over="ignore"):
        want = reference(*args).astype(np.float32).astype(np.float64)
    assert np.count_nonzero(want) == m - (m + 31) // 32  # codes 0 and 32 are 0
    assert np.array_equal(gemm(*args), want)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,fa,fb,pad,spad,alpha,accum", [
    FAST + ("e2m3", "e2m3", 0, 0, 1.0, False),         # minimum K depth
    (256, 256, 768, "e2m3", "e2m3", 0, 0, 1.0, False),  # every slot reused
    (512, 256, 256, "e3m2", "e3m2", 0, 0, 1.0, False),  # more than one block
    (256, 256, 384, "e2m3", "e3m2", 0, 0, 1.0, False),  # mixed, odd step count
    EDGE + ("e2m3", "e2m3", 0, 0, 1.0, False),          # spare bits set, tight
    EDGE + ("e3m2", "e2m3", 3, 1, 1.0, False),          # padded lda / ldsa
    (256, 256, 200, "e3m2", "e3m2", 0, 0, 1.0, False),  # k no multiple: edge
    FAST + ("e2m3", "e2m3", 0, 1, 1.0, False),          # scale stride: edge
    (256, 256, 512, "e2m3", "e3m2", 0, 0, 0.5, True),
    EDGE + ("e2m3", "e2m3", 0, 0, 0.5, True),
])
def test_exact_sums(m, n, k, fa, fb, pad, spad, alpha, accum):
    A, SA, B, SB = operands(m, n, k, fa, fb)
    C0 = np.random.default_rng(1).integers(-8, 9, (m, n)).astype(np.float64)
    got = gemm(A, SA, B, SB, fa, fb, alpha, pad, spad, C0 if accum else None)
    assert np.array_equal(got, alpha * reference(A, SA, B, SB, fa, fb)
                          + (C0 if accum else 0))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [FAST, EDGE])
def test_nan_scale(m, n, k):
    A, SA, B, SB = operands(m, n, k, "e2m3", "e3m2", seed=3)
    SA[m - 3, 1] = 255
    want = reference(A, SA, B, SB, "e2m3", "e3m2")
    assert np.isnan(want[m - 3]).all() and np.isnan(want).sum() == n
    assert np.array_equal(gemm(A, SA, B, SB, "e2m3", "e3m2"), want,
                          equal_nan=True)


# ------------------------------------------------------------- quantiser
TIES = {  # a block under scale 1: (input, expected) with every tie to even
    "e2m3": ([7.5, 0.0625, 0.1875, 2.125, 2.375, 4.25, 6.75, -2.125],
             [7.5, 0, 0.25, 2, 2.5, 4, 7, -2]),
    "e3m2": ([28, 0.03125, 0.09375, 1.125, 1.375, 4.5, 18, -9],
             [28, 0, 0.125, 1, 1.5, 4, 16, -8]),
}


def quant_reference(x, f):
    """(element values, S bytes) of x (rows x k, fp32): nearest table entry,
    ties to the even code."""
    rows, k = x.shape
    kb = (k + 31) // 32
    blocks = np.zeros((rows, kb * 32))
    blocks[:, :k] = x
    blocks = blocks.reshape(rows, kb, 32)
    amax = np.abs(blocks).max(axis=2)
    X = np.clip(np.frexp(amax)[1] - 1 - EMAX[f], -127, 127)  # floor(log2) - emax
    X[amax == 0] = 0
    lim = VAL[f][31]
    y = np.clip(blocks * np.exp2(-X.astype(np.float64))[:, :, None], -lim, lim)
    order = np.r_[0:32:2, 1:32:2]  # argmin takes the first: the even code
    code = order[np.abs(np.abs(y)[..., None] - VAL[f][order]).argmin(axis=-1)]
    return ((np.sign(y) * VAL[f][code]).reshape(rows, kb * 32)[:, :k],
            (X + 127).astype(np.uint8))


def quant_input(rows, k, f):
    rng = np.random.default_rng(5)
    kb = (k + 31) // 32
    mag = np.exp2(rng.uniform(-20, 20, (rows, kb)))
    x = rng.standard_normal((rows, k)) * np.repeat(mag, 32, axis=1)[:, :k]
    x[0, 0:32] = 0                                  # an all-zero block
    x[1, 32:64] = rng.uniform(-1, 1, 32)
    x[1, 40] = 32.0                                 # amax a power of two
    x[2, 64:min(k, 96)] = rng.uniform(-1, 1, min(k, 96) - 64)
    x[2, 70] = 1.9                                  # 1.9 * 2^emax clamps
    x[3, 0:32] = 0
    x[3, 0:8] = TIES[f][0]
    return x.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("f", ["e2m3", "e3m2"])
@pytest.mark.parametrize("rows,k,pad", [(64, 256, 0), (5, 77, 0), (64, 256, 4),
                                        (64, 256, 1)])
def test_quantiser(rows, k, pad, f):
    x = quant_input(rows, k, f)
    buf = np.zeros((rows, k + pad), dtype=np.float32)
    buf[:, :k] = x
    Q, S = _core.quantize_mxfp6_hip(buf.ravel(), rows, k, format=f, ldx=k + pad)
    want, wantS = quant_reference(x, f)
    assert list(want[3, :8]) == TIES[f][1]
    assert np.array_equal(S, wantS)
    assert np.array_equal(VAL[f][unpack(Q, k)], want)
    assert not (Q[:, -1] >> ((6 * k - 1) % 8 + 1)).any()  # spare bits are 0


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


def quantise_dag(ctx, x, mb, nb, tp, f):
    """x (rows x K, K % 4 == 0) in element tiles of mb x nb -> (X, Q, S)."""
    rows, k = x.shape
    X = tiled(ctx, x, mb, nb, np.float32)
    Q = tiled(ctx, np.zeros((rows, 3 * k // 4), np.uint8), 3 * mb // 4, nb,
              np.uint8)
    S = tiled(ctx, np.zeros((rows, (k + 31) // 32), np.uint8), mb // 32, nb,
              np.uint8)
    pm.insert_quantize_mxfp6(tp, X, Q, S, format=f)
    return X, Q, S


@pytest.mark.parametrize("f", ["e2m3", "e3m2"])
@pytest.mark.parametrize("rows,k,mb,nb", [(64, 256, 128, 32), (5, 76, 64, 4)])
def test_quantiser_cpu_chore(rows, k, mb, nb, f):
    ctx = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)  # CPU chores only
    x = quant_input(rows, k, f)
    tp = pm.Dtd(ctx)
    X, Q, S = quantise_dag(ctx, x, mb, nb, tp, f)
    tp.wait()
    want, wantS = quant_reference(x, f)
    assert np.array_equal(untiled(S, np.uint8), wantS)
    assert np.array_equal(VAL[f][unpack(untiled(Q, np.uint8), k)], want)
    del ctx


def check_dag(ctx, size, tile, alpha, fa="e2m3", fb="e3m2"):
    """Quantise fp32 operands (the exact-sum data times its block scales, a
    largest-magnitude code in every block, so the quantiser recovers codes
    and scales exactly), then multiply. Returns the number of inserted
    tasks."""
    A, SA, B, SB = operands(size, size, size, fa, fb, seed=6)
    A[:, ::32] = B[:, ::32] = 31
    xa = VAL[fa][A] * np.repeat(np.exp2(SA.astype(np.float64) - 127), 32, axis=1)
    xb = VAL[fb][B] * np.repeat(np.exp2(SB.astype(np.float64) - 127), 32, axis=1)
    tp = pm.Dtd(ctx)
    Xa, Qa, Sa = quantise_dag(ctx, xa, tile, tile, tp, fa)  # all stay alive
    Xb, Qb, Sb = quantise_dag(ctx, xb, tile, tile, tp, fb)  # until the wait
    C = pm.TiledMatrix(ctx, size, size, tile, tile, 1, 1, elem_size=4)
    pm.insert_gemm_mxfp6(tp, Qa, Sa, Qb, Sb, C, alpha=alpha, a_format=fa,
                         b_format=fb)
    tp.wait()
    for Q, S, c, scales, f in ((Qa, Sa, A, SA, fa), (Qb, Sb, B, SB, fb)):
        assert np.array_equal(untiled(S, np.uint8), scales)
        assert np.array_equal(VAL[f][unpack(untiled(Q, np.uint8), size)],
                              VAL[f][c])
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
