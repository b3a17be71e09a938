"""bf16 tile-GEMM for column-major operands: the NN, NT and TT layouts.

Inputs are integer-valued bf16 in [-4, 4] (C starts as small integers when
accumulating) and k <= 1024, so every partial sum is an integer below 2^14:
fp32 accumulation is exact in any order and the check is bitwise equality
with a float64 product of the same integers.
"""
import numpy as np
import pytest

import parsec_amd as pm
from parsec_amd import _core

LAYOUTS = [("N", "N"), ("N", "T"), ("T", "T")]
TILE = 256  # the fast kernel's block tile; its K-loop needs k >= 128, k % 32 == 0


def pack(x):
    """Integer-valued float array -> bf16 bit patterns (exact for |x| < 256)."""
    return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def lay(X, kmajor, ld=0):
    """Flat column-major buffer of X (rows x K): K-major stores K x rows,
    otherwise rows x K, with leading dimension ld (0: tight)."""
    S = X.T if kmajor else X
    ld = ld or S.shape[0]
    buf = np.zeros((S.shape[1], ld), dtype=np.uint16)
    buf[:, :S.shape[0]] = pack(S).T
    return buf.ravel()


def operands(m, n, k, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(-4, 5, (m, k)).astype(np.float64),
            rng.integers(-4, 5, (n, k)).astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("m,n,k,pad", [
    (16, 16, 32, 0),             # one MFMA
    (1, 1, 1, 0),                # everything guarded
    (TILE, TILE, 128, 0),        # fast path, minimum K-loop depth
    (TILE, TILE, 160, 0),        # one K step longer: the LDS ring wraps
    (130, 67, 45, 0),            # odd tight ld: element loads
    (130, 67, 45, 3),            # padded ld = stored rows + 3
    (TILE, TILE, 150, 0),        # k no multiple of the K step: edge kernel
])
def test_kernel_layouts(ta, tb, m, n, k, pad):
    A, B = operands(m, n, k)
    lda = ((m if ta == "N" else k) + pad) if pad else 0
    ldb = ((n if tb == "T" else k) + pad) if pad else 0
    C = np.zeros((n, m), dtype=np.float32)  # col-major m x n
    _core.gemm_bf16_hip(lay(A, ta == "T", lda), lay(B, tb == "N", ldb),
                        C.ravel(), m, n, k, transa=ta, transb=tb, lda=lda,
                        ldb=ldb)
    assert np.array_equal(C.T.astype(np.float64), A @ B.T)


@pytest.mark.gpu
@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("m,n,k", [(TILE, TILE, 128), (130, 67, 45)])
def test_kernel_overwrite_vs_accumulate(accum, m, n, k):
    A, B = operands(m, n, k, seed=1)
    C0 = np.random.default_rng(2).integers(-8, 9, (m, n)).astype(np.float64)
    C = np.ascontiguousarray(C0.T, dtype=np.float32)
    _core.gemm_bf16_hip(lay(A, False), lay(B, True), C.ravel(), m, n, k,
                        transa="N", transb="N", accum=accum)
    assert np.array_equal(C.T.astype(np.float64),
                          A @ B.T + (C0 if accum else 0))


def run_dag(ctx, A, B, tile, ta, tb):
    """C = A B^T (A: M x K, B: N x K integer-valued) through insert_gemm_bf16
    with the operands tiled in the given layouts."""
    def tiled(X, kmajor):
        S = X.T if kmajor else X
        T = pm.TiledMatrix(ctx, S.shape[0], S.shape[1], tile, tile, 1, 1,
                           elem_size=2)
        for i in range(T.mt):
            for j in range(T.nt):
                blk = S[i * tile:(i + 1) * tile, j * tile:(j + 1) * tile]
                T.tile_bytes_set(i, j, pack(blk).T.tobytes())
        return T

    At, Bt = tiled(A, ta == "T"), tiled(B, tb == "N")
    C = pm.TiledMatrix(ctx, A.shape[0], B.shape[0], tile, tile, 1, 1,
                       elem_size=4)
    tp = pm.Dtd(ctx)
    pm.insert_gemm_bf16(tp, At, Bt, C, transa=ta, transb=tb)
    tp.wait()
    got = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    for i in range(C.mt):
        for j in range(C.nt):
            raw = np.frombuffer(C.tile_bytes(i, j), dtype=np.float32)
            got[i * tile:(i + 1) * tile, j * tile:(j + 1) * tile] = \
                raw.reshape((tile, tile)).T
    return got


@pytest.mark.gpu
def test_dag_gpu_nn():
    ctx = pm.Context(nworkers=2, rank=0, world=1)
    A, B = operands(2 * TILE, 2 * TILE, 2 * TILE, seed=3)
    got = run_dag(ctx, A, B, TILE, "N", "N")
    assert ctx.gpu_stats()["tasks"] >= 8
    assert np.array_equal(got.astype(np.float64), A @ B.T)
    del ctx


def test_dag_cpu_layouts():
    ctx = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)  # CPU chores only
    A, B = operands(128, 128, 128, seed=4)
    tn = run_dag(ctx, A, B, 64, "T", "N")
    assert np.array_equal(tn.astype(np.float64), A @ B.T)
    for ta, tb in LAYOUTS:
        assert np.array_equal(run_dag(ctx, A, B, 64, ta, tb), tn), (ta, tb)
