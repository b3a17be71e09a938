// Hand-written CDNA4 (gfx950) fp64 MFMA tile kernels.
//
// The reference ships no compute kernels (JDF bodies call
// cuBLAS); these are the hand-optimized chores for the headline dense
// apps, written for the gfx950 execution model directly.
//
// v_mfma_f64_16x16x4f64: one wave computes a 16x16 fp64 tile with K-step 4,
// 2048 FLOP per instruction at ~64 cycles/SIMD (the fp64 matrix rate equals
// the fp64 vector rate on MI355X, ~78.6 TF/s chip peak). At that cadence an
// LDS-staged 128x128 block is compute-bound: staging and even bank
// conflicts hide under the matrix pipe, so the kernels aim for clean global
// coalescing and independent accumulators per wave (MI355X_MICROARCH.md:
// per-instruction constants; fragment maps per cdna4 ISA: A[i=l&15][k=l>>4],
// B[k=l>>4][j=l&15]; C/D element e of lane l is D[4*e + (l>>4)][l&15] —
// verified on gfx950 hardware: the register index strides ROWS by 4, unlike
// the f32/bf16 16x16 map where (l>>4) selects the 4-row group).
//
// What is here:
//  - k_dgemm_nt_v3<KIND>, the glds full-tile kernel: operands staged
//    global->LDS asynchronously, 16 B per lane. It needs full 128-blocks,
//    whole K-tiles and even leading dimensions (full_tiles below). Three
//    kinds share the body:
//      V3_GEMM  C -= A B^T, the Cholesky trailing update
//               (PARSEC_MCA_chore_gemm=hip|rocblas)
//      V3_SYRK  C -= A A^T on the lower block set only: the SYRK tile task
//               (chore_syrk) and, one launch per 128-panel, the trailing
//               update inside the blocked tile POTRF, in place of
//               rocblas_dsyrk's several small k=128 launches on the DAG's
//               critical path (chore_potrf_syrk=hip|rocblas)
//      V3_TRMM  X = B W^T with W = L^-1 lower triangular, the
//               TRSM-by-inverse product: each output block column's K loop
//               stops at its diagonal block, where a dense dgemm spends half
//               its flops on W's stored zeros (chore_trsm_inv=hip|rocblas)
//  - k_dgemm_nt_v2<TRI>, the bounds-checked kernel for every other GEMM and
//    SYRK shape: register-staged, zero-filled past the edges.
//  - k_dgemm_tn<KIND>, the bounds-checked kernel for C (+)= A^T B with
//    triangular kinds: the LAUUM phase of the SPD inverse
//    (chore_lauum=hip|rocblas, chore_gemm_tn=hip|rocblas).
//  - k_dgemm_nn, the bounds-checked kernel for C -= A B: the update of the
//    triangular solve sweeps and LU's trailing update
//    (chore_gemm_nn=hip|rocblas).
//  - k_potf2_mfma, the in-LDS Cholesky of one <=128 diagonal block.
#include "kernels_hip.hpp"

#include "kernels.hpp"
#include "kernels_bench.hpp"

namespace pa {

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define BM 128
#define BN 128
#define BKD 16

// Both GEMM kernels run 8 waves as 4(M) x 2(N) on a 128x128 block, each
// wave owning 32x64 as 2x4 MFMA fragments (64 accumulator VGPRs), with K
// double-buffered in LDS BKD deep. Two blocks are co-resident on a CU,
// which hides each one's staging under the other's MFMA phase (fp64 MFMA
// issue is 64 cyc/SIMD, so 4 co-resident waves/SIMD keep the matrix pipe
// fed without hand pipelining).

// 1-D grid with a bijective XCD-aware remap so consecutive blocks share B
// panels within one XCD's L2 (guide T1).
__device__ __forceinline__ int xcd_swizzle(int id, int nwg) {
  int q = nwg >> 3, r = nwg & 7;
  int xcd = id & 7, pos = id >> 3;
  // blocks per XCD: first r XCDs get q+1
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

// id -> (i >= j) over a lower-triangular set enumerated row by row.
__device__ __forceinline__ void tri_decode(int id, int& i, int& j) {
  i = 0;
  while (id > i) { i++; id -= i; }
  j = id;
}

// This block's (bx, by): in the nbx-wide full grid, or in the lower block
// set (SYRK writes only the lower blocks; diagonal blocks compute their
// full tile: the upper half of a diagonal tile is symmetric-valid and never
// read by the DAG).
__device__ __forceinline__ void block_decode(bool tri, int nbx, int& bx,
                                             int& by) {
  int id = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tri) {
    tri_decode(id, bx, by);
  } else {
    bx = id % nbx;
    by = id / nbx;
  }
}

// One BKD-deep K-tile into the wave's 2x4 accumulators. ap / bp point at
// this lane's element of the first A / B fragment in a [k][row] LDS image
// whose K-rows are ld doubles apart.
__device__ __forceinline__ void mfma_ktile(f64x4 (&acc)[2][4],
                                           const double* ap, const double* bp,
                                           int ld) {
#pragma unroll
  for (int kk = 0; kk < BKD; kk += 4) {
    double a[2], b[4];
#pragma unroll
    for (int f = 0; f < 2; f++) a[f] = ap[kk * ld + f * 16];
#pragma unroll
    for (int f = 0; f < 4; f++) b[f] = bp[kk * ld + f * 16];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] =
            __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
  }
}

// Accumulators to C: element e of fragment (i, j) is
// C[row0 + 16 i + 4 e][col0 + 16 j]. store writes C = acc, otherwise
// C -= acc; checked drops what lies outside m x n.
__device__ __forceinline__ void write_c(const f64x4 (&acc)[2][4], double* C,
                                        int ldc, int row0, int col0, int m,
                                        int n, bool checked, bool store) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    int col = col0 + j * 16;
    if (checked && col >= n) continue;
    double* cp = C + (size_t)col * ldc;
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        int row = row0 + i * 16 + e * 4;
        if (checked && row >= m) continue;
        if (store) cp[row] = acc[i][j][e];
        else cp[row] -= acc[i][j][e];
      }
    }
  }
}

// ------------------------------------------------------------------ v2
// Bounds-checked kernel: operands go through registers into a [k][129]
// padded LDS image, zero-filled outside m, n and k (LDS 66 KB). TRI
// selects the lower block set (SYRK).
template <bool TRI>
__launch_bounds__(512)
__global__ void k_dgemm_nt_v2(int m, int n, int k, const double* __restrict__ A,
                              int lda, const double* __restrict__ B, int ldb,
                              double* __restrict__ C, int ldc, int nbx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LDT = 129;
  double* As = (double*)smem;                  // [2][BKD][LDT]
  double* Bs = As + 2 * BKD * LDT;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  int bx, by;
  block_decode(TRI, nbx, bx, by);
  const int bm0 = bx * BM, bn0 = by * BN;
  const int ksub = lane >> 4, r16 = lane & 15;

  f64x4 acc[2][4] = {};

  auto stage = [&](int buf, int k0) {
    double* as = As + buf * BKD * LDT;
    double* bs = Bs + buf * BKD * LDT;
#pragma unroll
    for (int x = 0; x < BM * BKD; x += 512) {
      int xi = x + tid;
      int i = xi & (BM - 1), kk = xi >> 7;
      int gi = bm0 + i, gk = k0 + kk;
      as[kk * LDT + i] = (gi < m && gk < k) ? A[(size_t)gk * lda + gi] : 0.0;
    }
#pragma unroll
    for (int x = 0; x < BN * BKD; x += 512) {
      int xi = x + tid;
      int j = xi & (BN - 1), kk = xi >> 7;
      int gj = bn0 + j, gk = k0 + kk;
      bs[kk * LDT + j] = (gj < n && gk < k) ? B[(size_t)gk * ldb + gj] : 0.0;
    }
  };

  stage(0, 0);
  __syncthreads();
  const int ntiles = (k + BKD - 1) / BKD;
  for (int t = 0; t < ntiles; t++) {
    if (t + 1 < ntiles) stage((t + 1) & 1, (t + 1) * BKD);
    mfma_ktile(acc, As + ((t & 1) * BKD + ksub) * LDT + wr * 32 + r16,
               Bs + ((t & 1) * BKD + ksub) * LDT + wc * 64 + r16, LDT);
    __syncthreads();
  }
  write_c(acc, C, ldc, bm0 + wr * 32 + ksub, bn0 + wc * 64 + r16, m, n,
          /*checked=*/true, /*store=*/false);
}

// ------------------------------------------------------------------ v3
// glds-staged kernel (the structure that lifted the bf16 kernel 2x): async
// global->LDS (16 B/lane), [k][m] lane-linear LDS image (one K-row = 1 KB
// per glds), one drain barrier per K-tile (LDS 64 KB). Full tiles only.
//
// V3_TRMM has B (n x n, k == n) lower triangular: output block column `by`
// only sees k < (by+1)*BN, so its K loop stops there (the diagonal K-block
// still reads B's strictly-upper entries, which must be stored zeros), and
// the epilogue stores instead of subtracting (beta = 0: C is never read).
// Its block columns carry K lengths from BN to n, so the block order
// decides both the balance between XCDs (blocks are dealt to them
// round-robin by blockIdx) and the length of the tail. In the snake order
// used here each XCD owns whole block columns (its blocks share the W panel
// in that XCD's L2), dealt longest-first in a boustrophedon over the XCDs so
// every XCD gets the same total K; the grid is padded to
// 8 * ceil(nby/8) * nbx and padding blocks exit at once.
enum { V3_GEMM = 0, V3_SYRK = 1, V3_TRMM = 2 };

template <int KIND>
__launch_bounds__(512)
__global__ void k_dgemm_nt_v3(int m, int n, int k, const double* __restrict__ A,
                              int lda, const double* __restrict__ B, int ldb,
                              double* __restrict__ C, int ldc, int nbx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* As = (double*)smem;                  // [2][BKD][BM]
  double* Bs = As + 2 * BKD * BM;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  int bx, by;
  if (KIND == V3_TRMM) {
    const int nby = n / BN;
    const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
    const int round = pos / nbx;
    const int rank = round * 8 + ((round & 1) ? 7 - xcd : xcd);
    if (rank >= nby) return;  // padding block (whole block, before any barrier)
    bx = pos - round * nbx;
    by = nby - 1 - rank;
  } else {
    block_decode(KIND == V3_SYRK, nbx, bx, by);
  }
  const int bm0 = bx * BM, bn0 = by * BN;
  const int ksub = lane >> 4, r16 = lane & 15;
  const int kend = KIND == V3_TRMM ? (bn0 + BN < k ? bn0 + BN : k) : k;

  f64x4 acc[2][4] = {};

  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int p = 0; p < 2; p++) {
      int krow = wave * 2 + p;
      const double* srcA = A + (size_t)(k0 + krow) * lda + bm0 + 2 * lane;
      double* dstA = As + buf * BKD * BM + krow * BM;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)srcA,
          (__attribute__((address_space(3))) unsigned int*)dstA, 16, 0, 0);
      const double* srcB = B + (size_t)(k0 + krow) * ldb + bn0 + 2 * lane;
      double* dstB = Bs + buf * BKD * BN + krow * BN;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)srcB,
          (__attribute__((address_space(3))) unsigned int*)dstB, 16, 0, 0);
    }
  };

  stage(0, 0);
  __syncthreads();
  const int ntiles = kend / BKD;
  for (int t = 0; t < ntiles; t++) {
    if (t + 1 < ntiles) stage((t + 1) & 1, (t + 1) * BKD);
    mfma_ktile(acc, As + ((t & 1) * BKD + ksub) * BM + wr * 32 + r16,
               Bs + ((t & 1) * BKD + ksub) * BN + wc * 64 + r16, BM);
    __syncthreads();
  }
  write_c(acc, C, ldc, bm0 + wr * 32 + ksub, bn0 + wc * 64 + r16, m, n,
          /*checked=*/false, /*store=*/KIND == V3_TRMM);
}

// ------------------------------------------------------------------ tn
// C[m x n] (+)= A[k x m]^T B[k x n]: both operands are contiguous along K,
// the layout of the second half of the SPD inverse (A^-1 = W^T W with
// W = L^-1 lower). The v2 structure with another staging step: each thread
// reads along K (16 consecutive lanes cover one 128 B run of a column) and
// writes transposed into the same [k][129] LDS image, zero-filled outside
// m, n and k. Four kinds:
//   TN_GEMM   C += A^T B on the full grid
//   TN_SYRK   C += A^T A on the lower block set (B = A)
//   TN_TRMM   X = W^T B, W (m x m, k == m) lower triangular: element (p, i)
//             of W counts as 0 where p < i, so block row bx starts its K loop
//             at its diagonal block; X is stored, never read
//   TN_LAUUM  X = W^T W on the lower block set (m == n == k), both operands
//             masked the same way
// The mask is applied while staging, so whatever is stored above W's
// diagonal (a diagonal tile carries junk there) never reaches an
// accumulator and the MFMA loop stays branch-free. write_c subtracts, so
// the accumulating kinds stage -A.
enum { TN_GEMM = 0, TN_SYRK = 1, TN_TRMM = 2, TN_LAUUM = 3 };

template <int KIND>
__launch_bounds__(512)
__global__ void k_dgemm_tn(int m, int n, int k, const double* __restrict__ A,
                           int lda, const double* __restrict__ B, int ldb,
                           double* __restrict__ C, int ldc, int nbx) {
  constexpr bool TRI = KIND == TN_SYRK || KIND == TN_LAUUM;
  constexpr bool STORE = KIND == TN_TRMM || KIND == TN_LAUUM;
  constexpr bool MASK_B = KIND == TN_LAUUM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LDT = 129;
  double* As = (double*)smem;                  // [2][BKD][LDT]
  double* Bs = As + 2 * BKD * LDT;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  int bx, by;
  block_decode(TRI, nbx, bx, by);
  const int bm0 = bx * BM, bn0 = by * BN;
  const int ksub = lane >> 4, r16 = lane & 15;
  // rows of W^T before its diagonal block are all masked
  const int kbeg = STORE ? bm0 : 0;

  f64x4 acc[2][4] = {};

  auto stage = [&](int buf, int k0) {
    double* as = As + buf * BKD * LDT;
    double* bs = Bs + buf * BKD * LDT;
#pragma unroll
    for (int x = 0; x < BM * BKD; x += 512) {
      int xi = x + tid;
      int kk = xi & (BKD - 1), i = xi / BKD;
      int gi = bm0 + i, gk = k0 + kk;
      bool in = gi < m && gk < k && !(STORE && gk < gi);
      double v = in ? A[(size_t)gi * lda + gk] : 0.0;
      as[kk * LDT + i] = STORE ? v : -v;
    }
#pragma unroll
    for (int x = 0; x < BN * BKD; x += 512) {
      int xi = x + tid;
      int kk = xi & (BKD - 1), j = xi / BKD;
      int gj = bn0 + j, gk = k0 + kk;
      bool in = gj < n && gk < k && !(MASK_B && gk < gj);
      bs[kk * LDT + j] = in ? B[(size_t)gj * ldb + gk] : 0.0;
    }
  };

  stage(0, kbeg);
  __syncthreads();
  const int ntiles = (k - kbeg + BKD - 1) / BKD;
  for (int t = 0; t < ntiles; t++) {
    if (t + 1 < ntiles) stage((t + 1) & 1, kbeg + (t + 1) * BKD);
    mfma_ktile(acc, As + ((t & 1) * BKD + ksub) * LDT + wr * 32 + r16,
               Bs + ((t & 1) * BKD + ksub) * LDT + wc * 64 + r16, LDT);
    __syncthreads();
  }
  write_c(acc, C, ldc, bm0 + wr * 32 + ksub, bn0 + wc * 64 + r16, m, n,
          /*checked=*/true, /*store=*/STORE);
}

// ------------------------------------------------------------------ nn
// C[m x n] -= A[m x k] B[k x n]: A is contiguous along M and staged as v2
// stages its A, B is contiguous along K and staged as the TN kernel stages
// its B (read along K, written transposed), both into the same [k][129] LDS
// image, zero-filled outside m, n and k.
__launch_bounds__(512)
__global__ void k_dgemm_nn(int m, int n, int k, const double* __restrict__ A,
                           int lda, const double* __restrict__ B, int ldb,
                           double* __restrict__ C, int ldc, int nbx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LDT = 129;
  double* As = (double*)smem;                  // [2][BKD][LDT]
  double* Bs = As + 2 * BKD * LDT;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  int bx, by;
  block_decode(false, nbx, bx, by);
  const int bm0 = bx * BM, bn0 = by * BN;
  const int ksub = lane >> 4, r16 = lane & 15;

  f64x4 acc[2][4] = {};

  auto stage = [&](int buf, int k0) {
    double* as = As + buf * BKD * LDT;
    double* bs = Bs + buf * BKD * LDT;
#pragma unroll
    for (int x = 0; x < BM * BKD; x += 512) {
      int xi = x + tid;
      int i = xi & (BM - 1), kk = xi >> 7;
      int gi = bm0 + i, gk = k0 + kk;
      as[kk * LDT + i] = (gi < m && gk < k) ? A[(size_t)gk * lda + gi] : 0.0;
    }
#pragma unroll
    for (int x = 0; x < BN * BKD; x += 512) {
      int xi = x + tid;
      int kk = xi & (BKD - 1), j = xi / BKD;
      int gj = bn0 + j, gk = k0 + kk;
      bs[kk * LDT + j] = (gj < n && gk < k) ? B[(size_t)gj * ldb + gk] : 0.0;
    }
  };

  stage(0, 0);
  __syncthreads();
  const int ntiles = (k + BKD - 1) / BKD;
  for (int t = 0; t < ntiles; t++) {
    if (t + 1 < ntiles) stage((t + 1) & 1, (t + 1) * BKD);
    mfma_ktile(acc, As + ((t & 1) * BKD + ksub) * LDT + wr * 32 + r16,
               Bs + ((t & 1) * BKD + ksub) * LDT + wc * 64 + r16, LDT);
    __syncthreads();
  }
  write_c(acc, C, ldc, bm0 + wr * 32 + ksub, bn0 + wc * 64 + r16, m, n,
          /*checked=*/true, /*store=*/false);
}

// ------------------------------------------------------------- launchers
// Every kernel here asks for more dynamic LDS than a launch gets by
// default: raise that kernel's limit once, then launch.
template <auto Kern, typename... Args>
static void launch_lds(int grid, int block, size_t lds, hipStream_t stream,
                       Args... args) {
  static const bool raised = [lds] {
    PA_HIP_CHECK(hipFuncSetAttribute(
        (const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL(Kern, dim3(grid), dim3(block), lds, stream, args...);
}

constexpr size_t LDS_V2 = 4 * BKD * 129 * 8;
constexpr size_t LDS_V3 = 2 * BKD * (BM + BN) * 8;

// What the glds kernel can take: whole 128-blocks, whole K-tiles, and, as
// it stages 16 B per lane, operands whose every column starts 16-B aligned
// (even leading dimension).
static bool full_tiles(int m, int n, int k, int lda, int ldb) {
  return m % BM == 0 && n % BN == 0 && k % BKD == 0 && lda % 2 == 0 &&
         ldb % 2 == 0;
}

void launch_dgemm_nt(int m, int n, int k, const double* A, int lda,
                     const double* B, int ldb, double* C, int ldc,
                     hipStream_t stream) {
  const int nbx = (m + BM - 1) / BM, nby = (n + BN - 1) / BN;
  if (full_tiles(m, n, k, lda, ldb))
    launch_lds<k_dgemm_nt_v3<V3_GEMM>>(nbx * nby, 512, LDS_V3, stream, m, n, k,
                                       A, lda, B, ldb, C, ldc, nbx);
  else
    launch_lds<k_dgemm_nt_v2<false>>(nbx * nby, 512, LDS_V2, stream, m, n, k,
                                     A, lda, B, ldb, C, ldc, nbx);
}

void launch_dsyrk_ln(int n, int k, const double* A, int lda, double* C,
                     int ldc, hipStream_t stream) {
  const int ntb = (n + BM - 1) / BM;
  const int nblocks = ntb * (ntb + 1) / 2;
  if (full_tiles(n, n, k, lda, lda))
    launch_lds<k_dgemm_nt_v3<V3_SYRK>>(nblocks, 512, LDS_V3, stream, n, n, k,
                                       A, lda, A, lda, C, ldc, 0);
  else
    launch_lds<k_dgemm_nt_v2<true>>(nblocks, 512, LDS_V2, stream, n, n, k, A,
                                    lda, A, lda, C, ldc, 0);
}

void launch_dtrmm_rlt(int m, int n, const double* B, int ldb, const double* W,
                      int ldw, double* X, int ldx, hipStream_t stream) {
  PA_CHECK(m > 0 && n > 0 && full_tiles(m, n, n, ldb, ldw),
           "dtrmm_rlt needs full 128x128 blocks and even ld, got %d x %d, "
           "ldb %d, ldw %d", m, n, ldb, ldw);
  PA_CHECK(ldb >= m && ldx >= m && ldw >= n);
  const int nbx = m / BM, nby = n / BN;
  launch_lds<k_dgemm_nt_v3<V3_TRMM>>(8 * ((nby + 7) / 8) * nbx, 512, LDS_V3,
                                     stream, m, n, n, B, ldb, W, ldw, X, ldx,
                                     nbx);
}

void launch_dgemm_tn(int m, int n, int k, const double* A, int lda,
                     const double* B, int ldb, double* C, int ldc,
                     hipStream_t stream) {
  PA_CHECK(m > 0 && n > 0 && k > 0 && lda >= k && ldb >= k && ldc >= m,
           "dgemm_tn: bad shape %d x %d x %d, ld %d %d %d", m, n, k, lda, ldb,
           ldc);
  const int nbx = (m + BM - 1) / BM, nby = (n + BN - 1) / BN;
  launch_lds<k_dgemm_tn<TN_GEMM>>(nbx * nby, 512, LDS_V2, stream, m, n, k, A,
                                  lda, B, ldb, C, ldc, nbx);
}

void launch_dgemm_nn(int m, int n, int k, const double* A, int lda,
                     const double* B, int ldb, double* C, int ldc,
                     hipStream_t stream) {
  PA_CHECK(m > 0 && n > 0 && k > 0 && lda >= m && ldb >= k && ldc >= m,
           "dgemm_nn: bad shape %d x %d x %d, ld %d %d %d", m, n, k, lda, ldb,
           ldc);
  const int nbx = (m + BM - 1) / BM, nby = (n + BN - 1) / BN;
  launch_lds<k_dgemm_nn>(nbx * nby, 512, LDS_V2, stream, m, n, k, A, lda, B,
                         ldb, C, ldc, nbx);
}

void launch_dsyrk_lt(int n, int k, const double* A, int lda, double* C,
                     int ldc, hipStream_t stream) {
  PA_CHECK(n > 0 && k > 0 && lda >= k && ldc >= n,
           "dsyrk_lt: bad shape %d x %d, ld %d %d", n, k, lda, ldc);
  const int ntb = (n + BM - 1) / BM;
  launch_lds<k_dgemm_tn<TN_SYRK>>(ntb * (ntb + 1) / 2, 512, LDS_V2, stream, n,
                                  n, k, A, lda, A, lda, C, ldc, 0);
}

void launch_dtrmm_llt(int m, int n, const double* W, int ldw, const double* B,
                      int ldb, double* X, int ldx, hipStream_t stream) {
  PA_CHECK(m > 0 && n > 0 && ldw >= m && ldb >= m && ldx >= m,
           "dtrmm_llt: bad shape %d x %d, ld %d %d %d", m, n, ldw, ldb, ldx);
  const int nbx = (m + BM - 1) / BM, nby = (n + BN - 1) / BN;
  launch_lds<k_dgemm_tn<TN_TRMM>>(nbx * nby, 512, LDS_V2, stream, m, n, m, W,
                                  ldw, B, ldb, X, ldx, nbx);
}

void launch_dlauum_l(int n, const double* W, int ldw, double* X, int ldx,
                     hipStream_t stream) {
  PA_CHECK(n > 0 && ldw >= n && ldx >= n,
           "dlauum_l: bad shape %d, ld %d %d", n, ldw, ldx);
  const int ntb = (n + BM - 1) / BM;
  launch_lds<k_dgemm_tn<TN_LAUUM>>(ntb * (ntb + 1) / 2, 512, LDS_V2, stream, n,
                                   n, n, W, ldw, W, ldw, X, ldx, 0);
}

void gpu_gemm_hip(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  launch_dgemm_nt(a.m, a.n, a.k, (const double*)t.dev_ptr[0], a.ld,
                  (const double*)t.dev_ptr[1], a.ld, (double*)t.dev_ptr[2],
                  a.ld, g.stream);
}

// ------------------------------------------------------------------ potf2
// Unblocked-in-LDS Cholesky of a <=128 fp64 panel with MFMA trailing
// updates: 16-column micro-panels factor scalar-sequentially (cheap), the
// rank-16 trailing update runs on v_mfma_f64_16x16x4f64 over 16x16 LDS
// tiles. One workgroup (4 waves); replaces both rocSOLVER's potf2 (~233 us)
// and the scalar LDS version (~830 us) — the tile-POTRF panel is the
// critical path of the whole Cholesky DAG.
__global__ void __launch_bounds__(256) k_potf2_mfma(double* A, int n, int ld) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LDP = 129;
  double* S = (double*)smem;     // [<=128][LDP] column-major
  double* dinv = S + 128 * LDP;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  for (int x = tid; x < n * n; x += 256) {
    int j = x / n, i = x - j * n;
    if (i >= j) S[j * LDP + i] = A[(size_t)j * ld + i];
  }
  __syncthreads();
  for (int jb = 0; jb < n; jb += 16) {
    const int jbe = jb + 16 < n ? jb + 16 : n;
    // ---- factor the 16-column micro-panel (rows jb..n) ----
    for (int j = jb; j < jbe; j++) {
      if (tid == 0) {
        double d = S[j * LDP + j];
        S[j * LDP + j] = d = sqrt(d);
        *dinv = 1.0 / d;
      }
      __syncthreads();
      for (int i = j + 1 + tid; i < n; i += 256) S[j * LDP + i] *= *dinv;
      __syncthreads();
      // independent trailing columns of the micro-panel: one wave each
      for (int c = j + 1 + wave; c < jbe; c += 4) {
        double ljc = S[j * LDP + c];
        for (int i = c + lane; i < n; i += 64)
          S[c * LDP + i] -= S[j * LDP + i] * ljc;
      }
      __syncthreads();
    }
    // ---- rank-16 MFMA trailing update: S[t,t] -= P P^T, t >= jb+16 ----
    const int t0 = jbe;
    const int nt = (n - t0 + 15) >> 4;  // trailing 16-blocks
    if (nt > 0) {
      const int ntiles = nt * (nt + 1) / 2;
      const int r16 = lane & 15, g4 = lane >> 4;
      for (int idx = wave; idx < ntiles; idx += 4) {
        int ti, tj;  // over the lower-triangular set of 16-blocks
        tri_decode(idx, ti, tj);
        const int ro = t0 + ti * 16, co = t0 + tj * 16;
        const int arow = ro + r16, brow = co + r16;
        f64x4 acc;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          int r = ro + 4 * e + g4, c = co + r16;
          acc[e] = (r < n && c < n) ? S[c * LDP + r] : 0.0;
        }
#pragma unroll
        for (int kk = 0; kk < 16; kk += 4) {
          int kcol = jb + kk + g4;
          double a = (arow < n) ? -S[kcol * LDP + arow] : 0.0;
          double b = (brow < n) ? S[kcol * LDP + brow] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
          int r = ro + 4 * e + g4, c = co + r16;
          if (r < n && c < n && r >= c) S[c * LDP + r] = acc[e];
        }
      }
    }
    __syncthreads();
  }
  for (int x = tid; x < n * n; x += 256) {
    int j = x / n, i = x - j * n;
    if (i >= j) A[(size_t)j * ld + i] = S[j * LDP + i];
  }
}

void launch_potf2(double* A, int n, int ld, hipStream_t stream) {
  PA_CHECK(n <= 128);
  launch_lds<k_potf2_mfma>(1, 256, 128 * 129 * 8 + 16, stream, A, n, ld);
}

// ------------------------------------------------ test and bench entries
namespace {

__global__ void k_bench_fill(double* p, size_t n, uint32_t seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint64_t h = (i * 2654435761ull) ^ ((uint64_t)seed * 2246822519ull);
    h ^= h >> 13;
    h *= 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
    p[i] = (double)(h & 0xFFFFFF) / (double)0x1000000 - 0.5;
  }
}

// random-ish fill (never bench on zero-filled operands — DVFS inflates)
void bench_fill(DevArray<double>& a, uint32_t seed) {
  hipLaunchKernelGGL(k_bench_fill, dim3(2048), dim3(256), 0, 0, a.p,
                     a.bytes / 8, seed);
}

}  // namespace

void test_dgemm_nt_hip(int m, int n, int k, const double* A, int lda,
                       const double* B, int ldb, double* C, int ldc) {
  DevArray dA((size_t)lda * k, A), dB((size_t)ldb * k, B),
      dC((size_t)ldc * n, C);
  launch_dgemm_nt(m, n, k, dA.p, lda, dB.p, ldb, dC.p, ldc, 0);
  dC.download(C);
}

void test_dsyrk_ln_hip(int n, int k, const double* A, int lda, double* C,
                       int ldc) {
  DevArray dA((size_t)lda * k, A), dC((size_t)ldc * n, C);
  launch_dsyrk_ln(n, k, dA.p, lda, dC.p, ldc, 0);
  dC.download(C);
}

// X is uploaded too, so a caller can show that whatever the output buffer
// held is ignored (beta = 0).
void test_dtrmm_rlt_hip(int m, int n, const double* B, int ldb,
                        const double* W, int ldw, double* X, int ldx) {
  DevArray dB((size_t)ldb * n, B), dW((size_t)ldw * n, W),
      dX((size_t)ldx * n, X);
  launch_dtrmm_rlt(m, n, dB.p, ldb, dW.p, ldw, dX.p, ldx, 0);
  dX.download(X);
}

void test_dgemm_tn_hip(int m, int n, int k, const double* A, int lda,
                       const double* B, int ldb, double* C, int ldc) {
  DevArray dA((size_t)lda * m, A), dB((size_t)ldb * n, B),
      dC((size_t)ldc * n, C);
  launch_dgemm_tn(m, n, k, dA.p, lda, dB.p, ldb, dC.p, ldc, 0);
  dC.download(C);
}

void test_dgemm_nn_hip(int m, int n, int k, const double* A, int lda,
                       const double* B, int ldb, double* C, int ldc) {
  DevArray dA((size_t)lda * k, A), dB((size_t)ldb * n, B),
      dC((size_t)ldc * n, C);
  launch_dgemm_nn(m, n, k, dA.p, lda, dB.p, ldb, dC.p, ldc, 0);
  dC.download(C);
}

void test_dsyrk_lt_hip(int n, int k, const double* A, int lda, double* C,
                       int ldc) {
  DevArray dA((size_t)lda * n, A), dC((size_t)ldc * n, C);
  launch_dsyrk_lt(n, k, dA.p, lda, dC.p, ldc, 0);
  dC.download(C);
}

// X is uploaded for the two storing kinds, as in test_dtrmm_rlt_hip.
void test_dtrmm_llt_hip(int m, int n, const double* W, int ldw,
                        const double* B, int ldb, double* X, int ldx) {
  DevArray dW((size_t)ldw * m, W), dB((size_t)ldb * n, B),
      dX((size_t)ldx * n, X);
  launch_dtrmm_llt(m, n, dW.p, ldw, dB.p, ldb, dX.p, ldx, 0);
  dX.download(X);
}

void test_dlauum_l_hip(int n, const double* W, int ldw, double* X, int ldx) {
  DevArray dW((size_t)ldw * n, W), dX((size_t)ldx * n, X);
  launch_dlauum_l(n, dW.p, ldw, dX.p, ldx, 0);
  dX.download(X);
}

void test_potf2_hip(double* A, int n) {
  DevArray dA((size_t)n * n, A);
  launch_potf2(dA.p, n, n, 0);
  dA.download(A);
}

// The rocBLAS comparison lives in kernels_blas.cpp.
double bench_dgemm_hip(int m, int n, int k, int iters) {
  DevArray dA((size_t)m * k), dB((size_t)n * k), dC((size_t)m * n);
  bench_fill(dA, 11);
  bench_fill(dB, 12);
  bench_fill(dC, 13);
  return time_launches(iters, [&] {
    launch_dgemm_nt(m, n, k, dA.p, m, dB.p, n, dC.p, m, 0);
  });
}

// kind: TN_GEMM (m, n, k), TN_SYRK (n, k), TN_TRMM (m, n) or TN_LAUUM (n).
// What W holds above its diagonal is masked, so every operand is random.
double bench_dgemm_tn_hip(int kind, int m, int n, int k, int iters) {
  PA_CHECK(kind >= TN_GEMM && kind <= TN_LAUUM, "bench_dgemm_tn: kind %d",
           kind);
  if (kind == TN_SYRK || kind == TN_LAUUM) m = n;
  if (kind == TN_TRMM || kind == TN_LAUUM) k = m;
  DevArray dA((size_t)k * m), dB((size_t)k * n), dC((size_t)m * n);
  bench_fill(dA, 11);
  bench_fill(dB, 12);
  bench_fill(dC, 13);
  return time_launches(iters, [&] {
    switch (kind) {
      case TN_GEMM:
        launch_dgemm_tn(m, n, k, dA.p, k, dB.p, k, dC.p, m, 0);
        break;
      case TN_SYRK: launch_dsyrk_lt(n, k, dA.p, k, dC.p, n, 0); break;
      case TN_TRMM: launch_dtrmm_llt(m, n, dA.p, m, dB.p, m, dC.p, m, 0); break;
      default: launch_dlauum_l(n, dA.p, n, dC.p, n, 0);
    }
  });
}

// The rocBLAS comparison is bench_dgemm_nn_rocblas in kernels_blas.cpp.
double bench_dgemm_nn_hip(int m, int n, int k, int iters) {
  DevArray dA((size_t)m * k), dB((size_t)k * n), dC((size_t)m * n);
  bench_fill(dA, 11);
  bench_fill(dB, 12);
  bench_fill(dC, 13);
  return time_launches(iters, [&] {
    launch_dgemm_nn(m, n, k, dA.p, m, dB.p, k, dC.p, m, 0);
  });
}

// W is lower triangular with zeros above.
double bench_dtrmm_hip(int m, int n, int iters) {
  DevArray dB((size_t)m * n), dW((size_t)n * n), dX((size_t)m * n);
  bench_fill(dB, 11);
  bench_fill(dW, 12);
  // zero the strictly-upper part of W, column by column
  for (int c = 1; c < n; c++)
    PA_HIP_CHECK(hipMemsetAsync(dW.p + (size_t)c * n, 0, (size_t)c * 8, 0));
  return time_launches(iters, [&] {
    launch_dtrmm_rlt(m, n, dB.p, m, dW.p, n, dX.p, m, 0);
  });
}

}  // namespace pa
