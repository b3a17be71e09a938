// Hand-written CDNA4 (gfx950) fp32 MFMA tile kernels, the fp32 tile chores
// built on them, and the single-precision Cholesky DAG (insert_potrf_f32)
// with the fp64 <-> fp32 tile conversion (insert_convert).
//
// The fp32 matrix pipe does twice the fp64 work per cycle, so the kernel
// family of the fp64 Cholesky (GEMM, lower-block-set SYRK, the triangular
// TRSM-by-inverse product) is rebuilt here for 4-byte elements; it is not
// k_dgemm_nt_v4 with the type replaced.
//
// Which MFMA. v_mfma_f32_32x32x2_f32: 4096 flops from one A and one B VGPR,
// 16 passes (64 cycles per SIMD). v_mfma_f32_16x16x4_f32 gives 2048 flops
// from the same two operand registers, so the 32x32 form halves the LDS
// operand reads per flop. Its price is 16 accumulator VGPRs per fragment;
// the budget below has room for them.
//
// Wave tile and block. A wave owns 64 x 64 of C as 2 x 2 fragments of
// 32 x 32: 64 accumulator VGPRs, and two A plus two B ds_read_b32 feed four
// MFMAs (256 matrix-pipe cycles), a quarter of the LDS reads per flop of the
// fp64 kernels' 32 x 64 wave tile on the 16x16x4 form. The block stays
// 128 x 128, now 4 waves as 2 (M) x 2 (N), one per SIMD: the lower block set
// of SYRK, the diagonal cut of the triangular product and the 128-wide
// panels of the in-tile POTRF all count in 128-blocks, and a 256-row block
// would send every n = 128 (mod 256) trailing update to the edge kernel.
//
// Fragment maps (cdna4 ISA, v_mfma_f32_32x32x2_f32), lane l, h = l >> 5,
// r = l & 31:
//   A operand: A[i = r][k = h]     B operand: B[k = h][j = r]
//   C/D: 16 VGPRs in four groups of four; element e = 4 g + q of lane l is
//        D[8 g + 4 h + q][r]: each group is four consecutive rows of one
//        column, groups are 8 rows apart, the lane half selects the upper or
//        lower four rows of each 8-row group.
// (For comparison: in the 16x16x4_f32 map (l >> 4) selects the 4-row group,
// in the fp64 16x16x4 map it strides rows by 4, kernels_hip.cpp.) C is
// column-major, so a group is one 16-B vector: the full-tile epilogue moves C
// as float4, the bounds-checked one element by element. The maps are proved
// by tests/test_sgemm_kernel.py, not assumed.
//
// Staging of the full-tile kernel. global_load_lds, 16 B per lane, into a
// [k][row] LDS image with K-rows of 128 floats (512 B): a lane carries four
// floats, 32 lanes one K-row, so one wave instruction lays down two adjacent
// K-rows (h selects which). Per K-tile of BK = 16 K-rows that is 8
// instructions for A and 8 for B, two of each per wave. The ring has S = 4
// slots: D = S - 1 = 3 K-tiles of copies in flight, a counted vmcnt wait and
// one raw barrier per K-tile, the protocol of k_dgemm_nt_v4. Why these
// numbers: a K-row of a 128 x 128 block costs 128 matrix-pipe cycles here
// against 256 in fp64 (half the MFMA time) and 1 KB against 2 KB (half the
// bytes), so covering the same memory latency takes twice the K-rows in
// flight for the same bytes: D * BK = 48 K-rows (48 KB) where v4 keeps
// 32 (64 KB). The ring is 64 KB, so two blocks share a CU's 160 KB and each
// SIMD holds two waves, one block's epilogue and prologue hiding under the
// other's K loop.
//
// What is here:
//  - k_sgemm_nt<KIND, S, BK>, the full-tile kernel (sgemm_full_tiles), kinds
//    V3_GEMM / V3_SYRK / V3_TRMM as in kernels_hip.cpp
//  - k_sgemm_nt_edge<TRI>, the bounds-checked kernel for every other GEMM and
//    SYRK shape: register-staged, zero-filled past m, n and k
//  - k_convert, fp64 <-> fp32 on a tile
//  - k_spotf2, the in-LDS Cholesky of one <= 128 diagonal block
//  - the fp32 task classes spotrf, strtri, strsm, strsm_inv, ssyrk, sgemm and
//    convert, insert_potrf_f32 and insert_convert
//    (PARSEC_MCA_chore_ssyrk, chore_strsm_inv, chore_sgemm = hip|rocblas)
#include "kernels_f32.hpp"

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <rocblas/rocblas.h>

#include "gpu_blas.hpp"
#include "kernels.hpp"
#include "kernels_bench.hpp"
#include "kernels_blocks.hpp"

namespace pa {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// block rows and columns
#define SB 128
// the ring of k_sgemm_nt: slots and K-rows per slot
#define SG_S 4
#define SG_BK 16
// K-tile depth and padded K-row of the edge kernel's LDS image. 160 = 128 +
// 32 floats: the upper half-wave reads the next K-row, and the odd multiple
// of 32 banks puts it on the other half of the 64 LDS banks.
#define SE_BK 16
#define SE_LD 160

enum { V3_GEMM = 0, V3_SYRK = 1, V3_TRMM = 2 };

// One DEPTH-deep K-tile into the wave's 2 x 2 accumulators. ap / bp point at
// this lane's element (K-row h, row r) of the first A / B fragment in a
// [k][row] LDS image whose K-rows are ld floats apart.
template <int DEPTH>
__device__ __forceinline__ void smfma_ktile(f32x16 (&acc)[2][2],
                                            const float* ap, const float* bp,
                                            int ld) {
#pragma unroll
  for (int kk = 0; kk < DEPTH; kk += 2) {
    float a[2], b[2];
#pragma unroll
    for (int f = 0; f < 2; f++) a[f] = ap[kk * ld + f * 32];
#pragma unroll
    for (int f = 0; f < 2; f++) b[f] = bp[kk * ld + f * 32];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
        acc[i][j] =
            __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
  }
}

// Accumulators to C: group g of fragment (i, j) is the four rows from
// row0 + 32 i + 8 g of column col0 + 32 j, where row0 already holds the
// lane's 4 h and col0 its r. store writes C = acc, otherwise C -= acc.
// CHECKED drops what lies outside m x n and moves single floats; unchecked
// needs 16-B aligned columns.
template <bool CHECKED>
__device__ __forceinline__ void swrite_c(const f32x16 (&acc)[2][2], float* C,
                                         int ldc, int row0, int col0, int m,
                                         int n, bool store) {
#pragma unroll
  for (int j = 0; j < 2; j++) {
    int col = col0 + j * 32;
    if (CHECKED && col >= n) continue;
    float* cp = C + (size_t)col * ldc;
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        int row = row0 + i * 32 + g * 8;
        if (CHECKED) {
#pragma unroll
          for (int q = 0; q < 4; q++) {
            if (row + q >= m) continue;
            if (store) cp[row + q] = acc[i][j][4 * g + q];
            else cp[row + q] -= acc[i][j][4 * g + q];
          }
        } else {
          f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1],
                     acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          f32x4* p = (f32x4*)(cp + row);
          *p = store ? v : *p - v;
        }
      }
    }
  }
}

template <int N>
__device__ __forceinline__ void swait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ------------------------------------------------------------ full tiles
// Iteration t (slot t % S), as in k_dgemm_nt_v4:
//   s_waitcnt vmcnt(c)   this wave's copies of tile t have landed; c counts
//                        the copies of the later tiles already issued,
//                        CPS * (D - 1) in steady state, fewer in the drain
//   s_barrier            ... and so have every wave's; every wave is also
//                        done reading slot (t - 1) % S
//   issue tile t + D into slot (t + D) % S == (t - 1) % S, if t + D < ntiles
//   the MFMAs of tile t
// No copy is issued for a tile >= ntiles and the prologue issues
// min(D, ntiles) tiles, so k = BK works (ntiles = 1).
//
// V3_TRMM has B = W (n x n, k == n) lower triangular: output block column by
// only sees k < (by + 1) * 128, its K loop stops there (the diagonal K-block
// reads W's strictly-upper entries, which must be stored zeros), and the
// epilogue stores (beta = 0: X is never read).
template <int KIND, int S, int BK>
__launch_bounds__(256)
__global__ void k_sgemm_nt(int m, int n, int k, const float* __restrict__ A,
                           int lda, const float* __restrict__ B, int ldb,
                           float* __restrict__ C, int ldc, int nbx) {
  static_assert(S == 3 || S == 4, "the drain below covers D = 2 and D = 3");
  static_assert(BK % 8 == 0, "whole K-row pairs per wave and operand");
  constexpr int D = S - 1;
  constexpr int PPW = BK / 8;    // K-row pairs per wave, of A and of B
  constexpr int CPS = 2 * PPW;   // copies per lane and stage
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = (float*)smem;                    // [S][BK][SB]
  float* Bs = As + S * BK * SB;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int h = lane >> 5, r = lane & 31;
  int bx, by;
  if (KIND == V3_TRMM) {
    if (!snake_decode(nbx, n / SB, bx, by)) return;
  } else {
    block_decode(KIND == V3_SYRK, nbx, bx, by);
  }
  const int bm0 = bx * SB, bn0 = by * SB;
  const int kend = KIND == V3_TRMM ? (bn0 + SB < k ? bn0 + SB : k) : k;

  f32x16 acc[2][2] = {};

  auto stage = [&](int slot, int k0) {
#pragma unroll
    for (int p = 0; p < PPW; p++) {
      const int krow = 2 * (wave * PPW + p);  // this instruction's first K-row
      const float* srcA = A + (size_t)(k0 + krow + h) * lda + bm0 + 4 * r;
      float* dstA = As + (slot * BK + krow) * SB;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)srcA,
          (__attribute__((address_space(3))) unsigned int*)dstA, 16, 0, 0);
      const float* srcB = B + (size_t)(k0 + krow + h) * ldb + bn0 + 4 * r;
      float* dstB = Bs + (slot * BK + krow) * SB;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)srcB,
          (__attribute__((address_space(3))) unsigned int*)dstB, 16, 0, 0);
    }
  };

  const int ntiles = kend / BK;
  for (int t = 0; t < D && t < ntiles; t++) stage(t, t * BK);
  int rslot = 0, wslot = D;  // t % S and (t + D) % S
  for (int t = 0; t < ntiles; t++) {
    const int after = ntiles - 1 - t;  // tiles after t
    if (after >= D - 1) swait_vmcnt<CPS * (D - 1)>();
    else if (D == 3 && after == 1) swait_vmcnt<CPS>();
    else swait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (t + D < ntiles) stage(wslot, (t + D) * BK);
    smfma_ktile<BK>(acc, As + (rslot * BK + h) * SB + wr * 64 + r,
                    Bs + (rslot * BK + h) * SB + wc * 64 + r, SB);
    rslot = rslot + 1 == S ? 0 : rslot + 1;
    wslot = wslot + 1 == S ? 0 : wslot + 1;
  }
  swrite_c<false>(acc, C, ldc, bm0 + wr * 64 + 4 * h, bn0 + wc * 64 + r, m, n,
                  /*store=*/KIND == V3_TRMM);
}

// ------------------------------------------------------------------ edge
// Bounds-checked kernel: operands go through registers into a [k][SE_LD]
// padded LDS image, zero-filled outside m, n and k, double-buffered (40 KB).
// TRI selects the lower block set (SYRK). Same block, wave tile and fragment
// maps as the full-tile kernel.
template <bool TRI>
__launch_bounds__(256)
__global__ void k_sgemm_nt_edge(int m, int n, int k,
                                const float* __restrict__ A, int lda,
                                const float* __restrict__ B, int ldb,
                                float* __restrict__ C, int ldc, int nbx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = (float*)smem;                    // [2][SE_BK][SE_LD]
  float* Bs = As + 2 * SE_BK * SE_LD;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int h = lane >> 5, r = lane & 31;
  int bx, by;
  block_decode(TRI, nbx, bx, by);
  const int bm0 = bx * SB, bn0 = by * SB;

  f32x16 acc[2][2] = {};

  auto stage = [&](int buf, int k0) {
    float* as = As + buf * SE_BK * SE_LD;
    float* bs = Bs + buf * SE_BK * SE_LD;
#pragma unroll
    for (int x = 0; x < SB * SE_BK; x += 256) {
      int xi = x + tid;
      int i = xi & (SB - 1), kk = xi >> 7;
      int gi = bm0 + i, gk = k0 + kk;
      as[kk * SE_LD + i] = (gi < m && gk < k) ? A[(size_t)gk * lda + gi] : 0.f;
    }
#pragma unroll
    for (int x = 0; x < SB * SE_BK; x += 256) {
      int xi = x + tid;
      int j = xi & (SB - 1), kk = xi >> 7;
      int gj = bn0 + j, gk = k0 + kk;
      bs[kk * SE_LD + j] = (gj < n && gk < k) ? B[(size_t)gk * ldb + gj] : 0.f;
    }
  };

  stage(0, 0);
  __syncthreads();
  const int ntiles = (k + SE_BK - 1) / SE_BK;
  for (int t = 0; t < ntiles; t++) {
    if (t + 1 < ntiles) stage((t + 1) & 1, (t + 1) * SE_BK);
    smfma_ktile<SE_BK>(acc, As + ((t & 1) * SE_BK + h) * SE_LD + wr * 64 + r,
                       Bs + ((t & 1) * SE_BK + h) * SE_LD + wc * 64 + r, SE_LD);
    __syncthreads();
  }
  swrite_c<true>(acc, C, ldc, bm0 + wr * 64 + 4 * h, bn0 + wc * 64 + r, m, n,
                 /*store=*/false);
}

// --------------------------------------------------------------- convert
// dst = (D)src on a rows x cols block, both sides ld elements apart. A
// thread takes four consecutive rows of one column: with VEC (ld % 4 == 0
// and 16-B aligned bases) whole groups move as one float4 on the fp32 side
// and two 16-B vectors on the fp64 side; the last rows of a column that is
// no multiple of four, and everything without VEC, go element by element.
// The fp64 -> fp32 cast rounds to nearest even.
template <typename S, typename D, bool VEC>
__global__ void k_convert(const S* __restrict__ src, D* __restrict__ dst,
                          int rows, int cols, int ld) {
  typedef S sx4 __attribute__((ext_vector_type(4)));
  typedef D dx4 __attribute__((ext_vector_type(4)));
  const int groups = (rows + 3) / 4;
  const int total = groups * cols;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += gridDim.x * blockDim.x) {
    const int c = idx / groups, r0 = (idx - c * groups) * 4;
    const size_t off = (size_t)c * ld + r0;
    if (VEC && r0 + 4 <= rows) {
      sx4 v = *(const sx4*)(src + off);
      dx4 w = {(D)v[0], (D)v[1], (D)v[2], (D)v[3]};
      *(dx4*)(dst + off) = w;
    } else {
      for (int q = 0; q < 4 && r0 + q < rows; q++) dst[off + q] = (D)src[off + q];
    }
  }
}

template <typename S, typename D>
static void launch_convert_t(const S* src, D* dst, int rows, int cols, int ld,
                             hipStream_t stream) {
  PA_CHECK(rows > 0 && cols > 0 && ld >= rows, "convert: bad shape %d x %d, "
           "ld %d", rows, cols, ld);
  const bool vec = ld % 4 == 0 && (uintptr_t)src % (4 * sizeof(S)) == 0 &&
                   (uintptr_t)dst % (4 * sizeof(D)) == 0;
  const int total = (rows + 3) / 4 * cols;
  const int grid = std::min((total + 255) / 256, 4096);
  if (vec)
    hipLaunchKernelGGL((k_convert<S, D, true>), dim3(grid), dim3(256), 0,
                       stream, src, dst, rows, cols, ld);
  else
    hipLaunchKernelGGL((k_convert<S, D, false>), dim3(grid), dim3(256), 0,
                       stream, src, dst, rows, cols, ld);
}

void launch_convert(const double* src, float* dst, int rows, int cols, int ld,
                    hipStream_t stream) {
  launch_convert_t(src, dst, rows, cols, ld, stream);
}

void launch_convert(const float* src, double* dst, int rows, int cols, int ld,
                    hipStream_t stream) {
  launch_convert_t(src, dst, rows, cols, ld, stream);
}

// ------------------------------------------------------------- launchers
constexpr size_t LDS_FULL = (size_t)SG_S * SG_BK * 2 * SB * 4;
constexpr size_t LDS_EDGE = (size_t)2 * 2 * SE_BK * SE_LD * 4;

bool sgemm_full_tiles(int m, int n, int k, const float* A, int lda,
                      const float* B, int ldb, const float* C, int ldc) {
  return m > 0 && n > 0 && k > 0 && m % SB == 0 && n % SB == 0 &&
         k % SG_BK == 0 && lda % 4 == 0 && ldb % 4 == 0 && ldc % 4 == 0 &&
         ((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) % 16 == 0;
}

void launch_sgemm_nt(int m, int n, int k, const float* A, int lda,
                     const float* B, int ldb, float* C, int ldc,
                     hipStream_t stream) {
  PA_CHECK(m > 0 && n > 0 && k > 0 && lda >= m && ldb >= n && ldc >= m,
           "sgemm_nt: bad shape %d x %d x %d, ld %d %d %d", m, n, k, lda, ldb,
           ldc);
  const int nbx = (m + SB - 1) / SB, nby = (n + SB - 1) / SB;
  if (sgemm_full_tiles(m, n, k, A, lda, B, ldb, C, ldc))
    launch_lds<k_sgemm_nt<V3_GEMM, SG_S, SG_BK>>(
        nbx * nby, 256, LDS_FULL, stream, m, n, k, A, lda, B, ldb, C, ldc, nbx);
  else
    launch_lds<k_sgemm_nt_edge<false>>(nbx * nby, 256, LDS_EDGE, stream, m, n,
                                       k, A, lda, B, ldb, C, ldc, nbx);
}

void launch_ssyrk_ln(int n, int k, const float* A, int lda, float* C, int ldc,
                     hipStream_t stream) {
  PA_CHECK(n > 0 && k > 0 && lda >= n && ldc >= n,
           "ssyrk_ln: bad shape %d x %d, ld %d %d", n, k, lda, ldc);
  const int ntb = (n + SB - 1) / SB;
  const int nblocks = ntb * (ntb + 1) / 2;
  if (sgemm_full_tiles(n, n, k, A, lda, A, lda, C, ldc))
    launch_lds<k_sgemm_nt<V3_SYRK, SG_S, SG_BK>>(
        nblocks, 256, LDS_FULL, stream, n, n, k, A, lda, A, lda, C, ldc, 0);
  else
    launch_lds<k_sgemm_nt_edge<true>>(nblocks, 256, LDS_EDGE, stream, n, n, k,
                                      A, lda, A, lda, C, ldc, 0);
}

void launch_strmm_rlt(int m, int n, const float* B, int ldb, const float* W,
                      int ldw, float* X, int ldx, hipStream_t stream) {
  PA_CHECK(sgemm_full_tiles(m, n, n, B, ldb, W, ldw, X, ldx),
           "strmm_rlt needs full 128x128 blocks, ld %% 4 == 0 and 16-B aligned "
           "operands, got %d x %d, ld %d %d %d", m, n, ldb, ldw, ldx);
  PA_CHECK(ldb >= m && ldx >= m && ldw >= n);
  const int nbx = m / SB, nby = n / SB;
  launch_lds<k_sgemm_nt<V3_TRMM, SG_S, SG_BK>>(
      8 * ((nby + 7) / 8) * nbx, 256, LDS_FULL, stream, m, n, n, B, ldb, W, ldw,
      X, ldx, nbx);
}

// ----------------------------------------------------------------- potf2
// In-LDS Cholesky of one <= 128 diagonal block, one thread per row,
// left-looking: column j's entries are A_ij minus a dot product of length j
// that is summed first and subtracted once. A right-looking sweep (what
// rocsolver_spotrf does at this size) subtracts 127 small products one by
// one from a diagonal entry near n, each rounding at that entry's ulp: its
// residual is within Higham's bound and several times LAPACK's, which
// tests/test_potrf_f32.py does not allow. The strict upper triangle is
// neither read nor written.
__global__ void __launch_bounds__(128) k_spotf2(float* A, int n, int ld) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LDP = 129;
  float* L = (float*)smem;       // [<=128][LDP] column-major
  const int i = threadIdx.x;
  for (int j = 0; j < n; j++)
    if (i >= j && i < n) L[j * LDP + i] = A[(size_t)j * ld + i];
  __syncthreads();
  for (int j = 0; j < n; j++) {
    float v = 0;
    if (i >= j && i < n) {
      float s = 0;
      for (int k = 0; k < j; k++) s += L[k * LDP + i] * L[k * LDP + j];
      v = L[j * LDP + i] - s;
      if (i == j) L[j * LDP + j] = sqrtf(v);
    }
    __syncthreads();
    if (i > j && i < n) L[j * LDP + i] = v / L[j * LDP + j];
    __syncthreads();
  }
  for (int j = 0; j < n; j++)
    if (i >= j && i < n) A[(size_t)j * ld + i] = L[j * LDP + i];
}

static void launch_spotf2(float* A, int n, int ld, hipStream_t stream) {
  PA_CHECK(n > 0 && n <= 128);
  launch_lds<k_spotf2>(1, 128, 128 * 129 * 4, stream, A, n, ld);
}

// ------------------------------------------------ test and bench entries
void test_sgemm_nt_hip(int m, int n, int k, const float* A, int lda,
                       const float* B, int ldb, float* C, int ldc) {
  DevArray<float> dA((size_t)lda * k, A), dB((size_t)ldb * k, B),
      dC((size_t)ldc * n, C);
  launch_sgemm_nt(m, n, k, dA.p, lda, dB.p, ldb, dC.p, ldc, 0);
  dC.download(C);
}

void test_ssyrk_ln_hip(int n, int k, const float* A, int lda, float* C,
                       int ldc) {
  DevArray<float> dA((size_t)lda * k, A), dC((size_t)ldc * n, C);
  launch_ssyrk_ln(n, k, dA.p, lda, dC.p, ldc, 0);
  dC.download(C);
}

// X is uploaded too, so a caller can show that whatever the output buffer
// held is ignored (beta = 0).
void test_strmm_rlt_hip(int m, int n, const float* B, int ldb, const float* W,
                        int ldw, float* X, int ldx) {
  DevArray<float> dB((size_t)ldb * n, B), dW((size_t)ldw * n, W),
      dX((size_t)ldx * n, X);
  launch_strmm_rlt(m, n, dB.p, ldb, dW.p, ldw, dX.p, ldx, 0);
  dX.download(X);
}

void test_convert_d2s_hip(const double* src, float* dst, int rows, int cols,
                          int ld) {
  DevArray<double> dS((size_t)ld * cols, src);
  DevArray<float> dD((size_t)ld * cols, dst);
  launch_convert(dS.p, dD.p, rows, cols, ld, 0);
  dD.download(dst);
}

void test_convert_s2d_hip(const float* src, double* dst, int rows, int cols,
                          int ld) {
  DevArray<float> dS((size_t)ld * cols, src);
  DevArray<double> dD((size_t)ld * cols, dst);
  launch_convert(dS.p, dD.p, rows, cols, ld, 0);
  dD.download(dst);
}

namespace {

// random-ish fill in [-0.5, 0.5) (never bench on zero-filled operands)
__global__ void k_bench_fill_f32(float* p, size_t n, uint32_t seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint64_t x = (i * 2654435761ull) ^ ((uint64_t)seed * 2246822519ull);
    x ^= x >> 13;
    x *= 0x9E3779B97F4A7C15ull;
    x ^= x >> 32;
    p[i] = (float)(x & 0xFFFFFF) / (float)0x1000000 - 0.5f;
  }
}

}  // namespace

double bench_sgemm(int m, int n, int k, int iters, bool rocblas) {
  DevArray<float> dA((size_t)m * k), dB((size_t)n * k), dC((size_t)m * n);
  uint32_t seed = 11;
  for (DevArray<float>* a : {&dA, &dB, &dC})
    hipLaunchKernelGGL(k_bench_fill_f32, dim3(2048), dim3(256), 0, 0, a->p,
                       a->bytes / 4, seed++);
  if (!rocblas)
    return time_launches(iters, [&] {
      launch_sgemm_nt(m, n, k, dA.p, m, dB.p, n, dC.p, m, 0);
    });
  rocblas_handle hd;
  PA_BLAS_CHECK(rocblas_create_handle(&hd));
  const float mone = -1.f, one = 1.f;
  double dt = time_launches(iters, [&] {
    rocblas_sgemm(hd, rocblas_operation_none, rocblas_operation_transpose, m, n,
                  k, &mone, dA.p, m, dB.p, n, &one, dC.p, m);
  });
  rocblas_destroy_handle(hd);
  return dt;
}

// ------------------------------------------------------------ CPU chores
// Plain float loops (column-major, ld = tile rows): the no-GPU path. Every
// update sums its products first and subtracts once, as the GPU kernels do
// (C -= acc): hundreds of small subtractions from a diagonal entry near n
// would each round at that entry's ulp.
static void cpu_spotrf(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  float* A = (float*)t.flows[0].data->pull_to_host();
  const int n = a.n, ld = a.ld;
  for (int j = 0; j < n; j++) {
    float s = 0;
    for (int k = 0; k < j; k++) s += A[(size_t)k * ld + j] * A[(size_t)k * ld + j];
    float d = A[(size_t)j * ld + j] - s;
    PA_CHECK(d > 0, "spotrf: matrix not SPD at column %d", j);
    d = std::sqrt(d);
    A[(size_t)j * ld + j] = d;
    for (int i = j + 1; i < n; i++) {
      s = 0;
      for (int k = 0; k < j; k++) s += A[(size_t)k * ld + i] * A[(size_t)k * ld + j];
      A[(size_t)j * ld + i] = (A[(size_t)j * ld + i] - s) / d;
    }
  }
  t.flows[0].data->written_on(false);
}

// B = B * L^-T
static void cpu_strsm(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const float* L = (const float*)t.flows[0].data->pull_to_host();
  float* B = (float*)t.flows[1].data->pull_to_host();
  const int m = a.m, n = a.n, ld = a.ld;
  for (int j = 0; j < n; j++) {
    const float d = L[(size_t)j * ld + j];
    for (int i = 0; i < m; i++) {
      float s = 0;
      for (int k = 0; k < j; k++) s += B[(size_t)k * ld + i] * L[(size_t)k * ld + j];
      B[(size_t)j * ld + i] = (B[(size_t)j * ld + i] - s) / d;
    }
  }
  t.flows[1].data->written_on(false);
}

// W = L^-1 (lower; the rest of W zeroed)
static void cpu_strtri(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const float* L = (const float*)t.flows[0].data->pull_to_host();
  Data* wd = t.flows[1].data;
  float* W = (float*)wd->ensure_host();
  memset(W, 0, wd->bytes);
  const int n = a.n, ld = a.ld;
  for (int c = 0; c < n; c++) {
    W[(size_t)c * ld + c] = 1.f / L[(size_t)c * ld + c];
    for (int i = c + 1; i < n; i++) {
      float s = 0;
      for (int k = c; k < i; k++) s += L[(size_t)k * ld + i] * W[(size_t)c * ld + k];
      W[(size_t)c * ld + i] = -s / L[(size_t)i * ld + i];
    }
  }
  wd->written_on(false);
}

// B = B * W^T with W = L^-1 lower triangular
static void cpu_strsm_inv(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const float* W = (const float*)t.flows[0].data->pull_to_host();
  float* B = (float*)t.flows[1].data->pull_to_host();
  const int m = a.m, n = a.n, ld = a.ld;
  std::vector<float> tmp((size_t)n * m);
  for (int j = 0; j < n; j++)
    for (int i = 0; i < m; i++) tmp[(size_t)j * m + i] = B[(size_t)j * ld + i];
  for (int j = 0; j < n; j++)
    for (int i = 0; i < m; i++) {
      float s = 0;
      for (int k = 0; k <= j; k++)
        s += tmp[(size_t)k * m + i] * W[(size_t)k * ld + j];
      B[(size_t)j * ld + i] = s;
    }
  t.flows[1].data->written_on(false);
}

// C = C - A A^T on the lower triangle
static void cpu_ssyrk(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const float* A = (const float*)t.flows[0].data->pull_to_host();
  float* C = (float*)t.flows[1].data->pull_to_host();
  const int n = a.n, k = a.k, ld = a.ld;
  for (int j = 0; j < n; j++)
    for (int i = j; i < n; i++) {
      float s = 0;
      for (int p = 0; p < k; p++) s += A[(size_t)p * ld + i] * A[(size_t)p * ld + j];
      C[(size_t)j * ld + i] -= s;
    }
  t.flows[1].data->written_on(false);
}

// C = C - A B^T
static void cpu_sgemm(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const float* A = (const float*)t.flows[0].data->pull_to_host();
  const float* B = (const float*)t.flows[1].data->pull_to_host();
  float* C = (float*)t.flows[2].data->pull_to_host();
  const int m = a.m, n = a.n, k = a.k, ld = a.ld;
  for (int j = 0; j < n; j++)
    for (int i = 0; i < m; i++) {
      float s = 0;
      for (int p = 0; p < k; p++) s += A[(size_t)p * ld + i] * B[(size_t)p * ld + j];
      C[(size_t)j * ld + i] -= s;
    }
  t.flows[2].data->written_on(false);
}

// TileArgs.k carries the source element size.
static void cpu_convert(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const void* src = t.flows[0].data->pull_to_host();
  Data* dd = t.flows[1].data;
  void* dst = dd->ensure_host();
  for (int c = 0; c < a.n; c++)
    for (int r = 0; r < a.m; r++) {
      const size_t x = (size_t)c * a.ld + r;
      if (a.k == 8) ((float*)dst)[x] = (float)((const double*)src)[x];
      else ((double*)dst)[x] = (double)((const float*)src)[x];
    }
  dd->written_on(false);
}

// ------------------------------------------------------------ GPU chores
// The fp64 chores of kernels_blas.cpp in single precision.
//
// Blocked tile POTRF in 128-wide panels: the in-LDS k_spotf2 on the panel's
// diagonal block, rocblas_strsm on the rows below it, the hand lower-block
// SYRK on the trailing matrix, all in order on the task's stream.
static void gpu_spotrf(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  float* A = (float*)t.dev_ptr[0];
  const int n = a.n, ld = a.ld;
  const float one = 1.f;
  rocblas_handle hd = blas_handle(g);
  for (int j = 0; j < n; j += 128) {
    const int jb = std::min(128, n - j);
    float* Ajj = A + (size_t)j * ld + j;
    launch_spotf2(Ajj, jb, ld, g.stream);
    const int rest = n - j - jb;
    if (rest <= 0) continue;
    float* Aij = A + (size_t)j * ld + j + jb;
    PA_BLAS_CHECK(rocblas_strsm(hd, rocblas_side_right, rocblas_fill_lower,
                                rocblas_operation_transpose,
                                rocblas_diagonal_non_unit, rest, jb, &one, Ajj,
                                ld, Aij, ld));
    launch_ssyrk_ln(rest, jb, Aij, ld, A + (size_t)(j + jb) * ld + j + jb, ld,
                    g.stream);
  }
}

static void gpu_strsm(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  const float one = 1.f;
  PA_BLAS_CHECK(rocblas_strsm(
      blas_handle(g), rocblas_side_right, rocblas_fill_lower,
      rocblas_operation_transpose, rocblas_diagonal_non_unit, a.m, a.n, &one,
      (const float*)t.dev_ptr[0], a.ld, (float*)t.dev_ptr[1], a.ld));
}

static void gpu_strtri(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  PA_HIP_CHECK(
      hipMemsetAsync(t.dev_ptr[1], 0, t.flows[1].data->bytes, g.stream));
  PA_BLAS_CHECK(rocblas_strtri(
      blas_handle(g), rocblas_fill_lower, rocblas_diagonal_non_unit, a.n,
      (const float*)t.dev_ptr[0], a.ld, (float*)t.dev_ptr[1], a.ld));
}

// C -= A B^T through the library, the `rocblas` side of every selector.
static void lib_sgemm_nt(GpuTaskCtx& g, int m, int n, int k, float alpha,
                         const float* A, const float* B, float beta, float* C,
                         int ld) {
  PA_BLAS_CHECK(rocblas_sgemm(blas_handle(g), rocblas_operation_none,
                              rocblas_operation_transpose, m, n, k, &alpha, A,
                              ld, B, ld, &beta, C, ld));
}

// X = B W^T out of place into a fresh pool buffer that then becomes the
// tile's device copy. The hand kernel stops each block column's K loop at
// W's diagonal (half the flops of the dense product); a tile that is not
// whole 128-blocks, or chore_strsm_inv=rocblas, takes rocblas_sgemm.
static void gpu_strsm_inv(Task& t, GpuTaskCtx& g) {
  static const bool use_hip = param_str("chore_strsm_inv", "hip") == "hip";
  const TileArgs& a = t.arg<TileArgs>();
  const float* W = (const float*)t.dev_ptr[0];
  const float* B = (const float*)t.dev_ptr[1];
  float* X = (float*)fresh_tile(t, g, 1);
  if (use_hip && sgemm_full_tiles(a.m, a.n, a.n, B, a.ld, W, a.ld, X, a.ld))
    launch_strmm_rlt(a.m, a.n, B, a.ld, W, a.ld, X, a.ld, g.stream);
  else
    lib_sgemm_nt(g, a.m, a.n, a.n, 1.f, B, W, 0.f, X, a.ld);
  swap_in_tile(t, g, 1, (double*)X);
}

// chore_ssyrk=rocblas is the full-tile sgemm(A, A^T), as the fp64 library
// route is: twice the flops, and the upper triangle of a diagonal tile is
// never read by the DAG.
static void gpu_ssyrk(Task& t, GpuTaskCtx& g) {
  static const bool use_hip = param_str("chore_ssyrk", "hip") == "hip";
  const TileArgs& a = t.arg<TileArgs>();
  const float* A = (const float*)t.dev_ptr[0];
  float* C = (float*)t.dev_ptr[1];
  if (use_hip) launch_ssyrk_ln(a.n, a.k, A, a.ld, C, a.ld, g.stream);
  else lib_sgemm_nt(g, a.n, a.n, a.k, -1.f, A, A, 1.f, C, a.ld);
}

// PARSEC_MCA_chore_sgemm when it is not set. Alone the hand kernel is the
// slower one (126 against 150 TF at 4096^3); inside the Cholesky DAG at
// N = 32768, tile 2048, it is the faster (71.5 against 68.8 TF), beside the
// hand SYRK and TRSM-product blocks (profiles/RESULTS.md).
#define CHORE_SGEMM_DEFAULT "hip"

static void gpu_sgemm(Task& t, GpuTaskCtx& g) {
  static const bool use_hip =
      param_str("chore_sgemm", CHORE_SGEMM_DEFAULT) == "hip";
  const TileArgs& a = t.arg<TileArgs>();
  const float* A = (const float*)t.dev_ptr[0];
  const float* B = (const float*)t.dev_ptr[1];
  float* C = (float*)t.dev_ptr[2];
  if (use_hip)
    launch_sgemm_nt(a.m, a.n, a.k, A, a.ld, B, a.ld, C, a.ld, g.stream);
  else
    lib_sgemm_nt(g, a.m, a.n, a.k, -1.f, A, B, 1.f, C, a.ld);
}

static void gpu_convert(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  if (a.k == 8)
    launch_convert((const double*)t.dev_ptr[0], (float*)t.dev_ptr[1], a.m, a.n,
                   a.ld, g.stream);
  else
    launch_convert((const float*)t.dev_ptr[0], (double*)t.dev_ptr[1], a.m, a.n,
                   a.ld, g.stream);
}

// --------------------------------------------------------------- classes
#define PA_F32_CLASS(fn, name, id)                                        \
  static TaskClass& tc_##fn() {                                           \
    static TaskClass tc =                                                 \
        make_tc(name, TaskKind::GPU, cpu_##fn, gpu_##fn, id);             \
    return tc;                                                            \
  }
PA_F32_CLASS(spotrf, "spotrf", TC_SPOTRF)
PA_F32_CLASS(strtri, "strtri", TC_STRTRI)
PA_F32_CLASS(strsm, "strsm", TC_STRSM)
PA_F32_CLASS(strsm_inv, "strsm_inv", TC_STRSM_INV)
PA_F32_CLASS(ssyrk, "ssyrk", TC_SSYRK)
PA_F32_CLASS(sgemm, "sgemm", TC_SGEMM)
PA_F32_CLASS(convert, "convert", TC_CONVERT)
#undef PA_F32_CLASS

// ---------------------------------------------------------- DAG builders
// insert_potrf (kernels_blas.cpp) over the fp32 classes: the same tasks,
// flows, priorities and trsm_variant handling. It is written out beside the
// fp64 builder so that what insert_potrf inserts cannot change.
void insert_potrf_f32(Dtd& tp, TiledMatrix& A) {
  PA_CHECK(A.elem_size() == 4, "insert_potrf_f32: A holds %zu-byte elements, "
           "not fp32", A.elem_size());
  const int T = A.mt();
  const int ld = A.mb();
  constexpr int PANEL = 1 << 20;
  const bool invgemm = param_str("trsm_variant", "invgemm") == "invgemm";
  std::shared_ptr<TiledMatrix> W;
  if (invgemm) {
    W = std::make_shared<TiledMatrix>(A.ctx(), A.m(), A.n(), A.mb(), A.nb(),
                                      A.grid_p(), A.grid_q(), 4);
    tp.own(W);
  }
  for (int k = 0; k < T; k++) {
    TileArgs pa_args = tile_args(0, A.tile_cols(k), 0, ld);
    {
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_INOUT}};
      tp.insert(&tc_spotrf(), &pa_args, sizeof(pa_args), f, 1, PANEL + 1,
                A.rank_of(k, k));
    }
    if (invgemm && k + 1 < T) {
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_IN},
                           {W->tile(k, k), ACCESS_OUT}};
      tp.insert(&tc_strtri(), &pa_args, sizeof(pa_args), f, 2, PANEL,
                A.rank_of(k, k));
    }
    for (int m = k + 1; m < T; m++) {
      TileArgs a = tile_args(A.tile_rows(m), A.tile_cols(k), 0, ld);
      Dtd::FlowSpec f[] = {{invgemm ? W->tile(k, k) : A.tile(k, k), ACCESS_IN},
                           {A.tile(m, k), ACCESS_INOUT}};
      tp.insert(invgemm ? &tc_strsm_inv() : &tc_strsm(), &a, sizeof(a), f, 2,
                (1 << 18) - (m - k), A.rank_of(m, k));
    }
    for (int n = k + 1; n < T; n++) {
      {
        TileArgs a = tile_args(0, A.tile_rows(n), A.tile_cols(k), ld);
        Dtd::FlowSpec f[] = {{A.tile(n, k), ACCESS_IN},
                             {A.tile(n, n), ACCESS_INOUT}};
        tp.insert(&tc_ssyrk(), &a, sizeof(a), f, 2, -(n - k) * 4 + 1,
                  A.rank_of(n, n));
      }
      for (int m = n + 1; m < T; m++) {
        TileArgs a =
            tile_args(A.tile_rows(m), A.tile_rows(n), A.tile_cols(k), ld);
        Dtd::FlowSpec f[] = {{A.tile(m, k), ACCESS_IN},
                             {A.tile(n, k), ACCESS_IN},
                             {A.tile(m, n), ACCESS_INOUT}};
        tp.insert(&tc_sgemm(), &a, sizeof(a), f, 3, -(n - k) * 4,
                  A.rank_of(m, n));
      }
    }
  }
}

// One task per tile of Src that holds or is going to hold data: a tile that
// no inserted task writes and that has no valid copy (the upper tiles after
// insert_spd_fill) has nothing to convert and is left out.
void insert_convert(Dtd& tp, TiledMatrix& Src, TiledMatrix& Dst) {
  PA_CHECK((Src.elem_size() == 8 && Dst.elem_size() == 4) ||
               (Src.elem_size() == 4 && Dst.elem_size() == 8),
           "insert_convert: element sizes %zu -> %zu, want 8 -> 4 or 4 -> 8",
           Src.elem_size(), Dst.elem_size());
  PA_CHECK(Src.m() == Dst.m() && Src.n() == Dst.n() && Src.mb() == Dst.mb() &&
               Src.nb() == Dst.nb() && Src.grid_p() == Dst.grid_p() &&
               Src.grid_q() == Dst.grid_q(),
           "insert_convert: Src and Dst differ in shape, tiling or grid");
  for (int tm = 0; tm < Src.mt(); tm++)
    for (int tn = 0; tn < Src.nt(); tn++) {
      Data* s = Src.tile(tm, tn);
      bool has_data = s->version > 0;
      if (!has_data) {
        SpinGuard gd(s->lock);
        has_data = s->host_valid || s->dev_valid;
      }
      if (!has_data) continue;
      TileArgs a = tile_args(Src.tile_rows(tm), Src.tile_cols(tn),
                             (int)Src.elem_size(), Src.mb());
      Dtd::FlowSpec f[] = {{s, ACCESS_IN}, {Dst.tile(tm, tn), ACCESS_OUT}};
      tp.insert(&tc_convert(), &a, sizeof(a), f, 2, 0, Src.rank_of(tm, tn));
    }
}

}  // namespace pa
