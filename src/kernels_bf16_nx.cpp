// bf16 MFMA tile-GEMM for column-major operands: the NN, NT and TT layouts.
//
// C[m x n] (fp32, col-major) (+)= op(A) op(B) on v_mfma_f32_16x16x32_bf16,
// where each operand is stored either K-major (A "T": k x m col-major, B "N":
// k x n col-major; what the TN kernels of kernels_bf16.cpp take) or
// M/N-major (A "N": m x k col-major, B "T": n x k col-major). TN itself
// never comes here.
//
// The MFMA wants, in lane l, the 8 consecutive-K values of row l&15 at K
// offset (l>>4)*8 (fragment comment in k_gemm_bf16_tn). A K-major operand
// has them contiguous, so its LDS image is [row][K] and one ds_read_b128
// fetches a fragment. An M-major operand has them a leading dimension apart.
// It is staged as it lies in memory, into a [K][row] image, and the
// transposition happens in the LDS read: gfx950's ds_read_b64_tr_b16 has
// each lane of a 16-lane group name 4 contiguous bf16 (8 B), takes the 16
// lanes' 64 values as a 4 x 16 block (lanes 4j..4j+3 supply row j) and
// hands lane i column i of it. With row j = K index and the 16 columns = the
// fragment's 16 rows, lane i receives 4 consecutive K of row i: two such
// reads give the b128 fragment. Nothing is transposed in global memory or
// in a pass before the kernel.
//
// Fast kernel: 256x256 tile, 8 waves, the K-half ring of k_gemm_bf16_tn_v3
// (4 slots x 32 K, counted vmcnt, one raw barrier per phase). 256^2 rather
// than 128^2 because that pipeline is the one this project has measured
// fastest (v3 vs v2), it needs the same number of async copies per wave and
// phase whatever the layout (so the counted waits are shared), and a 256
// row K-slice is 512 B, which leaves the image swizzle below enough room.
// Edge kernel: 128x128, reg-staged, every access guarded, any m, n, k, ld.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "device_gpu.hpp"
#include "kernels_bf16.hpp"

namespace pa {

typedef short bf16x4 __attribute__((ext_vector_type(4)));
#define PA_LDS __attribute__((address_space(3)))
#define PA_GLOBAL __attribute__((address_space(1)))

#define GX_BM 256
#define GX_BN 256
#define GX_KH 32  // K per phase

// Swizzle key of K-slice kk in a [K][row] image. One transposing read of a
// wave touches, per 16-lane group g, the four K-slices 8g+4h..8g+4h+3 and in
// each the same 32 B (16 rows). A 64-bit LDS read is served half a wave at a
// time, 32 lanes x 8 B = all 64 banks once if nothing collides. K-slices
// are 512 B apart, a multiple of the 256 B bank period, so unswizzled the 8
// slices of a half wave (kk = 4h..4h+3 and 8+4h..8+4h+3) would all hit the
// same 8 banks: an 8-way conflict, and no row padding separates slices 0 and
// 8 while keeping the 32 B groups aligned. Instead the 32 B group index is
// XORed with a key that differs for those 8 slices: bits 0-1 and bit 3 of
// kk. Bit 2 of kk is h, constant within a read, and bit 4 only separates
// the two half waves. The 8 groups of a half wave then tile the 256 B
// period exactly. The async copy cannot scatter (it writes lane-linear),
// so the swizzle is applied to its source address in units of 16 B chunks
// (key << 1), and matched on the read side.
__device__ __forceinline__ int tr_key(int kk) {
  return (kk & 3) | ((kk >> 1) & 4);
}

__device__ __forceinline__ void glds16(const bf16* src, bf16* dst) {
  __builtin_amdgcn_global_load_lds((const PA_GLOBAL unsigned int*)src,
                                   (PA_LDS unsigned int*)dst, 16, 0, 0);
}

// Stage one operand's 256 x 32 K-half into its 16 KB image: 2 async copies
// of 1 KB per wave. G(r, kk) is the operand's element for tile row r0 + r.
template <bool MAJOR>
__device__ __forceinline__ void nx_stage(const bf16* __restrict__ G, int ld,
                                         int r0, int k0, bf16* img, int wave,
                                         int lane) {
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const int piece = wave * 2 + p;
    const bf16* src;
    if (!MAJOR) {
      // [row][K]: 16 rows x 64 B per piece, v3's XOR through the source
      int row = piece * 16 + (lane >> 2);
      int kc = 8 * ((lane & 3) ^ ((row >> 2) & 3));
      src = G + (size_t)(r0 + row) * ld + k0 + kc;
    } else {
      // [K][row]: 2 K-slices x 512 B per piece; a lane's 16 B is 8
      // consecutive rows at one K, so the global read stays coalesced
      int kk = piece * 2 + (lane >> 5);
      int chunk = (lane & 31) ^ (tr_key(kk) << 1);
      src = G + (size_t)(k0 + kk) * ld + r0 + chunk * 8;
    }
    glds16(src, img + piece * 512);
  }
}

// The MFMA fragment of tile rows row0..row0+15 out of a K-half image.
template <bool MAJOR>
__device__ __forceinline__ bf16x8 nx_frag(const bf16* img, int row0,
                                          int lane) {
  const int g16 = lane >> 4, r16 = lane & 15;
  if (!MAJOR) {
    int row = row0 + r16;
    return *(const bf16x8*)&img[row * GX_KH +
                                ((g16 * 8) ^ (((row >> 2) & 3) * 8))];
  } else {
    // lane names rows rr..rr+3 of K-slice kk; it receives K-slices
    // 8*g16+4h..+3 of row row0+r16
    const int rr = row0 + 4 * (r16 & 3);
    bf16x4 v[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      int kk = 8 * g16 + 4 * h + (r16 >> 2);
      int off = kk * GX_BM + ((((rr >> 3) ^ (tr_key(kk) << 1))) << 3) +
                (rr & 7);
      v[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (PA_LDS bf16x4*)(img + off));
    }
    return __builtin_shufflevector(v[0], v[1], 0, 1, 2, 3, 4, 5, 6, 7);
  }
}

template <bool A_MMAJOR, bool B_NMAJOR>
__launch_bounds__(512)
__global__ void k_gemm_bf16_nx(int m, int n, int k,
                               const bf16* __restrict__ A, int lda,
                               const bf16* __restrict__ B, int ldb,
                               float* __restrict__ C, int ldc, int nbx,
                               int accum) {
  static_assert(GX_BM == GX_BN, "one image shape serves both operands");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* ring = (bf16*)smem;  // 4 slots x [A image | B image], 16 KB each
  constexpr int IMG = GX_BM * GX_KH;  // bf16 elements
  constexpr int SLOT = 2 * IMG;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 2, wc = wave & 3;  // 2(M) x 4(N): 128x64 per wave
  int id = bf_swz(blockIdx.x, gridDim.x);
  const int bm0 = (id % nbx) * GX_BM, bn0 = (id / nbx) * GX_BN;
  const int g16 = lane >> 4, r16 = lane & 15;

  f32x4 acc[8][4] = {};

  // K-half `ph` into ring slot ph&3: 4 async copies per wave
  auto stage = [&](int ph) {
    bf16* slot = ring + (ph & 3) * SLOT;
    nx_stage<A_MMAJOR>(A, lda, bm0, ph * GX_KH, slot, wave, lane);
    nx_stage<B_NMAJOR>(B, ldb, bn0, ph * GX_KH, slot + IMG, wave, lane);
  };

  const int P = k / GX_KH;
  stage(0);
  if (P > 1) stage(1);
  if (P > 2) stage(2);
  for (int ph = 0; ph < P; ph++) {
    // counted wait: this phase's K-half (own copies) has landed; up to two
    // newer phases x 4 copies stay in flight across the barrier. (The
    // compiler does not know what the transposing read may alias and puts
    // its own vmcnt(0) in front of the first one of a phase, so today only
    // the copies issued after this phase's reads overlap the MFMAs; the
    // ring and the counted waits are what a read it understands would need.)
    if (ph + 2 <= P - 1) {
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else if (ph + 1 == P - 1) {
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const bf16* as = ring + (ph & 3) * SLOT;
    const bf16* bs = as + IMG;
    bf16x8 a[8], b[4];
#pragma unroll
    for (int f = 0; f < 8; f++)
      a[f] = nx_frag<A_MMAJOR>(as, wr * 128 + f * 16, lane);
#pragma unroll
    for (int f = 0; f < 4; f++)
      b[f] = nx_frag<B_NMAJOR>(bs, wc * 64 + f * 16, lane);
    // slot (ph+3)&3 was read in phase ph-1; every wave has passed this
    // phase's barrier since, so it is free
    if (ph + 3 < P) stage(ph + 3);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j],
                                                            acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  }

  // C/D map: col = lane&15, row = (lane>>4)*4 + e
#pragma unroll
  for (int j = 0; j < 4; j++) {
    int col = bn0 + wc * 64 + j * 16 + r16;
    float* cp = C + (size_t)col * ldc;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      int row0 = bm0 + wr * 128 + i * 16 + g16 * 4;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        int row = row0 + e;
        cp[row] = accum ? cp[row] + acc[i][j][e] : acc[i][j][e];
      }
    }
  }
}

// ------------------------------------------------------------ edge kernel
// Sibling of k_gemm_bf16_tn for any m, n, k >= 1 and any leading dimension:
// 128x128 block, 4 waves, BK=32, reg-staged into a padded [row][K] image so
// the fragment reads stay single ds_read_b128. An M-major operand is
// transposed on the LDS write (8 ds_write_b16 per 16 B loaded). Loads are
// 16 B where the host found pointer and leading dimension 16 B aligned
// (`vec`) and all 8 elements in range, guarded element loads otherwise;
// everything past an edge is zero-filled.
#define GE_BM 128
#define GE_BK 32
#define GE_LDSK (GE_BK + 8)  // +16 B row pad: bank de-phasing, as in the TN kernel

template <bool MAJOR>
__device__ __forceinline__ void edge_stage(const bf16* __restrict__ G, int ld,
                                           int rows, int k, int r0, int k0,
                                           bool vec, bf16* img, int tid) {
  const short* g = (const short*)G;
  short* s = (short*)img;
  for (int x = tid; x < GE_BM * (GE_BK / 8); x += 256) {
    bf16x8 v = {};
    if (!MAJOR) {
      // slot: 8 consecutive K of one row
      int row = x >> 2, ck = (x & 3) * 8;
      int gr = r0 + row, gk = k0 + ck;
      if (gr < rows) {
        size_t base = (size_t)gr * ld + gk;
        if (vec && gk + 7 < k) {
          v = *(const bf16x8*)&g[base];
        } else {
#pragma unroll
          for (int e = 0; e < 8; e++)
            if (gk + e < k) v[e] = g[base + e];
        }
      }
      *(bf16x8*)&s[row * GE_LDSK + ck] = v;
    } else {
      // slot: 8 consecutive rows at one K
      int kk = x >> 4, cr = (x & 15) * 8;
      int gk = k0 + kk, gr = r0 + cr;
      if (gk < k) {
        size_t base = (size_t)gk * ld + gr;
        if (vec && gr + 7 < rows) {
          v = *(const bf16x8*)&g[base];
        } else {
#pragma unroll
          for (int e = 0; e < 8; e++)
            if (gr + e < rows) v[e] = g[base + e];
        }
      }
#pragma unroll
      for (int e = 0; e < 8; e++) s[(cr + e) * GE_LDSK + kk] = v[e];
    }
  }
}

template <bool A_MMAJOR, bool B_NMAJOR>
__launch_bounds__(256)
__global__ void k_gemm_bf16_nx_edge(int m, int n, int k,
                                    const bf16* __restrict__ A, int lda,
                                    const bf16* __restrict__ B, int ldb,
                                    float* __restrict__ C, int ldc, int nbx,
                                    int accum, int avec, int bvec) {
  __shared__ __attribute__((aligned(16))) bf16 As[GE_BM * GE_LDSK];
  __shared__ __attribute__((aligned(16))) bf16 Bs[GE_BM * GE_LDSK];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;  // 2x2 waves of 64x64
  int id = bf_swz(blockIdx.x, gridDim.x);
  const int bm0 = (id % nbx) * GE_BM, bn0 = (id / nbx) * GE_BM;
  const int g16 = lane >> 4, r16 = lane & 15;

  f32x4 acc[4][4] = {};

  for (int k0 = 0; k0 < k; k0 += GE_BK) {
    edge_stage<A_MMAJOR>(A, lda, m, k, bm0, k0, avec, As, tid);
    edge_stage<B_NMAJOR>(B, ldb, n, k, bn0, k0, bvec, Bs, tid);
    __syncthreads();
    bf16x8 a[4], b[4];
#pragma unroll
    for (int f = 0; f < 4; f++)
      a[f] = *(const bf16x8*)&As[(wr * 64 + f * 16 + r16) * GE_LDSK + g16 * 8];
#pragma unroll
    for (int f = 0; f < 4; f++)
      b[f] = *(const bf16x8*)&Bs[(wc * 64 + f * 16 + r16) * GE_LDSK + g16 * 8];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j],
                                                            acc[i][j], 0, 0, 0);
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < 4; j++) {
    int col = bn0 + wc * 64 + j * 16 + r16;
    if (col >= n) continue;
    float* cp = C + (size_t)col * ldc;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int row0 = bm0 + wr * 64 + i * 16 + g16 * 4;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        int row = row0 + e;
        if (row < m) cp[row] = accum ? cp[row] + acc[i][j][e] : acc[i][j][e];
      }
    }
  }
}

// ---------------------------------------------------------------- dispatch
template <bool A_MMAJOR, bool B_NMAJOR>
static void launch_nx(int m, int n, int k, const bf16* A, int lda,
                      const bf16* B, int ldb, float* C, int ldc,
                      hipStream_t stream, int accum) {
  // the 16 B copies need 16 B aligned addresses: base pointer and leading
  // dimension multiples of 8 elements (tile origins and K steps already are)
  const bool avec = (uintptr_t)A % 16 == 0 && lda % 8 == 0;
  const bool bvec = (uintptr_t)B % 16 == 0 && ldb % 8 == 0;
  if (avec && bvec && m % GX_BM == 0 && n % GX_BN == 0 && k % GX_KH == 0 &&
      k >= 4 * GX_KH) {
    constexpr size_t lds = 4 * (GX_BM + GX_BN) * GX_KH * 2;  // 128 KB
    static bool attr = false;
    if (!attr) {
      PA_HIP_CHECK(hipFuncSetAttribute(
          (const void*)k_gemm_bf16_nx<A_MMAJOR, B_NMAJOR>,
          hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      attr = true;
    }
    int nbx = m / GX_BM, nby = n / GX_BN;
    hipLaunchKernelGGL((k_gemm_bf16_nx<A_MMAJOR, B_NMAJOR>), dim3(nbx * nby),
                       dim3(512), lds, stream, m, n, k, A, lda, B, ldb, C,
                       ldc, nbx, accum);
    return;
  }
  int nbx = (m + GE_BM - 1) / GE_BM, nby = (n + GE_BM - 1) / GE_BM;
  hipLaunchKernelGGL((k_gemm_bf16_nx_edge<A_MMAJOR, B_NMAJOR>),
                     dim3(nbx * nby), dim3(256), 0, stream, m, n, k, A, lda,
                     B, ldb, C, ldc, nbx, accum, (int)avec, (int)bvec);
}

void launch_gemm_bf16_nx(int m, int n, int k, const void* A, int lda,
                         const void* B, int ldb, float* C, int ldc,
                         hipStream_t stream, int accum, bool a_mmajor,
                         bool b_nmajor) {
  PA_CHECK(a_mmajor || b_nmajor, "TN belongs to the kernels_bf16.cpp kernels");
  PA_CHECK(m >= 1 && n >= 1 && k >= 1 && ldc >= m);
  PA_CHECK(lda >= (a_mmajor ? m : k) && ldb >= (b_nmajor ? n : k),
           "leading dimension below the stored row count");
  const bf16* a = (const bf16*)A;
  const bf16* b = (const bf16*)B;
  if (a_mmajor && !b_nmajor)
    launch_nx<true, false>(m, n, k, a, lda, b, ldb, C, ldc, stream, accum);
  else if (a_mmajor)
    launch_nx<true, true>(m, n, k, a, lda, b, ldb, C, ldc, stream, accum);
  else
    launch_nx<false, true>(m, n, k, a, lda, b, ldb, C, ldc, stream, accum);
}

}  // namespace pa
