// MXFP6 tile-GEMM (OCP MX: E2M3 / E3M2 elements of 6 bits, one E8M0
// power-of-two scale per 32 consecutive K elements) and the fp32 -> MXFP6
// quantiser.
//
//   C[i,j] = alpha * sum_b 2^(SA[i,b] + SB[j,b] - 254) * sum_{p in b} A[i,p] B[j,p]
//            (+ C[i,j] when accum)
//
// A is m rows and B n rows of k elements, K contiguous: element p of a row is
// bits [6p, 6p + 6) of the row read as a little-endian bit string, four
// elements to three bytes, a scale block to 24 bytes, a row ceil(3k/4) bytes,
// lda / ldb in bytes. Spare high bits of the last byte are ignored. E2M3 is
// s.ee.mmm, bias 1, at most 7.5; E3M2 s.eee.mm, bias 3, at most 28; neither
// has an inf or NaN code. Each operand picks its format at compile time
// (cbsz / blgp 2 or 3). SA / SB and C as in kernels_mxfp8.cpp.
//
// The instruction (v_mfma_scale_f32_16x16x128_f8f6f4) takes six VGPRs per
// 6-bit operand. Measured on MI355X with one code per row under a distinct
// scale byte (test_mxfp6_gemm.py::test_routing): the layout is the one the
// ISA text gives, as for 4-bit operands and unlike the 8-bit one
// (f8_frag_mx). Lane l's six VGPRs are the 32 consecutive K elements
// [32 g, +32), g = l >> 4, of row l & 15 of a 128-element slab, 24 bytes in
// the packing above, element 0 in the low bits of the first VGPR; byte 0 of
// lane l's scale register (op_sel 0) scales exactly that block; cbsz / blgp
// 2 decodes E2M3 and 3 E3M2.
//
// A slab row is 96 bytes and a block 24, neither a power of two, and a
// block splits evenly only into 12-byte halves: a cut at 8 or 16 bytes goes
// through an element. global_load_lds moves 12 bytes per lane as dwordx3,
// but, measured on MI355X with a probe that dumps LDS after one copy, it
// writes lane l's 12 bytes at 16 l, not 12 l: every fourth dword of the
// destination is left alone. A 12-byte unit therefore costs 16 bytes of LDS,
// a 96-byte slab row 128, and a 128-element step of a 256-row operand 32 KB,
// so three ring slots do not fit the CU's 160 KB and a dense 192-byte row of
// 256 elements (96 KB a slot through 16-byte copies) does not fit twice.
// What fits is the geometry of kernels_fp8.cpp with 12 bytes in each chunk:
//
//   image      [row][128 B]: eight 16-byte chunks, chunk 2g the low and
//              chunk 2g + 1 the high 16 elements of block g in bytes 0..11,
//              bytes 12..15 never written or read; chunk c of row r stored
//              at chunk c ^ f8_key(r).
//   staging    one dwordx3 copy moves 8 rows x 96 contiguous global bytes
//              (lane l: row l >> 3, unit (l & 7) ^ key) into 8 rows x 128 of
//              the image; rows and bases need 4-byte alignment only.
//   fragment   two ds_read_b96 (f6_frag), chunks 2g and 2g + 1 of the lane's
//              row, into six consecutive VGPRs: the operand as it is, no
//              shuffling. Each read touches the first 12 bytes of a chunk
//              the FP8 kernel reads whole, so the bank argument at the head
//              of kernels_fp8.cpp covers it: the 16 lanes served together
//              (one g, rows r0..r0+15) hit 16 distinct 16-byte bank groups.
//   scales     as k_gemm_mxfp8: one dword per row and step, one ds_read_u8
//              per fragment.
//   ring       two slots of [A image | B image] = 128 KB and two 2 KB scale
//              images, the step schedule of k_gemm_fp8 (counted vmcnt, raw
//              barriers, s_setprio). A step is 32 MFMAs per wave as there,
//              each half as long as an 8-bit one, against the same 24 LDS
//              reads, 9 copies and two barriers.
#include <atomic>
#include <cmath>
#include <cstring>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "device_gpu.hpp"
#include "kernels.hpp"
#include "kernels_bench.hpp"
#include "kernels_fp8.hpp"
#include "profiling.hpp"

namespace pa {

#define MX_BLK 32                       // K elements per scale
#define F6_BB 24                        // bytes per scale block
#define F6_STEP 128                     // K elements per step
#define F6_RB 96                        // bytes of a row per step
#define F6_SIMG (4 * (F8_BM + F8_BN))   // a slot's scale image, bytes

typedef int i32x3 __attribute__((ext_vector_type(3)));

// The operand of `row` for lane group g16 out of a swizzled step image.
__device__ __forceinline__ i32x8 f6_frag(const char* img, int row, int g16) {
  const char* p = img + row * F8_KS;
  const int key = f8_key(row);
  const i32x3 lo = *(const i32x3*)(p + (((2 * g16) ^ key) << 4));
  const i32x3 hi = *(const i32x3*)(p + (((2 * g16 + 1) ^ key) << 4));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, -1, -1);
}

// FA / FB: 0 = E2M3, 1 = E3M2 (cbsz / blgp 2 and 3). sa / sb: in byte 0 the
// E8M0 scale of K block l >> 4 of the lane's row.
template <int FA, int FB>
__device__ __forceinline__ f32x4 f6_mfma(i32x8 a, i32x8 b, f32x4 c, int sa,
                                         int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 2 + FA,
                                                          2 + FB, 0, sa, 0, sb);
}

__device__ __forceinline__ int f6_scale(const char* simg, int row, int g16) {
  return *(const uint8_t*)(simg + row * 4 + g16);
}

// ------------------------------------------------------------ fast kernel
// k_gemm_mxfp8's block, wave grid, two-slot ring and step schedule (see there
// and k_gemm_fp8) over the image above: wave w copies rows [32w, 32w + 32) of
// each image in four dwordx3 copies of 8 rows, the swizzle goes through the
// source address, and one dword copy per wave moves the scales, so a stage
// is 9 copies and the counted wait is vmcnt(9). A fragment is six VGPRs, so
// the twelve of a step (72 VGPRs) would fit beside the accumulators; the A
// fragments still come in two groups of four so that the second group's
// reads run under the first group's MFMAs.
template <int FA, int FB>
__launch_bounds__(512)
__global__ void k_gemm_mxfp6(int m, int n, int k,
                             const uint8_t* __restrict__ A, int lda,
                             const uint8_t* __restrict__ SA, int ldsa,
                             const uint8_t* __restrict__ B, int ldb,
                             const uint8_t* __restrict__ SB, int ldsb,
                             float* __restrict__ C, int ldc, int nbx,
                             float alpha, int accum) {
  extern __shared__ __attribute__((aligned(16))) char mx6_ring[];
  constexpr int IMG = F8_BM * F8_KS;  // one operand's step image, 32 KB
  constexpr int SLOT = 2 * IMG;       // [A image | B image]
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wr = wave >> 2, wc = wave & 3;
  const int id = bf_swz(blockIdx.x, gridDim.x);
  const int bm0 = (id % nbx) * F8_BM, bn0 = (id / nbx) * F8_BN;
  const int g16 = lane >> 4, r16 = lane & 15;

  const int srow = lane >> 3, schunk = lane & 7;
  unsigned offA[4], offB[4];
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int row = (wave * 4 + p) * 8 + srow;
    const int kc = 12 * (schunk ^ f8_key(row));
    offA[p] = (unsigned)row * lda + kc;
    offB[p] = (unsigned)row * ldb + kc;
  }
  const uint8_t* baseA = A + (size_t)bm0 * lda;
  const uint8_t* baseB = B + (size_t)bn0 * ldb;
  const int srow0 = (wave & 3) * 64;
  const uint8_t* baseS = wave < 4 ? SA + (size_t)(bm0 + srow0) * ldsa
                                  : SB + (size_t)(bn0 + srow0) * ldsb;
  const unsigned offS = (unsigned)lane * (wave < 4 ? ldsa : ldsb);
  char* const simg = mx6_ring + 2 * SLOT;
  auto stage = [&](int t) {
    char* slot = mx6_ring + (t & 1) * SLOT + wave * 32 * F8_KS;
    const uint8_t* sa = baseA + (size_t)t * F6_RB;
    const uint8_t* sb = baseB + (size_t)t * F6_RB;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(sa + offA[p]),
          (__attribute__((address_space(3))) unsigned int*)(slot +
                                                            p * 8 * F8_KS),
          12, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(sb + offB[p]),
          (__attribute__((address_space(3))) unsigned int*)(slot + IMG +
                                                            p * 8 * F8_KS),
          12, 0, 0);
    }
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(
            baseS + (size_t)t * 4 + offS),
        (__attribute__((address_space(3))) unsigned int*)(
            simg + (t & 1) * F6_SIMG + wave * 256),
        4, 0, 0);
  };

  f32x4 acc[8][4] = {};
  auto step = [&](int t, auto restage, auto last) {
    if constexpr (decltype(last)::value) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const char* as = mx6_ring + (t & 1) * SLOT;
    const char* bs = as + IMG;
    const char* ssa = simg + (t & 1) * F6_SIMG;
    const char* ssb = ssa + 4 * F8_BM;
    i32x8 b[4], a0[4], a1[4];
    int sb[4], sa0[4], sa1[4];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      b[f] = f6_frag(bs, wc * 64 + f * 16 + r16, g16);
      sb[f] = f6_scale(ssb, wc * 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int f = 0; f < 4; f++) {
      a0[f] = f6_frag(as, wr * 128 + f * 16 + r16, g16);
      sa0[f] = f6_scale(ssa, wr * 128 + f * 16 + r16, g16);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 4; j++)
      acc[0][j] = f6_mfma<FA, FB>(a0[0], b[j], acc[0][j], sa0[0], sb[j]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < 4; f++) {
      a1[f] = f6_frag(as, wr * 128 + 64 + f * 16 + r16, g16);
      sa1[f] = f6_scale(ssa, wr * 128 + 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int i = 1; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f6_mfma<FA, FB>(a0[i], b[j], acc[i][j], sa0[i], sb[j]);
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int i = 0; i < 16; i++) f8_pin(acc[i >> 2][i & 3]);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (decltype(restage)::value) stage(t + 2);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[4 + i][j] =
            f6_mfma<FA, FB>(a1[i], b[j], acc[4 + i][j], sa1[i], sb[j]);
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int i = 0; i < 16; i++) f8_pin(acc[4 + (i >> 2)][i & 3]);
    __builtin_amdgcn_sched_barrier(0);
  };
  const int T = k / F6_STEP;  // >= 2
  stage(0);
  stage(1);
  for (int t = 0; t < T - 2; t++) step(t, std::true_type{}, std::false_type{});
  step(T - 2, std::false_type{}, std::false_type{});
  step(T - 1, std::false_type{}, std::true_type{});

#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int col = bn0 + wc * 64 + j * 16 + r16;
    float* cp = C + (size_t)col * ldc;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int row0 = bm0 + wr * 128 + i * 16 + g16 * 4;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int row = row0 + e;
        const float v = alpha * acc[i][j][e];
        cp[row] = accum ? cp[row] + v : v;
      }
    }
  }
}

// ------------------------------------------------------------ edge kernel
// 128x128 block, 4 waves as 2 x 2, 64x64 per wave, one unringed step image
// in the fast kernel's layout, written from guarded loads: any m,
// n, k >= 1, any leading dimension and alignment. Bits of a row at and past
// 6k are zero; a row past m / n or a block past k takes scale byte 127, so
// the padding adds exact zeros and never meets a NaN scale.

// The 12-byte unit of a packed row at byte b0 into dst; nothing is read when
// !ok.
__device__ __forceinline__ void f6_load12(const uint8_t* row, bool ok, int b0,
                                          int k, unsigned* dst) {
  const int full = (int)((3LL * k) >> 2);      // whole bytes of the row
  const int rem = 2 * ((3 * (k & 3)) & 3);     // bits of the byte after them
  unsigned w[3] = {0, 0, 0};
  if (ok && b0 + 12 <= full) {
    __builtin_memcpy(w, row + b0, 12);
  } else if (ok) {
#pragma unroll
    for (int e = 0; e < 12; e++) {
      const int at = b0 + e;
      unsigned byte = 0;
      if (at < full)
        byte = row[at];
      else if (at == full && rem)
        byte = row[at] & ((1u << rem) - 1);
      w[e >> 2] |= byte << (8 * (e & 3));
    }
  }
  dst[0] = w[0];
  dst[1] = w[1];
  dst[2] = w[2];
}

template <int FA, int FB>
__launch_bounds__(256)
__global__ void k_gemm_mxfp6_edge(int m, int n, int k,
                                  const uint8_t* __restrict__ A, int lda,
                                  const uint8_t* __restrict__ SA, int ldsa,
                                  const uint8_t* __restrict__ B, int ldb,
                                  const uint8_t* __restrict__ SB, int ldsb,
                                  float* __restrict__ C, int ldc, int nbx,
                                  float alpha, int accum) {
  __shared__ __attribute__((aligned(16))) char As[F8E_BM * F8_KS];
  __shared__ __attribute__((aligned(16))) char Bs[F8E_BN * F8_KS];
  __shared__ __attribute__((aligned(16))) char Ss[2][F8E_BM * 4];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int id = bf_swz(blockIdx.x, gridDim.x);
  const int bm0 = (id % nbx) * F8E_BM, bn0 = (id / nbx) * F8E_BN;
  const int g16 = lane >> 4, r16 = lane & 15;
  const int kblocks = (k + MX_BLK - 1) / MX_BLK;
  // this thread's scale row: A rows for tid < 128, B rows after
  const int sop = tid >> 7, srow = tid & 127;
  const int sg = (sop ? bn0 : bm0) + srow;
  const bool sok = sg < (sop ? n : m);
  const uint8_t* sp = sop ? SB + (size_t)sg * ldsb : SA + (size_t)sg * ldsa;

  f32x4 acc[4][4] = {};
  for (int k0 = 0, b0 = 0; k0 < k; k0 += F6_STEP, b0 += F6_RB) {
#pragma unroll
    for (int x = tid; x < F8E_BM * 8; x += 256) {
      const int row = x >> 3, u = x & 7;  // 12-byte unit u of the row's slab
      const int off = row * F8_KS + ((u ^ f8_key(row)) << 4);
      const int gm = bm0 + row, gn = bn0 + row;
      f6_load12(A + (size_t)gm * lda, gm < m, b0 + 12 * u, k,
                (unsigned*)(As + off));
      f6_load12(B + (size_t)gn * ldb, gn < n, b0 + 12 * u, k,
                (unsigned*)(Bs + off));
    }
    unsigned sw = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int blk = k0 / MX_BLK + e;
      const unsigned byte = sok && blk < kblocks ? sp[blk] : 127u;
      sw |= byte << (8 * e);
    }
    *(unsigned*)(Ss[sop] + srow * 4) = sw;
    __syncthreads();
    i32x8 a[4], b[4];
    int sa[4], sb[4];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      a[f] = f6_frag(As, wr * 64 + f * 16 + r16, g16);
      sa[f] = f6_scale(Ss[0], wr * 64 + f * 16 + r16, g16);
      b[f] = f6_frag(Bs, wc * 64 + f * 16 + r16, g16);
      sb[f] = f6_scale(Ss[1], wc * 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f6_mfma<FA, FB>(a[i], b[j], acc[i][j], sa[i], sb[j]);
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int col = bn0 + wc * 64 + j * 16 + r16;
    if (col >= n) continue;
    float* cp = C + (size_t)col * ldc;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int row0 = bm0 + wr * 64 + i * 16 + g16 * 4;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int row = row0 + e;
        const float v = alpha * acc[i][j][e];
        if (row < m) cp[row] = accum ? cp[row] + v : v;
      }
    }
  }
}

// ---------------------------------------------------------------- dispatch
static int f6_kbytes(int k) { return (int)((3LL * k + 3) / 4); }

template <int FA, int FB>
static void launch_gemm_mxfp6_fmt(int m, int n, int k, const uint8_t* A,
                                  int lda, const uint8_t* SA, int ldsa,
                                  const uint8_t* B, int ldb, const uint8_t* SB,
                                  int ldsb, float* C, int ldc, float alpha,
                                  int accum, hipStream_t stream) {
  // whole 96-byte steps of dword-aligned 12-byte units, whole aligned scale
  // dwords, 32-bit lane offsets
  const bool fast = m % F8_BM == 0 && n % F8_BN == 0 && k % F6_STEP == 0 &&
                    k >= 2 * F6_STEP && lda % 4 == 0 && ldb % 4 == 0 &&
                    lda < (1 << 23) && ldb < (1 << 23) &&
                    ((uintptr_t)A | (uintptr_t)B) % 4 == 0 &&
                    ldsa % 4 == 0 && ldsb % 4 == 0 && ldsa < (1 << 23) &&
                    ldsb < (1 << 23) &&
                    ((uintptr_t)SA | (uintptr_t)SB) % 4 == 0;
  if (fast) {
    constexpr size_t lds = 2 * (F8_BM + F8_BN) * F8_KS + 2 * F6_SIMG;  // 132 KB
    static std::atomic<bool> attr[64];  // per device, as in kernels_fp8.cpp
    int dev = 0;
    PA_HIP_CHECK(hipGetDevice(&dev));
    PA_CHECK(dev >= 0 && dev < 64);
    if (!attr[dev].load(std::memory_order_acquire)) {
      PA_HIP_CHECK(hipFuncSetAttribute(
          (const void*)k_gemm_mxfp6<FA, FB>,
          hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      attr[dev].store(true, std::memory_order_release);
    }
    const int nbx = m / F8_BM, nby = n / F8_BN;
    hipLaunchKernelGGL((k_gemm_mxfp6<FA, FB>), dim3(nbx * nby), dim3(512), lds,
                       stream, m, n, k, A, lda, SA, ldsa, B, ldb, SB, ldsb, C,
                       ldc, nbx, alpha, accum);
    return;
  }
  const int nbx = (m + F8E_BM - 1) / F8E_BM, nby = (n + F8E_BN - 1) / F8E_BN;
  hipLaunchKernelGGL((k_gemm_mxfp6_edge<FA, FB>), dim3(nbx * nby), dim3(256),
                     0, stream, m, n, k, A, lda, SA, ldsa, B, ldb, SB, ldsb, C,
                     ldc, nbx, alpha, accum);
}

struct Mx6Operand {
  const void* p;   // packed elements, rows ld bytes apart
  int ld, fmt;     // fmt: 0 = E2M3, 1 = E3M2
  const void* s;   // scale bytes, rows lds apart
  int lds;
};

static void launch_gemm_mxfp6(int m, int n, int k, const Mx6Operand& a,
                              const Mx6Operand& b, float* C, int ldc,
                              float alpha, int accum, hipStream_t stream) {
  PA_CHECK(m >= 1 && n >= 1 && k >= 1);
  const int kbytes = f6_kbytes(k), kb = (k + MX_BLK - 1) / MX_BLK;
  PA_CHECK((a.fmt | b.fmt | 1) == 1, "fp6 format is 0 (e2m3) or 1 (e3m2)");
  PA_CHECK(a.ld >= kbytes && b.ld >= kbytes && ldc >= m && a.lds >= kb &&
           b.lds >= kb);
  auto go = [&](auto fa, auto fb) {
    launch_gemm_mxfp6_fmt<decltype(fa)::value, decltype(fb)::value>(
        m, n, k, (const uint8_t*)a.p, a.ld, (const uint8_t*)a.s, a.lds,
        (const uint8_t*)b.p, b.ld, (const uint8_t*)b.s, b.lds, C, ldc, alpha,
        accum, stream);
  };
  using F0 = std::integral_constant<int, 0>;
  using F1 = std::integral_constant<int, 1>;
  switch (a.fmt * 2 + b.fmt) {
    case 0: go(F0{}, F0{}); break;
    case 1: go(F0{}, F1{}); break;
    case 2: go(F1{}, F0{}); break;
    default: go(F1{}, F1{});
  }
}

// --------------------------------------------------------------- quantiser
// Per block of 32: amax = max|x|, X = floor(log2 amax) - emax clamped to
// [-127, 127] (emax 2 for E2M3, 4 for E3M2), scale byte X + 127, elements
// x * 2^-X clamped to +-7.5 / +-28 and rounded to nearest even. An all-zero
// block gets byte 127 and zero elements. With e the exponent field of amax
// the byte is max(e - emax, 0) and 2^-X the float with exponent field
// 254 - byte, as in kernels_mxfp8.cpp. The conversion is
// v_cvt_scalef32_2xpk16_{fp6,bf6}_f32 under scale 1.0 on the clamped values:
// only its in-range rounding is relied on. It packs 32 elements into six
// dwords; measured on MI355X (test_mxfp6_gemm.py::test_quantiser), element 2i
// comes from float i of its first source and element 2i + 1 from float i of
// its second.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x6 __attribute__((ext_vector_type(6)));

template <int F>
__device__ __forceinline__ int f6_scale_byte(float amax) {
  const int e = (__float_as_uint(amax) >> 23) & 0xff;
  return amax == 0.f ? 127 : max(e - (F ? 4 : 2), 0);
}

template <int F>
__device__ __forceinline__ float f6_scaled(float x, int byte, bool zero) {
  const float lim = F ? 28.f : 7.5f;
  const float y = x * __uint_as_float((unsigned)(254 - byte) << 23);
  return zero ? 0.f : fminf(fmaxf(y, -lim), lim);
}

// y[0..31] in element order -> the 24 bytes of the block
template <int F>
__device__ __forceinline__ u32x6 f6_cvt32(const float (&y)[32]) {
  f32x16 s0, s1;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    s0[i] = y[2 * i];
    s1[i] = y[2 * i + 1];
  }
  if constexpr (F)
    return __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(s0, s1, 1.0f);
  else
    return __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(s0, s1, 1.0f);
}

// Two lanes cover a block, 16 floats each (four float4 loads, the 12 bytes
// of 16 elements stored as three dwords), so a wave reads 4 KB contiguous
// along K (32 blocks); wave w of the grid takes segment w % nseg of row
// w / nseg. The block's amax is one xor shuffle. A lane converts its 16
// values as the low half of a block of 32 whose high half is zero and keeps
// the first three dwords. Needs k % 32 == 0 and 16- / 4-byte aligned X / Q
// rows.
template <int F>
__launch_bounds__(256)
__global__ void k_quant_mxfp6(int rows, int k, const float* __restrict__ X,
                              int ldx, uint8_t* __restrict__ Q, int ldq,
                              uint8_t* __restrict__ S, int lds, int nseg) {
  const size_t gw = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int row = (int)(gw / nseg), seg = (int)(gw % nseg);
  if (row >= rows) return;  // the whole wave
  const int k0 = seg * 1024 + lane * 16;
  const bool on = k0 < k;   // whole blocks: k % 32 == 0
  float y[32] = {};
  if (on) {
    const float4* x = (const float4*)(X + (size_t)row * ldx + k0);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float4 v = x[i];
      y[4 * i] = v.x;
      y[4 * i + 1] = v.y;
      y[4 * i + 2] = v.z;
      y[4 * i + 3] = v.w;
    }
  }
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) amax = fmaxf(amax, fabsf(y[i]));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  const int byte = f6_scale_byte<F>(amax);
  const bool zero = amax == 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) y[i] = f6_scaled<F>(y[i], byte, zero);
  const u32x6 w = f6_cvt32<F>(y);
  if (on) {
    unsigned* q = (unsigned*)(Q + (size_t)row * ldq + (k0 / 4) * 3);
    q[0] = w[0];
    q[1] = w[1];
    q[2] = w[2];
    if ((lane & 1) == 0) S[(size_t)row * lds + k0 / MX_BLK] = (uint8_t)byte;
  }
}

// Any k, leading dimension and alignment: one thread per block, bytewise;
// elements past k convert as zeros, so the spare bits of the last byte are 0.
template <int F>
__launch_bounds__(256)
__global__ void k_quant_mxfp6_any(int rows, int k, const float* __restrict__ X,
                                  int ldx, uint8_t* __restrict__ Q, int ldq,
                                  uint8_t* __restrict__ S, int lds) {
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * kb) return;
  const int row = (int)(idx / kb), blk = (int)(idx % kb);
  const int k0 = blk * MX_BLK, len = min(MX_BLK, k - k0);
  const float* x = X + (size_t)row * ldx + k0;
  uint8_t* q = Q + (size_t)row * ldq + (size_t)blk * F6_BB;
  float y[32];
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 32; e++) {
    y[e] = e < len ? x[e] : 0.f;
    amax = fmaxf(amax, fabsf(y[e]));
  }
  const int byte = f6_scale_byte<F>(amax);
  const bool zero = amax == 0.f;
#pragma unroll
  for (int e = 0; e < 32; e++) y[e] = f6_scaled<F>(y[e], byte, zero);
  const u32x6 w = f6_cvt32<F>(y);
  const int nbytes = (3 * len + 3) / 4;
#pragma unroll
  for (int e = 0; e < F6_BB; e++)
    if (e < nbytes) q[e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
  S[(size_t)row * lds + blk] = (uint8_t)byte;
}

static void launch_quant_mxfp6(int rows, int k, int fmt, const float* X,
                               int ldx, uint8_t* Q, int ldq, uint8_t* S,
                               int lds, hipStream_t stream) {
  PA_CHECK(rows >= 1 && k >= 1);
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  PA_CHECK((fmt | 1) == 1, "fp6 format is 0 (e2m3) or 1 (e3m2)");
  PA_CHECK(ldx >= k && ldq >= f6_kbytes(k) && lds >= kb);
  const bool fast = k % MX_BLK == 0 && ldx % 4 == 0 && ldq % 4 == 0 &&
                    (uintptr_t)X % 16 == 0 && (uintptr_t)Q % 4 == 0;
  if (fast) {
    const int nseg = (k + 1023) / 1024;
    const size_t waves = (size_t)rows * nseg;
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (fmt)
      hipLaunchKernelGGL(k_quant_mxfp6<1>, grid, dim3(256), 0, stream, rows, k,
                         X, ldx, Q, ldq, S, lds, nseg);
    else
      hipLaunchKernelGGL(k_quant_mxfp6<0>, grid, dim3(256), 0, stream, rows, k,
                         X, ldx, Q, ldq, S, lds, nseg);
    return;
  }
  const dim3 grid((unsigned)(((size_t)rows * kb + 255) / 256));
  if (fmt)
    hipLaunchKernelGGL(k_quant_mxfp6_any<1>, grid, dim3(256), 0, stream, rows,
                       k, X, ldx, Q, ldq, S, lds);
  else
    hipLaunchKernelGGL(k_quant_mxfp6_any<0>, grid, dim3(256), 0, stream, rows,
                       k, X, ldx, Q, ldq, S, lds);
}

// ------------------------------------------------------------------ chores
// The CPU chores are the formulas of the head comment in double.

// The value of every 6-bit code: [0] E2M3 (s.ee.mmm, bias 1), [1] E3M2
// (s.eee.mm, bias 3); there is no NaN or inf code.
struct Fp6Tables {
  double v[2][64];
  Fp6Tables() {
    for (int c = 0; c < 64; c++) {
      const double s = c & 32 ? -1.0 : 1.0;
      int e = (c >> 3) & 3, f = c & 7;
      v[0][c] = s * (e ? std::ldexp(8.0 + f, e - 4) : f / 8.0);
      e = (c >> 2) & 7, f = c & 3;
      v[1][c] = s * (e ? std::ldexp(4.0 + f, e - 5) : f / 16.0);
    }
  }
};
static const Fp6Tables fp6_tab;

static int fp6_format(const std::string& f) {
  PA_CHECK(f == "e2m3" || f == "e3m2", "fp6 format is \"e2m3\" or \"e3m2\"");
  return f == "e3m2";
}

// y within the format's range onto the nearest code, a tie to the even code.
static uint8_t fp6_encode(double y, int fmt) {
  const double a = std::fabs(y);
  int best = 0;
  for (int c = 1; c < 32; c++) {
    const double d = std::fabs(a - fp6_tab.v[fmt][c]);
    const double db = std::fabs(a - fp6_tab.v[fmt][best]);
    if (d < db || (d == db && !(c & 1))) best = c;
  }
  return (uint8_t)((std::signbit(y) ? 32 : 0) | best);
}

static void cpu_quant_mxfp6(Task& t) {
  const QuantMxfp6Args& a = t.arg<QuantMxfp6Args>();
  const float* X = (const float*)t.flows[0].data->pull_to_host();
  Data *qd = t.flows[1].data, *sd = t.flows[2].data;
  uint8_t* Q = (uint8_t*)qd->ensure_host();
  uint8_t* S = (uint8_t*)sd->ensure_host();
  const int emax = a.fmt ? 4 : 2;
  const double lim = a.fmt ? 28.0 : 7.5;
  for (int r = 0; r < a.rows; r++) {
    uint8_t* q = Q + (size_t)r * a.ldq;
    std::memset(q, 0, f6_kbytes(a.k));
    for (int k0 = 0; k0 < a.k; k0 += MX_BLK) {
      const int len = std::min(MX_BLK, a.k - k0);
      const float* x = X + (size_t)r * a.ldx + k0;
      double amax = 0;
      for (int e = 0; e < len; e++) amax = std::max(amax, std::fabs((double)x[e]));
      int ex = 0;
      if (amax > 0) ex = std::min(127, std::max(-127, std::ilogb(amax) - emax));
      S[(size_t)r * a.lds + k0 / MX_BLK] = (uint8_t)(ex + 127);
      for (int e = 0; e < len; e++) {
        const double y = std::ldexp((double)x[e], -ex);
        const unsigned c =
            amax > 0 ? fp6_encode(std::min(lim, std::max(-lim, y)), a.fmt) : 0;
        const int bit = 6 * (k0 + e);
        q[bit >> 3] |= (uint8_t)(c << (bit & 7));
        if ((bit & 7) > 2) q[(bit >> 3) + 1] |= (uint8_t)(c >> (8 - (bit & 7)));
      }
    }
  }
  qd->written_on(false);
  sd->written_on(false);
}

static void gpu_quant_mxfp6(Task& t, GpuTaskCtx& g) {
  const QuantMxfp6Args& a = t.arg<QuantMxfp6Args>();
  launch_quant_mxfp6(a.rows, a.k, a.fmt, (const float*)t.dev_ptr[0], a.ldx,
                     (uint8_t*)t.dev_ptr[1], a.ldq, (uint8_t*)t.dev_ptr[2],
                     a.lds, g.stream);
}

static void cpu_gemm_mxfp6(Task& t) {
  const GemmMxfp6Args& a = t.arg<GemmMxfp6Args>();
  const uint8_t* A = (const uint8_t*)t.flows[0].data->pull_to_host();
  const uint8_t* SA = (const uint8_t*)t.flows[1].data->pull_to_host();
  const uint8_t* B = (const uint8_t*)t.flows[2].data->pull_to_host();
  const uint8_t* SB = (const uint8_t*)t.flows[3].data->pull_to_host();
  Data* cd = t.flows[4].data;
  float* C = a.accum ? (float*)cd->pull_to_host() : (float*)cd->ensure_host();
  const int ldc = cd->coll->mb();
  auto el = [](const uint8_t* row, int p, int fmt) {
    const int bit = 6 * p;
    unsigned w = row[bit >> 3];
    if ((bit & 7) > 2) w |= (unsigned)row[(bit >> 3) + 1] << 8;
    return fp6_tab.v[fmt][(w >> (bit & 7)) & 63];
  };
  for (int j = 0; j < a.n; j++)
    for (int i = 0; i < a.m; i++) {
      const uint8_t* ar = A + (size_t)i * a.lda;
      const uint8_t* br = B + (size_t)j * a.ldb;
      const uint8_t* sa = SA + (size_t)i * a.ldsa;
      const uint8_t* sb = SB + (size_t)j * a.ldsb;
      double s = 0;
      for (int k0 = 0; k0 < a.k; k0 += MX_BLK) {
        const int ea = sa[k0 / MX_BLK], eb = sb[k0 / MX_BLK];
        double d = 0;
        for (int p = k0; p < std::min(a.k, k0 + MX_BLK); p++)
          d += el(ar, p, a.fmt_a) * el(br, p, a.fmt_b);
        s += ea == 255 || eb == 255 ? (double)NAN : std::ldexp(d, ea + eb - 254);
      }
      float& c = C[(size_t)j * ldc + i];
      c = (float)(a.accum ? c + a.alpha * s : a.alpha * s);
    }
  cd->written_on(false);
}

static void gpu_gemm_mxfp6(Task& t, GpuTaskCtx& g) {
  const GemmMxfp6Args& a = t.arg<GemmMxfp6Args>();
  launch_gemm_mxfp6(a.m, a.n, a.k,
                    {t.dev_ptr[0], a.lda, a.fmt_a, t.dev_ptr[1], a.ldsa},
                    {t.dev_ptr[2], a.ldb, a.fmt_b, t.dev_ptr[3], a.ldsb},
                    (float*)t.dev_ptr[4], t.flows[4].data->coll->mb(), a.alpha,
                    a.accum, g.stream);
}

TaskClass& tc_gemm_mxfp6() {
  static TaskClass tc = make_tc("gemm_mxfp6", TaskKind::GPU, cpu_gemm_mxfp6,
                                gpu_gemm_mxfp6, TC_GEMM_MXFP6);
  return tc;
}
TaskClass& tc_quant_mxfp6() {
  static TaskClass tc = make_tc("quant_mxfp6", TaskKind::GPU, cpu_quant_mxfp6,
                                gpu_quant_mxfp6, TC_QUANT_MXFP6);
  return tc;
}

// ------------------------------------------------------------ DAG builders
// S holds the scales of the packed operand A (3K/4 bytes x rows): K/32 rows,
// one per 24 bytes, in tiles of A.mb()/24 rows and the column tiling of A, so
// that tile (k, m) of S belongs to tile (k, m) of A.
static void check_scales6(TiledMatrix& A, TiledMatrix& S) {
  PA_CHECK(A.elem_size() == 1 && S.elem_size() == 1);
  PA_CHECK(A.mb() % F6_BB == 0, "the K tile must be a multiple of 24 bytes");
  PA_CHECK(A.m() % 3 == 0, "K must be a multiple of 4 elements");
  PA_CHECK(S.m() == (A.m() + F6_BB - 1) / F6_BB && S.mb() == A.mb() / F6_BB &&
               S.n() == A.n() && S.nb() == A.nb() && S.mt() == A.mt() &&
               S.nt() == A.nt(),
           "scales are K/32 x rows in tiles of mb/24 x nb");
}

void insert_gemm_mxfp6(Dtd& tp, TiledMatrix& A, TiledMatrix& SA,
                       TiledMatrix& B, TiledMatrix& SB, TiledMatrix& C,
                       float alpha, const std::string& a_format,
                       const std::string& b_format) {
  PA_CHECK(C.elem_size() == 4);
  check_scales6(A, SA);
  check_scales6(B, SB);
  PA_CHECK(A.m() == B.m() && A.mb() == B.mb(), "K tilings must match");
  PA_CHECK(A.n() == C.m() && B.n() == C.n() && A.nb() == C.mb() &&
               B.nb() == C.nb(),
           "A is 3K/4 x M, B is 3K/4 x N, C is M x N with matching tiles");
  GemmMxfp6Args a;
  a.alpha = alpha;
  a.fmt_a = fp6_format(a_format);
  a.fmt_b = fp6_format(b_format);
  a.lda = A.mb();
  a.ldb = B.mb();
  a.ldsa = SA.mb();
  a.ldsb = SB.mb();
  for (int m = 0; m < C.mt(); m++)
    for (int n = 0; n < C.nt(); n++)
      for (int k = 0; k < A.mt(); k++) {
        a.m = A.tile_cols(m);
        a.n = B.tile_cols(n);
        a.k = A.tile_rows(k) / 3 * 4;
        a.accum = (k != 0);
        Dtd::FlowSpec f[] = {{A.tile(k, m), ACCESS_IN},
                             {SA.tile(k, m), ACCESS_IN},
                             {B.tile(k, n), ACCESS_IN},
                             {SB.tile(k, n), ACCESS_IN},
                             {C.tile(m, n),
                              k == 0 ? ACCESS_OUT : ACCESS_INOUT}};
        tp.insert(&tc_gemm_mxfp6(), &a, sizeof(a), f, 5, -(k),
                  C.rank_of(m, n));
      }
}

// X is fp32, K x rows in column-major tiles (a tile's column is an operand
// row), Q its packed elements, 3K/4 x rows with three quarters of the K
// tile, S the scales as check_scales6 wants.
void insert_quantize_mxfp6(Dtd& tp, TiledMatrix& X, TiledMatrix& Q,
                           TiledMatrix& S, const std::string& format) {
  PA_CHECK(X.elem_size() == 4);
  PA_CHECK(3 * (long)X.m() == 4 * (long)Q.m() && X.n() == Q.n() &&
               3 * (long)X.mb() == 4 * (long)Q.mb() && X.nb() == Q.nb(),
           "X is K x rows and Q 3K/4 x rows with 3/4 of the K tile");
  check_scales6(Q, S);
  QuantMxfp6Args a;
  a.fmt = fp6_format(format);
  a.ldx = X.mb();
  a.ldq = Q.mb();
  a.lds = S.mb();
  for (int k = 0; k < X.mt(); k++)
    for (int r = 0; r < X.nt(); r++) {
      a.rows = X.tile_cols(r);
      a.k = X.tile_rows(k);
      Dtd::FlowSpec f[] = {{X.tile(k, r), ACCESS_IN},
                           {Q.tile(k, r), ACCESS_OUT},
                           {S.tile(k, r), ACCESS_OUT}};
      tp.insert(&tc_quant_mxfp6(), &a, sizeof(a), f, 3, 0, Q.rank_of(k, r));
    }
}

// ------------------------------------------------- bench and test entries
// Synthetic bytes: hashed bits (every 6-bit code is a finite value), or scale
// bytes hashed into 120..134 (none a NaN).
__global__ void k_fill_mx6(uint8_t* p, size_t nbytes, uint32_t seed,
                           int scales) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < nbytes; i += (size_t)gridDim.x * blockDim.x) {
    const uint8_t b = fp8_fill_byte(i, seed);
    p[i] = scales ? 120 + b % 15 : b;
  }
}

// Synthetic fp32 input of the quantiser: hashed integers in [-95, 96].
__global__ void k_fill_mx6_f32(float* p, size_t n, uint32_t seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = (float)fp8_fill_byte(i, seed) - 95.f;
}

// kernel-level microbench (TFLOP/s)
double bench_gemm_mxfp6(int m, int n, int k, int iters, int fmt_a, int fmt_b) {
  const int kbytes = f6_kbytes(k), kb = (k + MX_BLK - 1) / MX_BLK;
  DevArray<uint8_t> dA((size_t)m * kbytes), dB((size_t)n * kbytes);
  DevArray<uint8_t> dSA((size_t)m * kb), dSB((size_t)n * kb);
  DevArray<float> dC((size_t)m * n);
  auto fill = [](DevArray<uint8_t>& d, uint32_t seed, int scales) {
    hipLaunchKernelGGL(k_fill_mx6, dim3(2048), dim3(256), 0, 0, d.p, d.bytes,
                       seed, scales);
  };
  fill(dA, 1u, 0);
  fill(dB, 2u, 0);
  fill(dSA, 3u, 1);
  fill(dSB, 4u, 1);
  PA_HIP_CHECK(hipMemset(dC.p, 0, dC.bytes));
  double dt = time_launches(iters, [&] {
    launch_gemm_mxfp6(m, n, k, {dA.p, kbytes, fmt_a, dSA.p, kb},
                      {dB.p, kbytes, fmt_b, dSB.p, kb}, dC.p, m, 1.f, 1, 0);
  });
  return 2.0 * m * n * k * iters / dt / 1e12;
}

// quantiser microbench: GB/s over the bytes read and written
double bench_quantize_mxfp6(int rows, int k, int iters, int fmt) {
  const int kbytes = f6_kbytes(k), kb = (k + MX_BLK - 1) / MX_BLK;
  DevArray<float> dX((size_t)rows * k);
  DevArray<uint8_t> dQ((size_t)rows * kbytes), dS((size_t)rows * kb);
  hipLaunchKernelGGL(k_fill_mx6_f32, dim3(2048), dim3(256), 0, 0, dX.p,
                     (size_t)rows * k, 5u);
  double dt = time_launches(iters, [&] {
    launch_quant_mxfp6(rows, k, fmt, dX.p, k, dQ.p, kbytes, dS.p, kb, 0);
  });
  return (double)(dX.bytes + dQ.bytes + dS.bytes) * iters / dt / 1e9;
}

// host-I/O numerics harnesses; every leading dimension is given
void test_gemm_mxfp6_hip(int m, int n, int k, const uint8_t* A, int fmt_a,
                         const uint8_t* SA, const uint8_t* B, int fmt_b,
                         const uint8_t* SB, float* C, float alpha, int lda,
                         int ldb, int ldsa, int ldsb, int accum) {
  DevArray<uint8_t> dA((size_t)lda * m, A), dB((size_t)ldb * n, B);
  DevArray<uint8_t> dSA((size_t)ldsa * m, SA), dSB((size_t)ldsb * n, SB);
  DevArray<float> dC((size_t)m * n, C);
  launch_gemm_mxfp6(m, n, k, {dA.p, lda, fmt_a, dSA.p, ldsa},
                    {dB.p, ldb, fmt_b, dSB.p, ldsb}, dC.p, m, alpha, accum, 0);
  dC.download(C);
}

// X: rows x k floats ldx apart; Q (rows x ceil(3k/4)) and S (rows x
// ceil(k/32)) tight
void test_quantize_mxfp6_hip(int rows, int k, int fmt, const float* X, int ldx,
                             uint8_t* Q, uint8_t* S) {
  const int kbytes = f6_kbytes(k), kb = (k + MX_BLK - 1) / MX_BLK;
  DevArray<float> dX((size_t)ldx * rows, X);
  DevArray<uint8_t> dQ((size_t)rows * kbytes), dS((size_t)rows * kb);
  launch_quant_mxfp6(rows, k, fmt, dX.p, ldx, dQ.p, kbytes, dS.p, kb, 0);
  dQ.download(Q);
  dS.download(S);
}

}  // namespace pa
