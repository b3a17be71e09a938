// MXFP4 tile-GEMM (OCP MX: E2M1 elements two to a byte, one E8M0
// power-of-two scale per 32 consecutive K elements) and the fp32 -> MXFP4
// quantiser.
//
//   C[i,j] = alpha * sum_b 2^(SA[i,b] + SB[j,b] - 254) * sum_{p in b} A[i,p] B[j,p]
//            (+ C[i,j] when accum)
//
// A is m rows and B n rows of k E2M1 elements, K contiguous: element 2q in
// the low nibble of byte q of the row and element 2q + 1 in the high one, a
// row ceil(k/2) bytes, lda / ldb in bytes. When k is odd the spare high
// nibble of the last byte is ignored. The code is s.ee.m: 0, 0.5, 1, 1.5, 2,
// 3, 4, 6 and their negatives. SA / SB and C as in kernels_mxfp8.cpp.
//
// The step image and its swizzle are those of kernels_fp8.cpp, a row of 128
// bytes, which now is 256 K elements and 8 scale blocks. The instruction
// (cbsz = blgp = 4) takes four VGPRs per operand, so the eight VGPRs of
// f8_frag (chunks 2g and 2g + 1 of the lane's row, g = l >> 4) are the
// operands of two MFMAs: the low four carry elements [64 g, +32), block 2g,
// the high four [64 g + 32, +32), block 2g + 1 (f4_mfma). A step's copies,
// LDS reads and barriers are those of the FP8 kernel and feed twice the
// MFMAs. Measured on MI355X with one-hot operands under distinct scale
// bytes (test_mxfp4_gemm.py::test_routing): for 4-bit operands the layout is
// the one the ISA text gives, unlike the 8-bit one (f8_frag_mx). Lane l's
// four VGPRs are the 32 consecutive K elements [32 g, +32) of row l & 15, low
// nibble first, and op_sel 0 / 1 takes byte 0 / 1 of lane l's scale register
// as the scale of exactly those elements.
//
// Scale image of a K step: 8 bytes per row, [A|B][256] rows = 4 KB per ring
// slot, after the 128 KB operand ring. A lane's two blocks are adjacent, so
// it reads both bytes as one ds_read_u16 at row * 8 + 2g and gives the
// register to both MFMAs of the pair, op_sel 0 and 1: one scale register and
// one LDS read per fragment, as in k_gemm_mxfp8.
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

#define MX_BLK 32                        // K elements per scale
#define F4_STEP (2 * F8_KS)              // K elements per step
#define MX4_SIMG (8 * (F8_BM + F8_BN))   // a slot's scale image, bytes

// ------------------------------------------------------------ fast kernel
// k_gemm_mxfp8's block, wave grid, two-slot ring, swizzle and step schedule
// (see there and k_gemm_fp8). Scales: per step and wave two 4-byte
// global->LDS copies, each 32 rows x 8 bytes lane-linear (lane l: row l >> 1,
// half l & 1), waves 0..3 the 256 rows of A, waves 4..7 those of B, so a
// stage is 10 copies per wave and the counted wait is vmcnt(10). Each
// (A fragment, B fragment) pair takes two MFMAs, 64 per step and wave; the
// two of a pair are issued four apart.
__launch_bounds__(512)
__global__ void k_gemm_mxfp4(int m, int n, int k,
                             const uint8_t* __restrict__ A, int lda,
                             const uint8_t* __restrict__ SA, int ldsa,
                             const uint8_t* __restrict__ B, int ldb,
                             const uint8_t* __restrict__ SB, int ldsb,
                             float* __restrict__ C, int ldc, int nbx,
                             float alpha, int accum) {
  extern __shared__ __attribute__((aligned(16))) char mx4_ring[];
  constexpr int IMG = F8_BM * F8_KS;  // one operand's step image, 32 KB
  constexpr int SLOT = 2 * IMG;       // [A image | B image]
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wr = wave >> 2, wc = wave & 3;
  const int id = bf_swz(blockIdx.x, gridDim.x);
  const int bm0 = (id % nbx) * F8_BM, bn0 = (id / nbx) * F8_BN;
  const int g16 = lane >> 4, r16 = lane & 15;

  // operand staging as in k_gemm_fp8
  const int srow = lane >> 3, schunk = lane & 7;
  unsigned offA[4], offB[4];
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int row = (wave * 4 + p) * 8 + srow;
    const int kc = 16 * (schunk ^ f8_key(row));
    offA[p] = (unsigned)row * lda + kc;
    offB[p] = (unsigned)row * ldb + kc;
  }
  const uint8_t* baseA = A + (size_t)bm0 * lda;
  const uint8_t* baseB = B + (size_t)bn0 * ldb;
  // scale staging: copy p of wave w moves the step's 8 bytes of rows
  // 64 (w & 3) + 32 p + (l >> 1) of A (w < 4) or B, a dword per lane
  const int srow0 = (wave & 3) * 64;
  const int lds_s = wave < 4 ? ldsa : ldsb;
  const uint8_t* baseS = wave < 4 ? SA + (size_t)(bm0 + srow0) * ldsa
                                  : SB + (size_t)(bn0 + srow0) * ldsb;
  const unsigned offS = (unsigned)(lane >> 1) * lds_s + 4 * (lane & 1);
  const unsigned offS1 = offS + 32u * lds_s;
  char* const simg = mx4_ring + 2 * SLOT;
  auto stage = [&](int t) {
    char* slot = mx4_ring + (t & 1) * SLOT + wave * 32 * F8_KS;
    const uint8_t* sa = baseA + (size_t)t * F8_KS;
    const uint8_t* sb = baseB + (size_t)t * F8_KS;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(sa + offA[p]),
          (__attribute__((address_space(3))) unsigned int*)(slot +
                                                            p * 8 * F8_KS),
          16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(sb + offB[p]),
          (__attribute__((address_space(3))) unsigned int*)(slot + IMG +
                                                            p * 8 * F8_KS),
          16, 0, 0);
    }
    char* sdst = simg + (t & 1) * MX4_SIMG + wave * 512;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(
            baseS + (size_t)t * 8 + offS),
        (__attribute__((address_space(3))) unsigned int*)sdst, 4, 0, 0);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(
            baseS + (size_t)t * 8 + offS1),
        (__attribute__((address_space(3))) unsigned int*)(sdst + 256), 4, 0,
        0);
  };

  f32x4 acc[8][4] = {};
  auto step = [&](int t, auto restage, auto last) {
    if constexpr (decltype(last)::value) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const char* as = mx4_ring + (t & 1) * SLOT;
    const char* bs = as + IMG;
    const char* ssa = simg + (t & 1) * MX4_SIMG;
    const char* ssb = ssa + 8 * F8_BM;
    i32x8 b[4], a0[4], a1[4];
    int sb[4], sa0[4], sa1[4];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      b[f] = f8_frag(bs, wc * 64 + f * 16 + r16, g16);
      sb[f] = f4_scale2(ssb, wc * 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int f = 0; f < 4; f++) {
      a0[f] = f8_frag(as, wr * 128 + f * 16 + r16, g16);
      sa0[f] = f4_scale2(ssa, wr * 128 + f * 16 + r16, g16);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 4; j++)
      acc[0][j] = f4_mfma<0>(a0[0], b[j], acc[0][j], sa0[0], sb[j]);
#pragma unroll
    for (int j = 0; j < 4; j++)
      acc[0][j] = f4_mfma<1>(a0[0], b[j], acc[0][j], sa0[0], sb[j]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < 4; f++) {
      a1[f] = f8_frag(as, wr * 128 + 64 + f * 16 + r16, g16);
      sa1[f] = f4_scale2(ssa, wr * 128 + 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int i = 1; i < 4; i++) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f4_mfma<0>(a0[i], b[j], acc[i][j], sa0[i], sb[j]);
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f4_mfma<1>(a0[i], b[j], acc[i][j], sa0[i], sb[j]);
    }
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
    for (int i = 0; i < 4; i++) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[4 + i][j] = f4_mfma<0>(a1[i], b[j], acc[4 + i][j], sa1[i], sb[j]);
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[4 + i][j] = f4_mfma<1>(a1[i], b[j], acc[4 + i][j], sa1[i], sb[j]);
    }
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int i = 0; i < 16; i++) f8_pin(acc[4 + (i >> 2)][i & 3]);
    __builtin_amdgcn_sched_barrier(0);
  };
  const int T = k / F4_STEP;  // >= 2
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
// k_gemm_mxfp8_edge over packed rows: any m, n, k >= 1, any leading
// dimension and alignment, the fast kernel's image, fragment split and
// op_sel scheme. Bytes past ceil(k/2) are zero and for odd k so is the high
// nibble of the last byte; a row past m / n or a block past k takes scale
// byte 127, so the padding adds exact zeros and never meets a NaN scale.
__device__ __forceinline__ i32x4 f4_load16(const uint8_t* row, bool ok, int b0,
                                           int k) {
  const int kbytes = (k + 1) >> 1;
  i32x4 v = f8_load16(row, ok, b0, kbytes);
  const int last = kbytes - 1 - b0;  // the byte with the spare nibble
  if ((k & 1) && last >= 0 && last < 16) {
    const int mask = ~(0xF0 << (8 * (last & 3)));
#pragma unroll
    for (int e = 0; e < 4; e++)
      if ((last >> 2) == e) v[e] &= mask;
  }
  return v;
}

__launch_bounds__(256)
__global__ void k_gemm_mxfp4_edge(int m, int n, int k,
                                  const uint8_t* __restrict__ A, int lda,
                                  const uint8_t* __restrict__ SA, int ldsa,
                                  const uint8_t* __restrict__ B, int ldb,
                                  const uint8_t* __restrict__ SB, int ldsb,
                                  float* __restrict__ C, int ldc, int nbx,
                                  float alpha, int accum) {
  __shared__ __attribute__((aligned(16))) char As[F8E_BM * F8_KS];
  __shared__ __attribute__((aligned(16))) char Bs[F8E_BN * F8_KS];
  __shared__ __attribute__((aligned(16))) char Ss[2][F8E_BM * 8];
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
  for (int k0 = 0; k0 < k; k0 += F4_STEP) {
#pragma unroll
    for (int x = tid; x < F8E_BM * 8; x += 256) {
      const int row = x >> 3, c = x & 7;
      const int off = row * F8_KS + ((c ^ f8_key(row)) << 4);
      const int gm = bm0 + row, gn = bn0 + row;
      *(i32x4*)(As + off) =
          f4_load16(A + (size_t)gm * lda, gm < m, k0 / 2 + c * 16, k);
      *(i32x4*)(Bs + off) =
          f4_load16(B + (size_t)gn * ldb, gn < n, k0 / 2 + c * 16, k);
    }
    unsigned sw[2] = {0, 0};
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int blk = k0 / MX_BLK + e;
      const unsigned byte = sok && blk < kblocks ? sp[blk] : 127u;
      sw[e >> 2] |= byte << (8 * (e & 3));
    }
    *(uint2*)(Ss[sop] + srow * 8) = make_uint2(sw[0], sw[1]);
    __syncthreads();
    i32x8 a[4], b[4];
    int sa[4], sb[4];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      a[f] = f8_frag(As, wr * 64 + f * 16 + r16, g16);
      sa[f] = f4_scale2(Ss[0], wr * 64 + f * 16 + r16, g16);
      b[f] = f8_frag(Bs, wc * 64 + f * 16 + r16, g16);
      sb[f] = f4_scale2(Ss[1], wc * 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f4_mfma<0>(a[i], b[j], acc[i][j], sa[i], sb[j]);
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f4_mfma<1>(a[i], b[j], acc[i][j], sa[i], sb[j]);
    }
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
struct Mx4Operand {
  const void* p;   // packed elements, rows ld bytes apart
  int ld;
  const void* s;   // scale bytes, rows lds apart
  int lds;
};

static void launch_gemm_mxfp4(int m, int n, int k, const Mx4Operand& a,
                              const Mx4Operand& b, float* C, int ldc,
                              float alpha, int accum, hipStream_t stream) {
  const int kbytes = (k + 1) / 2, kb = (k + MX_BLK - 1) / MX_BLK;
  PA_CHECK(m >= 1 && n >= 1 && k >= 1 && a.ld >= kbytes && b.ld >= kbytes &&
           ldc >= m && a.lds >= kb && b.lds >= kb);
  const uint8_t *A = (const uint8_t*)a.p, *SA = (const uint8_t*)a.s;
  const uint8_t *B = (const uint8_t*)b.p, *SB = (const uint8_t*)b.s;
  // whole 128-byte steps of 16-byte chunks, whole aligned scale dwords
  const bool fast = m % F8_BM == 0 && n % F8_BN == 0 && k % F4_STEP == 0 &&
                    k >= 2 * F4_STEP && a.ld % 16 == 0 && b.ld % 16 == 0 &&
                    a.ld < (1 << 23) && b.ld < (1 << 23) &&
                    ((uintptr_t)A | (uintptr_t)B) % 16 == 0 &&
                    a.lds % 4 == 0 && b.lds % 4 == 0 && a.lds < (1 << 23) &&
                    b.lds < (1 << 23) &&
                    ((uintptr_t)SA | (uintptr_t)SB) % 4 == 0;
  if (fast) {
    constexpr size_t lds = 2 * (F8_BM + F8_BN) * F8_KS + 2 * MX4_SIMG;  // 136 KB
    static std::atomic<bool> attr[64];  // per device, as in kernels_fp8.cpp
    int dev = 0;
    PA_HIP_CHECK(hipGetDevice(&dev));
    PA_CHECK(dev >= 0 && dev < 64);
    if (!attr[dev].load(std::memory_order_acquire)) {
      PA_HIP_CHECK(hipFuncSetAttribute(
          (const void*)k_gemm_mxfp4,
          hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      attr[dev].store(true, std::memory_order_release);
    }
    const int nbx = m / F8_BM, nby = n / F8_BN;
    hipLaunchKernelGGL(k_gemm_mxfp4, dim3(nbx * nby), dim3(512), lds, stream,
                       m, n, k, A, a.ld, SA, a.lds, B, b.ld, SB, b.lds, C, ldc,
                       nbx, alpha, accum);
    return;
  }
  const int nbx = (m + F8E_BM - 1) / F8E_BM, nby = (n + F8E_BN - 1) / F8E_BN;
  hipLaunchKernelGGL(k_gemm_mxfp4_edge, dim3(nbx * nby), dim3(256), 0, stream,
                     m, n, k, A, a.ld, SA, a.lds, B, b.ld, SB, b.lds, C, ldc,
                     nbx, alpha, accum);
}

// --------------------------------------------------------------- quantiser
// Per block of 32: amax = max|x|, X = floor(log2 amax) - 2 clamped to
// [-127, 127], scale byte X + 127, elements x * 2^-X clamped to +-6 and
// rounded to nearest even onto E2M1. An all-zero block gets byte 127 and
// zero elements. With e the exponent field of amax the byte is max(e - 2, 0)
// and 2^-X the float with exponent field 254 - byte, as in kernels_mxfp8.cpp.
// The conversion is v_cvt_scalef32_pk_fp4_f32 under scale 1.0 on the clamped
// value: only its in-range rounding is relied on.
__device__ __forceinline__ int f4_scale_byte(float amax) {
  const int e = (__float_as_uint(amax) >> 23) & 0xff;
  return amax == 0.f ? 127 : max(e - 2, 0);
}

__device__ __forceinline__ float f4_scaled(float x, int byte, bool zero) {
  const float y = x * __uint_as_float((unsigned)(254 - byte) << 23);
  return zero ? 0.f : fminf(fmaxf(y, -6.f), 6.f);
}

// x0 into the low and x1 into the high nibble of byte SEL of old
template <int SEL>
__device__ __forceinline__ unsigned f4_cvt2(unsigned old, float x0, float x1) {
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, x0, x1, 1.0f, SEL);
}

// Four lanes cover a block, eight floats each (two float4 loads, one dword
// of eight nibbles stored), so a wave reads 2 KB contiguous along K (16
// blocks); wave w of the grid takes segment w % nseg of row w / nseg. The
// block's amax is a two-step xor shuffle among its four lanes. Needs
// k % 32 == 0 and 16- / 4-byte aligned X / Q rows.
__launch_bounds__(256)
__global__ void k_quant_mxfp4(int rows, int k, const float* __restrict__ X,
                              int ldx, uint8_t* __restrict__ Q, int ldq,
                              uint8_t* __restrict__ S, int lds, int nseg) {
  const size_t gw = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int row = (int)(gw / nseg), seg = (int)(gw % nseg);
  if (row >= rows) return;  // the whole wave
  const int k0 = seg * 512 + lane * 8;
  const bool on = k0 < k;   // whole blocks: k % 32 == 0
  float4 u = {0.f, 0.f, 0.f, 0.f}, v = u;
  if (on) {
    const float4* x = (const float4*)(X + (size_t)row * ldx + k0);
    u = x[0];
    v = x[1];
  }
  float amax = fmaxf(fmaxf(fmaxf(fabsf(u.x), fabsf(u.y)),
                           fmaxf(fabsf(u.z), fabsf(u.w))),
                     fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)),
                           fmaxf(fabsf(v.z), fabsf(v.w))));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  amax = fmaxf(amax, __shfl_xor(amax, 2));
  const int byte = f4_scale_byte(amax);
  const bool zero = amax == 0.f;
  auto sc = [&](float x) { return f4_scaled(x, byte, zero); };
  unsigned w = f4_cvt2<0>(0u, sc(u.x), sc(u.y));
  w = f4_cvt2<1>(w, sc(u.z), sc(u.w));
  w = f4_cvt2<2>(w, sc(v.x), sc(v.y));
  w = f4_cvt2<3>(w, sc(v.z), sc(v.w));
  if (on) {
    *(unsigned*)(Q + (size_t)row * ldq + k0 / 2) = w;
    if ((lane & 3) == 0) S[(size_t)row * lds + k0 / MX_BLK] = (uint8_t)byte;
  }
}

// Any k, leading dimension and alignment: one thread per block, bytewise;
// the spare nibble of an odd k is written as 0.
__launch_bounds__(256)
__global__ void k_quant_mxfp4_any(int rows, int k, const float* __restrict__ X,
                                  int ldx, uint8_t* __restrict__ Q, int ldq,
                                  uint8_t* __restrict__ S, int lds) {
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * kb) return;
  const int row = (int)(idx / kb), blk = (int)(idx % kb);
  const int k0 = blk * MX_BLK, len = min(MX_BLK, k - k0);
  const float* x = X + (size_t)row * ldx + k0;
  uint8_t* q = Q + (size_t)row * ldq + k0 / 2;
  float amax = 0.f;
  for (int e = 0; e < len; e++) amax = fmaxf(amax, fabsf(x[e]));
  const int byte = f4_scale_byte(amax);
  const bool zero = amax == 0.f;
  for (int e = 0; e < len; e += 2) {
    const float y0 = f4_scaled(x[e], byte, zero);
    const float y1 = e + 1 < len ? f4_scaled(x[e + 1], byte, zero) : 0.f;
    q[e >> 1] = (uint8_t)f4_cvt2<0>(0u, y0, y1);
  }
  S[(size_t)row * lds + blk] = (uint8_t)byte;
}

static void launch_quant_mxfp4(int rows, int k, const float* X, int ldx,
                               uint8_t* Q, int ldq, uint8_t* S, int lds,
                               hipStream_t stream) {
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  PA_CHECK(rows >= 1 && k >= 1 && ldx >= k && ldq >= (k + 1) / 2 && lds >= kb);
  const bool fast = k % MX_BLK == 0 && ldx % 4 == 0 && ldq % 4 == 0 &&
                    (uintptr_t)X % 16 == 0 && (uintptr_t)Q % 4 == 0;
  if (fast) {
    const int nseg = (k + 511) / 512;
    const size_t waves = (size_t)rows * nseg;
    hipLaunchKernelGGL(k_quant_mxfp4, dim3((unsigned)((waves + 3) / 4)),
                       dim3(256), 0, stream, rows, k, X, ldx, Q, ldq, S, lds,
                       nseg);
    return;
  }
  const dim3 grid((unsigned)(((size_t)rows * kb + 255) / 256));
  hipLaunchKernelGGL(k_quant_mxfp4_any, grid, dim3(256), 0, stream, rows, k, X,
                     ldx, Q, ldq, S, lds);
}

// ------------------------------------------------------------------ chores
// The CPU chores are the formulas of the head comment in double.

// |y| <= 6 onto the nearest E2M1 code, a tie to the even code.
static uint8_t fp4_encode(double y) {
  const double a = std::fabs(y);
  int best = 0;
  for (int c = 1; c < 8; c++) {
    const double d = std::fabs(a - fp4_value[c]);
    const double db = std::fabs(a - fp4_value[best]);
    if (d < db || (d == db && !(c & 1))) best = c;
  }
  return (uint8_t)((std::signbit(y) ? 8 : 0) | best);
}

static void cpu_quant_mxfp4(Task& t) {
  const QuantMxfp4Args& a = t.arg<QuantMxfp4Args>();
  const float* X = (const float*)t.flows[0].data->pull_to_host();
  Data *qd = t.flows[1].data, *sd = t.flows[2].data;
  uint8_t* Q = (uint8_t*)qd->ensure_host();
  uint8_t* S = (uint8_t*)sd->ensure_host();
  for (int r = 0; r < a.rows; r++)
    for (int k0 = 0; k0 < a.k; k0 += MX_BLK) {
      const int len = std::min(MX_BLK, a.k - k0);
      const float* x = X + (size_t)r * a.ldx + k0;
      uint8_t* q = Q + (size_t)r * a.ldq + k0 / 2;
      double amax = 0;
      for (int e = 0; e < len; e++) amax = std::max(amax, std::fabs((double)x[e]));
      int ex = 0;
      if (amax > 0) ex = std::min(127, std::max(-127, std::ilogb(amax) - 2));
      S[(size_t)r * a.lds + k0 / MX_BLK] = (uint8_t)(ex + 127);
      for (int e = 0; e < len; e++) {
        const double y = std::ldexp((double)x[e], -ex);
        const uint8_t c =
            amax > 0 ? fp4_encode(std::min(6.0, std::max(-6.0, y))) : 0;
        q[e >> 1] = e & 1 ? (uint8_t)(q[e >> 1] | (c << 4)) : c;
      }
    }
  qd->written_on(false);
  sd->written_on(false);
}

static void gpu_quant_mxfp4(Task& t, GpuTaskCtx& g) {
  const QuantMxfp4Args& a = t.arg<QuantMxfp4Args>();
  launch_quant_mxfp4(a.rows, a.k, (const float*)t.dev_ptr[0], a.ldx,
                     (uint8_t*)t.dev_ptr[1], a.ldq, (uint8_t*)t.dev_ptr[2],
                     a.lds, g.stream);
}

static void cpu_gemm_mxfp4(Task& t) {
  const GemmMxfp4Args& a = t.arg<GemmMxfp4Args>();
  const uint8_t* A = (const uint8_t*)t.flows[0].data->pull_to_host();
  const uint8_t* SA = (const uint8_t*)t.flows[1].data->pull_to_host();
  const uint8_t* B = (const uint8_t*)t.flows[2].data->pull_to_host();
  const uint8_t* SB = (const uint8_t*)t.flows[3].data->pull_to_host();
  Data* cd = t.flows[4].data;
  float* C = a.accum ? (float*)cd->pull_to_host() : (float*)cd->ensure_host();
  const int ldc = cd->coll->mb();
  auto el = [](const uint8_t* row, int p) {
    return (double)fp4_value[(row[p >> 1] >> (4 * (p & 1))) & 15];
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
          d += el(ar, p) * el(br, p);
        s += ea == 255 || eb == 255 ? (double)NAN : std::ldexp(d, ea + eb - 254);
      }
      float& c = C[(size_t)j * ldc + i];
      c = (float)(a.accum ? c + a.alpha * s : a.alpha * s);
    }
  cd->written_on(false);
}

static void gpu_gemm_mxfp4(Task& t, GpuTaskCtx& g) {
  const GemmMxfp4Args& a = t.arg<GemmMxfp4Args>();
  launch_gemm_mxfp4(a.m, a.n, a.k, {t.dev_ptr[0], a.lda, t.dev_ptr[1], a.ldsa},
                    {t.dev_ptr[2], a.ldb, t.dev_ptr[3], a.ldsb},
                    (float*)t.dev_ptr[4], t.flows[4].data->coll->mb(), a.alpha,
                    a.accum, g.stream);
}

TaskClass& tc_gemm_mxfp4() {
  static TaskClass tc = make_tc("gemm_mxfp4", TaskKind::GPU, cpu_gemm_mxfp4,
                                gpu_gemm_mxfp4, TC_GEMM_MXFP4);
  return tc;
}
TaskClass& tc_quant_mxfp4() {
  static TaskClass tc = make_tc("quant_mxfp4", TaskKind::GPU, cpu_quant_mxfp4,
                                gpu_quant_mxfp4, TC_QUANT_MXFP4);
  return tc;
}

// ------------------------------------------------------------ DAG builders
// S holds the scales of the packed operand A (K/2 bytes x rows): K/32 rows,
// one per 16 bytes, in tiles of A.mb()/16 rows and the column tiling of A, so
// that tile (k, m) of S belongs to tile (k, m) of A.
static void check_scales4(TiledMatrix& A, TiledMatrix& S) {
  constexpr int BB = MX_BLK / 2;  // bytes per scale block
  PA_CHECK(A.elem_size() == 1 && S.elem_size() == 1);
  PA_CHECK(A.mb() % BB == 0, "the K tile must be a multiple of 16 bytes");
  PA_CHECK(S.m() == (A.m() + BB - 1) / BB && S.mb() == A.mb() / BB &&
               S.n() == A.n() && S.nb() == A.nb() && S.mt() == A.mt() &&
               S.nt() == A.nt(),
           "scales are K/32 x rows in tiles of mb/16 x nb");
}

void insert_gemm_mxfp4(Dtd& tp, TiledMatrix& A, TiledMatrix& SA,
                       TiledMatrix& B, TiledMatrix& SB, TiledMatrix& C,
                       float alpha) {
  PA_CHECK(C.elem_size() == 4);
  check_scales4(A, SA);
  check_scales4(B, SB);
  PA_CHECK(A.m() == B.m() && A.mb() == B.mb(), "K tilings must match");
  PA_CHECK(A.n() == C.m() && B.n() == C.n() && A.nb() == C.mb() &&
               B.nb() == C.nb(),
           "A is K/2 x M, B is K/2 x N, C is M x N with matching tiles");
  GemmMxfp4Args a;
  a.alpha = alpha;
  a.lda = A.mb();
  a.ldb = B.mb();
  a.ldsa = SA.mb();
  a.ldsb = SB.mb();
  for (int m = 0; m < C.mt(); m++)
    for (int n = 0; n < C.nt(); n++)
      for (int k = 0; k < A.mt(); k++) {
        a.m = A.tile_cols(m);
        a.n = B.tile_cols(n);
        a.k = 2 * A.tile_rows(k);
        a.accum = (k != 0);
        Dtd::FlowSpec f[] = {{A.tile(k, m), ACCESS_IN},
                             {SA.tile(k, m), ACCESS_IN},
                             {B.tile(k, n), ACCESS_IN},
                             {SB.tile(k, n), ACCESS_IN},
                             {C.tile(m, n),
                              k == 0 ? ACCESS_OUT : ACCESS_INOUT}};
        tp.insert(&tc_gemm_mxfp4(), &a, sizeof(a), f, 5, -(k),
                  C.rank_of(m, n));
      }
}

// X is fp32, K x rows in column-major tiles (a tile's column is an operand
// row), Q its packed elements, K/2 x rows with half the K tile, S the scales
// as check_scales4 wants.
void insert_quantize_mxfp4(Dtd& tp, TiledMatrix& X, TiledMatrix& Q,
                           TiledMatrix& S) {
  PA_CHECK(X.elem_size() == 4);
  PA_CHECK(X.m() == 2 * Q.m() && X.n() == Q.n() && X.mb() == 2 * Q.mb() &&
               X.nb() == Q.nb(),
           "X is K x rows and Q K/2 x rows with half the K tile");
  check_scales4(Q, S);
  QuantMxfp4Args a;
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
      tp.insert(&tc_quant_mxfp4(), &a, sizeof(a), f, 3, 0, Q.rank_of(k, r));
    }
}

// ------------------------------------------------- bench and test entries
// Synthetic bytes: two hashed E2M1 codes (every byte is a valid pair), or
// scale bytes hashed into 120..134 (none a NaN).
__global__ void k_fill_mx4(uint8_t* p, size_t nbytes, uint32_t seed,
                           int scales) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < nbytes; i += (size_t)gridDim.x * blockDim.x) {
    const uint8_t b = fp8_fill_byte(i, seed);
    p[i] = scales ? 120 + b % 15 : b;
  }
}

// Synthetic fp32 input of the quantiser: hashed integers in [-95, 96].
__global__ void k_fill_mx4_f32(float* p, size_t n, uint32_t seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = (float)fp8_fill_byte(i, seed) - 95.f;
}

// kernel-level microbench (TFLOP/s)
double bench_gemm_mxfp4(int m, int n, int k, int iters) {
  const int kbytes = (k + 1) / 2, kb = (k + MX_BLK - 1) / MX_BLK;
  DevArray<uint8_t> dA((size_t)m * kbytes), dB((size_t)n * kbytes);
  DevArray<uint8_t> dSA((size_t)m * kb), dSB((size_t)n * kb);
  DevArray<float> dC((size_t)m * n);
  auto fill = [](DevArray<uint8_t>& d, uint32_t seed, int scales) {
    hipLaunchKernelGGL(k_fill_mx4, dim3(2048), dim3(256), 0, 0, d.p, d.bytes,
                       seed, scales);
  };
  fill(dA, 1u, 0);
  fill(dB, 2u, 0);
  fill(dSA, 3u, 1);
  fill(dSB, 4u, 1);
  PA_HIP_CHECK(hipMemset(dC.p, 0, dC.bytes));
  double dt = time_launches(iters, [&] {
    launch_gemm_mxfp4(m, n, k, {dA.p, kbytes, dSA.p, kb},
                      {dB.p, kbytes, dSB.p, kb}, dC.p, m, 1.f, 1, 0);
  });
  return 2.0 * m * n * k * iters / dt / 1e12;
}

// quantiser microbench: GB/s over the bytes read and written
double bench_quantize_mxfp4(int rows, int k, int iters) {
  const int kbytes = (k + 1) / 2, kb = (k + MX_BLK - 1) / MX_BLK;
  DevArray<float> dX((size_t)rows * k);
  DevArray<uint8_t> dQ((size_t)rows * kbytes), dS((size_t)rows * kb);
  hipLaunchKernelGGL(k_fill_mx4_f32, dim3(2048), dim3(256), 0, 0, dX.p,
                     (size_t)rows * k, 5u);
  double dt = time_launches(iters, [&] {
    launch_quant_mxfp4(rows, k, dX.p, k, dQ.p, kbytes, dS.p, kb, 0);
  });
  return (double)(dX.bytes + dQ.bytes + dS.bytes) * iters / dt / 1e9;
}

// host-I/O numerics harnesses; every leading dimension is given
void test_gemm_mxfp4_hip(int m, int n, int k, const uint8_t* A,
                         const uint8_t* SA, const uint8_t* B,
                         const uint8_t* SB, float* C, float alpha, int lda,
                         int ldb, int ldsa, int ldsb, int accum) {
  DevArray<uint8_t> dA((size_t)lda * m, A), dB((size_t)ldb * n, B);
  DevArray<uint8_t> dSA((size_t)ldsa * m, SA), dSB((size_t)ldsb * n, SB);
  DevArray<float> dC((size_t)m * n, C);
  launch_gemm_mxfp4(m, n, k, {dA.p, lda, dSA.p, ldsa}, {dB.p, ldb, dSB.p, ldsb},
                    dC.p, m, alpha, accum, 0);
  dC.download(C);
}

// X: rows x k floats ldx apart; Q (rows x ceil(k/2)) and S (rows x
// ceil(k/32)) tight
void test_quantize_mxfp4_hip(int rows, int k, const float* X, int ldx,
                             uint8_t* Q, uint8_t* S) {
  const int kbytes = (k + 1) / 2, kb = (k + MX_BLK - 1) / MX_BLK;
  DevArray<float> dX((size_t)ldx * rows, X);
  DevArray<uint8_t> dQ((size_t)rows * kbytes), dS((size_t)rows * kb);
  launch_quant_mxfp4(rows, k, dX.p, ldx, dQ.p, kbytes, dS.p, kb, 0);
  dQ.download(Q);
  dS.download(S);
}

}  // namespace pa
