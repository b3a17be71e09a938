// MXFP8 tile-GEMM (OCP MX: E4M3 / E5M2 elements, one E8M0 power-of-two scale
// per 32 consecutive K elements) and the fp32 -> MXFP8 quantiser.
//
//   C[i,j] = alpha * sum_b 2^(SA[i,b] + SB[j,b] - 254) * sum_{p in b} A[i,p] B[j,p]
//            (+ C[i,j] when accum)
//
// Operands as in kernels_fp8.cpp: A m rows of k bytes lda apart, B n rows of
// k bytes ldb apart, K contiguous, C fp32 column-major. SA is m rows of
// ceil(k/32) scale bytes ldsa apart, SB n rows likewise: K-major like the
// operand it belongs to. Byte e means 2^(e-127), byte 255 is NaN.
//
// The step image, swizzle and MFMA are those of kernels_fp8.cpp
// (kernels_fp8.hpp). The instruction takes lane l's scale register (byte 0,
// op_sel 0) for row (l & 15) and K block (l >> 4) of the step, but a lane's
// eight VGPRs do not hold that block: they hold K bytes [16 g, +16) and
// [64 + 16 g, +16), g = l >> 4 (measured, see f8_frag_mx). The fragment is
// therefore read in that order, chunks g and 4 + g of the row, and beside it
// the lane reads one scale byte: that of (row l & 15, block l >> 4).
//
// Scale image of a K step: one dword per row (its 4 blocks of 32), [A|B][256]
// dwords = 2 KB per ring slot, after the 128 KB operand ring. The byte of
// (row, block g) is at row * 4 + g, one ds_read_u8, zero-extended, which is
// the scale register as the instruction wants it. The 16 rows of a fragment
// are 16 consecutive dwords and the 4 lanes of a row share a dword: 16 banks,
// no conflict under the model kernels_fp8.cpp states.
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
#define MX_SIMG (4 * (F8_BM + F8_BN))   // a slot's scale image, bytes

__device__ __forceinline__ int mx_scale(const char* simg, int row, int g16) {
  return *(const uint8_t*)(simg + row * 4 + g16);
}

// ------------------------------------------------------------ fast kernel
// k_gemm_fp8's block, wave grid, two-slot ring, swizzle and step schedule
// (see there), with the scales staged beside the operands: per step and
// wave one 4-byte global->LDS copy moves the scale dwords of 64 rows, waves
// 0..3 those of A, waves 4..7 those of B, so a stage is 9 copies per wave
// and the counted wait is vmcnt(9). Each scale byte is read next to its
// fragment, 12 per step and wave, and the second A group's scales go into
// the registers of the first, as its fragments do.
template <int FA, int FB>
__launch_bounds__(512)
__global__ void k_gemm_mxfp8(int m, int n, int k,
                             const uint8_t* __restrict__ A, int lda,
                             const uint8_t* __restrict__ SA, int ldsa,
                             const uint8_t* __restrict__ B, int ldb,
                             const uint8_t* __restrict__ SB, int ldsb,
                             float* __restrict__ C, int ldc, int nbx,
                             float alpha, int accum) {
  extern __shared__ __attribute__((aligned(16))) char mx_ring[];
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
  // scale staging: lane l of wave w copies the step's dword of row
  // 64 (w & 3) + l of A (w < 4) or B, lane-linear into the scale image
  const int srow0 = (wave & 3) * 64;
  const uint8_t* baseS = wave < 4 ? SA + (size_t)(bm0 + srow0) * ldsa
                                  : SB + (size_t)(bn0 + srow0) * ldsb;
  const unsigned offS = (unsigned)lane * (wave < 4 ? ldsa : ldsb);
  char* const simg = mx_ring + 2 * SLOT;
  auto stage = [&](int t) {
    char* slot = mx_ring + (t & 1) * SLOT + wave * 32 * F8_KS;
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
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(
            baseS + (size_t)t * 4 + offS),
        (__attribute__((address_space(3))) unsigned int*)(
            simg + (t & 1) * MX_SIMG + wave * 256),
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
    const char* as = mx_ring + (t & 1) * SLOT;
    const char* bs = as + IMG;
    const char* ssa = simg + (t & 1) * MX_SIMG;
    const char* ssb = ssa + 4 * F8_BM;
    i32x8 b[4], a0[4], a1[4];
    int sb[4], sa0[4], sa1[4];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      b[f] = f8_frag_mx(bs, wc * 64 + f * 16 + r16, g16);
      sb[f] = mx_scale(ssb, wc * 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int f = 0; f < 4; f++) {
      a0[f] = f8_frag_mx(as, wr * 128 + f * 16 + r16, g16);
      sa0[f] = mx_scale(ssa, wr * 128 + f * 16 + r16, g16);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 4; j++)
      acc[0][j] = f8_mfma<FA, FB>(a0[0], b[j], acc[0][j], sa0[0], sb[j]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < 4; f++) {
      a1[f] = f8_frag_mx(as, wr * 128 + 64 + f * 16 + r16, g16);
      sa1[f] = mx_scale(ssa, wr * 128 + 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int i = 1; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f8_mfma<FA, FB>(a0[i], b[j], acc[i][j], sa0[i], sb[j]);
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
            f8_mfma<FA, FB>(a1[i], b[j], acc[4 + i][j], sa1[i], sb[j]);
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int i = 0; i < 16; i++) f8_pin(acc[4 + (i >> 2)][i & 3]);
    __builtin_amdgcn_sched_barrier(0);
  };
  const int T = k / F8_KS;  // >= 2
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
// k_gemm_fp8_edge with a scale image per operand: any m, n, k >= 1, any
// leading dimension and alignment. Thread (op, row) loads its row's 4 scale
// bytes of the step one by one; a row past m / n or a block past k takes
// byte 127 (2^0), so with the zero padding bytes of the operands the padding
// adds exact zeros and never meets a NaN scale.
template <int FA, int FB>
__launch_bounds__(256)
__global__ void k_gemm_mxfp8_edge(int m, int n, int k,
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
  for (int k0 = 0; k0 < k; k0 += F8_KS) {
#pragma unroll
    for (int x = tid; x < F8E_BM * 8; x += 256) {
      const int row = x >> 3, c = x & 7;
      const int off = row * F8_KS + ((c ^ f8_key(row)) << 4);
      const int gm = bm0 + row, gn = bn0 + row;
      *(i32x4*)(As + off) =
          f8_load16(A + (size_t)gm * lda, gm < m, k0 + c * 16, k);
      *(i32x4*)(Bs + off) =
          f8_load16(B + (size_t)gn * ldb, gn < n, k0 + c * 16, k);
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
      a[f] = f8_frag_mx(As, wr * 64 + f * 16 + r16, g16);
      sa[f] = mx_scale(Ss[0], wr * 64 + f * 16 + r16, g16);
      b[f] = f8_frag_mx(Bs, wc * 64 + f * 16 + r16, g16);
      sb[f] = mx_scale(Ss[1], wc * 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f8_mfma<FA, FB>(a[i], b[j], acc[i][j], sa[i], sb[j]);
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
template <int FA, int FB>
static void launch_gemm_mxfp8_fmt(int m, int n, int k, const uint8_t* A,
                                  int lda, const uint8_t* SA, int ldsa,
                                  const uint8_t* B, int ldb, const uint8_t* SB,
                                  int ldsb, float* C, int ldc, float alpha,
                                  int accum, hipStream_t stream) {
  // the fp8 kernel's conditions, and whole aligned scale dwords per step
  const bool fast = m % F8_BM == 0 && n % F8_BN == 0 && k % F8_KS == 0 &&
                    k >= 2 * F8_KS && lda % 16 == 0 && ldb % 16 == 0 &&
                    lda < (1 << 23) && ldb < (1 << 23) &&
                    ((uintptr_t)A | (uintptr_t)B) % 16 == 0 &&
                    ldsa % 4 == 0 && ldsb % 4 == 0 && ldsa < (1 << 23) &&
                    ldsb < (1 << 23) &&
                    ((uintptr_t)SA | (uintptr_t)SB) % 4 == 0;
  if (fast) {
    constexpr size_t lds = 2 * (F8_BM + F8_BN) * F8_KS + 2 * MX_SIMG;  // 132 KB
    static std::atomic<bool> attr[64];  // per device, as in kernels_fp8.cpp
    int dev = 0;
    PA_HIP_CHECK(hipGetDevice(&dev));
    PA_CHECK(dev >= 0 && dev < 64);
    if (!attr[dev].load(std::memory_order_acquire)) {
      PA_HIP_CHECK(hipFuncSetAttribute(
          (const void*)k_gemm_mxfp8<FA, FB>,
          hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      attr[dev].store(true, std::memory_order_release);
    }
    const int nbx = m / F8_BM, nby = n / F8_BN;
    hipLaunchKernelGGL((k_gemm_mxfp8<FA, FB>), dim3(nbx * nby), dim3(512), lds,
                       stream, m, n, k, A, lda, SA, ldsa, B, ldb, SB, ldsb, C,
                       ldc, nbx, alpha, accum);
    return;
  }
  const int nbx = (m + F8E_BM - 1) / F8E_BM, nby = (n + F8E_BN - 1) / F8E_BN;
  hipLaunchKernelGGL((k_gemm_mxfp8_edge<FA, FB>), dim3(nbx * nby), dim3(256),
                     0, stream, m, n, k, A, lda, SA, ldsa, B, ldb, SB, ldsb, C,
                     ldc, nbx, alpha, accum);
}

struct MxOperand {
  const void* p;   // element bytes, rows ld apart
  int ld, fmt;
  const void* s;   // scale bytes, rows lds apart
  int lds;
};

static void launch_gemm_mxfp8(int m, int n, int k, const MxOperand& a,
                              const MxOperand& b, float* C, int ldc,
                              float alpha, int accum, hipStream_t stream) {
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  PA_CHECK((a.fmt | b.fmt | 1) == 1, "fp8 format is 0 (e4m3) or 1 (e5m2)");
  PA_CHECK(m >= 1 && n >= 1 && k >= 1 && a.ld >= k && b.ld >= k && ldc >= m &&
           a.lds >= kb && b.lds >= kb);
  auto go = [&](auto fa, auto fb) {
    launch_gemm_mxfp8_fmt<decltype(fa)::value, decltype(fb)::value>(
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
// [-127, 127] (emax 8 for E4M3, 15 for E5M2), scale byte X + 127, elements
// x * 2^-X clamped to the largest finite value and rounded to nearest even.
// An all-zero block gets byte 127 and +0 elements.
//
// floor(log2 amax) is the float's exponent field e minus 127, so the byte is
// max(e - emax, 0): a subnormal amax (e = 0) clamps to byte 0 like every
// e < emax, and the largest e (254) stays below 255. 2^-X is the float with
// exponent field 254 - byte, between 2^-119 and 2^127, so the product is
// exact unless it is far below the format's smallest subnormal, where it
// rounds to zero either way. The conversion is v_cvt_pk_{fp8,bf8}_f32 (OCP
// formats on gfx950, round to nearest even) on the clamped value.
template <int FMT>
__device__ __forceinline__ int mx_scale_byte(float amax) {
  const int e = (__float_as_uint(amax) >> 23) & 0xff;
  return amax == 0.f ? 127 : max(e - (FMT ? 15 : 8), 0);
}

template <int FMT>
__device__ __forceinline__ float mx_scaled(float x, int byte, bool zero) {
  const float lim = FMT ? 57344.f : 448.f;
  const float y = x * __uint_as_float((unsigned)(254 - byte) << 23);
  return zero ? 0.f : fminf(fmaxf(y, -lim), lim);
}

// two values into the low (hi = false) or high 16 bits of old
template <int FMT, bool HI>
__device__ __forceinline__ int mx_cvt2(float x0, float x1, int old) {
  if constexpr (FMT)
    return __builtin_amdgcn_cvt_pk_bf8_f32(x0, x1, old, HI);
  else
    return __builtin_amdgcn_cvt_pk_fp8_f32(x0, x1, old, HI);
}

// Eight lanes cover a block, a float4 each, so a wave reads 1 KB contiguous
// along K (8 blocks); wave w of the grid takes segment w % nseg of row
// w / nseg. The block's amax is a three-step xor shuffle among its eight
// lanes. Needs k % 32 == 0 and 16- / 4-byte aligned X / Q rows.
template <int FMT>
__launch_bounds__(256)
__global__ void k_quant_mxfp8(int rows, int k, const float* __restrict__ X,
                              int ldx, uint8_t* __restrict__ Q, int ldq,
                              uint8_t* __restrict__ S, int lds, int nseg) {
  const size_t gw = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int row = (int)(gw / nseg), seg = (int)(gw % nseg);
  if (row >= rows) return;  // the whole wave
  const int k0 = seg * 256 + lane * 4;
  const bool on = k0 < k;   // whole blocks: k % 32 == 0
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (on) v = *(const float4*)(X + (size_t)row * ldx + k0);
  float amax = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)),
                     fmaxf(fabsf(v.z), fabsf(v.w)));
#pragma unroll
  for (int d = 1; d < 8; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
  const int byte = mx_scale_byte<FMT>(amax);
  const bool zero = amax == 0.f;
  int w = mx_cvt2<FMT, false>(mx_scaled<FMT>(v.x, byte, zero),
                              mx_scaled<FMT>(v.y, byte, zero), 0);
  w = mx_cvt2<FMT, true>(mx_scaled<FMT>(v.z, byte, zero),
                         mx_scaled<FMT>(v.w, byte, zero), w);
  if (on) {
    *(int*)(Q + (size_t)row * ldq + k0) = w;
    if ((lane & 7) == 0) S[(size_t)row * lds + k0 / MX_BLK] = (uint8_t)byte;
  }
}

// Any k, leading dimension and alignment: one thread per block, bytewise.
template <int FMT>
__launch_bounds__(256)
__global__ void k_quant_mxfp8_any(int rows, int k, const float* __restrict__ X,
                                  int ldx, uint8_t* __restrict__ Q, int ldq,
                                  uint8_t* __restrict__ S, int lds) {
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * kb) return;
  const int row = (int)(idx / kb), blk = (int)(idx % kb);
  const int k0 = blk * MX_BLK, len = min(MX_BLK, k - k0);
  const float* x = X + (size_t)row * ldx + k0;
  uint8_t* q = Q + (size_t)row * ldq + k0;
  float amax = 0.f;
  for (int e = 0; e < len; e++) amax = fmaxf(amax, fabsf(x[e]));
  const int byte = mx_scale_byte<FMT>(amax);
  const bool zero = amax == 0.f;
  for (int e = 0; e < len; e++) {
    const float y = mx_scaled<FMT>(x[e], byte, zero);
    q[e] = (uint8_t)mx_cvt2<FMT, false>(y, y, 0);
  }
  S[(size_t)row * lds + blk] = (uint8_t)byte;
}

static void launch_quant_mxfp8(int rows, int k, int fmt, const float* X,
                               int ldx, uint8_t* Q, int ldq, uint8_t* S,
                               int lds, hipStream_t stream) {
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  PA_CHECK((fmt | 1) == 1, "fp8 format is 0 (e4m3) or 1 (e5m2)");
  PA_CHECK(rows >= 1 && k >= 1 && ldx >= k && ldq >= k && lds >= kb);
  const bool fast = k % MX_BLK == 0 && ldx % 4 == 0 && ldq % 4 == 0 &&
                    (uintptr_t)X % 16 == 0 && (uintptr_t)Q % 4 == 0;
  if (fast) {
    const int nseg = (k + 255) / 256;
    const size_t waves = (size_t)rows * nseg;
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (fmt)
      hipLaunchKernelGGL(k_quant_mxfp8<1>, grid, dim3(256), 0, stream, rows, k,
                         X, ldx, Q, ldq, S, lds, nseg);
    else
      hipLaunchKernelGGL(k_quant_mxfp8<0>, grid, dim3(256), 0, stream, rows, k,
                         X, ldx, Q, ldq, S, lds, nseg);
    return;
  }
  const dim3 grid((unsigned)(((size_t)rows * kb + 255) / 256));
  if (fmt)
    hipLaunchKernelGGL(k_quant_mxfp8_any<1>, grid, dim3(256), 0, stream, rows,
                       k, X, ldx, Q, ldq, S, lds);
  else
    hipLaunchKernelGGL(k_quant_mxfp8_any<0>, grid, dim3(256), 0, stream, rows,
                       k, X, ldx, Q, ldq, S, lds);
}

// ------------------------------------------------------------------ chores
// The CPU chores are the formulas of the head comment in double.

// y, already clamped to the format's finite range, rounded to nearest even.
static uint8_t fp8_encode(double y, int fmt) {
  const int M = fmt ? 2 : 3, bias = fmt ? 15 : 7;
  const uint8_t sign = std::signbit(y) ? 0x80 : 0;
  const double a = std::fabs(y);
  if (a == 0) return sign;
  int e = std::ilogb(a);
  if (e < 1 - bias) e = 1 - bias;  // subnormal: the quantum stays 2^(1-bias-M)
  // a in units of 2^(e - M): [2^M, 2^(M+1)] when normal, where the leading
  // one adds 1 to the exponent field and a round-up to 2^(M+1) carries on
  const int q = (int)std::nearbyint(std::ldexp(a, M - e));
  return sign | (uint8_t)(q + ((e + bias - 1) << M));
}

static void cpu_quant_mxfp8(Task& t) {
  const QuantMxfp8Args& a = t.arg<QuantMxfp8Args>();
  const float* X = (const float*)t.flows[0].data->pull_to_host();
  Data *qd = t.flows[1].data, *sd = t.flows[2].data;
  uint8_t* Q = (uint8_t*)qd->ensure_host();
  uint8_t* S = (uint8_t*)sd->ensure_host();
  const int emax = a.fmt ? 15 : 8;
  const double lim = a.fmt ? 57344.0 : 448.0;
  for (int r = 0; r < a.rows; r++)
    for (int k0 = 0; k0 < a.k; k0 += MX_BLK) {
      const int len = std::min(MX_BLK, a.k - k0);
      const float* x = X + (size_t)r * a.ldx + k0;
      uint8_t* q = Q + (size_t)r * a.ldq + k0;
      double amax = 0;
      for (int e = 0; e < len; e++) amax = std::max(amax, std::fabs((double)x[e]));
      int ex = 0;
      if (amax > 0) ex = std::min(127, std::max(-127, std::ilogb(amax) - emax));
      S[(size_t)r * a.lds + k0 / MX_BLK] = (uint8_t)(ex + 127);
      for (int e = 0; e < len; e++) {
        const double y = std::ldexp((double)x[e], -ex);
        q[e] = amax > 0 ? fp8_encode(std::min(lim, std::max(-lim, y)), a.fmt)
                        : 0;
      }
    }
  qd->written_on(false);
  sd->written_on(false);
}

static void gpu_quant_mxfp8(Task& t, GpuTaskCtx& g) {
  const QuantMxfp8Args& a = t.arg<QuantMxfp8Args>();
  launch_quant_mxfp8(a.rows, a.k, a.fmt, (const float*)t.dev_ptr[0], a.ldx,
                     (uint8_t*)t.dev_ptr[1], a.ldq, (uint8_t*)t.dev_ptr[2],
                     a.lds, g.stream);
}

static void cpu_gemm_mxfp8(Task& t) {
  static const Fp8Tables tab;
  const GemmMxfp8Args& a = t.arg<GemmMxfp8Args>();
  const uint8_t* A = (const uint8_t*)t.flows[0].data->pull_to_host();
  const uint8_t* SA = (const uint8_t*)t.flows[1].data->pull_to_host();
  const uint8_t* B = (const uint8_t*)t.flows[2].data->pull_to_host();
  const uint8_t* SB = (const uint8_t*)t.flows[3].data->pull_to_host();
  Data* cd = t.flows[4].data;
  float* C = a.accum ? (float*)cd->pull_to_host() : (float*)cd->ensure_host();
  const float* da = tab.v[a.fmt_a];
  const float* db = tab.v[a.fmt_b];
  const int ldc = cd->coll->mb();
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
          d += (double)da[ar[p]] * (double)db[br[p]];
        s += ea == 255 || eb == 255 ? (double)NAN : std::ldexp(d, ea + eb - 254);
      }
      float& c = C[(size_t)j * ldc + i];
      c = (float)(a.accum ? c + a.alpha * s : a.alpha * s);
    }
  cd->written_on(false);
}

static void gpu_gemm_mxfp8(Task& t, GpuTaskCtx& g) {
  const GemmMxfp8Args& a = t.arg<GemmMxfp8Args>();
  launch_gemm_mxfp8(a.m, a.n, a.k,
                    {t.dev_ptr[0], a.lda, a.fmt_a, t.dev_ptr[1], a.ldsa},
                    {t.dev_ptr[2], a.ldb, a.fmt_b, t.dev_ptr[3], a.ldsb},
                    (float*)t.dev_ptr[4], t.flows[4].data->coll->mb(), a.alpha,
                    a.accum, g.stream);
}

TaskClass& tc_gemm_mxfp8() {
  static TaskClass tc = make_tc("gemm_mxfp8", TaskKind::GPU, cpu_gemm_mxfp8,
                                gpu_gemm_mxfp8, TC_GEMM_MXFP8);
  return tc;
}
TaskClass& tc_quant_mxfp8() {
  static TaskClass tc = make_tc("quant_mxfp8", TaskKind::GPU, cpu_quant_mxfp8,
                                gpu_quant_mxfp8, TC_QUANT_MXFP8);
  return tc;
}

// ------------------------------------------------------------ DAG builders
// S holds the scales of the one-byte operand A (K x rows): K/32 rows in
// tiles of A.mb()/32, the column tiling of A, so that tile (k, m) of S
// belongs to tile (k, m) of A.
static void check_scales(TiledMatrix& A, TiledMatrix& S) {
  PA_CHECK(A.elem_size() == 1 && S.elem_size() == 1);
  PA_CHECK(A.mb() % MX_BLK == 0, "the K tile must be a multiple of 32");
  PA_CHECK(S.m() == (A.m() + MX_BLK - 1) / MX_BLK &&
               S.mb() == A.mb() / MX_BLK && S.n() == A.n() &&
               S.nb() == A.nb() && S.mt() == A.mt() && S.nt() == A.nt(),
           "scales are K/32 x rows in tiles of mb/32 x nb");
}

void insert_gemm_mxfp8(Dtd& tp, TiledMatrix& A, TiledMatrix& SA,
                       TiledMatrix& B, TiledMatrix& SB, TiledMatrix& C,
                       const std::string& fmt_a, const std::string& fmt_b,
                       float alpha) {
  PA_CHECK(C.elem_size() == 4);
  check_scales(A, SA);
  check_scales(B, SB);
  PA_CHECK(A.m() == B.m() && A.mb() == B.mb(), "K tilings must match");
  PA_CHECK(A.n() == C.m() && B.n() == C.n() && A.nb() == C.mb() &&
               B.nb() == C.nb(),
           "A is K x M, B is K x N, C is M x N with matching tiles");
  GemmMxfp8Args a;
  a.fmt_a = fp8_format(fmt_a);
  a.fmt_b = fp8_format(fmt_b);
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
        a.k = A.tile_rows(k);
        a.accum = (k != 0);
        Dtd::FlowSpec f[] = {{A.tile(k, m), ACCESS_IN},
                             {SA.tile(k, m), ACCESS_IN},
                             {B.tile(k, n), ACCESS_IN},
                             {SB.tile(k, n), ACCESS_IN},
                             {C.tile(m, n),
                              k == 0 ? ACCESS_OUT : ACCESS_INOUT}};
        tp.insert(&tc_gemm_mxfp8(), &a, sizeof(a), f, 5, -(k),
                  C.rank_of(m, n));
      }
}

// X is fp32, K x rows in column-major tiles (a tile's column is an operand
// row), Q its bytes in the same tiling, S the scales as check_scales wants.
void insert_quantize_mxfp8(Dtd& tp, TiledMatrix& X, TiledMatrix& Q,
                           TiledMatrix& S, const std::string& fmt) {
  PA_CHECK(X.elem_size() == 4);
  PA_CHECK(X.m() == Q.m() && X.n() == Q.n() && X.mb() == Q.mb() &&
               X.nb() == Q.nb(),
           "X and Q are K x rows with the same tiles");
  check_scales(Q, S);
  QuantMxfp8Args a;
  a.fmt = fp8_format(fmt);
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
      tp.insert(&tc_quant_mxfp8(), &a, sizeof(a), f, 3, 0, Q.rank_of(k, r));
    }
}

// ------------------------------------------------- bench and test entries
// Synthetic bytes: operand bytes as insert_fill_fp8 makes them, or scale
// bytes hashed into 120..134 (none a NaN).
__global__ void k_fill_mx(uint8_t* p, size_t nbytes, uint32_t seed,
                          int scales) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < nbytes; i += (size_t)gridDim.x * blockDim.x) {
    const uint8_t b = fp8_fill_byte(i, seed);
    p[i] = scales ? 120 + b % 15 : b;
  }
}

// Synthetic fp32 input of the quantiser: hashed integers in [-95, 96].
__host__ __device__ static inline float mx_fill_f32(size_t i, uint32_t seed) {
  return (float)fp8_fill_byte(i, seed) - 95.f;
}

__global__ void k_fill_f32(float* p, size_t n, uint32_t seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = mx_fill_f32(i, seed);
}

static void cpu_fill_f32(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  Data* d = t.flows[0].data;
  float* p = (float*)d->ensure_host();
  for (size_t i = 0; i < d->bytes / 4; i++) p[i] = mx_fill_f32(i, a.seed);
  d->written_on(false);
}

static void gpu_fill_f32(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  hipLaunchKernelGGL(k_fill_f32, dim3(2048), dim3(256), 0, g.stream,
                     (float*)t.dev_ptr[0], t.flows[0].data->bytes / 4, a.seed);
}

TaskClass& tc_fill_f32() {
  static TaskClass tc = make_tc("fill_f32", TaskKind::GPU, cpu_fill_f32,
                                gpu_fill_f32, TC_FILL_F32);
  return tc;
}

void insert_fill_f32(Dtd& tp, TiledMatrix& A, uint32_t seed) {
  PA_CHECK(A.elem_size() == 4);
  for (int tm = 0; tm < A.mt(); tm++)
    for (int tn = 0; tn < A.nt(); tn++) {
      TileArgs a;
      a.seed = seed ^ (uint32_t)(tm * 9973 + tn);
      Dtd::FlowSpec f[] = {{A.tile(tm, tn), ACCESS_OUT}};
      tp.insert(&tc_fill_f32(), &a, sizeof(a), f, 1, 0, A.rank_of(tm, tn));
    }
}

// kernel-level microbench (TFLOP/s)
double bench_gemm_mxfp8(int m, int n, int k, int iters, int fmt_a, int fmt_b) {
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  DevArray<uint8_t> dA((size_t)m * k), dB((size_t)n * k);
  DevArray<uint8_t> dSA((size_t)m * kb), dSB((size_t)n * kb);
  DevArray<float> dC((size_t)m * n);
  auto fill = [](DevArray<uint8_t>& d, uint32_t seed, int scales) {
    hipLaunchKernelGGL(k_fill_mx, dim3(2048), dim3(256), 0, 0, d.p, d.bytes,
                       seed, scales);
  };
  fill(dA, 1u, 0);
  fill(dB, 2u, 0);
  fill(dSA, 3u, 1);
  fill(dSB, 4u, 1);
  PA_HIP_CHECK(hipMemset(dC.p, 0, dC.bytes));
  double dt = time_launches(iters, [&] {
    launch_gemm_mxfp8(m, n, k, {dA.p, k, fmt_a, dSA.p, kb},
                      {dB.p, k, fmt_b, dSB.p, kb}, dC.p, m, 1.f, 1, 0);
  });
  return 2.0 * m * n * k * iters / dt / 1e12;
}

// quantiser microbench: GB/s over the bytes read and written
double bench_quantize_mxfp8(int rows, int k, int iters, int fmt) {
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  DevArray<float> dX((size_t)rows * k);
  DevArray<uint8_t> dQ((size_t)rows * k), dS((size_t)rows * kb);
  hipLaunchKernelGGL(k_fill_f32, dim3(2048), dim3(256), 0, 0, dX.p,
                     (size_t)rows * k, 5u);
  double dt = time_launches(iters, [&] {
    launch_quant_mxfp8(rows, k, fmt, dX.p, k, dQ.p, k, dS.p, kb, 0);
  });
  return (double)(dX.bytes + dQ.bytes + dS.bytes) * iters / dt / 1e9;
}

// host-I/O numerics harnesses; every leading dimension is given
void test_gemm_mxfp8_hip(int m, int n, int k, const uint8_t* A, int fmt_a,
                         const uint8_t* SA, const uint8_t* B, int fmt_b,
                         const uint8_t* SB, float* C, float alpha, int lda,
                         int ldb, int ldsa, int ldsb, int accum) {
  DevArray<uint8_t> dA((size_t)lda * m, A), dB((size_t)ldb * n, B);
  DevArray<uint8_t> dSA((size_t)ldsa * m, SA), dSB((size_t)ldsb * n, SB);
  DevArray<float> dC((size_t)m * n, C);
  launch_gemm_mxfp8(m, n, k, {dA.p, lda, fmt_a, dSA.p, ldsa},
                    {dB.p, ldb, fmt_b, dSB.p, ldsb}, dC.p, m, alpha, accum, 0);
  dC.download(C);
}

// X: rows x k floats ldx apart; Q (rows x k) and S (rows x ceil(k/32)) tight
void test_quantize_mxfp8_hip(int rows, int k, int fmt, const float* X, int ldx,
                             uint8_t* Q, uint8_t* S) {
  const int kb = (k + MX_BLK - 1) / MX_BLK;
  DevArray<float> dX((size_t)ldx * rows, X);
  DevArray<uint8_t> dQ((size_t)rows * k), dS((size_t)rows * kb);
  launch_quant_mxfp8(rows, k, fmt, dX.p, ldx, dQ.p, k, dS.p, kb, 0);
  dQ.download(Q);
  dS.download(S);
}

}  // namespace pa
