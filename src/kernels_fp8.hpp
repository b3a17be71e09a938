// What the fp8 kernel files share (kernels_fp8.cpp: unit block scales;
// kernels_mxfp8.cpp: MX block scales and the quantiser; kernels_mxfp4.cpp:
// the same over packed E2M1 elements): the step image and
// its swizzle, the fragment read, the scaled MFMA, the guarded 16-byte load,
// the synthetic byte and the value tables of the CPU chores. The layout is
// described at the head of kernels_fp8.cpp.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels_bf16.hpp"  // f32x4, bf_swz

namespace pa {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

#define F8_KS 128            // K bytes per step = LDS row stride
#define F8_UNIT 0x7f7f7f7f   // E8M0 2^0 in every scale byte
#define F8_BM 256            // fast kernel block
#define F8_BN 256
#define F8E_BM 128           // edge kernel block
#define F8E_BN 128

__device__ __forceinline__ int f8_key(int row) { return (row >> 1) & 7; }

// The fragment of `row` for lane group g16 out of a swizzled step image.
__device__ __forceinline__ i32x8 f8_frag(const char* img, int row, int g16) {
  const char* p = img + row * F8_KS;
  const int key = f8_key(row);
  i32x4 lo = *(const i32x4*)(p + (((2 * g16) ^ key) << 4));
  i32x4 hi = *(const i32x4*)(p + (((2 * g16 + 1) ^ key) << 4));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The fragment in the instruction's own K order, which the block scales go
// by. Measured on MI355X with one-hot operands under distinct scale bytes:
// lane l's first four VGPRs are K bytes [16 g, +16) of the step and its last
// four [64 + 16 g, +16), g = l >> 4, and the scale of lane l serves K block
// g (bytes [32 g, +32)) of row l & 15. f8_frag's 32 contiguous bytes are a
// permutation of that, the same in A and B, which a product under unit
// scales cannot tell apart. Chunks g and 4 + g are conflict-free by the
// argument at the head of kernels_fp8.cpp, which holds for any one chunk.
__device__ __forceinline__ i32x8 f8_frag_mx(const char* img, int row,
                                            int g16) {
  const char* p = img + row * F8_KS;
  const int key = f8_key(row);
  i32x4 lo = *(const i32x4*)(p + ((g16 ^ key) << 4));
  i32x4 hi = *(const i32x4*)(p + (((4 + g16) ^ key) << 4));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// FA/FB: 0 = E4M3, 1 = E5M2 (the cbsz / blgp encodings). sa / sb: in byte 0
// (op_sel 0) the E8M0 scale of K block l >> 4 of the lane's row of A / B;
// the unit word makes it a plain product.
template <int FA, int FB>
__device__ __forceinline__ f32x4 f8_mfma(i32x8 a, i32x8 b, f32x4 c,
                                         int sa = F8_UNIT, int sb = F8_UNIT) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, 0,
                                                          sa, 0, sb);
}

// FP4 (E2M1, two elements to a byte, element 2q in the low nibble of byte
// q): the same instruction with cbsz = blgp = 4 takes four VGPRs per operand,
// 32 K elements per lane, so f8_frag's eight VGPRs are two FP4 operands: half
// H (0: the low four, chunk 2g of the row; 1: the high four, chunk 2g + 1)
// is elements [64 g + 32 H, +32) of a 256-element step, its scale block
// 2g + H. sa / sb hold the two E8M0 bytes of blocks 2g and 2g + 1 in bytes 0
// and 1 and op_sel H picks the half's own. Measured on MI355X as
// f8_frag_mx's layout was: here the ISA text holds as it stands.
template <int H>
__device__ __forceinline__ f32x4 f4_mfma(i32x8 a, i32x8 b, f32x4 c, int sa,
                                         int sb) {
  constexpr int o = 4 * H;
  const i32x8 ah = __builtin_shufflevector(a, a, o, o + 1, o + 2, o + 3, -1,
                                           -1, -1, -1);
  const i32x8 bh = __builtin_shufflevector(b, b, o, o + 1, o + 2, o + 3, -1,
                                           -1, -1, -1);
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ah, bh, c, 4, 4, H,
                                                          sa, H, sb);
}

// The scale bytes of blocks 2g and 2g + 1 of `row` out of a scale image of
// 8 bytes (one 256-element step) per row: one 16-bit read.
__device__ __forceinline__ int f4_scale2(const char* simg, int row, int g16) {
  return *(const uint16_t*)(simg + row * 8 + 2 * g16);
}

// The value of every E2M1 code s.ee.m; there is no NaN or inf code.
inline constexpr float fp4_value[16] = {0.f,  0.5f,  1.f,  1.5f,  2.f,  3.f,
                                        4.f,  6.f,   -0.f, -0.5f, -1.f, -1.5f,
                                        -2.f, -3.f,  -4.f, -6.f};

// An accumulator's MFMA chain up to here stays above this point: the
// results are used only in the epilogue, and the compiler otherwise sinks
// the MFMAs of the last K steps into it, with their fragments spilled.
__device__ __forceinline__ void f8_pin(f32x4& v) {
  asm volatile("" : "+v"(v));
}

// 16 bytes of a row at K offset k0, zero past k; nothing is read when !ok.
__device__ __forceinline__ i32x4 f8_load16(const uint8_t* row, bool ok, int k0,
                                           int k) {
  i32x4 v = {};
  if (ok && k0 + 16 <= k) {
    __builtin_memcpy(&v, row + k0, 16);
  } else if (ok) {
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; e++)
      if (k0 + e < k) w[e >> 2] |= (unsigned)row[k0 + e] << (8 * (e & 3));
    v = i32x4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
  }
  return v;
}

// A hashed byte with the top exponent bit cleared: the exponent field stays
// below its all-ones value in either format, so no code is a NaN or an inf
// and |x| < 2.
__host__ __device__ static inline uint8_t fp8_fill_byte(size_t i,
                                                        uint32_t seed) {
  uint64_t h = (i * 2654435761ull) ^ ((uint64_t)seed * 2246822519ull);
  h ^= h >> 13;
  h *= 0x9E3779B97F4A7C15ull;
  h ^= h >> 32;
  return (uint8_t)(h & 0xBF);
}

// The value of every byte code: [0] E4M3 (e4m3fn: S.1111.111 is NaN, there
// is no inf), [1] E5M2 (IEEE-like: exponent 31 is inf / NaN).
struct Fp8Tables {
  float v[2][256];
  Fp8Tables() {
    for (int b = 0; b < 256; b++) {
      const float s = b & 0x80 ? -1.f : 1.f;
      int e = (b >> 3) & 15, f = b & 7;
      v[0][b] = e == 15 && f == 7 ? NAN
                : e == 0          ? s * std::ldexp((float)f, -9)
                                  : s * std::ldexp(8.f + f, e - 10);
      e = (b >> 2) & 31, f = b & 3;
      v[1][b] = e == 31  ? (f ? NAN : s * INFINITY)
                : e == 0 ? s * std::ldexp((float)f, -16)
                         : s * std::ldexp(4.f + f, e - 17);
    }
  }
};

// An fp8 format name as the kernels' format number.
inline int fp8_format(const std::string& f) {
  PA_CHECK(f == "e4m3" || f == "e5m2", "fp8 format is \"e4m3\" or \"e5m2\"");
  return f == "e5m2";
}

}  // namespace pa
