// Pieces the bf16 tile-GEMM kernels share: the TN kernels of
// kernels_bf16.cpp and the column-major layouts of kernels_bf16_nx.cpp.
#pragma once

#include <hip/hip_runtime.h>

namespace pa {

typedef __bf16 bf16;
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// XCD-aware block swizzle: consecutive block ids land on the 8 XCDs round
// robin; remap so each XCD works on a contiguous run of tiles.
__device__ __forceinline__ int bf_swz(int id, int nwg) {
  int q = nwg >> 3, r = nwg & 7;
  int xcd = id & 7, pos = id >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

// C[m x n] (fp32, col-major) (+)= op(A) op(B) for the layouts other than TN
// (kernels_bf16_nx.cpp). a_mmajor: A is m x k col-major (lda >= m), else
// k x m col-major (lda >= k). b_nmajor: B is n x k col-major (ldb >= n),
// else k x n col-major (ldb >= k).
void launch_gemm_bf16_nx(int m, int n, int k, const void* A, int lda,
                         const void* B, int ldb, float* C, int ldc,
                         hipStream_t stream, int accum, bool a_mmajor,
                         bool b_nmajor);

}  // namespace pa
