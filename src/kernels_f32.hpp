// Launch API of the hand-written fp32 MFMA kernels (kernels_f32.cpp). All
// matrices are column-major; every launcher enqueues on `stream` and returns.
#pragma once

#include "device_gpu.hpp"

namespace pa {

// What the full-tile kernel takes: whole 128-blocks, k % 16 == 0, and, as it
// moves 16 B per lane, leading dimensions that are multiples of 4 and 16-B
// aligned operands. The first two launchers send every other shape to the
// bounds-checked kernel.
bool sgemm_full_tiles(int m, int n, int k, const float* A, int lda,
                      const float* B, int ldb, const float* C, int ldc);
// C[m x n] -= A[m x k] * B[n x k]^T
void launch_sgemm_nt(int m, int n, int k, const float* A, int lda,
                     const float* B, int ldb, float* C, int ldc,
                     hipStream_t stream);
// C[n x n] -= A[n x k] * A^T on the lower-triangular set of 128-blocks
// (diagonal blocks are computed whole)
void launch_ssyrk_ln(int n, int k, const float* A, int lda, float* C, int ldc,
                     hipStream_t stream);
// X[m x n] = B[m x n] * W[n x n]^T, W lower triangular with stored zeros
// above its diagonal; X is not read. sgemm_full_tiles(m, n, n, ...) shapes
// only (callers dispatch).
void launch_strmm_rlt(int m, int n, const float* B, int ldb, const float* W,
                      int ldw, float* X, int ldx, hipStream_t stream);
// dst = (float)src, round to nearest even, or dst = (double)src, on a
// rows x cols block; both sides have the leading dimension ld (in elements).
void launch_convert(const double* src, float* dst, int rows, int cols, int ld,
                    hipStream_t stream);
void launch_convert(const float* src, double* dst, int rows, int cols, int ld,
                    hipStream_t stream);

// Host-memory entry points for the Python test bindings: upload, one launch
// on the null stream, download.
void test_sgemm_nt_hip(int m, int n, int k, const float* A, int lda,
                       const float* B, int ldb, float* C, int ldc);
void test_ssyrk_ln_hip(int n, int k, const float* A, int lda, float* C,
                       int ldc);
void test_strmm_rlt_hip(int m, int n, const float* B, int ldb, const float* W,
                        int ldw, float* X, int ldx);
void test_convert_d2s_hip(const double* src, float* dst, int rows, int cols,
                          int ld);
void test_convert_s2d_hip(const float* src, double* dst, int rows, int cols,
                          int ld);

// Seconds for `iters` launches of C -= A B^T, device resident: the hand
// kernel or rocblas_sgemm.
double bench_sgemm(int m, int n, int k, int iters, bool rocblas);

}  // namespace pa
