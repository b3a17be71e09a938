// Launch API of the hand-written fp64 MFMA kernels (kernels_hip.cpp).
// All matrices are column-major; every launcher enqueues on `stream` and
// returns.
#pragma once

#include "device_gpu.hpp"

namespace pa {

// C[m x n] -= A[m x k] * B[n x k]^T
void launch_dgemm_nt(int m, int n, int k, const double* A, int lda,
                     const double* B, int ldb, double* C, int ldc,
                     hipStream_t stream);
// C[n x n] -= A[n x k] * A^T on the lower-triangular set of 128-blocks
// (diagonal blocks are computed whole)
void launch_dsyrk_ln(int n, int k, const double* A, int lda, double* C,
                     int ldc, hipStream_t stream);
// X[m x n] = B[m x n] * W[n x n]^T, W lower triangular with stored zeros
// above its diagonal. Full 128-blocks and even leading dimensions only
// (callers dispatch).
void launch_dtrmm_rlt(int m, int n, const double* B, int ldb, const double* W,
                      int ldw, double* X, int ldx, hipStream_t stream);
// The TN family (operands contiguous along K), bounds-checked: any shape and
// leading dimension. W is lower triangular and whatever is stored above its
// diagonal is ignored.
// C[m x n] += A[k x m]^T * B[k x n]
void launch_dgemm_tn(int m, int n, int k, const double* A, int lda,
                     const double* B, int ldb, double* C, int ldc,
                     hipStream_t stream);
// C[n x n] += A[k x n]^T * A on the lower-triangular set of 128-blocks
// (diagonal blocks are computed whole)
void launch_dsyrk_lt(int n, int k, const double* A, int lda, double* C,
                     int ldc, hipStream_t stream);
// X[m x n] = W[m x m]^T * B[m x n]; X is not read and must not overlap B
void launch_dtrmm_llt(int m, int n, const double* W, int ldw, const double* B,
                      int ldb, double* X, int ldx, hipStream_t stream);
// X[n x n] = W[n x n]^T * W on the lower-triangular set of 128-blocks
// (diagonal blocks whole, so symmetric); X is not read, must not overlap W,
// and its other blocks are left alone
void launch_dlauum_l(int n, const double* W, int ldw, double* X, int ldx,
                     hipStream_t stream);
// C[m x n] -= A[m x k] * B[k x n], bounds-checked: any shape and leading
// dimension
void launch_dgemm_nn(int m, int n, int k, const double* A, int lda,
                     const double* B, int ldb, double* C, int ldc,
                     hipStream_t stream);
// In-place lower Cholesky of an n x n block, n <= 128; the strict upper
// triangle is neither read nor written.
void launch_potf2(double* A, int n, int ld, hipStream_t stream);

// The chore_gemm=hip incarnation of the GEMM tile task.
void gpu_gemm_hip(Task& t, GpuTaskCtx& g);

// Host-memory entry points for the Python test bindings: upload, one
// launch on the null stream, download.
void test_dgemm_nt_hip(int m, int n, int k, const double* A, int lda,
                       const double* B, int ldb, double* C, int ldc);
void test_dsyrk_ln_hip(int n, int k, const double* A, int lda, double* C,
                       int ldc);
void test_dtrmm_rlt_hip(int m, int n, const double* B, int ldb,
                        const double* W, int ldw, double* X, int ldx);
void test_dgemm_tn_hip(int m, int n, int k, const double* A, int lda,
                       const double* B, int ldb, double* C, int ldc);
void test_dgemm_nn_hip(int m, int n, int k, const double* A, int lda,
                       const double* B, int ldb, double* C, int ldc);
void test_dsyrk_lt_hip(int n, int k, const double* A, int lda, double* C,
                       int ldc);
void test_dtrmm_llt_hip(int m, int n, const double* W, int ldw,
                        const double* B, int ldb, double* X, int ldx);
void test_dlauum_l_hip(int n, const double* W, int ldw, double* X, int ldx);
void test_potf2_hip(double* A, int n);

// Timed device-resident launch loops; return seconds for `iters` launches.
double bench_dgemm_hip(int m, int n, int k, int iters);
// kind 0 gemm (m, n, k), 1 syrk (n, k), 2 trmm (m, n), 3 lauum (n)
double bench_dgemm_tn_hip(int kind, int m, int n, int k, int iters);
double bench_dgemm_nn_hip(int m, int n, int k, int iters);
double bench_dtrmm_hip(int m, int n, int iters);

}  // namespace pa
