// Shared pieces of the bench and test entry points: a scoped device array,
// a timed launch loop, and the declarations of the entry points that live
// outside kernels_hip.cpp (those are in kernels_hip.hpp).
#pragma once

#include <cstdint>

#include "device_gpu.hpp"

namespace pa {

// A device array for the host-memory entry points: allocated, and uploaded
// when a host image is given, on construction; freed on scope exit.
template <typename T = double>
struct DevArray {
  T* p = nullptr;
  size_t bytes;
  explicit DevArray(size_t nelem, const T* host = nullptr)
      : bytes(nelem * sizeof(T)) {
    PA_HIP_CHECK(hipMalloc(&p, bytes));
    if (host) PA_HIP_CHECK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
  }
  DevArray(const DevArray&) = delete;
  ~DevArray() { PA_HIP_CHECK(hipFree(p)); }
  // what the launches so far left in it (the copy waits for the null
  // stream; synchronize a non-blocking stream first)
  void download(T* host) {
    PA_HIP_CHECK(hipGetLastError());
    PA_HIP_CHECK(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost));
  }
};

// One warm-up launch, then the seconds that iters launches take. The waits
// are for the whole device, or for `stream` alone when one is given.
template <typename F>
double time_launches(int iters, F run, hipStream_t stream = nullptr) {
  auto sync = [&] {
    if (stream)
      PA_HIP_CHECK(hipStreamSynchronize(stream));
    else
      PA_HIP_CHECK(hipDeviceSynchronize());
  };
  run();
  sync();
  double t0 = now_s();
  for (int i = 0; i < iters; i++) run();
  sync();
  return now_s() - t0;
}

// The synthetic SPD fill kernel on a rows x cols block whose first element
// has the global index (i0, j0): the fill chore's kernel, and the operand
// fill of the library bench loops (kernels_blas.cpp).
void launch_spd_fill(double* t, int rows, int cols, int ld, int64_t i0,
                     int64_t j0, int64_t N, uint32_t seed, hipStream_t s);

// Timed library loops for the A/B against the hand kernels; seconds for
// `iters` calls (dgemm: kernels_blas.cpp, tn: kernels_inv.cpp).
double bench_dgemm_rocblas(int m, int n, int k, int iters);
double bench_dgemm_nn_rocblas(int m, int n, int k, int iters);
double bench_tn_rocblas(int kind, int m, int n, int k, int iters);

// bf16 GEMM: TFLOP/s of the kernel, and its host-memory test entry
// (kernels_bf16.cpp). a_mmajor: A is m x k col-major instead of k x m;
// b_nmajor: B is n x k col-major instead of k x n.
double bench_gemm_bf16(int m, int n, int k, int iters, bool a_mmajor = false,
                       bool b_nmajor = false);
void test_gemm_bf16_hip(int m, int n, int k, const uint16_t* A,
                        const uint16_t* B, float* C, bool a_mmajor = false,
                        bool b_nmajor = false, int lda = 0, int ldb = 0,
                        int accum = 1);

// fp8 GEMM, C = alpha A B^T with K-major byte operands: TFLOP/s of the
// kernel, and its host-memory test entry (kernels_fp8.cpp). fmt: 0 = E4M3,
// 1 = E5M2; a leading dimension of 0 means k.
double bench_gemm_fp8(int m, int n, int k, int iters, int fmt_a = 0,
                      int fmt_b = 0);
void test_gemm_fp8_hip(int m, int n, int k, const uint8_t* A, int fmt_a,
                       const uint8_t* B, int fmt_b, float* C, float alpha = 1.f,
                       int lda = 0, int ldb = 0, int accum = 0);

// MXFP8 GEMM and quantiser (kernels_mxfp8.cpp): TFLOP/s of the GEMM kernel
// on synthetic operands with scale bytes in 120..134, GB/s of the quantiser
// over the bytes it reads and writes, and the host-memory test entries. SA /
// SB hold ceil(k/32) scale bytes per row, ldsa / ldsb apart; the quantiser
// writes Q (rows x k) and S (rows x ceil(k/32)) tight.
double bench_gemm_mxfp8(int m, int n, int k, int iters, int fmt_a = 0,
                        int fmt_b = 0);
double bench_quantize_mxfp8(int rows, int k, int iters, int fmt = 0);
void test_gemm_mxfp8_hip(int m, int n, int k, const uint8_t* A, int fmt_a,
                         const uint8_t* SA, const uint8_t* B, int fmt_b,
                         const uint8_t* SB, float* C, float alpha, int lda,
                         int ldb, int ldsa, int ldsb, int accum);
void test_quantize_mxfp8_hip(int rows, int k, int fmt, const float* X, int ldx,
                             uint8_t* Q, uint8_t* S);

// MXFP4 GEMM and quantiser (kernels_mxfp4.cpp), as the MXFP8 entries above:
// k counts E2M1 elements, two to a byte, lda / ldb are in bytes; the
// quantiser writes Q (rows x ceil(k/2)) and S (rows x ceil(k/32)) tight.
double bench_gemm_mxfp4(int m, int n, int k, int iters);
double bench_quantize_mxfp4(int rows, int k, int iters);
void test_gemm_mxfp4_hip(int m, int n, int k, const uint8_t* A,
                         const uint8_t* SA, const uint8_t* B,
                         const uint8_t* SB, float* C, float alpha, int lda,
                         int ldb, int ldsa, int ldsb, int accum);
void test_quantize_mxfp4_hip(int rows, int k, const float* X, int ldx,
                             uint8_t* Q, uint8_t* S);

// MXFP6 GEMM and quantiser (kernels_mxfp6.cpp), as the MXFP8 entries above:
// k counts 6-bit elements, four to three bytes, lda / ldb are in bytes,
// fmt 0 = E2M3, 1 = E3M2; the quantiser writes Q (rows x ceil(3k/4)) and S
// (rows x ceil(k/32)) tight.
double bench_gemm_mxfp6(int m, int n, int k, int iters, int fmt_a, int fmt_b);
double bench_quantize_mxfp6(int rows, int k, int iters, int fmt);
void test_gemm_mxfp6_hip(int m, int n, int k, const uint8_t* A, int fmt_a,
                         const uint8_t* SA, const uint8_t* B, int fmt_b,
                         const uint8_t* SB, float* C, float alpha, int lda,
                         int ldb, int ldsa, int ldsb, int accum);
void test_quantize_mxfp6_hip(int rows, int k, int fmt, const float* X, int ldx,
                             uint8_t* Q, uint8_t* S);

// What bench_qr_factor times (kernels_qr.cpp); seconds for `iters`
// factorizations of an m x k tile.
enum QrBenchMode {
  QR_BENCH_FULL = 0,          // qr_factor_hand: panels, trailing apply, T
  QR_BENCH_PANELS = 1,        // the panel kernel launches alone
  QR_BENCH_ROCSOLVER = 2,     // rocsolver_dgeqrf
  QR_BENCH_PANELS_TIMED = 5,  // as PANELS, and print the in-kernel timers
};
double bench_qr_factor(int m, int k, int ts_split, int iters, int mode);

}  // namespace pa
