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
// (kernels_bf16.cpp).
double bench_gemm_bf16(int m, int n, int k, int iters);
void test_gemm_bf16_hip(int m, int n, int k, const uint16_t* A,
                        const uint16_t* B, float* C);

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
