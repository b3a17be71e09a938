// Per-stream rocBLAS state shared by every GPU chore that calls rocBLAS or
// rocSOLVER.
//
// One handle PER EXEC STREAM, not one per process: rocBLAS/rocSOLVER keep
// device workspace on the handle (e.g. dtrsm's invA), so concurrent kernels
// on different streams must not share one. Every call on a handle is
// enqueued on that handle's own stream, so the algorithms that share a
// stream's handle are ordered by the stream. Hooks for a stream run on one
// thread only, so thread_local maps are race-free; being function-local
// statics of inline functions, they are one object per thread across
// translation units.
#pragma once

#include <map>

#include <rocblas/rocblas.h>

#include "device_gpu.hpp"

namespace pa {

inline rocblas_handle blas_handle(GpuTaskCtx& g) {
  static thread_local std::map<void*, rocblas_handle> handles;
  rocblas_handle& h = handles[(void*)g.stream];
  if (!h) {
    PA_CHECK(rocblas_create_handle(&h) == rocblas_status_success);
    rocblas_set_pointer_mode(h, rocblas_pointer_mode_host);
    rocblas_set_stream(h, g.stream);
  }
  return h;
}

// The device `info` word rocSOLVER factorizations report into.
inline rocblas_int* dev_info(GpuTaskCtx& g) {
  static thread_local std::map<void*, rocblas_int*> infos;
  rocblas_int*& p = infos[(void*)g.stream];
  if (!p) PA_HIP_CHECK(hipMalloc(&p, sizeof(rocblas_int)));
  return p;
}

}  // namespace pa
