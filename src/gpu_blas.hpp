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

#include "data.hpp"
#include "device_gpu.hpp"

// Evaluate a rocBLAS / rocSOLVER call; any status but success is fatal.
#define PA_BLAS_CHECK(expr)                                                  \
  do {                                                                       \
    rocblas_status _s = (expr);                                              \
    if (_s != rocblas_status_success)                                        \
      ::pa::fatal("rocBLAS status %d at %s:%d: %s", (int)_s, __FILE__,       \
                  __LINE__, #expr);                                          \
  } while (0)

namespace pa {

inline rocblas_handle blas_handle(GpuTaskCtx& g) {
  static thread_local std::map<void*, rocblas_handle> handles;
  rocblas_handle& h = handles[(void*)g.stream];
  if (!h) {
    PA_BLAS_CHECK(rocblas_create_handle(&h));
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

// A fresh pool buffer for flow f's tile and, once the kernels that fill it
// are enqueued, its swap-in as the tile's device copy: an operation that
// cannot run in place needs no copy back. The old buffer returns to the pool
// only after the task's kernels complete (the engine's deferred frees).
inline double* fresh_tile(Task& t, GpuTaskCtx& g, int f) {
  return (double*)g.engine->dev_alloc(t.flows[f].data->bytes);
}
inline void swap_in_tile(Task& t, GpuTaskCtx& g, int f, double* X) {
  Data* d = t.flows[f].data;
  {
    SpinGuard gd(d->lock);
    g.deferred_frees->emplace_back(d->dev_ptr, d->bytes);
    d->dev_ptr = X;
  }
  t.dev_ptr[f] = X;
}

}  // namespace pa
