// Block-index decoding and the dynamic-LDS launch shared by the hand tile
// kernels of every element type (kernels_hip.cpp fp64, kernels_f32.cpp fp32).
// Device code: include from HIP translation units only.
#pragma once

#include <hip/hip_runtime.h>

#include "device_gpu.hpp"

namespace pa {

// 1-D grid with a bijective XCD-aware remap so consecutive blocks share B
// panels within one XCD's L2 (guide T1).
__device__ __forceinline__ int xcd_swizzle(int id, int nwg) {
  int q = nwg >> 3, r = nwg & 7;
  int xcd = id & 7, pos = id >> 3;
  // blocks per XCD: first r XCDs get q+1
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

// id -> (i >= j) over a lower-triangular set enumerated row by row.
__device__ __forceinline__ void tri_decode(int id, int& i, int& j) {
  i = 0;
  while (id > i) { i++; id -= i; }
  j = id;
}

// This block's (bx, by): in the nbx-wide full grid, or in the lower block
// set (SYRK writes only the lower blocks; diagonal blocks compute their
// full tile: the upper half of a diagonal tile is symmetric-valid and never
// read by the DAG).
__device__ __forceinline__ void block_decode(bool tri, int nbx, int& bx,
                                             int& by) {
  int id = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tri) {
    tri_decode(id, bx, by);
  } else {
    bx = id % nbx;
    by = id / nbx;
  }
}

// The snake order of the triangular product X = B W^T (kernels_hip.cpp, v3):
// a grid of 8 * ceil(nby / 8) * nbx blocks in which each XCD owns whole block
// columns, dealt longest-K-first in a boustrophedon over the XCDs. False for
// a padding block, which must leave before any barrier.
__device__ __forceinline__ bool snake_decode(int nbx, int nby, int& bx,
                                             int& by) {
  const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
  const int round = pos / nbx;
  const int rank = round * 8 + ((round & 1) ? 7 - xcd : xcd);
  if (rank >= nby) return false;
  bx = pos - round * nbx;
  by = nby - 1 - rank;
  return true;
}

// Every tile kernel asks for more dynamic LDS than a launch gets by
// default: raise that kernel's limit once, then launch.
template <auto Kern, typename... Args>
static void launch_lds(int grid, int block, size_t lds, hipStream_t stream,
                       Args... args) {
  static const bool raised = [lds] {
    PA_HIP_CHECK(hipFuncSetAttribute(
        (const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL(Kern, dim3(grid), dim3(block), lds, stream, args...);
}

}  // namespace pa
