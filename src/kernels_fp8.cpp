// FP8 (OCP E4M3 / E5M2) tile-GEMM on gfx950's 8-bit matrix-core path.
//
// C (fp32, col-major m x n) = alpha * A * B^T (+ C), A m x k and B n x k with
// K contiguous (row i of A is k bytes at A + i*lda): the "TN" convention of
// the bf16 kernels, so both operand fragments are K-contiguous in LDS. Each
// operand is E4M3 (e4m3fn: no inf, max 448) or E5M2, chosen per operand at
// compile time through the instruction's cbsz/blgp immediates.
//
// The instruction is v_mfma_scale_f32_16x16x128_f8f6f4 with both hardware
// block scales pinned to 1.0 (E8M0 127 in every byte, so the byte select
// does not matter); the per-GEMM scale alpha is applied in the epilogue. One
// MFMA consumes a 16 x 128-byte slab of each operand:
//
//   fragment   lane l holds row (l & 15), K bytes [(l >> 4) * 32, +32) of
//              the step in 8 VGPRs. That is a permutation of the order the
//              instruction numbers K in (kernels_fp8.hpp, f8_frag_mx), the
//              same in A and B, so the product under unit scales is the same.
//   result     lane l holds column (l & 15), rows (l >> 4) * 4 + 0..3, as
//              every 16x16 MFMA.
//
// LDS image of a K step: [row][128 B], the 16-byte chunk c of row r stored
// at chunk c ^ key(r), key(r) = (r >> 1) & 7. A fragment is two ds_read_b128
// (chunks 2g and 2g+1 of the lane's row, g = l >> 4). The model assumed here,
// the one the bf16 kernels' swizzle rests on and not confirmed with counters
// on this part, is that a b128 read is served 16 consecutive lanes at a
// time over 64 banks of 4 bytes. Under it those 16 lanes (rows r0..r0+15,
// r0 % 16 == 0, one g) must touch the 16 distinct 16-byte bank groups of
// the 256-byte bank line. The bank group of (r, chunk c') is (r*8 + c') % 16 =
// (r & 1)*8 + c'. With c' = c ^ key(r), c fixed: the even rows have keys
// 0..7, so their c' are a permutation of 0..7 (groups 0..7); the odd rows
// likewise fill groups 8..15. All 16 differ for c = 2g and for c = 2g+1, so
// both reads of a fragment are conflict-free. Unswizzled, the 16 rows would
// share two groups (an 8-way conflict).
//
// MX block scales (live scale registers on the same operand path) and the
// fp32 -> MXFP8 quantiser are in kernels_mxfp8.cpp; what both files share is
// in kernels_fp8.hpp, and the same over packed FP4 (E2M1) elements is in
// kernels_mxfp4.cpp. Out of scope here: M/N-major operands, FP6, mixed
// FP8 x FP4 operand pairs, bf16 output.
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

// ------------------------------------------------------------ fast kernel
// 256x256 block, 8 waves as 2(M) x 4(N), 128x64 per wave: 8x4 f32x4
// accumulators (128 VGPRs). One K step is 128 bytes per row, so a step's A
// and B images are 32 KB each and the ring has two slots (128 KB, one block
// per CU, 2 waves per SIMD, 256 registers per lane). A step is 32 MFMAs per
// wave against 24 ds_read_b128 and 8 global->LDS copies.
//
// Per step t (slot t & 1):
//   s_waitcnt vmcnt(8)   this wave's copies of step t have landed; the 8 of
//                        step t+1 stay in flight across the barrier
//   s_barrier            ... and so have everyone else's
//   read the 4 B fragments and A fragments 0..3, 4 MFMAs
//   read A fragments 4..7 under the other 12 MFMAs of A fragments 0..3
//   lgkmcnt(0), s_barrier: every wave has the slot in registers
//   issue the 8 copies of step t+2 into it, the 16 MFMAs of A fragments 4..7
// The A fragments come in two groups of four, and the second group's reads
// go into registers the first group has finished with, so at most 96 VGPRs
// hold fragments beside the 128 of the accumulators (234 VGPRs in all, no
// scratch). The copies issued in the middle of step t have the rest of it
// and all of step t+1 to land. The last two steps issue no copies, so the
// loop is peeled there and every step is straight-line code; sched_barrier
// keeps the compiler from sinking the first MFMA group below the second
// barrier, which serialises a step into reads, barrier, MFMAs.
template <int FA, int FB>
__launch_bounds__(512)
__global__ void k_gemm_fp8(int m, int n, int k, const uint8_t* __restrict__ A,
                           int lda, const uint8_t* __restrict__ B, int ldb,
                           float* __restrict__ C, int ldc, int nbx,
                           float alpha, int accum) {
  extern __shared__ __attribute__((aligned(16))) char f8_ring[];
  constexpr int IMG = F8_BM * F8_KS;  // one operand's step image, 32 KB
  constexpr int SLOT = 2 * IMG;       // [A image | B image]
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wr = wave >> 2, wc = wave & 3;
  const int id = bf_swz(blockIdx.x, gridDim.x);
  const int bm0 = (id % nbx) * F8_BM, bn0 = (id / nbx) * F8_BN;
  const int g16 = lane >> 4, r16 = lane & 15;

  // staging: one copy instruction moves 64 lanes x 16 B = 8 rows of 128 B,
  // lane-linear in LDS; the swizzle goes through the source address. Wave w
  // copies rows [32w, 32w + 32) of each image in 4 pieces. Lane offsets are
  // 32-bit (256 rows x ld < 2^31) on a block- and step-uniform base.
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
  auto stage = [&](int t) {
    char* slot = f8_ring + (t & 1) * SLOT + wave * 32 * F8_KS;
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
  };

  f32x4 acc[8][4] = {};
  // one K step; restage: issue the copies of step t+2, last: nothing newer
  // than step t is in flight
  auto step = [&](int t, auto restage, auto last) {
    if constexpr (decltype(last)::value) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const char* as = f8_ring + (t & 1) * SLOT;
    const char* bs = as + IMG;
    i32x8 b[4], a0[4], a1[4];
#pragma unroll
    for (int f = 0; f < 4; f++)
      b[f] = f8_frag(bs, wc * 64 + f * 16 + r16, g16);
#pragma unroll
    for (int f = 0; f < 4; f++)
      a0[f] = f8_frag(as, wr * 128 + f * 16 + r16, g16);
    __builtin_amdgcn_sched_barrier(0);
    // the first MFMAs go ahead of the second group's reads, so that their
    // wait covers the 16 reads above and not all 24
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 4; j++)
      acc[0][j] = f8_mfma<FA, FB>(a0[0], b[j], acc[0][j]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < 4; f++)
      a1[f] = f8_frag(as, wr * 128 + 64 + f * 16 + r16, g16);
#pragma unroll
    for (int i = 1; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f8_mfma<FA, FB>(a0[i], b[j], acc[i][j]);
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
        acc[4 + i][j] = f8_mfma<FA, FB>(a1[i], b[j], acc[4 + i][j]);
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
// Any m, n, k >= 1 and any lda, ldb >= k: 128x128 block, 4 waves as 2x2 of
// 64x64, the same step image, fragments and MFMA as the fast kernel, staged
// through registers with guarded loads. Rows past m / n and bytes past k are
// zero bytes, which is +0 in both formats, so the padding adds exact zeros.

template <int FA, int FB>
__launch_bounds__(256)
__global__ void k_gemm_fp8_edge(int m, int n, int k,
                                const uint8_t* __restrict__ A, int lda,
                                const uint8_t* __restrict__ B, int ldb,
                                float* __restrict__ C, int ldc, int nbx,
                                float alpha, int accum) {
  __shared__ __attribute__((aligned(16))) char As[F8E_BM * F8_KS];
  __shared__ __attribute__((aligned(16))) char Bs[F8E_BN * F8_KS];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int id = bf_swz(blockIdx.x, gridDim.x);
  const int bm0 = (id % nbx) * F8E_BM, bn0 = (id / nbx) * F8E_BN;
  const int g16 = lane >> 4, r16 = lane & 15;

  f32x4 acc[4][4] = {};
  for (int k0 = 0; k0 < k; k0 += F8_KS) {
    // 128 rows x 8 chunks per image, 4 chunks per thread and operand
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
    __syncthreads();
    i32x8 a[4], b[4];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      a[f] = f8_frag(As, wr * 64 + f * 16 + r16, g16);
      b[f] = f8_frag(Bs, wc * 64 + f * 16 + r16, g16);
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = f8_mfma<FA, FB>(a[i], b[j], acc[i][j]);
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
static void launch_gemm_fp8_fmt(int m, int n, int k, const uint8_t* A, int lda,
                                const uint8_t* B, int ldb, float* C, int ldc,
                                float alpha, int accum, hipStream_t stream) {
  // the global->LDS copies move aligned 16-byte chunks of whole K steps
  const bool fast = m % F8_BM == 0 && n % F8_BN == 0 && k % F8_KS == 0 &&
                    k >= 2 * F8_KS && lda % 16 == 0 && ldb % 16 == 0 &&
                    lda < (1 << 23) && ldb < (1 << 23) &&
                    ((uintptr_t)A | (uintptr_t)B) % 16 == 0;
  if (fast) {
    constexpr size_t lds = 2 * (F8_BM + F8_BN) * F8_KS;  // 128 KB
    // the attribute belongs to the device: once per device of the process.
    // Two threads racing here both set the same value, which is harmless.
    static std::atomic<bool> attr[64];
    int dev = 0;
    PA_HIP_CHECK(hipGetDevice(&dev));
    PA_CHECK(dev >= 0 && dev < 64);
    if (!attr[dev].load(std::memory_order_acquire)) {
      PA_HIP_CHECK(hipFuncSetAttribute(
          (const void*)k_gemm_fp8<FA, FB>,
          hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      attr[dev].store(true, std::memory_order_release);
    }
    const int nbx = m / F8_BM, nby = n / F8_BN;
    hipLaunchKernelGGL((k_gemm_fp8<FA, FB>), dim3(nbx * nby), dim3(512), lds,
                       stream, m, n, k, A, lda, B, ldb, C, ldc, nbx, alpha,
                       accum);
    return;
  }
  const int nbx = (m + F8E_BM - 1) / F8E_BM, nby = (n + F8E_BN - 1) / F8E_BN;
  hipLaunchKernelGGL((k_gemm_fp8_edge<FA, FB>), dim3(nbx * nby), dim3(256), 0,
                     stream, m, n, k, A, lda, B, ldb, C, ldc, nbx, alpha,
                     accum);
}

// C (m x n, col-major, ldc) = alpha A B^T (+ C when accum). fmt: 0 = E4M3,
// 1 = E5M2. A is m rows of k bytes lda apart, B n rows of k bytes ldb apart.
static void launch_gemm_fp8(int m, int n, int k, const void* A, int lda,
                            int fmtA, const void* B, int ldb, int fmtB,
                            float* C, int ldc, float alpha, int accum,
                            hipStream_t stream) {
  PA_CHECK((fmtA | fmtB | 1) == 1, "fp8 format is 0 (e4m3) or 1 (e5m2)");
  PA_CHECK(m >= 1 && n >= 1 && k >= 1 && lda >= k && ldb >= k && ldc >= m);
  const uint8_t* a = (const uint8_t*)A;
  const uint8_t* b = (const uint8_t*)B;
  switch (fmtA * 2 + fmtB) {
    case 0:
      launch_gemm_fp8_fmt<0, 0>(m, n, k, a, lda, b, ldb, C, ldc, alpha, accum,
                                stream);
      break;
    case 1:
      launch_gemm_fp8_fmt<0, 1>(m, n, k, a, lda, b, ldb, C, ldc, alpha, accum,
                                stream);
      break;
    case 2:
      launch_gemm_fp8_fmt<1, 0>(m, n, k, a, lda, b, ldb, C, ldc, alpha, accum,
                                stream);
      break;
    default:
      launch_gemm_fp8_fmt<1, 1>(m, n, k, a, lda, b, ldb, C, ldc, alpha, accum,
                                stream);
  }
}

// -------------------------------------------------------------------- fill
// four bytes per store; nbytes is rounded down to a word, the tail bytewise
__global__ void k_fill_fp8(uint8_t* p, size_t nbytes, uint32_t seed) {
  const size_t nw = nbytes / 4;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < nw; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; e++)
      w |= (uint32_t)fp8_fill_byte(4 * i + e, seed) << (8 * e);
    ((uint32_t*)p)[i] = w;
  }
  if (blockIdx.x == 0 && threadIdx.x < nbytes - 4 * nw)
    p[4 * nw + threadIdx.x] = fp8_fill_byte(4 * nw + threadIdx.x, seed);
}

static void cpu_fill_fp8(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  Data* d = t.flows[0].data;
  uint8_t* p = (uint8_t*)d->ensure_host();
  for (size_t i = 0; i < d->bytes; i++) p[i] = fp8_fill_byte(i, a.seed);
  d->written_on(false);
}

static void gpu_fill_fp8(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  hipLaunchKernelGGL(k_fill_fp8, dim3(2048), dim3(256), 0, g.stream,
                     (uint8_t*)t.dev_ptr[0], t.flows[0].data->bytes, a.seed);
}

// ------------------------------------------------------------------ chores
static void cpu_gemm_fp8(Task& t) {
  static const Fp8Tables tab;
  const GemmFp8Args& a = t.arg<GemmFp8Args>();
  const uint8_t* A = (const uint8_t*)t.flows[0].data->pull_to_host();
  const uint8_t* B = (const uint8_t*)t.flows[1].data->pull_to_host();
  Data* cd = t.flows[2].data;
  float* C = a.accum ? (float*)cd->pull_to_host() : (float*)cd->ensure_host();
  const float* da = tab.v[a.fmt_a];
  const float* db = tab.v[a.fmt_b];
  const int ldc = cd->coll->mb();
  for (int j = 0; j < a.n; j++)
    for (int i = 0; i < a.m; i++) {
      const uint8_t* ar = A + (size_t)i * a.lda;
      const uint8_t* br = B + (size_t)j * a.ldb;
      float s = 0;
      for (int p = 0; p < a.k; p++) s += da[ar[p]] * db[br[p]];
      float& c = C[(size_t)j * ldc + i];
      c = a.accum ? c + a.alpha * s : a.alpha * s;
    }
  cd->written_on(false);
}

static void gpu_gemm_fp8(Task& t, GpuTaskCtx& g) {
  const GemmFp8Args& a = t.arg<GemmFp8Args>();
  launch_gemm_fp8(a.m, a.n, a.k, t.dev_ptr[0], a.lda, a.fmt_a, t.dev_ptr[1],
                  a.ldb, a.fmt_b, (float*)t.dev_ptr[2],
                  t.flows[2].data->coll->mb(), a.alpha, a.accum, g.stream);
}

TaskClass& tc_fill_fp8() {
  static TaskClass tc = make_tc("fill_fp8", TaskKind::GPU, cpu_fill_fp8,
                                gpu_fill_fp8, TC_FILL_FP8);
  return tc;
}
TaskClass& tc_gemm_fp8() {
  static TaskClass tc = make_tc("gemm_fp8", TaskKind::GPU, cpu_gemm_fp8,
                                gpu_gemm_fp8, TC_GEMM_FP8);
  return tc;
}

// ------------------------------------------------------------ DAG builders
void insert_fill_fp8(Dtd& tp, TiledMatrix& A, uint32_t seed) {
  PA_CHECK(A.elem_size() == 1);
  for (int tm = 0; tm < A.mt(); tm++)
    for (int tn = 0; tn < A.nt(); tn++) {
      TileArgs a;
      a.seed = seed ^ (uint32_t)(tm * 9973 + tn);
      Dtd::FlowSpec f[] = {{A.tile(tm, tn), ACCESS_OUT}};
      tp.insert(&tc_fill_fp8(), &a, sizeof(a), f, 1, 0, A.rank_of(tm, tn));
    }
}

// The K chain of C(m, n) runs k = 0 (overwrite), 1, 2, ... (accumulate),
// each step adding alpha times its product: the chain sums to alpha A^T B.
void insert_gemm_fp8(Dtd& tp, TiledMatrix& A, TiledMatrix& B, TiledMatrix& C,
                     const std::string& fmt_a, const std::string& fmt_b,
                     float alpha) {
  PA_CHECK(A.elem_size() == 1 && B.elem_size() == 1 && C.elem_size() == 4);
  PA_CHECK(A.m() == B.m() && A.mb() == B.mb(), "K tilings must match");
  PA_CHECK(A.n() == C.m() && B.n() == C.n() && A.nb() == C.mb() &&
               B.nb() == C.nb(),
           "A is K x M, B is K x N, C is M x N with matching tiles");
  GemmFp8Args a;
  a.fmt_a = fp8_format(fmt_a);
  a.fmt_b = fp8_format(fmt_b);
  a.alpha = alpha;
  a.lda = A.mb();
  a.ldb = B.mb();
  for (int m = 0; m < C.mt(); m++)
    for (int n = 0; n < C.nt(); n++)
      for (int k = 0; k < A.mt(); k++) {
        a.m = A.tile_cols(m);
        a.n = B.tile_cols(n);
        a.k = A.tile_rows(k);
        a.accum = (k != 0);
        Dtd::FlowSpec f[] = {{A.tile(k, m), ACCESS_IN},
                             {B.tile(k, n), ACCESS_IN},
                             {C.tile(m, n),
                              k == 0 ? ACCESS_OUT : ACCESS_INOUT}};
        tp.insert(&tc_gemm_fp8(), &a, sizeof(a), f, 3, -(k),
                  C.rank_of(m, n));
      }
}

// kernel-level microbench (TFLOP/s)
double bench_gemm_fp8(int m, int n, int k, int iters, int fmt_a, int fmt_b) {
  DevArray<uint8_t> dA((size_t)m * k), dB((size_t)n * k);
  DevArray<float> dC((size_t)m * n);
  hipLaunchKernelGGL(k_fill_fp8, dim3(2048), dim3(256), 0, 0, dA.p,
                     (size_t)m * k, 1u);
  hipLaunchKernelGGL(k_fill_fp8, dim3(2048), dim3(256), 0, 0, dB.p,
                     (size_t)n * k, 2u);
  PA_HIP_CHECK(hipMemset(dC.p, 0, dC.bytes));
  double dt = time_launches(iters, [&] {
    launch_gemm_fp8(m, n, k, dA.p, k, fmt_a, dB.p, k, fmt_b, dC.p, m, 1.f, 1,
                    0);
  });
  return 2.0 * m * n * k * iters / dt / 1e12;
}

// host-I/O numerics harness: A holds m rows of lda bytes, B n rows of ldb, C
// m x n col-major; a leading dimension of 0 means k.
void test_gemm_fp8_hip(int m, int n, int k, const uint8_t* A, int fmt_a,
                       const uint8_t* B, int fmt_b, float* C, float alpha,
                       int lda, int ldb, int accum) {
  if (!lda) lda = k;
  if (!ldb) ldb = k;
  DevArray<uint8_t> dA((size_t)lda * m, A), dB((size_t)ldb * n, B);
  DevArray<float> dC((size_t)m * n, C);
  launch_gemm_fp8(m, n, k, dA.p, lda, fmt_a, dB.p, ldb, fmt_b, dC.p, m, alpha,
                  accum, 0);
  dC.download(C);
}

}  // namespace pa
