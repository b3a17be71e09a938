// Tile QR (dgeqrf) — DTD headline app #2 (BASELINE.json config 4).
//
// Flat-tree tile QR in the PLASMA style the reference's users run through
// DPLASMA: GEQRT (panel QR + T factor), UNMQR (apply panel Q^T across the
// row), TSQRT (triangular-on-top-of-square QR combining R_kk with A_mk),
// TSMQR (apply the TS reflectors to row pairs). GPU chores compose
// rocSOLVER dgeqrf/dlarft/dlarfb with D2D stacking copies on the task
// stream; CPU chores are self-contained Householder reference code used by
// the no-GPU tests.
//
// Storage note (deviation from PLASMA, documented): the TS reflector block
// V has a non-identity top block here (generic dgeqrf on the stacked 2nb x
// nb matrix), so V is stored in a dedicated workspace collection V2(m,k)
// of 2nb x nb tiles instead of overwriting A(m,k); R lands in the upper
// triangles of A as usual. The factorization is verified via R^T R = A^T A.
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "device_gpu.hpp"
#include "gpu_blas.hpp"
#include "kernels.hpp"
#include "kernels_bench.hpp"
#include "profiling.hpp"

namespace pa {

// ============================================================ CPU reference
namespace {

inline double vval(const double* V, int ld, int r, int q) {
  // column q of a unit-lower reflector block: 0 above diag, 1 on diag
  return r < q ? 0.0 : (r == q ? 1.0 : V[(size_t)q * ld + r]);
}

void cpu_geqrf_kern(int m, int n, double* A, int ld, double* tau) {
  int kmax = m < n ? m : n;
  for (int j = 0; j < kmax; j++) {
    double alpha = A[(size_t)j * ld + j];
    double xnorm2 = 0;
    for (int i = j + 1; i < m; i++) {
      double v = A[(size_t)j * ld + i];
      xnorm2 += v * v;
    }
    if (xnorm2 == 0) {
      tau[j] = 0;
      continue;
    }
    double beta = -copysign(sqrt(alpha * alpha + xnorm2), alpha);
    tau[j] = (beta - alpha) / beta;
    double scal = 1.0 / (alpha - beta);
    for (int i = j + 1; i < m; i++) A[(size_t)j * ld + i] *= scal;
    A[(size_t)j * ld + j] = beta;
    for (int c = j + 1; c < n; c++) {
      double w = A[(size_t)c * ld + j];
      for (int i = j + 1; i < m; i++)
        w += A[(size_t)j * ld + i] * A[(size_t)c * ld + i];
      w *= tau[j];
      A[(size_t)c * ld + j] -= w;
      for (int i = j + 1; i < m; i++)
        A[(size_t)c * ld + i] -= w * A[(size_t)j * ld + i];
    }
  }
}

// forward/columnwise T factor: H_0 H_1 ... H_{k-1} = I - V T V^T
void cpu_larft_kern(int n, int k, const double* V, int ld, const double* tau,
                    double* T, int ldt) {
  std::vector<double> w(k);
  for (int i = 0; i < k; i++) {
    T[(size_t)i * ldt + i] = tau[i];
    for (int c = 0; c < i; c++) {
      double s = 0;
      for (int r = i; r < n; r++) s += vval(V, ld, r, c) * vval(V, ld, r, i);
      w[c] = s;
    }
    for (int r = 0; r < i; r++) {
      double s = 0;
      for (int c = r; c < i; c++) s += T[(size_t)c * ldt + r] * w[c];
      T[(size_t)i * ldt + r] = -tau[i] * s;
    }
  }
}

// C = (I - V T V^T)^T C = C - V T^T (V^T C)   (side=left, trans=T)
void cpu_larfb_kern(int m, int n, int k, const double* V, int ldv,
                    const double* T, int ldt, double* C, int ldc) {
  std::vector<double> W((size_t)k * n), W2((size_t)k * n);
  for (int c = 0; c < n; c++)
    for (int q = 0; q < k; q++) {
      double s = 0;
      for (int r = q; r < m; r++)
        s += vval(V, ldv, r, q) * C[(size_t)c * ldc + r];
      W[(size_t)c * k + q] = s;
    }
  for (int c = 0; c < n; c++)
    for (int q = 0; q < k; q++) {
      double s = 0;
      for (int sdx = 0; sdx <= q; sdx++)
        s += T[(size_t)q * ldt + sdx] * W[(size_t)c * k + sdx];
      W2[(size_t)c * k + q] = s;
    }
  for (int c = 0; c < n; c++)
    for (int r = 0; r < m; r++) {
      double s = 0;
      int qmax = r < k - 1 ? r : k - 1;
      for (int q = 0; q <= qmax; q++)
        s += vval(V, ldv, r, q) * W2[(size_t)c * k + q];
      C[(size_t)c * ldc + r] -= s;
    }
}

void stack_tiles(double* S, const double* top, bool triu_top,
                 const double* bot, bool triu_bot, int nb, int ld) {
  for (int c = 0; c < nb; c++) {
    for (int r = 0; r < nb; r++) {
      double v = top[(size_t)c * ld + r];
      S[(size_t)c * 2 * nb + r] = (triu_top && r > c) ? 0.0 : v;
    }
    for (int r = 0; r < nb; r++) {
      double v = bot[(size_t)c * ld + r];
      // tree combines: the bottom tile holds its level-0 V below the
      // diagonal — only its R triangle participates
      S[(size_t)c * 2 * nb + nb + r] = (triu_bot && r > c) ? 0.0 : v;
    }
  }
}

}  // namespace

// ------------------------------------------------------------ CPU chores
static void cpu_geqrt(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  double* A = (double*)t.flows[0].data->pull_to_host();
  Data* td = t.flows[1].data;
  double* T = (double*)td->ensure_host();
  memset(T, 0, td->bytes);
  std::vector<double> tau(a.n);
  cpu_geqrf_kern(a.n, a.n, A, a.ld, tau.data());
  cpu_larft_kern(a.n, a.n, A, a.ld, tau.data(), T, a.ld);
  t.flows[0].data->written_on(false);
  td->written_on(false);
}

static void cpu_unmqr(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const double* V = (const double*)t.flows[0].data->pull_to_host();
  const double* T = (const double*)t.flows[1].data->pull_to_host();
  double* C = (double*)t.flows[2].data->pull_to_host();
  cpu_larfb_kern(a.m, a.n, a.m, V, a.ld, T, a.ld, C, a.ld);
  t.flows[2].data->written_on(false);
}

static void cpu_tsqrt(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const int nb = a.n, ld = a.ld;
  double* Akk = (double*)t.flows[0].data->pull_to_host();
  double* Amk = (double*)t.flows[1].data->pull_to_host();
  Data* vd = t.flows[2].data;
  Data* td = t.flows[3].data;
  double* V2 = (double*)vd->ensure_host();
  double* T1 = (double*)td->ensure_host();
  memset(T1, 0, td->bytes);
  stack_tiles(V2, Akk, true, Amk, a.k != 0, nb, ld);
  std::vector<double> tau(nb);
  cpu_geqrf_kern(2 * nb, nb, V2, 2 * nb, tau.data());
  cpu_larft_kern(2 * nb, nb, V2, 2 * nb, tau.data(), T1, ld);
  // R update: upper triangle back into Akk
  for (int c = 0; c < nb; c++)
    for (int r = 0; r <= c; r++)
      Akk[(size_t)c * ld + r] = V2[(size_t)c * 2 * nb + r];
  t.flows[0].data->written_on(false);
  t.flows[1].data->written_on(false);
  vd->written_on(false);
  td->written_on(false);
}

static void cpu_tsmqr(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const int nb = a.m, cols = a.n, ld = a.ld;
  const double* V2 = (const double*)t.flows[0].data->pull_to_host();
  const double* T1 = (const double*)t.flows[1].data->pull_to_host();
  double* Ckn = (double*)t.flows[2].data->pull_to_host();
  double* Cmn = (double*)t.flows[3].data->pull_to_host();
  std::vector<double> S((size_t)2 * nb * cols);
  for (int c = 0; c < cols; c++) {
    memcpy(&S[(size_t)c * 2 * nb], &Ckn[(size_t)c * ld], nb * 8);
    memcpy(&S[(size_t)c * 2 * nb + nb], &Cmn[(size_t)c * ld], nb * 8);
  }
  cpu_larfb_kern(2 * nb, cols, nb, V2, 2 * nb, T1, ld, S.data(), 2 * nb);
  for (int c = 0; c < cols; c++) {
    memcpy(&Ckn[(size_t)c * ld], &S[(size_t)c * 2 * nb], nb * 8);
    memcpy(&Cmn[(size_t)c * ld], &S[(size_t)c * 2 * nb + nb], nb * 8);
  }
  t.flows[2].data->written_on(false);
  t.flows[3].data->written_on(false);
}

// ------------------------------------------------------------ GPU chores
namespace {

__global__ void k_qr_fill(double* p, size_t n, uint32_t seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint64_t h = i * 0x9E3779B97F4A7C15ull + seed;
    h ^= h >> 13;
    h *= 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
    p[i] = (double)(h & 0xFFFFFF) / (double)0x1000000 - 0.5;
  }
}

// Slots of qr_scratch: one growing device buffer per (stream, slot). Every
// user of a slot enqueues on the stream that keys it, so two users of one
// slot are ordered by the stream and the second finds the first one's work
// done. That is all that makes the shared slots below safe.
enum QrSlot {
  QR_SLOT_TAU = 0,       // tau of the tile (hand and rocSOLVER routes)
  QR_SLOT_V = 1,         // unit-lower V for G = V^T V; also TSMQR's stacked S
  QR_SLOT_G128 = 2,      // G of one 128-column panel
  QR_SLOT_T128 = 3,      // T of one 128-column panel
  QR_SLOT_LARFB = 4,     // larfb_gemm's V, W, W2 (4, 5, 6): panels and UNMQR
  QR_SLOT_G = 7,         // G over all k columns
  QR_SLOT_X = 8,         // blocked T combine
  QR_SLOT_T16S = 9,      // the panel kernel's 16x16 T blocks
  QR_SLOT_CNT = 10,      // the panel kernel's publish/ack counters
  // TSMQR's larfb_gemm (8, 9, 10) shares X, T16S and CNT on purpose: a
  // factorization and a TSMQR never overlap on one stream.
  QR_SLOT_LARFB_TS = 8,
};

double* qr_scratch(GpuTaskCtx& g, int slot, size_t bytes) {
  static thread_local std::map<std::pair<void*, int>,
                               std::pair<void*, size_t>> bufs;
  auto& e = bufs[{(void*)g.stream, slot}];
  if (e.second < bytes) {
    // the old buffer may still be referenced by earlier kernels on this
    // stream: return it to the pool only after this task retires
    if (e.first) g.deferred_frees->emplace_back(e.first, e.second);
    if (g.engine) {
      e.first = g.engine->dev_alloc(bytes);
    } else {
      PA_HIP_CHECK(hipMalloc(&e.first, bytes));  // standalone micro-bench
    }
    e.second = bytes;
  }
  return (double*)e.first;
}

__global__ void k_stack_triu(double* S, const double* top, const double* bot,
                             int nb, int ld, int triu_bot) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int total = nb * nb;
  for (; idx < total; idx += gridDim.x * blockDim.x) {
    int c = idx / nb, r = idx - c * nb;
    double v = top[(size_t)c * ld + r];
    S[(size_t)c * 2 * nb + r] = (r > c) ? 0.0 : v;
    double w = bot[(size_t)c * ld + r];
    S[(size_t)c * 2 * nb + nb + r] = (triu_bot && r > c) ? 0.0 : w;
  }
}

__global__ void k_stack(double* S, const double* top, const double* bot,
                        int nb, int cols, int ld) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int total = nb * cols;
  for (; idx < total; idx += gridDim.x * blockDim.x) {
    int c = idx / nb, r = idx - c * nb;
    S[(size_t)c * 2 * nb + r] = top[(size_t)c * ld + r];
    S[(size_t)c * 2 * nb + nb + r] = bot[(size_t)c * ld + r];
  }
}

__global__ void k_unstack(const double* S, double* top, double* bot, int nb,
                          int cols, int ld) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int total = nb * cols;
  for (; idx < total; idx += gridDim.x * blockDim.x) {
    int c = idx / nb, r = idx - c * nb;
    top[(size_t)c * ld + r] = S[(size_t)c * 2 * nb + r];
    bot[(size_t)c * ld + r] = S[(size_t)c * 2 * nb + nb + r];
  }
}

__global__ void k_copy_triu(double* dst, const double* src, int nb, int lds,
                            int ldd) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int total = nb * nb;
  for (; idx < total; idx += gridDim.x * blockDim.x) {
    int c = idx / nb, r = idx - c * nb;
    if (r <= c) dst[(size_t)c * ldd + r] = src[(size_t)c * lds + r];
  }
}

inline dim3 grid1d(int total) {
  int g = (total + 255) / 256;
  return dim3(g > 2048 ? 2048 : g);
}

}  // namespace

__global__ void k_unitlow(double* V, const double* A, int m, int k, int lda,
                          int ldv) {
  // V = unit-lower copy of A's reflector block (zeros above, 1 on diag)
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int total = m * k;
  for (; idx < total; idx += gridDim.x * blockDim.x) {
    int c = idx / m, r = idx - c * m;
    double v = r < c ? 0.0 : (r == c ? 1.0 : A[(size_t)c * lda + r]);
    V[(size_t)c * ldv + r] = v;
  }
}

// C = (I - V T V^T)^T C via three full-rate dgemms (rocSOLVER's dlarfb
// decomposes into micro-kernels at these sizes: profiles/RESULTS.md).
// V: m x k reflectors (unit-lower inside A-storage), T: k x k upper
// (zeros elsewhere), C: m x n. Scratch: V expanded, W and W2 (k x n) in the
// three slots from `slot` on.
static void larfb_gemm(GpuTaskCtx& g, int m, int n, int k, const double* A,
                       int lda, const double* T, int ldt, double* C, int ldc,
                       QrSlot slot) {
  rocblas_handle h = blas_handle(g);
  double* V = qr_scratch(g, slot, (size_t)m * k * 8);
  double* W = qr_scratch(g, slot + 1, (size_t)k * n * 8);
  hipLaunchKernelGGL(k_unitlow, grid1d(m * k), dim3(256), 0, g.stream, V, A,
                     m, k, lda, m);
  const double one = 1.0, zero = 0.0, mone = -1.0;
  // W = V^T C
  PA_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_transpose,
                              rocblas_operation_none, k, n, m, &one, V, m, C,
                              ldc, &zero, W, k));
  // W = T^T W  (T upper-triangular, stored dense with zero lower)
  double* W2 = qr_scratch(g, slot + 2, (size_t)k * n * 8);
  PA_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_transpose,
                              rocblas_operation_none, k, n, k, &one, T, ldt, W,
                              k, &zero, W2, k));
  // C -= V W2
  PA_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none,
                              m, n, k, &mone, V, m, W2, k, &one, C, ldc));
}

// ---------------------------------------------------------- hand panel QR
// rocSOLVER's dgeqrf at tile sizes runs an unblocked host-synced column
// loop (~350 us of idle per column; profiles/RESULTS.md). These kernels do
// the panel factorization device-side:
//  - k_geqr2: one workgroup factors an (m x 128) panel column-by-column
//    (norm reduce + scale + wave-parallel trailing update, all in-kernel);
//  - T factors come from G = V^T V (one full-rate dgemm) via k_larft_diag
//    (per-128-block upper-triangular recurrence) and a blocked combine
//    (two dgemms per block column).
__global__ void __launch_bounds__(1024) k_geqr2(double* A, int m, int ncols,
                                                int ld, double* tau) {
  __shared__ double red[1024];
  __shared__ double bc[3];  // beta, tau_j, scal
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = 0; j < ncols; j++) {
    // 1) norm^2 of the sub-diagonal part of column j
    double acc = 0;
    for (int i = j + 1 + tid; i < m; i += 1024) {
      double v = A[(size_t)j * ld + i];
      acc += v * v;
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) {
      double alpha = A[(size_t)j * ld + j];
      double nrm2 = red[0];
      if (nrm2 == 0.0) {
        bc[0] = alpha;
        bc[1] = 0.0;
        bc[2] = 0.0;
        tau[j] = 0.0;
      } else {
        double beta = -copysign(sqrt(alpha * alpha + nrm2), alpha);
        bc[0] = beta;
        bc[1] = (beta - alpha) / beta;
        bc[2] = 1.0 / (alpha - beta);
        tau[j] = bc[1];
      }
    }
    __syncthreads();
    const double tau_j = bc[1], scal = bc[2];
    if (tau_j != 0.0) {
      for (int i = j + 1 + tid; i < m; i += 1024)
        A[(size_t)j * ld + i] *= scal;
      if (tid == 0) A[(size_t)j * ld + j] = bc[0];
    }
    __syncthreads();
    if (tau_j != 0.0) {
      // 2) apply H_j to trailing columns, one wave per column round-robin
      for (int c = j + 1 + wave; c < ncols; c += 16) {
        double dot = (lane == 0) ? A[(size_t)c * ld + j] : 0.0;
        for (int i = j + 1 + lane; i < m; i += 64)
          dot += A[(size_t)j * ld + i] * A[(size_t)c * ld + i];
        for (int s = 32; s > 0; s >>= 1) dot += __shfl_down(dot, s);
        dot = __shfl(dot, 0);
        double w = tau_j * dot;
        if (lane == 0) A[(size_t)c * ld + j] -= w;
        for (int i = j + 1 + lane; i < m; i += 64)
          A[(size_t)c * ld + i] -= w * A[(size_t)j * ld + i];
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------- multi-WG panel QR
// One LAUNCH factors a whole 128-column panel (vs k_geqr2's one-WG column
// loop at 0.7 TF, profiles/RESULTS.md) as a producer/consumer pipeline
// with no grid-wide barrier:
//  - WG 0 factors 16-column sub-panels held in LDS (norm reduce + rank-1
//    updates never leave the CU; one barrier per column, piggybacked norms,
//    deferred scaling), builds the 16x16 T block from a parallel
//    G = V^T V, then PUBLISHES the sub-panel: cnt[0] = si + 1.
//  - helper pool A (WGs 1..nA) applies each published block reflector to
//    the remaining FACTOR columns and ACKS: cnt[1] += 1. WG 0 only stages
//    sub-panel s+1 after ack(s), so the factor chain never waits on the
//    trailing matrix.
//  - pool B (the rest) streams the same applies over the trailing columns
//    asynchronously, in publication order (each column has a fixed owner,
//    so per-column apply order is the program order).
// Memory protocol per MI355X_MICROARCH.md "Workgroup dispatch": plain
// stores -> release fence + vmcnt(0) asm -> relaxed counter; consumers
// poll relaxed, acquire-fence once, then plain loads. Waiters spin, so all
// nwg workgroups must be resident at once (QR_PANEL_MAX_WGS).
//
// A two-segment row map skips the structurally-zero block of stacked
// [R (upper-tri); B] TSQRT tiles, capping active rows at top_block + B
// regardless of the panel offset.
// LDS budget: rows * W * 8 <= 147456 (W=16 up to 1152 rows, W=8 to 2304).
namespace {

#define QR_DEV __device__ __forceinline__

constexpr int QR_LDS_DOUBLES = 18432;  // 144 KiB panel + ~8 KiB reduction
constexpr int QR_MAX_ROWS_W16 = 1152;
constexpr int QR_MAX_ROWS_W8 = 2304;
// T16s holds one 16x16 block per sub-panel: a 128-column panel is 8
// sub-panels at W=16 and 16 at W=8.
constexpr int QR_MAX_SUBPANELS = 16;

// Row map: local row r < len0 -> global base0 + r ; else base1 + (r-len0).
struct QrRowMap {
  int base0, len0, base1, len1;
  __host__ __device__ int rows() const { return len0 + len1; }
  QR_DEV int global_row(int r) const {
    return r < len0 ? base0 + r : base1 + (r - len0);
  }
  // Global column gcol as two pointers, BOTH indexed by local row: seg0[r]
  // for r < len0, seg1[r] for r >= len0.
  QR_DEV double* seg0(double* A, int ld, int gcol) const {
    return A + (size_t)gcol * ld + base0;
  }
  QR_DEV double* seg1(double* A, int ld, int gcol) const {
    return A + (size_t)gcol * ld + base1 - len0;
  }
};

struct QrPanelArgs {
  double* A;
  int ld;
  int pcol0;     // panel base column (global)
  QrRowMap rm;   // reflector row segments
  int pc;        // total columns from pcol0 (factor + apply targets)
  int fcols;     // columns to FACTOR (<=128)
  int W;         // sub-panel width (8|16)
  double* tau;   // of the panel's columns
  double* T16s;  // 16x16 per sub-panel
  int* cnt;      // [0] sub-panels published, [1] pool A acks
  int nwg, nA, amode, look;
  unsigned long long* dbg;  // phase timers (bench_qr_factor), or null
};

// Householder parameters of a column with diagonal entry alpha and squared
// norm nrm2 below it: the unscaled reflector is (vd, x), beta replaces
// alpha, and tfac = tau / vd^2 applies it before the deferred scaling.
struct QrHouse {
  double vd, beta, tfac, tau;
};
QR_DEV QrHouse qr_house(double alpha, double nrm2) {
  QrHouse h{1.0, alpha, 0.0, 0.0};
  if (nrm2 != 0.0) {
    h.beta = -copysign(sqrt(alpha * alpha + nrm2), alpha);
    h.vd = alpha - h.beta;
    h.tau = (h.beta - alpha) / h.beta;
    h.tfac = h.tau / (h.vd * h.vd);
  }
  return h;
}

// Release side, one lane: what this workgroup stored before its last
// barrier is visible to whoever then reads the counter.
QR_DEV void qr_release() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
QR_DEV void qr_publish(int* cnt, int value) {
  qr_release();
  __hip_atomic_store(cnt, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
QR_DEV void qr_signal_add(int* cnt) {
  qr_release();
  __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Acquire side, one lane; the caller's barrier then lets the others read.
QR_DEV void qr_wait_ge(int* cnt, int value) {
  while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <
         value)
    __builtin_amdgcn_s_sleep(2);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// Phase timer of bench_qr_factor's timed mode: lap(slot) adds the ticks
// since the previous lap to dbg[slot]. A no-op when dbg is null.
struct QrTimer {
  unsigned long long* dbg;
  unsigned long long t0;
  QR_DEV explicit QrTimer(unsigned long long* d)
      : dbg(d), t0(d ? __builtin_amdgcn_s_memrealtime() : 0) {}
  QR_DEV void lap(int slot) {
    if (!dbg) return;
    unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    dbg[slot] += t1 - t0;
    t0 = t1;
  }
};

typedef double f64x4q __attribute__((ext_vector_type(4)));

// One thread's view of the panel kernel: the launch arguments, the shared
// arrays (declared in k_qr_panel_mw), its ids, and the current sub-panel.
struct QrPanel : QrPanelArgs {
  double* sp;   // sub-panel / V image
  double* red;  // norm partials (staging)
  double* bcs;  // per-col {vd, beta, tfac}
  double* tl;   // per-col tau (LDS copy)
  double* wy;   // dots + y for 4 columns
  double* gt;   // G (16x16) + local T (16x16)
  int tid, wave, lane;
  int len0, rows;
  int c0, w;    // first column and width of sub-panel si
  double* T16;  // its T block

  QR_DEV int subpanels() const { return (fcols + W - 1) / W; }
  QR_DEV void select(int si) {
    c0 = si * W;
    w = min(W, fcols - c0);
    T16 = T16s + (size_t)si * 256;
  }
  QR_DEV void set_house(int j, const QrHouse& h) {
    bcs[3 * j] = h.vd;
    bcs[3 * j + 1] = h.beta;
    bcs[3 * j + 2] = h.tfac;
    tl[j] = h.tau;
    tau[c0 + j] = h.tau;
  }

  // ------------------------------------------------------------- WG 0
  // Step 1: stage the sub-panel's columns into LDS, reducing the first
  // column's norm on the way; thread 0 sets up that column's reflector.
  QR_DEV void stage() {
    double acc0 = 0;
    for (int q = 0; q < w; q++) {
      const double* A0 = rm.seg0(A, ld, pcol0 + c0 + q);
      const double* A1 = rm.seg1(A, ld, pcol0 + c0 + q);
      double* spq = sp + (size_t)q * rows;
      for (int r = tid; r < len0; r += 1024) {
        double v = A0[r];
        spq[r] = v;
        if (q == 0 && r > c0) acc0 += v * v;
      }
      for (int r = len0 + tid; r < rows; r += 1024) {
        double v = A1[r];
        spq[r] = v;
        if (q == 0) acc0 += v * v;
      }
    }
    for (int sh = 32; sh > 0; sh >>= 1) acc0 += __shfl_down(acc0, sh);
    if (lane == 0) red[wave] = acc0;
    __syncthreads();
    if (tid == 0) {
      double nrm2 = 0;
      for (int v = 0; v < 16; v++) nrm2 += red[v];
      set_house(0, qr_house(sp[c0], nrm2));
    }
    __syncthreads();
  }

  // Step 2: the column loop, one barrier per column. Wave q > j applies
  // reflector j to column q; wave j + 1 reduces the next column's norm
  // while it updates it, and sets up reflector j + 1.
  QR_DEV void factor_columns() {
    for (int j = 0; j < w; j++) {
      const int d = c0 + j;
      const double vd = bcs[3 * j], tfac = bcs[3 * j + 2];
      if (wave > j && wave < w) {
        const double* col = sp + (size_t)j * rows;
        double* cc = sp + (size_t)wave * rows;
        double dot = (lane == 0) ? vd * cc[d] : 0.0;
        double dot1 = 0.0;
        for (int i = d + 1 + lane; i < rows; i += 128) dot += col[i] * cc[i];
        for (int i = d + 65 + lane; i < rows; i += 128)
          dot1 += col[i] * cc[i];
        dot += dot1;
        for (int sh = 32; sh > 0; sh >>= 1) dot += __shfl_down(dot, sh);
        dot = __shfl(dot, 0);
        const double wj = tfac * dot;
        if (lane == 0) cc[d] -= wj * vd;
        double nacc = 0;
        const bool mine = (wave == j + 1);
        for (int i = d + 1 + lane; i < rows; i += 64) {
          double nv = cc[i] - wj * col[i];
          cc[i] = nv;
          if (mine && i > d + 1) nacc += nv * nv;
        }
        if (mine) {
          for (int sh = 32; sh > 0; sh >>= 1) nacc += __shfl_down(nacc, sh);
          if (lane == 0) set_house(j + 1, qr_house(cc[d + 1], nacc));
        }
      }
      __syncthreads();
    }
  }

  // Step 3: the deferred scaling (v = x / vd, beta on the diagonal), then
  // the factored columns go back to global memory.
  QR_DEV void scale_writeback() {
    if (wave < w) {
      const int d = c0 + wave;
      double* col = sp + (size_t)wave * rows;
      const double inv = 1.0 / bcs[3 * wave];
      for (int i = d + 1 + lane; i < rows; i += 64) col[i] *= inv;
      if (lane == 0) col[d] = bcs[3 * wave + 1];
    }
    __syncthreads();
    for (int q = 0; q < w; q++) {
      double* A0 = rm.seg0(A, ld, pcol0 + c0 + q);
      double* A1 = rm.seg1(A, ld, pcol0 + c0 + q);
      const double* spq = sp + (size_t)q * rows;
      for (int r = tid; r < len0; r += 1024) A0[r] = spq[r];
      for (int r = len0 + tid; r < rows; r += 1024) A1[r] = spq[r];
    }
    __syncthreads();
  }

  // Step 4: G = V^T V by 64 units of 16 lanes over the (sc < q) pairs, then
  // wave 0 runs the T recurrence in LDS and writes the 16x16 block out.
  QR_DEV void build_t16() {
    const int unit = wave * 4 + (lane >> 4), l16 = lane & 15;
    const int npairs = w * (w - 1) / 2;
    for (int idx = unit; idx < npairs; idx += 64) {
      // decode idx -> (sq pair): q = row in triangle
      int q = 1;
      int rem = idx;
      while (rem >= q) {
        rem -= q;
        q++;
      }
      int sc = rem;  // 0 <= sc < q
      const int dq = c0 + q;
      const double* cs = sp + (size_t)sc * rows;
      const double* cq = sp + (size_t)q * rows;
      // i >= dq > ds always: v_s = cs[i]; v_q = 1 at dq, cq[i] below
      double dot = (l16 == 0) ? cs[dq] : 0.0;
      double d1 = 0.0;
      for (int i = dq + 1 + l16; i < rows; i += 32) dot += cs[i] * cq[i];
      for (int i = dq + 17 + l16; i < rows; i += 32) d1 += cs[i] * cq[i];
      dot += d1;
      for (int sh = 8; sh > 0; sh >>= 1) dot += __shfl_down(dot, sh, 16);
      if (l16 == 0) gt[sc * 16 + q] = dot;  // G(sc, q)
    }
    __syncthreads();
    if (wave == 0) {
      double* Tl = gt + 256;
      const double* G = gt;
      for (int j = 0; j < w; j++) {
        double tj = tl[j];
        double sacc = 0;
        if (lane < j) {
          for (int q = lane; q < j; q++)
            sacc += Tl[q * 16 + lane] * G[q * 16 + j];
          sacc *= -tj;
        }
        if (lane < j) Tl[j * 16 + lane] = sacc;
        if (lane == j) Tl[j * 16 + j] = tj;
      }
      if (lane < 16)
        for (int j = 0; j < 16; j++)
          T16[j * 16 + lane] =
              (j < w && lane <= j) ? Tl[j * 16 + lane] : 0.0;
    }
    __syncthreads();
  }

  // ------------------------------- VALU apply of the block reflector
  // (I - V T V^T)^T on up to four columns at a time, V read from sp:
  //  1. dots: the 16-lane unit (wave q, group ci) reduces w_q = v_q . C_ci
  //     into wy[ci * 16 + q];
  //  2. y = T^T w into wy[64 + ci * 16 + q];
  //  3. C_ci -= V y, 256 threads per column.
  // Phase 1 sums in a different order on WG 0 and on the helpers, so it
  // stays two functions; phases 2 and 3 are shared.

  // Phase 1 on WG 0's raw sub-panel (R above the diagonal, no unit diagonal
  // stored): start below the diagonal and add the diagonal term by hand.
  // Two partial sums at stride 32.
  QR_DEV void dots_raw(int gcol, int ci) {
    const int l16 = lane & 15, cloc = c0 + wave;
    const double* v = sp + (size_t)wave * rows;
    const double* A0 = rm.seg0(A, ld, gcol);
    const double* A1 = rm.seg1(A, ld, gcol);
    double dot = (l16 == 0) ? A0[cloc] : 0.0;
    double d1 = 0;
    for (int r = cloc + 1 + l16; r < len0; r += 32) dot += v[r] * A0[r];
    for (int r = cloc + 17 + l16; r < len0; r += 32) d1 += v[r] * A0[r];
    for (int r = len0 + l16; r < rows; r += 32) dot += v[r] * A1[r];
    for (int r = len0 + 16 + l16; r < rows; r += 32) d1 += v[r] * A1[r];
    dot += d1;
    for (int sh = 8; sh > 0; sh >>= 1) dot += __shfl_down(dot, sh, 16);
    if (l16 == 0) wy[ci * 16 + wave] = dot;
  }

  // Phase 1 on a helper's unit-lower V image: four partial sums at stride
  // 64.
  QR_DEV void dots_image(int gcol, int ci) {
    const int l16 = lane & 15, cloc = c0 + wave;
    const double* v = sp + (size_t)wave * rows;
    const double* A0 = rm.seg0(A, ld, gcol);
    const double* A1 = rm.seg1(A, ld, gcol);
    double d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    for (int r = cloc + l16; r < len0; r += 64) d0 += v[r] * A0[r];
    for (int r = cloc + 16 + l16; r < len0; r += 64) d1 += v[r] * A0[r];
    for (int r = cloc + 32 + l16; r < len0; r += 64) d2 += v[r] * A0[r];
    for (int r = cloc + 48 + l16; r < len0; r += 64) d3 += v[r] * A0[r];
    for (int r = len0 + l16; r < rows; r += 64) d0 += v[r] * A1[r];
    for (int r = len0 + 16 + l16; r < rows; r += 64) d1 += v[r] * A1[r];
    for (int r = len0 + 32 + l16; r < rows; r += 64) d2 += v[r] * A1[r];
    for (int r = len0 + 48 + l16; r < rows; r += 64) d3 += v[r] * A1[r];
    double dot = (d0 + d1) + (d2 + d3);
    for (int sh = 8; sh > 0; sh >>= 1) dot += __shfl_down(dot, sh, 16);
    if (l16 == 0) wy[ci * 16 + wave] = dot;
  }

  // Phases 2 and 3 for nc columns, column i being panel column col(i).
  // RAW_SP: sp is WG 0's raw sub-panel, so the unit-lower mask is applied
  // on the fly in the top segment; a helper's image has it built in.
  template <bool RAW_SP, typename ColOf>
  QR_DEV void apply_finish(int nc, ColOf col) {
    __syncthreads();
    if (tid < 16 * nc) {
      const int q = tid & 15, c = tid >> 4;
      double sacc = 0;
      for (int p2 = 0; p2 <= q; p2++)
        sacc += T16[q * 16 + p2] * wy[c * 16 + p2];
      wy[64 + c * 16 + q] = sacc;
    }
    __syncthreads();
    const int c = tid >> 8, t2 = tid & 255;  // 4 cols x 256 threads
    if (c < nc) {
      double* A0 = rm.seg0(A, ld, pcol0 + col(c));
      double* A1 = rm.seg1(A, ld, pcol0 + col(c));
      const double* y = wy + 64 + c * 16;
      for (int r = c0 + t2; r < len0; r += 256) {
        double sacc = 0;
        for (int q = 0; q < w; q++) {
          double v = sp[(size_t)q * rows + r];
          if (RAW_SP) v = r < c0 + q ? 0.0 : (r == c0 + q ? 1.0 : v);
          sacc += v * y[q];
        }
        A0[r] -= sacc;
      }
      for (int r = len0 + t2; r < rows; r += 256) {
        double sacc = 0;
        for (int q = 0; q < w; q++) sacc += sp[(size_t)q * rows + r] * y[q];
        A1[r] -= sacc;
      }
    }
    __syncthreads();
  }

  // Step 6: apply this block to the NEXT sub-panel's columns, so that pool
  // A's pass over them is off the factor chain.
  QR_DEV void self_apply() {
    const int cend = min(c0 + 2 * W, fcols), ci = lane >> 4;
    for (int c = c0 + w; look && c < cend; c += 4) {
      const int nc = min(4, cend - c);
      if (ci < nc && wave < w) dots_raw(pcol0 + c + ci, ci);
      apply_finish<true>(nc, [=](int i) { return c + i; });
    }
  }

  QR_DEV void run_wg0() {
    for (int si = 0; si < subpanels(); si++) {
      select(si);
      QrTimer tm(tid == 0 ? dbg : nullptr);
      stage();
      tm.lap(1);
      factor_columns();
      tm.lap(2);
      scale_writeback();
      tm.lap(3);
      build_t16();
      tm.lap(4);
      // Step 5: publish sub-panel si, then wait for pool A to finish
      // sub-panel si-1 everywhere: its range [c0-W+2W, fcols) includes OUR
      // self-apply window, and the si-1 reflectors must land on those
      // columns before si's do. The factor of si overlapped pool A's si-1
      // pass, so this wait is the pipeline's only rendezvous. With
      // qr_lookahead=0 the self-apply is off and the wait covers pool A
      // through si instead.
      if (tid == 0) {
        qr_publish(&cnt[0], si + 1);
        qr_wait_ge(&cnt[1], (si + (look ? 0 : 1)) * nA);
      }
      __syncthreads();
      tm.lap(0);
      self_apply();
    }
  }

  // ------------------------------------------------ helper workgroups
  // Cache the scaled V image (unit-lower) of the published sub-panel.
  QR_DEV void build_v_image() {
    for (int q = 0; q < w; q++) {
      const int cloc = c0 + q;
      const double* A0 = rm.seg0(A, ld, pcol0 + cloc);
      const double* A1 = rm.seg1(A, ld, pcol0 + cloc);
      double* spq = sp + (size_t)q * rows;
      for (int r = tid; r < len0; r += 1024)
        spq[r] = r < cloc ? 0.0 : (r == cloc ? 1.0 : A0[r]);
      for (int r = len0 + tid; r < rows; r += 1024) spq[r] = A1[r];
    }
  }

  // Rows [ck, ck + clen) of V into Vc, transposed [r][q] with unit-lower
  // semantics, zero-padded to 256 x 16.
  QR_DEV void stage_v_chunk(int ck, int clen, double* Vc) {
    for (int x = tid; x < 256 * 16; x += 1024) {
      const int q = x >> 8, rr = x & 255;
      const int r = ck + rr;
      double v = 0;
      if (rr < clen && q < w) {
        const int cloc = c0 + q;
        if (r == cloc) {
          v = 1.0;
        } else if (r > cloc) {
          v = A[(size_t)(pcol0 + cloc) * ld + rm.global_row(r)];
        }
      }
      Vc[rr * 16 + q] = v;
    }
  }

  // MFMA block-reflector apply for up to 16 columns cg[0..nc) at once
  // through v_mfma_f64_16x16x4f64, staging 256-row chunks of the V image
  // and of C in LDS carved from sp: W = V^T C and C -= V Y become
  // matrix-core work instead of latency-bound 16-lane dot units
  // (profiles/qr_round2.md headroom note).
  // Layout notes: operands stored [k][m] in LDS ([row*16 + q] for V), MFMA
  // lane map a = A[m=r16][k=ksub], D(row=ksub+4e, col=r16): the repo's fp64
  // GEMM conventions (kernels_hip.cpp).
  __device__ void apply_mfma16(const int* cg, int nc) {
    double* Vc = sp;               // [256][16]
    double* Cc = sp + 256 * 16;    // [256][16]
    double* Wr = sp + 2 * 256 * 16;  // [16 waves][16][16] partial W
    double* Ys = sp + 2 * 256 * 16 + 16 * 256;  // [16][16] col-major [c][q]
    const int r16 = lane & 15, ksub = lane >> 4;

    // ---------------- step A: W = V^T C ----------------
    f64x4q accW = {0, 0, 0, 0};
    for (int ck = 0; ck < rows; ck += 256) {
      const int clen = min(256, rows - ck);
      stage_v_chunk(ck, clen, Vc);
      // stage C chunk ([r][c], zero pad)
      for (int x = tid; x < 256 * 16; x += 1024) {
        const int c = x >> 8, rr = x & 255;
        double v = 0;
        if (rr < clen && c < nc)
          v = A[(size_t)(pcol0 + cg[c]) * ld + rm.global_row(ck + rr)];
        Cc[rr * 16 + c] = v;
      }
      __syncthreads();
      // wave `wave` covers k-rows [wave*16, wave*16+16) of this chunk
      const int k0 = wave * 16;
#pragma unroll
      for (int kk = 0; kk < 16; kk += 4) {
        double a = Vc[(k0 + kk + ksub) * 16 + r16];
        double b = Cc[(k0 + kk + ksub) * 16 + r16];
        accW = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, accW, 0, 0, 0);
      }
      __syncthreads();
    }
    // reduce the 16 per-wave W partials, then Y = T^T W
#pragma unroll
    for (int e = 0; e < 4; e++)
      Wr[wave * 256 + (ksub + 4 * e) * 16 + r16] = accW[e];
    __syncthreads();
    if (tid < 256) {
      const int q = tid & 15, c = tid >> 4;
      double wsum = 0;
      for (int wv = 0; wv < 16; wv++) wsum += Wr[wv * 256 + q * 16 + c];
      // W(q, c) lands in [q][c] at the front of Wr: a word that only this
      // thread reads in this step
      Wr[q * 16 + c] = wsum;
    }
    __syncthreads();
    if (tid < 256) {
      const int q = tid & 15, c = tid >> 4;
      double y = 0;
      for (int p2 = 0; p2 <= q; p2++) y += T16[q * 16 + p2] * Wr[p2 * 16 + c];
      Ys[(q)*16 + c] = y;  // Y stored [k=q][c]
    }
    __syncthreads();

    // ---------------- step B: C -= V * Y ----------------
    for (int ck = 0; ck < rows; ck += 256) {
      const int clen = min(256, rows - ck);
      stage_v_chunk(ck, clen, Vc);
      __syncthreads();
      // wave owns the 16-row m-tile [wave*16, wave*16+16) of the chunk
      f64x4q accU = {0, 0, 0, 0};
#pragma unroll
      for (int kk = 0; kk < 16; kk += 4) {
        double a = Vc[(wave * 16 + r16) * 16 + kk + ksub];
        double b = Ys[(kk + ksub) * 16 + r16];
        accU = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, accU, 0, 0, 0);
      }
      // D(row=ksub+4e, col=r16) -> Cc[(wave*16+row)][col]
#pragma unroll
      for (int e = 0; e < 4; e++)
        Cc[(wave * 16 + ksub + 4 * e) * 16 + r16] = accU[e];
      __syncthreads();
      // coalesced global RMW per column
      for (int x = tid; x < 256 * 16; x += 1024) {
        const int c = x >> 8, rr = x & 255;
        const int r = ck + rr;
        if (rr < clen && c < nc && r >= c0)
          A[(size_t)(pcol0 + cg[c]) * ld + rm.global_row(r)] -=
              Cc[rr * 16 + c];
      }
      __syncthreads();
    }
  }

  // Apply the block reflector to this workgroup's share of the panel
  // columns [cbeg, cend): 16 at a time by MFMA, or 4 at a time by the VALU
  // phases on the V image.
  // Column ownership must be ABSOLUTE (c mod stride == phase), not
  // relative to cbeg: cbeg advances with the sub-panel, and a column whose
  // owner changed between sub-panels would receive reflector applies from
  // two helpers with NO mutual ordering (measured: rare mid-panel
  // corruption, first bad column inside pool A's range).
  QR_DEV void apply_range(int cbeg, int cend, int stride, int phase,
                          bool mfma) {
    int first = cbeg + (((phase - cbeg) % stride) + stride) % stride;
    if (amode && mfma) {
      int cg[16];
      int nc = 0;
      for (int c = first; c < cend; c += stride) {
        cg[nc++] = c;
        if (nc == 16) {
          apply_mfma16(cg, 16);
          nc = 0;
        }
      }
      if (nc) apply_mfma16(cg, nc);
      return;
    }
    // wave >= w has no reflector: with W=8 its sp + wave * rows lies past
    // the V image (past sp itself at 2304 rows)
    auto apply4 = [&](const int* cg, int nc) {
      const int ci = lane >> 4;
      if (ci < nc && wave < w) dots_image(pcol0 + cg[ci], ci);
      apply_finish<false>(nc, [=](int i) { return cg[i]; });
    };
    int cg[4];
    int nc = 0;
    for (int c = first; c < cend; c += stride) {
      cg[nc++] = c;
      if (nc == 4) {
        apply4(cg, 4);
        nc = 0;
      }
    }
    if (nc) apply4(cg, nc);
  }

  QR_DEV void run_helper(int wg) {
    const int nB = nwg - 1 - nA;
    const bool poolA = wg <= nA;
    // the first helper of each pool keeps the timers
    const int dslot = (wg == 1) ? 5 : (wg == nA + 1 ? 8 : -1);
    for (int si = 0; si < subpanels(); si++) {
      select(si);
      QrTimer tm((dslot >= 0 && tid == 0) ? dbg : nullptr);
      if (tid == 0) qr_wait_ge(&cnt[0], si + 1);
      __syncthreads();
      tm.lap(dslot);  // publish poll wait
      // the VALU apply reads V from LDS; the MFMA path streams V chunks
      // itself
      if (!amode || poolA) build_v_image();
      __syncthreads();
      tm.lap(dslot + 1);  // V image build
      if (poolA) {
        // small within-panel groups: the latency-optimized VALU units win;
        // the MFMA path pays per-256-row chunk staging regardless of nc
        apply_range(look ? min(c0 + 2 * W, fcols) : c0 + w, fcols, nA,
                    wg - 1, false);
        __syncthreads();
        tm.lap(dslot + 2);  // apply
        if (tid == 0) qr_signal_add(&cnt[1]);
        if (nB == 0)  // no pool B: pool A also covers the trailing columns
          apply_range(fcols, pc, nA, wg - 1, true);
      } else {
        apply_range(fcols, pc, nB, wg - 1 - nA, true);
        tm.lap(dslot + 2);  // apply
      }
    }
  }
};

__global__ void __launch_bounds__(1024) k_qr_panel_mw(QrPanelArgs args) {
  __shared__ double sp[QR_LDS_DOUBLES];
  __shared__ double red[16];
  __shared__ double bcs[3 * 16];
  __shared__ double tl[16];
  __shared__ double wy[2 * 64];
  __shared__ double gt[512];
  const int tid = threadIdx.x;
  QrPanel p{args, sp, red, bcs, tl, wy, gt, tid, tid >> 6, tid & 63,
            args.rm.len0, args.rm.rows(), 0, 0, nullptr};
  if (blockIdx.x == 0)
    p.run_wg0();
  else
    p.run_helper(blockIdx.x);
}

#undef QR_DEV

}  // namespace

// T diag blocks: for block b, columns j: T(0:j,j) = -tau_j T(0:j,0:j) g
// where g = G(blk rows, j) restricted to the block. G is V^T V of the
// unit-lower V; T upper-triangular, T(j,j) = tau_j.
__global__ void __launch_bounds__(128) k_larft_diag(const double* G, int ldg,
                                                    const double* tau,
                                                    double* T, int ldt,
                                                    int k) {
  // The whole 128x128 T block lives in LDS during the column recurrence
  // (global-memory round trips per column made this kernel 1.5 ms and 9%
  // of QR GPU time — gpurun_out/qr_kernel_stats.csv); one barrier per
  // column, write-back once at the end.
  __shared__ double Ts[128 * 128];
  const int b0 = blockIdx.x * 128;
  const int tid = threadIdx.x;  // 128 threads
  const int nb = min(128, k - b0);
  for (int j = 0; j < nb; j++) {
    int gj = b0 + j;
    // col = -tau_j * T(0:j,0:j) * G(b0..b0+j, gj)
    double s = 0;
    if (tid < j) {
      const double* Gc = G + (size_t)gj * ldg + b0;
      for (int q = tid; q < j; q++) s += Ts[q * 128 + tid] * Gc[q];
      s *= -tau[gj];
    }
    if (tid < j) Ts[j * 128 + tid] = s;
    if (tid == j) Ts[j * 128 + j] = tau[gj];
    __syncthreads();
  }
  for (int j = 0; j < nb; j++)
    if (tid <= j) T[(size_t)(b0 + j) * ldt + b0 + tid] = Ts[j * 128 + tid];
}

// The tunables of the panel kernel. The chores and bench_qr_factor fill
// them from the parameters of the same names; test_qr_factor_hip sets them
// per call.
struct QrPanelCfg {
  int nwg = 48;             // qr_panel_wgs: workgroups per panel launch
  int nA = 15;              // qr_panel_poolA: helpers on the panel columns
  int amode = 1;            // qr_apply: 0 = valu helper apply, 1 = MFMA
  bool apply_gemm = false;  // qr_apply=gemm: trailing columns by larfb dgemms
  int look = 1;             // qr_lookahead
  // kernel | valu | gemm; anything else is "kernel"
  void set_apply(const std::string& kind) {
    apply_gemm = kind == "gemm";
    amode = kind == "valu" ? 0 : 1;
  }
  // WG 0 factors, so there is at least one helper, and pool A is never
  // empty: nobody else applies a sub-panel to the panel's own columns. The
  // workgroups wait on each other, so no more than can be resident at once.
  void clamp() {
    nwg = std::min(QR_PANEL_MAX_WGS, std::max(2, nwg));
    nA = std::min(nwg - 1, std::max(1, nA));
  }
};

static QrPanelCfg qr_cfg_from_params() {
  // qr_apply is read once per process, the others on every call
  static const std::string apply_kind = param_str("qr_apply", "kernel");
  QrPanelCfg c;
  c.nwg = (int)param_int("qr_panel_wgs", 48);
  c.nA = (int)param_int("qr_panel_poolA", 15);
  c.look = (int)param_int("qr_lookahead", 1);
  c.set_apply(apply_kind);
  c.clamp();
  return c;
}

// Row map and sub-panel width of the pc-column panel at (p, p) of an m-row
// tile: a dense panel, or with ts_split > 0 the triangular top (pc rows of
// R) plus the dense bottom. W = 0: too many rows for the panel kernel.
struct QrPanelGeom {
  QrRowMap rm;
  int W;
};
static QrPanelGeom qr_panel_geom(int m, int p, int pc, int ts_split) {
  QrRowMap rm{p, m - p, 0, 0};
  if (ts_split > 0)
    rm = {p, std::min(pc, ts_split - p), ts_split, m - ts_split};
  const int rows = rm.rows();
  const int W = rows <= QR_MAX_ROWS_W16 ? 16 : (rows <= QR_MAX_ROWS_W8 ? 8 : 0);
  return {rm, W};
}

// One panel-kernel launch: factor the pc columns at column p of A and apply
// them to the apply_cols columns from p on (the panel's own included).
static void launch_qr_panel(GpuTaskCtx& g, const QrPanelCfg& cfg, double* A,
                            int ld, int p, const QrPanelGeom& geo,
                            int apply_cols, int pc, double* tau,
                            unsigned long long* dbg) {
  double* T16s =
      qr_scratch(g, QR_SLOT_T16S, (size_t)QR_MAX_SUBPANELS * 256 * 8);
  int* cnt = (int*)qr_scratch(g, QR_SLOT_CNT, 256);
  PA_HIP_CHECK(hipMemsetAsync(cnt, 0, 2 * sizeof(int), g.stream));
  const QrPanelArgs a{A, ld, p, geo.rm, /*pc=*/apply_cols, /*fcols=*/pc,
                      geo.W, tau + p, T16s, cnt, cfg.nwg, cfg.nA, cfg.amode,
                      cfg.look, dbg};
  hipLaunchKernelGGL(k_qr_panel_mw, dim3(cfg.nwg), dim3(1024), 0, g.stream,
                     a);
}

// T128 of the factored pc-column panel at (p, p) from G = V^T V, then
// larfb_gemm on the `rest` columns to its right.
static void qr_larfb_trailing(GpuTaskCtx& g, double* A, int m, int ld, int p,
                              int pc, int rest, const double* tau) {
  rocblas_handle h = blas_handle(g);
  const double one = 1.0, zero = 0.0;
  const int prows = m - p;
  double* panel = A + (size_t)p * ld + p;
  double* V = qr_scratch(g, QR_SLOT_V, (size_t)prows * 128 * 8);
  double* G = qr_scratch(g, QR_SLOT_G128, (size_t)128 * 128 * 8);
  hipLaunchKernelGGL(k_unitlow, grid1d(prows * pc), dim3(256), 0, g.stream,
                     V, panel, prows, pc, ld, prows);
  PA_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_transpose,
                              rocblas_operation_none, pc, pc, prows, &one, V,
                              prows, V, prows, &zero, G, pc));
  double* T128 = qr_scratch(g, QR_SLOT_T128, (size_t)128 * 128 * 8);
  PA_HIP_CHECK(hipMemsetAsync(T128, 0, (size_t)pc * pc * 8, g.stream));
  hipLaunchKernelGGL(k_larft_diag, dim3(1), dim3(128), 0, g.stream, G, pc,
                     tau + p, T128, pc, pc);
  larfb_gemm(g, prows, rest, pc, panel, ld, T128, pc,
             A + (size_t)(p + pc) * ld + p, ld, QR_SLOT_LARFB);
}

// Full tile/stacked-panel QR: factor 128-wide panels with the multi-WG
// panel kernel (k_geqr2 single-WG fallback for oversized rows), apply to
// the trailing columns with gemm-larfb, then build the full k x k T.
// ts_split > 0 marks a stacked [R (upper-tri, ts_split rows); B] tile:
// the panel kernel then skips the structurally-zero block below R's
// diagonal band, capping active rows at 128 + (m - ts_split).
static void qr_factor_hand(GpuTaskCtx& g, double* A, int m, int k, int ld,
                           double* T, int ldt, int ts_split,
                           const QrPanelCfg& cfg) {
  rocblas_handle h = blas_handle(g);
  double* tau = qr_scratch(g, QR_SLOT_TAU, (size_t)k * 8);
  const double one = 1.0, zero = 0.0, mone = -1.0;
  PA_HIP_CHECK(hipMemsetAsync(T, 0, (size_t)ldt * k * 8, g.stream));
  for (int p = 0; p < k; p += 128) {
    const int pc = std::min(128, k - p);
    const int rest = k - p - pc;
    const QrPanelGeom geo = qr_panel_geom(m, p, pc, ts_split);
    if (geo.W) {
      // qr_apply=kernel (default): the panel kernel both factors and
      // applies to ALL remaining tile columns (no per-panel dgemms).
      // qr_apply=gemm: the kernel applies within the 128 panel columns
      // only; the trailing matrix goes through T128 + larfb dgemms at
      // Tensile rates (A/B: the in-kernel apply units are latency-bound,
      // profiles/qr_round2.md).
      launch_qr_panel(g, cfg, A, ld, p, geo, cfg.apply_gemm ? pc : k - p, pc,
                      tau, nullptr);
      if (cfg.apply_gemm && rest > 0)
        qr_larfb_trailing(g, A, m, ld, p, pc, rest, tau);
      continue;
    }
    hipLaunchKernelGGL(k_geqr2, dim3(1), dim3(1024), 0, g.stream,
                       A + (size_t)p * ld + p, m - p, pc, ld, tau + p);
    if (rest > 0) qr_larfb_trailing(g, A, m, ld, p, pc, rest, tau);
  }
  // Full T: G = V^T V over all k columns, diag blocks in one launch,
  // off-diagonal blocks by blocked combine (T[0:J,blk] = -T·G·T_blk).
  double* V = qr_scratch(g, QR_SLOT_V, (size_t)m * k * 8);
  double* G = qr_scratch(g, QR_SLOT_G, (size_t)k * k * 8);
  hipLaunchKernelGGL(k_unitlow, grid1d(m * k), dim3(256), 0, g.stream, V, A,
                     m, k, ld, m);
  PA_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_transpose,
                              rocblas_operation_none, k, k, m, &one, V, m, V, m,
                              &zero, G, k));
  hipLaunchKernelGGL(k_larft_diag, dim3((k + 127) / 128), dim3(128), 0,
                     g.stream, G, k, tau, T, ldt, k);
  double* X = qr_scratch(g, QR_SLOT_X, (size_t)k * 128 * 8);
  for (int b = 128; b < k; b += 128) {
    int bc2 = std::min(128, k - b);
    // X = T(0:b,0:b) * G(0:b, b:b+bc)
    PA_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_none,
                                rocblas_operation_none, b, bc2, b, &one, T, ldt,
                                G + (size_t)b * k, k, &zero, X, b));
    // T(0:b, blk) = -X * T_blk
    PA_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_none,
                                rocblas_operation_none, b, bc2, bc2, &mone, X,
                                b, T + (size_t)b * ldt + b, ldt, &zero,
                                T + (size_t)b * ldt, ldt));
  }
}

// The chore_qr=rocsolver route: library dgeqrf, then dlarft for T (t_bytes
// of it are cleared first).
static void qr_factor_rocsolver(GpuTaskCtx& g, double* A, int m, int k,
                                int ld, double* T, int ldt, size_t t_bytes) {
  double* tau = qr_scratch(g, QR_SLOT_TAU, (size_t)k * 8);
  rocblas_handle h = blas_handle(g);
  PA_HIP_CHECK(hipMemsetAsync(T, 0, t_bytes, g.stream));
  PA_BLAS_CHECK(rocsolver_dgeqrf(h, m, k, A, ld, tau));
  PA_BLAS_CHECK(rocsolver_dlarft(h, rocblas_forward_direction,
                                 rocblas_column_wise, m, k, A, ld, tau, T,
                                 ldt));
}

static void gpu_geqrt(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  double* A = (double*)t.dev_ptr[0];
  double* T = (double*)t.dev_ptr[1];
  static const bool use_rocsolver =
      param_str("chore_qr", "hand") == "rocsolver";
  if (!use_rocsolver) {
    qr_factor_hand(g, A, a.n, a.n, a.ld, T, a.ld, 0, qr_cfg_from_params());
    return;
  }
  qr_factor_rocsolver(g, A, a.n, a.n, a.ld, T, a.ld, t.flows[1].data->bytes);
}

static void gpu_unmqr(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  larfb_gemm(g, a.m, a.n, a.m, (const double*)t.dev_ptr[0], a.ld,
             (const double*)t.dev_ptr[1], a.ld, (double*)t.dev_ptr[2], a.ld,
             QR_SLOT_LARFB);
}

static void gpu_tsqrt(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  const int nb = a.n, ld = a.ld;
  double* Akk = (double*)t.dev_ptr[0];
  double* Amk = (double*)t.dev_ptr[1];
  double* V2 = (double*)t.dev_ptr[2];
  double* T1 = (double*)t.dev_ptr[3];
  hipLaunchKernelGGL(k_stack_triu, grid1d(nb * nb), dim3(256), 0, g.stream,
                     V2, Akk, Amk, nb, ld, a.k);
  static const bool use_rocsolver =
      param_str("chore_qr", "hand") == "rocsolver";
  if (!use_rocsolver) {
    qr_factor_hand(g, V2, 2 * nb, nb, 2 * nb, T1, ld, /*ts_split=*/nb,
                   qr_cfg_from_params());
  } else {
    qr_factor_rocsolver(g, V2, 2 * nb, nb, 2 * nb, T1, ld,
                        t.flows[3].data->bytes);
  }
  hipLaunchKernelGGL(k_copy_triu, grid1d(nb * nb), dim3(256), 0, g.stream,
                     Akk, V2, nb, 2 * nb, ld);
}

static void gpu_tsmqr(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  const int nb = a.m, cols = a.n, ld = a.ld;
  double* V2 = (double*)t.dev_ptr[0];
  double* T1 = (double*)t.dev_ptr[1];
  double* Ckn = (double*)t.dev_ptr[2];
  double* Cmn = (double*)t.dev_ptr[3];
  double* S = qr_scratch(g, QR_SLOT_V, (size_t)2 * nb * cols * 8);
  hipLaunchKernelGGL(k_stack, grid1d(nb * cols), dim3(256), 0, g.stream, S,
                     Ckn, Cmn, nb, cols, ld);
  larfb_gemm(g, 2 * nb, cols, nb, V2, 2 * nb, T1, ld, S, 2 * nb,
             QR_SLOT_LARFB_TS);
  hipLaunchKernelGGL(k_unstack, grid1d(nb * cols), dim3(256), 0, g.stream, S,
                     Ckn, Cmn, nb, cols, ld);
}

// ------------------------------------------------------------ task classes
TaskClass& tc_geqrt() {
  // rocSOLVER panel factorizations host-sync internally: run them on
  // worker threads (gpu_blocking) so the manager keeps the trailing
  // updates flowing. The hand panel path is fully device-side (multi-WG
  // panel kernel), so it pipelines through the manager like any chore.
  // PARSEC_MCA_qr_blocking_panels=0 restores manager execution.
  static TaskClass tc = [] {
    TaskClass c = make_tc("geqrt", TaskKind::GPU, cpu_geqrt, gpu_geqrt,
                          TC_GEQRT);
    bool rocs = param_str("chore_qr", "hand") == "rocsolver";
    c.gpu_blocking = rocs && param_int("qr_blocking_panels", 1) != 0;
    return c;
  }();
  return tc;
}
TaskClass& tc_unmqr() {
  static TaskClass tc =
      make_tc("unmqr", TaskKind::GPU, cpu_unmqr, gpu_unmqr, TC_UNMQR);
  return tc;
}
TaskClass& tc_tsqrt() {
  static TaskClass tc = [] {
    TaskClass c = make_tc("tsqrt", TaskKind::GPU, cpu_tsqrt, gpu_tsqrt,
                          TC_TSQRT);
    bool rocs = param_str("chore_qr", "hand") == "rocsolver";
    c.gpu_blocking = rocs && param_int("qr_blocking_panels", 1) != 0;
    return c;
  }();
  return tc;
}
TaskClass& tc_tsmqr() {
  static TaskClass tc =
      make_tc("tsmqr", TaskKind::GPU, cpu_tsmqr, gpu_tsmqr, TC_TSMQR);
  return tc;
}

// ------------------------------------------------------------ DAG builder
// The trailing columns of one QR sweep: A's own column tiles and, when a
// right-hand side rides along (insert_gels), B's column tiles after them.
// Trailing column n >= A.nt() is B's column tile n - A.nt(); it keeps that
// index in the priority formulas, so every A column goes first.
namespace {
struct QrTrail {
  TiledMatrix& A;
  TiledMatrix* B;
  int end() const { return A.nt() + (B ? B->nt() : 0); }
  Data* tile(int m, int n) const {
    return n < A.nt() ? A.tile(m, n) : B->tile(m, n - A.nt());
  }
  int rank_of(int m, int n) const {
    return n < A.nt() ? A.rank_of(m, n) : B->rank_of(m, n - A.nt());
  }
  int cols(int n) const {
    return n < A.nt() ? A.nb() : B->tile_cols(n - A.nt());
  }
};
}  // namespace

// Binary TS-reduction tree per panel column (the reference ecosystem's
// HQR trees): every row tile is GEQRT'd independently (level 0), then
// pairs combine through TSQRT/TSMQR with stride-doubling — panel depth
// O(log M) instead of O(M). More total flops than the flat chain (the
// per-row UNMQR applies), but the host-synced panel kernels run
// CONCURRENTLY on blocking workers, which is what bounds QR here.
static void insert_geqrf_tree(Dtd& tp, const QrTrail& tr, TiledMatrix& WT,
                              TiledMatrix& T1, TiledMatrix& V2) {
  TiledMatrix& A = tr.A;
  const int T = A.mt();
  const int nb = A.nb(), ld = A.mb();
  constexpr int PANEL = 1 << 20;
  TileArgs pa_args;
  pa_args.m = nb;
  pa_args.n = nb;
  pa_args.ld = ld;
  for (int k = 0; k < A.nt(); k++) {
    // level 0: factor every row tile of the column, apply across its row
    for (int m = k; m < T; m++) {
      Dtd::FlowSpec f[] = {{A.tile(m, k), ACCESS_INOUT},
                           {WT.tile(m, k), ACCESS_OUT}};
      tp.insert(&tc_geqrt(), &pa_args, sizeof(pa_args), f, 2, PANEL + 1,
                A.rank_of(m, k));
      for (int n = k + 1; n < tr.end(); n++) {
        TileArgs ua = pa_args;
        ua.n = tr.cols(n);
        Dtd::FlowSpec fu[] = {{A.tile(m, k), ACCESS_IN},
                              {WT.tile(m, k), ACCESS_IN},
                              {tr.tile(m, n), ACCESS_INOUT}};
        tp.insert(&tc_unmqr(), &ua, sizeof(ua), fu, 3, (1 << 18) - (n - k),
                  tr.rank_of(m, n));
      }
    }
    // reduction tree: combine (a, a+step) pairs, doubling the stride
    for (int step = 1; k + step < T; step *= 2) {
      for (int a = k; a + step < T; a += 2 * step) {
        const int b = a + step;
        {
          TileArgs ta = pa_args;
          ta.k = 1;  // bottom tile participates by its R triangle only
          Dtd::FlowSpec f[] = {{A.tile(a, k), ACCESS_INOUT},
                               {A.tile(b, k), ACCESS_INOUT},
                               {V2.tile(b, k), ACCESS_OUT},
                               {T1.tile(b, k), ACCESS_OUT}};
          tp.insert(&tc_tsqrt(), &ta, sizeof(ta), f, 4, PANEL,
                    A.rank_of(b, k));
        }
        for (int n = k + 1; n < tr.end(); n++) {
          TileArgs ua = pa_args;
          ua.n = tr.cols(n);
          Dtd::FlowSpec f[] = {{V2.tile(b, k), ACCESS_IN},
                               {T1.tile(b, k), ACCESS_IN},
                               {tr.tile(a, n), ACCESS_INOUT},
                               {tr.tile(b, n), ACCESS_INOUT}};
          tp.insert(&tc_tsmqr(), &ua, sizeof(ua), f, 4, -(n - k) * 4,
                    tr.rank_of(b, n));
        }
      }
    }
  }
}

// The QR sweep of A (M >= N, whole square tiles) over k < A.nt(), m < A.mt().
// With B, its column tiles are trailing columns too and end up holding
// Q^T B. For square A without B this inserts what insert_geqrf always did:
// the same tasks in the same order with the same priorities and ranks.
static void insert_qr_sweep(Dtd& tp, TiledMatrix& A, TiledMatrix* B) {
  const QrTrail tr{A, B};
  const int T = A.mt();
  const int nb = A.nb(), ld = A.mb();
  constexpr int PANEL = 1 << 20;
  auto* ctx = A.ctx();
  auto WT = std::make_shared<TiledMatrix>(ctx, A.m(), A.n(), nb, nb,
                                          A.grid_p(), A.grid_q());
  auto T1 = std::make_shared<TiledMatrix>(ctx, A.m(), A.n(), nb, nb,
                                          A.grid_p(), A.grid_q());
  auto V2 = std::make_shared<TiledMatrix>(ctx, (int64_t)2 * A.m(), A.n(),
                                          2 * nb, nb, A.grid_p(), A.grid_q());
  tp.own(WT);
  tp.own(T1);
  tp.own(V2);
  if (param_str("qr_tree", "flat") == "binary") {
    insert_geqrf_tree(tp, tr, *WT, *T1, *V2);
    return;
  }
  for (int k = 0; k < A.nt(); k++) {
    TileArgs pa_args;
    pa_args.m = nb;
    pa_args.n = nb;
    pa_args.ld = ld;
    {
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_INOUT},
                           {WT->tile(k, k), ACCESS_OUT}};
      tp.insert(&tc_geqrt(), &pa_args, sizeof(pa_args), f, 2, PANEL + 1,
                A.rank_of(k, k));
    }
    for (int n = k + 1; n < tr.end(); n++) {
      TileArgs ua = pa_args;
      ua.n = tr.cols(n);
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_IN},
                           {WT->tile(k, k), ACCESS_IN},
                           {tr.tile(k, n), ACCESS_INOUT}};
      tp.insert(&tc_unmqr(), &ua, sizeof(ua), f, 3, (1 << 18) - (n - k),
                tr.rank_of(k, n));
    }
    for (int m = k + 1; m < T; m++) {
      {
        Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_INOUT},
                             {A.tile(m, k), ACCESS_INOUT},
                             {V2->tile(m, k), ACCESS_OUT},
                             {T1->tile(m, k), ACCESS_OUT}};
        tp.insert(&tc_tsqrt(), &pa_args, sizeof(pa_args), f, 4, PANEL,
                  A.rank_of(m, k));
      }
      for (int n = k + 1; n < tr.end(); n++) {
        TileArgs ua = pa_args;
        ua.n = tr.cols(n);
        Dtd::FlowSpec f[] = {{V2->tile(m, k), ACCESS_IN},
                             {T1->tile(m, k), ACCESS_IN},
                             {tr.tile(k, n), ACCESS_INOUT},
                             {tr.tile(m, n), ACCESS_INOUT}};
        tp.insert(&tc_tsmqr(), &ua, sizeof(ua), f, 4, -(n - k) * 4,
                  tr.rank_of(m, n));
      }
    }
  }
}

// Tall A (M >= N) is accepted: the sweep runs over A.nt() panel columns and
// A.mt() row tiles, and R ends up in the upper tiles of the first A.nt()
// tile rows.
void insert_geqrf(Dtd& tp, TiledMatrix& A) {
  PA_CHECK(A.m() % A.nb() == 0 && A.n() % A.nb() == 0 && A.mb() == A.nb() &&
               A.m() >= A.n(),
           "insert_geqrf: M >= N, both multiples of the (square) tile size");
  insert_qr_sweep(tp, A, nullptr);
}

// Householder least squares / solve (LAPACK dgels, M >= N, full column
// rank) without keeping Q: B's column tiles ride through the QR sweep of A as
// extra trailing columns and receive Q^T B, then one backward sweep with R
// leaves X in B's first N rows. Rows [N, M) of B keep the part of Q^T B
// orthogonal to range(A): its column norms are the residual norms. The
// diagonal solves are true triangular solves, as this entry point is the
// one for ill-conditioned input.
void insert_gels(Dtd& tp, TiledMatrix& A, TiledMatrix& B) {
  PA_CHECK(A.mb() == A.nb(), "insert_gels: A needs square tiles, got %d x %d",
           A.mb(), A.nb());
  PA_CHECK(A.m() % A.nb() == 0 && A.n() % A.nb() == 0,
           "insert_gels: M and N must be multiples of the tile size %d",
           A.nb());
  PA_CHECK(A.m() >= A.n(), "insert_gels: M >= N (overdetermined or square)");
  PA_CHECK(B.mb() == A.mb() && B.mt() == A.mt(),
           "insert_gels: B must have A's row tiling (mb %d, mt %d)", A.mb(),
           A.mt());
  PA_CHECK(A.elem_size() == 8 && B.elem_size() == 8 && A.ctx() == B.ctx(),
           "insert_gels: fp64 matrices of one context");
  insert_qr_sweep(tp, A, &B);
  // backward: R X = (Q^T B)[0:N], R upper non-unit
  for (int j = 0; j < B.nt(); j++)
    insert_tri_sweep(tp, A, A.nt(), B, j, /*upper=*/true, /*trans=*/false,
                     /*unit=*/false);
}

// Standalone micro-benchmark of the TS/tile panel factorization path, by
// QrBenchMode. Returns seconds for `iters` factorizations of an m x k tile.
double bench_qr_factor(int m, int k, int ts_split, int iters, int mode) {
  PA_CHECK(mode == QR_BENCH_FULL || mode == QR_BENCH_PANELS ||
               mode == QR_BENCH_ROCSOLVER || mode == QR_BENCH_PANELS_TIMED,
           "bench_qr_factor: mode %d", mode);
  DevArray dA((size_t)m * k), dT((size_t)k * k);
  DevArray<unsigned long long> dbg(16);
  PA_HIP_CHECK(hipMemset(dbg.p, 0, dbg.bytes));
  const bool timed = mode == QR_BENCH_PANELS_TIMED;
  hipStream_t s;
  PA_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  std::vector<std::pair<void*, size_t>> defer;
  GpuTaskCtx g{s, 0, nullptr, &defer};
  double* tau = qr_scratch(g, QR_SLOT_TAU, (size_t)k * 8);
  const QrPanelCfg cfg = qr_cfg_from_params();
  double dt = time_launches(iters, [&] {
    hipLaunchKernelGGL(k_qr_fill, dim3(2048), dim3(256), 0, s, dA.p,
                       (size_t)m * k, 7);
    if (mode == QR_BENCH_FULL) {
      qr_factor_hand(g, dA.p, m, k, m, dT.p, k, ts_split, cfg);
    } else if (mode == QR_BENCH_ROCSOLVER) {
      PA_BLAS_CHECK(rocsolver_dgeqrf(blas_handle(g), m, k, dA.p, m, tau));
    } else {
      for (int p = 0; p < k; p += 128) {
        const int pc = std::min(128, k - p);
        const QrPanelGeom geo = qr_panel_geom(m, p, pc, ts_split);
        PA_CHECK(geo.W, "bench: rows too large");
        launch_qr_panel(g, cfg, dA.p, m, p, geo, k - p, pc, tau,
                        timed ? dbg.p : nullptr);
      }
    }
  }, s);
  if (timed) {
    unsigned long long h[16];
    dbg.download(h);
    const char* names[] = {"wg0 ack-wait", "wg0 stage", "wg0 factor",
                           "wg0 scale+wb", "wg0 G16+T16", "A poll",
                           "A vbuild", "A apply", "B poll", "B vbuild",
                           "B apply"};
    for (int i = 0; i < 11; i++)
      fprintf(stderr, "[qrdbg] %-12s %8.1f us/tile\n", names[i],
              h[i] / 0.1 / (iters + 1));  // 100 MHz ticks
  }
  return dt;
}

// One panel factorization from host buffers, for the tests: A (a_elems
// doubles, column-major with leading dimension lda; what lies past column k
// travels to the device and back untouched) is factored in place, T (k x k,
// leading dimension k) receives the block reflector's triangular factor.
// impl 0 = qr_factor_hand with the tunables the caller overrides (wgs,
// poolA > 0; apply non-empty; lookahead >= 0), 1 = the rocSOLVER route of
// chore_qr=rocsolver, 2 = the CPU chore's kernels (no GPU touched).
void test_qr_factor_hip(double* A, size_t a_elems, int m, int k, int lda,
                        int ts_split, int impl, int wgs, int poolA,
                        const std::string& apply, int lookahead, double* T) {
  if (impl == 2) {
    std::vector<double> tau(k);
    memset(T, 0, (size_t)k * k * 8);
    cpu_geqrf_kern(m, k, A, lda, tau.data());
    cpu_larft_kern(m, k, A, lda, tau.data(), T, k);
    return;
  }
  // one stream per calling thread, kept: qr_scratch and blas_handle key
  // their per-thread state on it
  static thread_local hipStream_t s = nullptr;
  if (!s) PA_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  DevArray dA(a_elems, A), dT((size_t)k * k);
  std::vector<std::pair<void*, size_t>> defer;
  GpuTaskCtx g{s, 0, nullptr, &defer};
  if (impl == 0) {
    QrPanelCfg cfg = qr_cfg_from_params();
    if (wgs > 0) cfg.nwg = wgs;
    if (poolA > 0) cfg.nA = poolA;
    if (!apply.empty()) cfg.set_apply(apply);
    if (lookahead >= 0) cfg.look = lookahead;
    cfg.clamp();
    qr_factor_hand(g, dA.p, m, k, lda, dT.p, k, ts_split, cfg);
  } else {
    qr_factor_rocsolver(g, dA.p, m, k, lda, dT.p, k, (size_t)k * k * 8);
  }
  PA_HIP_CHECK(hipStreamSynchronize(s));
  dA.download(A);
  dT.download(T);
  // scratch that grew during this call was replaced, not freed
  for (auto& d : defer) PA_HIP_CHECK(hipFree(d.first));
}

}  // namespace pa
