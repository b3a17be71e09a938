// The tile chores of the Cholesky factorization and its DAG builder, the
// synthetic SPD fill, and the two generic chores every solve and inverse is
// built from (gemm_nn, trsm_solve). Each class has a library (rocBLAS /
// rocSOLVER) or hand-kernel GPU chore and a CPU reference chore. make_tc,
// through which every kernels_*.cpp builds its classes, lives here too.
//
// CPU chores are straightforward reference implementations used by the
// no-GPU test path (numerics tests compare the HIP path against these / a
// NumPy fp64 reference); the GPU path is the production path.
#include "kernels.hpp"

#include <cmath>
#include <map>
#include <mutex>
#include <string>

#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "device_gpu.hpp"
#include "gpu_blas.hpp"
#include "kernels_bench.hpp"
#include "kernels_hip.hpp"
#include "profiling.hpp"

namespace pa {

// ------------------------------------------------------------------ fill
// Deterministic synthetic SPD matrix: symmetric hash values in [-0.5, 0.5),
// + N on the diagonal (diagonally dominant => positive definite).
__host__ __device__ inline double spd_val(int64_t i, int64_t j, int64_t N,
                                          uint32_t seed) {
  uint64_t a = (uint64_t)(i < j ? i : j), b = (uint64_t)(i < j ? j : i);
  uint64_t h = (a * 2654435761ull) ^ (b * 40503ull) ^
               ((uint64_t)seed * 2246822519ull);
  h ^= h >> 13;
  h *= 0x9E3779B97F4A7C15ull;
  h ^= h >> 32;
  double v = (double)(h & 0xFFFFFF) / (double)0x1000000 - 0.5;
  return i == j ? v + (double)N : v;
}

__global__ void k_spd_fill(double* t, int rows, int cols, int ld, int64_t i0,
                           int64_t j0, int64_t N, uint32_t seed) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int total = rows * cols;
  for (; idx < total; idx += gridDim.x * blockDim.x) {
    int c = idx / rows, r = idx - c * rows;
    t[(size_t)c * ld + r] = spd_val(i0 + r, j0 + c, N, seed);
  }
}

void launch_spd_fill(double* t, int rows, int cols, int ld, int64_t i0,
                     int64_t j0, int64_t N, uint32_t seed, hipStream_t s) {
  int total = rows * cols;
  int block = 256;
  int grid = std::min((total + block - 1) / block, 4096);
  hipLaunchKernelGGL(k_spd_fill, dim3(grid), dim3(block), 0, s, t, rows, cols,
                     ld, i0, j0, N, seed);
}

static void cpu_spd_fill(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  Data* d = t.flows[0].data;
  double* p = (double*)d->ensure_host();
  for (int c = 0; c < a.n; c++)
    for (int r = 0; r < a.m; r++)
      p[(size_t)c * a.ld + r] = spd_val(a.i0 + r, a.j0 + c, a.N, a.seed);
  d->written_on(false);
}

static void gpu_spd_fill(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  launch_spd_fill((double*)t.dev_ptr[0], a.m, a.n, a.ld, a.i0, a.j0, a.N,
                  a.seed, g.stream);
}

// ------------------------------------------------------------------ CPU chores
// Naive fp64 reference bodies (column-major, ld = tile rows).
static void cpu_potrf(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  double* A = (double*)t.flows[0].data->pull_to_host();
  const int n = a.n, ld = a.ld;
  for (int j = 0; j < n; j++) {
    double d = A[(size_t)j * ld + j];
    for (int k = 0; k < j; k++) d -= A[(size_t)k * ld + j] * A[(size_t)k * ld + j];
    PA_CHECK(d > 0, "potrf: matrix not SPD at column %d", j);
    d = std::sqrt(d);
    A[(size_t)j * ld + j] = d;
    for (int i = j + 1; i < n; i++) {
      double s = A[(size_t)j * ld + i];
      for (int k = 0; k < j; k++) s -= A[(size_t)k * ld + i] * A[(size_t)k * ld + j];
      A[(size_t)j * ld + i] = s / d;
    }
  }
  t.flows[0].data->written_on(false);
}

// B = B * L^{-T}  (right, lower, transposed, non-unit) — TRSM of the tile panel.
static void cpu_trsm(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const double* L = (const double*)t.flows[0].data->pull_to_host();
  double* B = (double*)t.flows[1].data->pull_to_host();
  const int m = a.m, n = a.n, ld = a.ld;
  for (int j = 0; j < n; j++) {
    double inv = 1.0 / L[(size_t)j * ld + j];
    for (int i = 0; i < m; i++) {
      double s = B[(size_t)j * ld + i];
      for (int k = 0; k < j; k++) s -= B[(size_t)k * ld + i] * L[(size_t)k * ld + j];
      B[(size_t)j * ld + i] = s * inv;
    }
  }
  t.flows[1].data->written_on(false);
}

// C = C - A*A^T (lower part only guaranteed; full tile computed is fine)
static void cpu_syrk(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const double* A = (const double*)t.flows[0].data->pull_to_host();
  double* C = (double*)t.flows[1].data->pull_to_host();
  const int n = a.n, k = a.k, ld = a.ld;
  for (int j = 0; j < n; j++)
    for (int i = j; i < n; i++) {
      double s = 0;
      for (int p = 0; p < k; p++) s += A[(size_t)p * ld + i] * A[(size_t)p * ld + j];
      C[(size_t)j * ld + i] -= s;
    }
  t.flows[1].data->written_on(false);
}

void cpu_trtri_lower(int n, const double* L, int ldl, double* W, int ldw) {
  for (int c = 0; c < n; c++) {
    W[(size_t)c * ldw + c] = 1.0 / L[(size_t)c * ldl + c];
    for (int i = c + 1; i < n; i++) {
      double s = 0;
      for (int k = c; k < i; k++) s += L[(size_t)k * ldl + i] * W[(size_t)c * ldw + k];
      W[(size_t)c * ldw + i] = -s / L[(size_t)i * ldl + i];
    }
  }
}

// W = L^{-1} (lower triangular inverse; upper of W zeroed)
static void cpu_trtri(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const double* L = (const double*)t.flows[0].data->pull_to_host();
  Data* wd = t.flows[1].data;
  double* W = (double*)wd->ensure_host();
  memset(W, 0, wd->bytes);
  cpu_trtri_lower(a.n, L, a.ld, W, a.ld);
  wd->written_on(false);
}

// B = B * W^T where W = L^{-1}  (the TRSM-as-GEMM variant)
static void cpu_trsm_inv(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const double* W = (const double*)t.flows[0].data->pull_to_host();
  double* B = (double*)t.flows[1].data->pull_to_host();
  const int m = a.m, n = a.n, ld = a.ld;
  std::vector<double> tmp((size_t)n * m);
  for (int j = 0; j < n; j++)
    for (int i = 0; i < m; i++) tmp[(size_t)j * m + i] = B[(size_t)j * ld + i];
  for (int j = 0; j < n; j++)
    for (int i = 0; i < m; i++) {
      double s = 0;
      for (int k = 0; k < n; k++)
        s += tmp[(size_t)k * m + i] * W[(size_t)k * ld + j];
      B[(size_t)j * ld + i] = s;
    }
  t.flows[1].data->written_on(false);
}

// C = C - A*B^T
static void cpu_gemm(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const double* A = (const double*)t.flows[0].data->pull_to_host();
  const double* B = (const double*)t.flows[1].data->pull_to_host();
  double* C = (double*)t.flows[2].data->pull_to_host();
  const int m = a.m, n = a.n, k = a.k, ld = a.ld;
  for (int j = 0; j < n; j++)
    for (int i = 0; i < m; i++) {
      double s = 0;
      for (int p = 0; p < k; p++) s += A[(size_t)p * ld + i] * B[(size_t)p * ld + j];
      C[(size_t)j * ld + i] -= s;
    }
  t.flows[2].data->written_on(false);
}

// ------------------------------------------------------------------ GPU chores
// Blocked tile POTRF: 128-wide LDS panel factorization (hand kernel) +
// rocBLAS panel-TRSM + trailing SYRK, all in-order on the task's stream.
// Critical-path op: measured ~3x faster than rocsolver_dpotrf at nb=2048.
// The trailing update runs on the hand triangular MFMA kernel
// (launch_dsyrk_ln: lower block set only, one launch per panel; glds path
// when the trailing size is a multiple of 128, bounds-checked path
// otherwise) instead of rocblas_dsyrk's k=128 decomposition into several
// small Tensile + syrkx launches per panel. It also writes the upper half
// of the trailing diagonal 128-blocks, which nothing reads.
// PARSEC_MCA_chore_potrf_syrk=rocblas restores the library update.
static void gpu_potrf_blocked(Task& t, GpuTaskCtx& g) {
  static const bool syrk_hip = param_str("chore_potrf_syrk", "hip") == "hip";
  const TileArgs& a = t.arg<TileArgs>();
  double* A = (double*)t.dev_ptr[0];
  const int n = a.n, ld = a.ld;
  const double one = 1.0, mone = -1.0;
  rocblas_handle h = blas_handle(g);
  for (int j = 0; j < n; j += 128) {
    int jb = std::min(128, n - j);
    double* Ajj = A + (size_t)j * ld + j;
    launch_potf2(Ajj, jb, ld, g.stream);
    int rest = n - j - jb;
    if (rest > 0) {
      double* Aij = A + (size_t)j * ld + j + jb;
      PA_BLAS_CHECK(rocblas_dtrsm(h, rocblas_side_right, rocblas_fill_lower,
                                  rocblas_operation_transpose,
                                  rocblas_diagonal_non_unit, rest, jb, &one,
                                  Ajj, ld, Aij, ld));
      double* Att = A + (size_t)(j + jb) * ld + j + jb;
      if (syrk_hip) {
        launch_dsyrk_ln(rest, jb, Aij, ld, Att, ld, g.stream);
        continue;
      }
      PA_BLAS_CHECK(rocblas_dsyrk(h, rocblas_fill_lower,
                                  rocblas_operation_none, rest, jb, &mone, Aij,
                                  ld, &one, Att, ld));
    }
  }
}

static void gpu_potrf(Task& t, GpuTaskCtx& g) {
  static const bool use_rocsolver =
      param_str("chore_potrf", "hip") == "rocsolver";
  if (!use_rocsolver) { gpu_potrf_blocked(t, g); return; }
  const TileArgs& a = t.arg<TileArgs>();
  PA_BLAS_CHECK(rocsolver_dpotrf(blas_handle(g), rocblas_fill_lower, a.n,
                                 (double*)t.dev_ptr[0], a.ld, dev_info(g)));
}

static void gpu_trsm(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  const double one = 1.0;
  PA_BLAS_CHECK(rocblas_dtrsm(
      blas_handle(g), rocblas_side_right, rocblas_fill_lower,
      rocblas_operation_transpose, rocblas_diagonal_non_unit, a.m, a.n, &one,
      (const double*)t.dev_ptr[0], a.ld, (double*)t.dev_ptr[1], a.ld));
}

static void gpu_syrk(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  const double mone = -1.0, one = 1.0;
  static const std::string chore = param_str("chore_syrk", "hip");
  static const bool use_syrkx = chore == "syrkx";
  static const bool use_hip = chore == "hip";
  if (use_hip) {
    // hand MFMA kernel over the lower-triangular block set only: half the
    // FLOPs of the full-tile dgemm route.
    launch_dsyrk_ln(a.n, a.k, (const double*)t.dev_ptr[0], a.ld,
                    (double*)t.dev_ptr[1], a.ld, g.stream);
    return;
  }
  if (!use_syrkx) {
    // SYRK as full-tile DGEMM(A, A^T): 2x the FLOPs but ~4x faster wall on
    // MI355X (rocBLAS syrkx measured 7.5 TF vs dgemm 60 TF at nb=2048);
    // the upper triangle of diagonal tiles is never read by the DAG.
    PA_BLAS_CHECK(rocblas_dgemm(
        blas_handle(g), rocblas_operation_none, rocblas_operation_transpose,
        a.n, a.n, a.k, &mone, (const double*)t.dev_ptr[0], a.ld,
        (const double*)t.dev_ptr[0], a.ld, &one, (double*)t.dev_ptr[1], a.ld));
    return;
  }
  PA_BLAS_CHECK(rocblas_dsyrk(blas_handle(g), rocblas_fill_lower,
                              rocblas_operation_none, a.n, a.k, &mone,
                              (const double*)t.dev_ptr[0], a.ld, &one,
                              (double*)t.dev_ptr[1], a.ld));
}

static void gpu_trtri(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  Data* wd = t.flows[1].data;
  PA_HIP_CHECK(hipMemsetAsync(t.dev_ptr[1], 0, wd->bytes, g.stream));
  PA_BLAS_CHECK(rocblas_dtrtri(
      blas_handle(g), rocblas_fill_lower, rocblas_diagonal_non_unit, a.n,
      (const double*)t.dev_ptr[0], a.ld, (double*)t.dev_ptr[1], a.ld));
}

// TRSM via the per-step inverse: B <- B * W^T is one full-rate DGEMM
// instead of rocBLAS dtrsm's ~44-kernel decomposition (measured ~9 TF vs
// ~60-75 TF for dgemm at these tile sizes). W is computed once per panel
// step and broadcast like the diagonal tile. By default the product runs on
// the triangular-aware hand kernel (launch_dtrmm_rlt, half the flops);
// PARSEC_MCA_chore_trsm_inv=rocblas keeps the dense dgemm.
static void gpu_trsm_inv(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  double* B = (double*)t.dev_ptr[1];
  // Out-of-place X = B * W^T into a fresh pool buffer, then swap it in as
  // the tile's device copy — no D2D copy (was ~13% of the Cholesky step).
  double* X = fresh_tile(t, g, 1);
  // W is lower triangular (gpu_trtri zero-fills the rest), so half of a
  // dense dgemm multiplies by zeros: the hand kernel cuts each output block
  // column's K range at its diagonal block. It needs full 128x128 blocks
  // and 16-B aligned columns; anything else takes the dense rocBLAS dgemm.
  static const bool use_hip = param_str("chore_trsm_inv", "hip") == "hip";
  if (use_hip && a.m % 128 == 0 && a.n % 128 == 0 && a.ld % 2 == 0) {
    launch_dtrmm_rlt(a.m, a.n, B, a.ld, (const double*)t.dev_ptr[0], a.ld, X,
                     a.ld, g.stream);
  } else {
    const double one = 1.0, zero = 0.0;
    PA_BLAS_CHECK(rocblas_dgemm(
        blas_handle(g), rocblas_operation_none, rocblas_operation_transpose,
        a.m, a.n, a.n, &one, B, a.ld, (const double*)t.dev_ptr[0], a.ld,
        &zero, X, a.ld));
  }
  swap_in_tile(t, g, 1, X);
}

static void gpu_gemm(Task& t, GpuTaskCtx& g) {
  static const bool use_hip = param_str("chore_gemm", "rocblas") == "hip";
  if (use_hip) { gpu_gemm_hip(t, g); return; }
  const TileArgs& a = t.arg<TileArgs>();
  const double mone = -1.0, one = 1.0;
  PA_BLAS_CHECK(rocblas_dgemm(
      blas_handle(g), rocblas_operation_none, rocblas_operation_transpose,
      a.m, a.n, a.k, &mone, (const double*)t.dev_ptr[0], a.ld,
      (const double*)t.dev_ptr[1], a.ld, &one, (double*)t.dev_ptr[2], a.ld));
}

// Timed rocBLAS dgemm NT loop for kernel-level A/B against the hand kernel.
// C -= A B^T (B stored n x k) or, with nn, C -= A B (B stored k x n).
static double bench_dgemm_lib(int m, int n, int k, int iters, bool nn) {
  const int brows = nn ? k : n, bcols = nn ? n : k;
  DevArray dA((size_t)m * k), dB((size_t)n * k), dC((size_t)m * n);
  launch_spd_fill(dA.p, m, k, m, 0, 0, 0, 11u, 0);
  launch_spd_fill(dB.p, brows, bcols, brows, 7, 3, 0, 12u, 0);
  launch_spd_fill(dC.p, m, n, m, 1, 9, 0, 13u, 0);
  rocblas_handle h;
  PA_BLAS_CHECK(rocblas_create_handle(&h));
  const double mone = -1.0, one = 1.0;
  double dt = time_launches(iters, [&] {
    rocblas_dgemm(h, rocblas_operation_none,
                  nn ? rocblas_operation_none : rocblas_operation_transpose, m,
                  n, k, &mone, dA.p, m, dB.p, brows, &one, dC.p, m);
  });
  rocblas_destroy_handle(h);
  return dt;
}

double bench_dgemm_rocblas(int m, int n, int k, int iters) {
  return bench_dgemm_lib(m, n, k, iters, /*nn=*/false);
}

double bench_dgemm_nn_rocblas(int m, int n, int k, int iters) {
  return bench_dgemm_lib(m, n, k, iters, /*nn=*/true);
}

// ------------------------------------------------------------------ classes
TaskClass make_tc(const char* name, TaskKind kind, void (*cpu)(Task&),
                  void (*gpu)(Task&, GpuTaskCtx&), TaskClassId id,
                  bool blocking) {
  {
    static std::mutex mtx;
    static std::map<int, std::string> names;
    std::lock_guard<std::mutex> lk(mtx);
    auto it = names.emplace((int)id, name).first;
    PA_CHECK(it->second == name,
             "task-class id %d of '%s' is already taken by '%s'", (int)id,
             name, it->second.c_str());
  }
  Profiler::inst().register_class(id, name);
  TaskClass tc;
  tc.name = name;
  tc.kind = kind;
  tc.cpu_hook = cpu;
  tc.gpu_hook = gpu;
  tc.id = id;
  tc.gpu_blocking = blocking;
  return tc;
}

TaskClass& tc_spd_fill() {
  static TaskClass tc =
      make_tc("spd_fill", TaskKind::GPU, cpu_spd_fill, gpu_spd_fill, TC_SPD_FILL);
  return tc;
}
TaskClass& tc_potrf() {
  static TaskClass tc =
      make_tc("potrf", TaskKind::GPU, cpu_potrf, gpu_potrf, TC_POTRF);
  return tc;
}
TaskClass& tc_trsm() {
  static TaskClass tc =
      make_tc("trsm", TaskKind::GPU, cpu_trsm, gpu_trsm, TC_TRSM);
  return tc;
}
TaskClass& tc_trtri() {
  static TaskClass tc =
      make_tc("trtri", TaskKind::GPU, cpu_trtri, gpu_trtri, TC_TRTRI);
  return tc;
}
TaskClass& tc_trsm_inv() {
  static TaskClass tc = make_tc("trsm_inv", TaskKind::GPU, cpu_trsm_inv,
                                gpu_trsm_inv, TC_TRSM_INV);
  return tc;
}
TaskClass& tc_syrk() {
  static TaskClass tc =
      make_tc("syrk", TaskKind::GPU, cpu_syrk, gpu_syrk, TC_SYRK);
  return tc;
}
TaskClass& tc_gemm() {
  static TaskClass tc =
      make_tc("gemm", TaskKind::GPU, cpu_gemm, gpu_gemm, TC_GEMM);
  return tc;
}

// ------------------------------------------------------------------ DAG builders
// The synthetic fill of A's tiles: the lower triangle for SPD input, or the
// full matrix (QR and GEMM inputs read above the diagonal too).
static void insert_fill(Dtd& tp, TiledMatrix& A, uint32_t seed, bool full) {
  for (int tm = 0; tm < A.mt(); tm++)
    for (int tn = 0; (full || tn <= tm) && tn < A.nt(); tn++) {
      TileArgs a = fill_args(A, tm, tn, seed);
      Dtd::FlowSpec f[] = {{A.tile(tm, tn), ACCESS_OUT}};
      tp.insert(&tc_spd_fill(), &a, sizeof(a), f, 1, 0, A.rank_of(tm, tn));
    }
}

void insert_spd_fill(Dtd& tp, TiledMatrix& A, uint32_t seed) {
  insert_fill(tp, A, seed, /*full=*/false);
}

void insert_full_fill(Dtd& tp, TiledMatrix& A, uint32_t seed) {
  insert_fill(tp, A, seed, /*full=*/true);
}

// Right-looking tiled Cholesky, lower triangular (the reference's headline
// dpotrf DAG shape; DPLASMA dpotrf_L equivalent).
void insert_potrf(Dtd& tp, TiledMatrix& A) {
  const int T = A.mt();
  const int ld = A.mb();
  // Critical-path priorities (DPLASMA dpotrf style): panel ops (POTRF/TRSM)
  // always outrank trailing updates, and an update targeting column n at
  // step k is more urgent the sooner column n becomes the panel (n-k small).
  // This is what creates lookahead: panel k+1 preempts the bulk of step-k
  // GEMMs in the GPU engine's priority queue.
  constexpr int PANEL = 1 << 20;
  // TRSM variant: "invgemm" (default) computes W_k = L(k,k)^{-1} once per
  // step (TRTRI task on the panel stream) and does each TRSM as a single
  // full-rate DGEMM; "rocblas" calls dtrsm directly. Must be uniform across
  // ranks (the DAG shape depends on it).
  const bool invgemm = param_str("trsm_variant", "invgemm") == "invgemm";
  std::shared_ptr<TiledMatrix> W;
  if (invgemm) {
    W = std::make_shared<TiledMatrix>(A.ctx(), A.m(), A.n(), A.mb(), A.nb(),
                                      A.grid_p(), A.grid_q());
    tp.own(W);
  }
  for (int k = 0; k < T; k++) {
    TileArgs pa_args = tile_args(0, A.tile_cols(k), 0, ld);
    {
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_INOUT}};
      tp.insert(&tc_potrf(), &pa_args, sizeof(pa_args), f, 1, PANEL + 1,
                A.rank_of(k, k));
    }
    if (invgemm && k + 1 < T) {
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_IN},
                           {W->tile(k, k), ACCESS_OUT}};
      tp.insert(&tc_trtri(), &pa_args, sizeof(pa_args), f, 2, PANEL,
                A.rank_of(k, k));
    }
    for (int m = k + 1; m < T; m++) {
      TileArgs a = tile_args(A.tile_rows(m), A.tile_cols(k), 0, ld);
      // Below the express-stream threshold (1<<19): TRSMs are urgent in the
      // queue but must spread across bulk streams, not serialize on the
      // panel stream.
      if (invgemm) {
        Dtd::FlowSpec f[] = {{W->tile(k, k), ACCESS_IN},
                             {A.tile(m, k), ACCESS_INOUT}};
        tp.insert(&tc_trsm_inv(), &a, sizeof(a), f, 2, (1 << 18) - (m - k),
                  A.rank_of(m, k));
      } else {
        Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_IN},
                             {A.tile(m, k), ACCESS_INOUT}};
        tp.insert(&tc_trsm(), &a, sizeof(a), f, 2, (1 << 18) - (m - k),
                  A.rank_of(m, k));
      }
    }
    for (int n = k + 1; n < T; n++) {
      {
        TileArgs a = tile_args(0, A.tile_rows(n), A.tile_cols(k), ld);
        Dtd::FlowSpec f[] = {{A.tile(n, k), ACCESS_IN},
                             {A.tile(n, n), ACCESS_INOUT}};
        tp.insert(&tc_syrk(), &a, sizeof(a), f, 2, -(n - k) * 4 + 1,
                  A.rank_of(n, n));
      }
      for (int m = n + 1; m < T; m++) {
        TileArgs a =
            tile_args(A.tile_rows(m), A.tile_rows(n), A.tile_cols(k), ld);
        Dtd::FlowSpec f[] = {{A.tile(m, k), ACCESS_IN},
                             {A.tile(n, k), ACCESS_IN},
                             {A.tile(m, n), ACCESS_INOUT}};
        tp.insert(&tc_gemm(), &a, sizeof(a), f, 3, -(n - k) * 4,
                  A.rank_of(m, n));
      }
    }
  }
}

// ------------------------------------------------------- plain NN GEMM DAG
// Tiled C = A * B (fp64, rocBLAS NN per tile). The k==0 task overwrites C
// (beta = 0, OUTPUT flow), later k accumulate — which makes the whole DAG
// IDEMPOTENT: replaying it (e.g. from a captured hipGraph, gpu_graph.hpp)
// reproduces the same C from the same A/B.
static void cpu_gemm_nn(Task& t) {
  const GemmNNArgs& a = t.arg<GemmNNArgs>();
  const double* A = (const double*)t.flows[0].data->pull_to_host();
  const double* B = (const double*)t.flows[1].data->pull_to_host();
  // beta == 0 rides an OUTPUT-only flow: nothing valid to pull yet
  double* C = a.beta == 0.0 ? (double*)t.flows[2].data->ensure_host()
                            : (double*)t.flows[2].data->pull_to_host();
  for (int j = 0; j < a.n; j++)
    for (int i = 0; i < a.m; i++) {
      double s = 0;
      for (int p = 0; p < a.k; p++)
        s += (a.transA ? A[(size_t)i * a.lda + p] : A[(size_t)p * a.lda + i]) *
             B[(size_t)j * a.ldb + p];
      double c0 = a.beta == 0.0 ? 0.0 : a.beta * C[(size_t)j * a.ldc + i];
      C[(size_t)j * a.ldc + i] = c0 + a.alpha * s;
    }
  t.flows[2].data->written_on(false);
}

// Thin-C tiles (vector iterations, skinny updates): a library GEMM is all
// launch overhead at n<=4, and a plain kernel is trivially capture-safe.
__global__ void k_gemm_nn_thin(int m, int n, int k, double alpha,
                               const double* A, int lda, const double* B,
                               int ldb, double beta, double* C, int ldc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int j = blockIdx.y;
  if (i >= m || j >= n) return;
  double s = 0;
  for (int p = 0; p < k; p++)
    s += A[(size_t)p * lda + i] * B[(size_t)j * ldb + p];
  double c0 = beta == 0.0 ? 0.0 : beta * C[(size_t)j * ldc + i];
  C[(size_t)j * ldc + i] = c0 + alpha * s;
}

bool gemm_nn_hip() {
  static const bool v = param_str("chore_gemm_nn", "rocblas") == "hip";
  return v;
}

static void gpu_gemm_nn(Task& t, GpuTaskCtx& g) {
  const GemmNNArgs& a = t.arg<GemmNNArgs>();
  // chore_gemm_nn=hip: the update of a solve sweep, C -= A B, on more than
  // the thin kernel's columns
  if (gemm_nn_hip() && !a.transA && a.alpha == -1.0 && a.beta == 1.0 &&
      a.n > 4) {
    launch_dgemm_nn(a.m, a.n, a.k, (const double*)t.dev_ptr[0], a.lda,
                    (const double*)t.dev_ptr[1], a.ldb, (double*)t.dev_ptr[2],
                    a.ldc, g.stream);
    return;
  }
  if (a.n <= 4 && !a.transA) {
    hipLaunchKernelGGL(k_gemm_nn_thin, dim3((a.m + 63) / 64, a.n), dim3(64),
                       0, g.stream, a.m, a.n, a.k, a.alpha,
                       (const double*)t.dev_ptr[0], a.lda,
                       (const double*)t.dev_ptr[1], a.ldb, a.beta,
                       (double*)t.dev_ptr[2], a.ldc);
    return;
  }
  PA_BLAS_CHECK(rocblas_dgemm(
      blas_handle(g),
      a.transA ? rocblas_operation_transpose : rocblas_operation_none,
      rocblas_operation_none, a.m, a.n, a.k, &a.alpha,
      (const double*)t.dev_ptr[0], a.lda, (const double*)t.dev_ptr[1],
      a.ldb, &a.beta, (double*)t.dev_ptr[2], a.ldc));
}

TaskClass& tc_gemm_nn() {
  static TaskClass tc =
      make_tc("gemm_nn", TaskKind::GPU, cpu_gemm_nn, gpu_gemm_nn, TC_GEMM_NN);
  return tc;
}

void insert_gemm_fp64(Dtd& tp, TiledMatrix& A, TiledMatrix& B,
                      TiledMatrix& C) {
  PA_CHECK(A.nt() == B.mt() && A.mt() == C.mt() && B.nt() == C.nt(),
           "insert_gemm_fp64: tile-grid mismatch");
  for (int i = 0; i < C.mt(); i++)
    for (int j = 0; j < C.nt(); j++)
      for (int p = 0; p < A.nt(); p++) {
        // tiles are stored at the collection's full ld (= mb), partial
        // edge tiles included (see tile_numpy / TiledMatrix layout)
        GemmNNArgs a{C.tile_rows(i), C.tile_cols(j), A.tile_cols(p),
                     A.mb(),         B.mb(),         C.mb(),
                     1.0,            p == 0 ? 0.0 : 1.0};
        Dtd::FlowSpec f[] = {{A.tile(i, p), ACCESS_IN},
                             {B.tile(p, j), ACCESS_IN},
                             {C.tile(i, j), p == 0 ? ACCESS_OUT
                                                   : ACCESS_INOUT}};
        tp.insert(&tc_gemm_nn(), &a, sizeof(a), f, 3, 0, C.rank_of(i, j));
      }
}

// ------------------------------------------------------------- trsm_solve
// A triangular solve from the left with the factor in a diagonal tile: the
// diagonal step of the tile sweeps in kernels_solve.cpp and of insert_trtri.
// The library chore is rocblas_dtrsm (left; triangle, trans and unit from
// the arguments).
static void cpu_trsm_solve(Task& t) {
  const TrsmSolveArgs& a = t.arg<TrsmSolveArgs>();
  const double* L = (const double*)t.flows[0].data->pull_to_host();
  double* B = (double*)t.flows[1].data->pull_to_host();
  // forward order for {lower, N} and {upper, T}; backward otherwise
  const bool fwd = (a.upper == 0) != (a.trans != 0);
  auto elem = [&](int i, int p) {
    return a.trans ? L[(size_t)i * a.lda + p] : L[(size_t)p * a.lda + i];
  };
  for (int j = 0; j < a.n; j++) {
    double* b = B + (size_t)j * a.ldb;
    if (fwd) {
      for (int i = 0; i < a.m; i++) {
        double s = b[i];
        for (int p = 0; p < i; p++) s -= elem(i, p) * b[p];
        b[i] = a.unit ? s : s / L[(size_t)i * a.lda + i];
      }
    } else {
      for (int i = a.m - 1; i >= 0; i--) {
        double s = b[i];
        for (int p = i + 1; p < a.m; p++) s -= elem(i, p) * b[p];
        b[i] = a.unit ? s : s / L[(size_t)i * a.lda + i];
      }
    }
  }
  t.flows[1].data->written_on(false);
}

static void gpu_trsm_solve(Task& t, GpuTaskCtx& g) {
  const TrsmSolveArgs& a = t.arg<TrsmSolveArgs>();
  const double one = 1.0;
  PA_BLAS_CHECK(rocblas_dtrsm(
      blas_handle(g), rocblas_side_left,
      a.upper ? rocblas_fill_upper : rocblas_fill_lower,
      a.trans ? rocblas_operation_transpose : rocblas_operation_none,
      a.unit ? rocblas_diagonal_unit : rocblas_diagonal_non_unit, a.m, a.n,
      &one, (const double*)t.dev_ptr[0], a.lda, (double*)t.dev_ptr[1],
      a.ldb));
}

TaskClass& tc_trsm_solve() {
  static TaskClass tc = make_tc("trsm_solve", TaskKind::GPU, cpu_trsm_solve,
                                gpu_trsm_solve, TC_TRSM_SOLVE);
  return tc;
}

// Pre-create the per-stream rocBLAS handle and give it a fixed device
// workspace so no allocation can happen inside a hipStream capture
// (gpu_graph.cpp calls this for each capture stream before BeginCapture;
// same thread, so the thread_local handle map matches the replay).
void blas_warm_stream_for_capture(hipStream_t s) {
  GpuTaskCtx g{s, 0, nullptr, nullptr};
  rocblas_handle h = blas_handle(g);
  static thread_local std::map<void*, void*> ws;
  void*& w = ws[(void*)s];
  if (!w) {
    const size_t bytes = 1u << 26;
    PA_HIP_CHECK(hipMalloc(&w, bytes));
    PA_BLAS_CHECK(rocblas_set_workspace(h, w, bytes));
  }
}

}  // namespace pa
