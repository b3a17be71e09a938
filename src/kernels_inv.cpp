// SPD inverse in place on the lower tiles (dplasma dtrtri/dlauum/dpotri/
// dpoinv analogs): W = L^-1 by tile TRTRI, then A^-1 = W^T W by tile LAUUM.
//
// The strict upper triangle of a diagonal tile is junk (insert_potrf leaves
// symmetric leftovers there): every chore below reads the lower triangle of
// a diagonal tile only. What they leave above it is zero or the symmetric
// value, one convention per chore family so that the accumulating SYRK-T
// keeps it: the CPU and library chores keep diagonal tiles symmetric, the
// hand chores keep the diagonal 128-blocks symmetric and the rest zero.
#include "kernels.hpp"

#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "device_gpu.hpp"
#include "gpu_blas.hpp"
#include "kernels_bench.hpp"
#include "kernels_hip.hpp"

namespace pa {

static bool lauum_hip() {
  static const bool v = param_str("chore_lauum", "rocblas") == "hip";
  return v;
}
static bool gemm_tn_hip() {
  static const bool v = param_str("chore_gemm_tn", "rocblas") == "hip";
  return v;
}

// Strict upper triangle <- transpose of the strict lower one.
__global__ void k_mirror_lower(double* A, int n, int ld) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  for (; idx < n * n; idx += gridDim.x * blockDim.x) {
    int c = idx / n, r = idx - c * n;
    if (r < c) A[(size_t)c * ld + r] = A[(size_t)r * ld + c];
  }
}

static void launch_mirror_lower(double* A, int n, int ld, hipStream_t s) {
  int grid = std::min((n * n + 255) / 256, 4096);
  hipLaunchKernelGGL(k_mirror_lower, dim3(grid), dim3(256), 0, s, A, n, ld);
}

// B <- -B * L^-1 (right, lower, no-trans): column k of W below its diagonal
// tile. Columns are solved last to first.
static void cpu_inv_trsm_r(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const double* L = (const double*)t.flows[0].data->pull_to_host();
  double* B = (double*)t.flows[1].data->pull_to_host();
  const int m = a.m, n = a.n, ld = a.ld;
  for (int j = n - 1; j >= 0; j--) {
    double inv = 1.0 / L[(size_t)j * ld + j];
    for (int i = 0; i < m; i++) {
      double s = -B[(size_t)j * ld + i];
      for (int p = j + 1; p < n; p++)
        s -= B[(size_t)p * ld + i] * L[(size_t)j * ld + p];
      B[(size_t)j * ld + i] = s * inv;
    }
  }
  t.flows[1].data->written_on(false);
}

static void gpu_inv_trsm_r(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  const double mone = -1.0;
  PA_BLAS_CHECK(rocblas_dtrsm(
      blas_handle(g), rocblas_side_right, rocblas_fill_lower,
      rocblas_operation_none, rocblas_diagonal_non_unit, a.m, a.n, &mone,
      (const double*)t.dev_ptr[0], a.ld, (double*)t.dev_ptr[1], a.ld));
}

// T <- T^-1 on the lower triangle of a diagonal tile; zeros above.
static void cpu_trtri_inplace(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  double* T = (double*)t.flows[0].data->pull_to_host();
  const int n = a.n, ld = a.ld;
  std::vector<double> W((size_t)n * n, 0.0);
  cpu_trtri_lower(n, T, ld, W.data(), n);
  for (int c = 0; c < n; c++)
    for (int i = 0; i < n; i++) T[(size_t)c * ld + i] = W[(size_t)c * n + i];
  t.flows[0].data->written_on(false);
}

static void gpu_trtri_inplace(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  double* X = fresh_tile(t, g, 0);
  PA_HIP_CHECK(hipMemsetAsync(X, 0, t.flows[0].data->bytes, g.stream));
  PA_BLAS_CHECK(rocblas_dtrtri(
      blas_handle(g), rocblas_fill_lower, rocblas_diagonal_non_unit, a.n,
      (const double*)t.dev_ptr[0], a.ld, X, a.ld));
  swap_in_tile(t, g, 0, X);
}

// C += A^T A, A k x n: the diagonal-tile update of the LAUUM phase. The
// lower triangle is computed and mirrored.
static void cpu_syrk_t(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const double* A = (const double*)t.flows[0].data->pull_to_host();
  double* C = (double*)t.flows[1].data->pull_to_host();
  const int n = a.n, k = a.k, ld = a.ld;
  for (int j = 0; j < n; j++)
    for (int i = j; i < n; i++) {
      double s = 0;
      for (int p = 0; p < k; p++) s += A[(size_t)i * ld + p] * A[(size_t)j * ld + p];
      C[(size_t)j * ld + i] += s;
      C[(size_t)i * ld + j] = C[(size_t)j * ld + i];
    }
  t.flows[1].data->written_on(false);
}

static void gpu_syrk_t(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  if (lauum_hip()) {
    launch_dsyrk_lt(a.n, a.k, (const double*)t.dev_ptr[0], a.ld,
                    (double*)t.dev_ptr[1], a.ld, g.stream);
    return;
  }
  // full-tile dgemm as in gpu_syrk; the tile is symmetric on entry (the
  // LAUUM chore below mirrors it) and stays so
  const double one = 1.0;
  PA_BLAS_CHECK(rocblas_dgemm(
      blas_handle(g), rocblas_operation_transpose, rocblas_operation_none,
      a.n, a.n, a.k, &one, (const double*)t.dev_ptr[0], a.ld,
      (const double*)t.dev_ptr[0], a.ld, &one, (double*)t.dev_ptr[1], a.ld));
}

// B <- W^T B, W m x m lower (left, lower, trans). Row i of the product
// needs rows >= i of B only, so ascending rows run in place.
static void cpu_trmm_llt(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const double* W = (const double*)t.flows[0].data->pull_to_host();
  double* B = (double*)t.flows[1].data->pull_to_host();
  const int m = a.m, n = a.n, ld = a.ld;
  for (int j = 0; j < n; j++)
    for (int i = 0; i < m; i++) {
      double s = 0;
      for (int p = i; p < m; p++) s += W[(size_t)i * ld + p] * B[(size_t)j * ld + p];
      B[(size_t)j * ld + i] = s;
    }
  t.flows[1].data->written_on(false);
}

static void gpu_trmm_llt(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  double* B = (double*)t.dev_ptr[1];
  if (lauum_hip()) {
    double* X = fresh_tile(t, g, 1);
    launch_dtrmm_llt(a.m, a.n, (const double*)t.dev_ptr[0], a.ld, B, a.ld, X,
                     a.ld, g.stream);
    swap_in_tile(t, g, 1, X);
    return;
  }
  // rocBLAS's three-matrix trmm with C = B is the in-place legacy form
  const double one = 1.0;
  PA_BLAS_CHECK(rocblas_dtrmm(
      blas_handle(g), rocblas_side_left, rocblas_fill_lower,
      rocblas_operation_transpose, rocblas_diagonal_non_unit, a.m, a.n, &one,
      (const double*)t.dev_ptr[0], a.ld, B, a.ld, B, a.ld));
}

// T <- W^T W for the lower triangular W in a diagonal tile; the result is
// written whole (symmetric).
static void cpu_lauum(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  double* T = (double*)t.flows[0].data->pull_to_host();
  const int n = a.n, ld = a.ld;
  std::vector<double> W((size_t)n * n);
  for (int c = 0; c < n; c++)
    for (int i = 0; i < n; i++)
      W[(size_t)c * n + i] = i >= c ? T[(size_t)c * ld + i] : 0.0;
  for (int j = 0; j < n; j++)
    for (int i = j; i < n; i++) {
      double s = 0;
      for (int p = i; p < n; p++) s += W[(size_t)i * n + p] * W[(size_t)j * n + p];
      T[(size_t)j * ld + i] = s;
      T[(size_t)i * ld + j] = s;
    }
  t.flows[0].data->written_on(false);
}

static void gpu_lauum(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  if (lauum_hip()) {
    // the kernel writes the lower block set only: clear the rest
    double* X = fresh_tile(t, g, 0);
    PA_HIP_CHECK(hipMemsetAsync(X, 0, t.flows[0].data->bytes, g.stream));
    launch_dlauum_l(a.n, (const double*)t.dev_ptr[0], a.ld, X, a.ld, g.stream);
    swap_in_tile(t, g, 0, X);
    return;
  }
  double* T = (double*)t.dev_ptr[0];
  PA_BLAS_CHECK(
      rocsolver_dlauum(blas_handle(g), rocblas_fill_lower, a.n, T, a.ld));
  launch_mirror_lower(T, a.n, a.ld, g.stream);
}

// C += A^T B with gemm_nn's arguments (transA = 1, alpha = beta = 1): the
// library chore is gemm_nn's, chore_gemm_tn=hip takes the hand kernel.
static void gpu_gemm_tn(Task& t, GpuTaskCtx& g) {
  if (!gemm_tn_hip()) { tc_gemm_nn().gpu_hook(t, g); return; }
  const GemmNNArgs& a = t.arg<GemmNNArgs>();
  PA_CHECK(a.transA && a.alpha == 1.0 && a.beta == 1.0);
  launch_dgemm_tn(a.m, a.n, a.k, (const double*)t.dev_ptr[0], a.lda,
                  (const double*)t.dev_ptr[1], a.ldb, (double*)t.dev_ptr[2],
                  a.ldc, g.stream);
}

static TaskClass& tc_inv_trsm_r() {
  static TaskClass tc = make_tc("inv_trsm_r", TaskKind::GPU, cpu_inv_trsm_r,
                                gpu_inv_trsm_r, TC_INV_TRSM_R);
  return tc;
}
static TaskClass& tc_trtri_inplace() {
  static TaskClass tc =
      make_tc("trtri_inplace", TaskKind::GPU, cpu_trtri_inplace,
              gpu_trtri_inplace, TC_TRTRI_INPLACE);
  return tc;
}
static TaskClass& tc_syrk_t() {
  static TaskClass tc =
      make_tc("syrk_t", TaskKind::GPU, cpu_syrk_t, gpu_syrk_t, TC_SYRK_T);
  return tc;
}
static TaskClass& tc_gemm_tn() {
  static TaskClass tc = make_tc("gemm_tn", TaskKind::GPU,
                                tc_gemm_nn().cpu_hook, gpu_gemm_tn, TC_GEMM_TN);
  return tc;
}
static TaskClass& tc_trmm_llt() {
  static TaskClass tc = make_tc("trmm_llt", TaskKind::GPU, cpu_trmm_llt,
                                gpu_trmm_llt, TC_TRMM_LLT);
  return tc;
}
static TaskClass& tc_lauum() {
  static TaskClass tc =
      make_tc("lauum", TaskKind::GPU, cpu_lauum, gpu_lauum, TC_LAUUM);
  return tc;
}

static void check_inv_shape(TiledMatrix& A, const char* who) {
  PA_CHECK(A.mt() == A.nt() && A.m() == A.n() && A.mb() == A.nb(),
           "%s: A must be square with square tiles", who);
}

// Priorities as in insert_potrf: the diagonal-tile operation of a step goes
// to the panel stream, the triangular operations next to it stay urgent
// below the express threshold, bulk updates are ordered by how soon their
// target is needed.
constexpr int INV_PANEL = 1 << 20;
constexpr int INV_NEAR = 1 << 18;

void insert_trtri(Dtd& tp, TiledMatrix& A) {
  check_inv_shape(A, "insert_trtri");
  const int T = A.mt(), ld = A.mb();
  for (int k = 0; k < T; k++) {
    for (int m = k + 1; m < T; m++) {
      TileArgs a = tile_args(A.tile_rows(m), A.tile_cols(k), 0, ld);
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_IN},
                           {A.tile(m, k), ACCESS_INOUT}};
      tp.insert(&tc_inv_trsm_r(), &a, sizeof(a), f, 2, INV_NEAR - (m - k),
                A.rank_of(m, k));
    }
    // row m = k+1 is the next step's row of left solves
    for (int m = k + 1; m < T; m++)
      for (int n = 0; n < k; n++) {
        GemmNNArgs a{A.tile_rows(m), A.tile_cols(n), A.tile_cols(k),
                     ld,             ld,             ld,
                     1.0,            1.0};
        Dtd::FlowSpec f[] = {{A.tile(m, k), ACCESS_IN},
                             {A.tile(k, n), ACCESS_IN},
                             {A.tile(m, n), ACCESS_INOUT}};
        tp.insert(&tc_gemm_nn(), &a, sizeof(a), f, 3, -(m - k) * 4,
                  A.rank_of(m, n));
      }
    for (int n = 0; n < k; n++) {
      TrsmSolveArgs a{A.tile_rows(k), A.tile_cols(n), ld, ld, 0};
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_IN},
                           {A.tile(k, n), ACCESS_INOUT}};
      tp.insert(&tc_trsm_solve(), &a, sizeof(a), f, 2, INV_NEAR - (k - n),
                A.rank_of(k, n));
    }
    {
      TileArgs a = tile_args(0, A.tile_rows(k), 0, ld);
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_INOUT}};
      tp.insert(&tc_trtri_inplace(), &a, sizeof(a), f, 1, INV_PANEL,
                A.rank_of(k, k));
    }
  }
}

void insert_lauum(Dtd& tp, TiledMatrix& A) {
  check_inv_shape(A, "insert_lauum");
  lauum_hip();  // registered for param_dump wherever the DAG is built
  gemm_tn_hip();
  const int T = A.mt(), ld = A.mb();
  for (int k = 0; k < T; k++) {
    for (int n = 0; n < k; n++) {
      TileArgs a = tile_args(0, A.tile_cols(n), A.tile_rows(k), ld);
      Dtd::FlowSpec f[] = {{A.tile(k, n), ACCESS_IN},
                           {A.tile(n, n), ACCESS_INOUT}};
      tp.insert(&tc_syrk_t(), &a, sizeof(a), f, 2, -(k - n) * 4 + 1,
                A.rank_of(n, n));
    }
    for (int n = 0; n < k; n++)
      for (int m = n + 1; m < k; m++) {
        GemmNNArgs a{A.tile_cols(m), A.tile_cols(n), A.tile_rows(k),
                     ld,             ld,             ld,
                     1.0,            1.0};
        a.transA = 1;
        Dtd::FlowSpec f[] = {{A.tile(k, m), ACCESS_IN},
                             {A.tile(k, n), ACCESS_IN},
                             {A.tile(m, n), ACCESS_INOUT}};
        tp.insert(&tc_gemm_tn(), &a, sizeof(a), f, 3, -(k - n) * 4,
                  A.rank_of(m, n));
      }
    for (int n = 0; n < k; n++) {
      TileArgs a = tile_args(A.tile_rows(k), A.tile_cols(n), 0, ld);
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_IN},
                           {A.tile(k, n), ACCESS_INOUT}};
      tp.insert(&tc_trmm_llt(), &a, sizeof(a), f, 2, INV_NEAR - (k - n),
                A.rank_of(k, n));
    }
    {
      TileArgs a = tile_args(0, A.tile_rows(k), 0, ld);
      Dtd::FlowSpec f[] = {{A.tile(k, k), ACCESS_INOUT}};
      tp.insert(&tc_lauum(), &a, sizeof(a), f, 1, INV_PANEL, A.rank_of(k, k));
    }
  }
}

void insert_potri(Dtd& tp, TiledMatrix& A) {
  insert_trtri(tp, A);
  insert_lauum(tp, A);
}

void insert_poinv(Dtd& tp, TiledMatrix& A) {
  insert_potrf(tp, A);
  insert_potri(tp, A);
}

// Timed library routes of the LAUUM-phase tile operations, for the A/B
// against bench_dgemm_tn_hip (same kinds: 0 dgemm TN, 1 syrk-t as full
// dgemm, 2 trmm, 3 lauum + mirror). TRMM and LAUUM overwrite their operand,
// so every iteration restores it first; only the library calls are between
// the timing events. Returns seconds for `iters` calls.
double bench_tn_rocblas(int kind, int m, int n, int k, int iters) {
  PA_CHECK(kind >= 0 && kind <= 3, "bench_tn_rocblas: kind %d", kind);
  if (kind == 1 || kind == 3) m = n;
  if (kind >= 2) k = m;
  const size_t welems = (size_t)m * n;
  DevArray A((size_t)k * m), B((size_t)k * n), Orig(welems), Work(welems);
  double *dA = A.p, *dB = B.p, *dOrig = Orig.p, *dWork = Work.p;
  launch_spd_fill(dB, k, n, k, 5, 1, 0, 13u, 0);
  launch_spd_fill(dA, k, m, k, 0, 0, 0, 11u, 0);
  launch_spd_fill(dOrig, m, n, m, 7, 3, 0, 12u, 0);
  rocblas_handle h;
  PA_BLAS_CHECK(rocblas_create_handle(&h));
  hipEvent_t e0, e1;
  PA_HIP_CHECK(hipEventCreate(&e0));
  PA_HIP_CHECK(hipEventCreate(&e1));
  const double one = 1.0;
  auto run = [&] {
    if (kind == 0) {
      PA_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_transpose,
                                  rocblas_operation_none, m, n, k, &one, dA, k,
                                  dB, k, &one, dWork, m));
    } else if (kind == 1) {
      PA_BLAS_CHECK(rocblas_dgemm(h, rocblas_operation_transpose,
                                  rocblas_operation_none, n, n, k, &one, dA, k,
                                  dA, k, &one, dWork, n));
    } else if (kind == 2) {
      PA_BLAS_CHECK(rocblas_dtrmm(h, rocblas_side_left, rocblas_fill_lower,
                                  rocblas_operation_transpose,
                                  rocblas_diagonal_non_unit, m, n, &one, dA, m,
                                  dWork, m, dWork, m));
    } else {
      PA_BLAS_CHECK(rocsolver_dlauum(h, rocblas_fill_lower, n, dWork, n));
      launch_mirror_lower(dWork, n, n, 0);
    }
  };
  double total = 0;
  for (int i = -1; i < iters; i++) {  // i == -1 warms up
    PA_HIP_CHECK(hipMemcpyAsync(dWork, dOrig, welems * 8,
                                hipMemcpyDeviceToDevice, 0));
    PA_HIP_CHECK(hipEventRecord(e0, 0));
    run();
    PA_HIP_CHECK(hipEventRecord(e1, 0));
    PA_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    PA_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (i >= 0) total += ms * 1e-3;
  }
  PA_HIP_CHECK(hipEventDestroy(e0));
  PA_HIP_CHECK(hipEventDestroy(e1));
  rocblas_destroy_handle(h);
  return total;
}

}  // namespace pa
