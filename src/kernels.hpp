// Tile task-classes for the dense linear-algebra headline apps.
//
// The reference runtime ships no compute kernels — JDF bodies call cuBLAS
// via dyld (tests/runtime/cuda/stress.jdf:133-137) and dense drivers live in
// DPLASMA. Here the tile kernel set IS part of the framework (SURVEY.md §6
// north star): fp64 POTRF/TRSM/SYRK/GEMM tile bodies with two chore
// incarnations each — rocBLAS/rocSOLVER ("library" chore) and hand-written
// CDNA4 MFMA HIP kernels (kernels_hip.cpp) — selected by the `chore_gemm`
// etc. params, mirroring the reference's chore/incarnation machinery
// (parsec_internal.h:411-459).
#pragma once

#include "dtd.hpp"

namespace pa {

enum class Reshape : uint8_t;
TaskClass& tc_reshape();
size_t reshape_bytes(size_t src_bytes, Reshape kind, size_t src_elem);
void fill_reshape_args(void* argbuf, Reshape kind, int m, int n, int ld);
size_t reshape_args_bytes();

struct TileArgs {
  int m = 0, n = 0, k = 0, ld = 0;
  int64_t i0 = 0, j0 = 0, N = 0;
  uint32_t seed = 0;
};

// The operation shape of a tile chore; the other fields stay zero.
inline TileArgs tile_args(int m, int n, int k, int ld) {
  TileArgs a;
  a.m = m;
  a.n = n;
  a.k = k;
  a.ld = ld;
  return a;
}

// Tile (tm, tn) of A for the synthetic fill: its extent and leading
// dimension, the global index of its first element, the matrix order, seed.
inline TileArgs fill_args(TiledMatrix& A, int tm, int tn, uint32_t seed) {
  TileArgs a = tile_args(A.tile_rows(tm), A.tile_cols(tn), 0, A.mb());
  a.i0 = (int64_t)tm * A.mb();
  a.j0 = (int64_t)tn * A.nb();
  a.N = A.m();
  a.seed = seed;
  return a;
}

// Arguments of tc_gemm_nn: C = alpha op(A) B + beta C.
struct GemmNNArgs {
  int m, n, k, lda, ldb, ldc;
  double alpha, beta;
  int transA = 0;  // 1: C = alpha*A^T*B + beta*C
};

// Arguments of tc_trsm_solve: a triangular solve from the left with the
// factor in a diagonal tile.
struct TrsmSolveArgs {
  int m, n, lda, ldb;
  int trans;  // 0: solve T Z = B; 1: solve T^T Z = B
  int upper = 0;  // triangle of the diagonal tile holding the factor
  int unit = 0;   // unit diagonal (LU's L)
};

// Every task-class id of the process in one place: the id is the key of the
// trace header's class dictionary (profiling.cpp) and the row of the PINS
// per-class counters (pins_modules.cpp), so two classes must never share
// one. Python-defined classes (pybind.cpp) all share TC_PY_TASK; giving each
// its own id would need dynamic assignment.
enum TaskClassId : int {
  // kernels_blas.cpp
  TC_SPD_FILL = 1, TC_POTRF = 2, TC_TRSM = 3, TC_SYRK = 4, TC_GEMM = 5,
  TC_TRTRI = 6, TC_TRSM_INV = 7,
  // kernels_qr.cpp
  TC_GEQRT = 10, TC_UNMQR = 11, TC_TSQRT = 12, TC_TSMQR = 13,
  // kernels_bf16.cpp
  TC_FILL_BF16 = 20, TC_GEMM_BF16 = 21,
  // kernels_panel.cpp
  TC_PANEL_FILL = 24, TC_PANEL_FACTOR = 25, TC_PANEL_UPDATE = 26,
  // kernels_collections.cpp
  TC_COPY_TILE = 30, TC_SCALE = 31, TC_ADD_TILE = 32, TC_ADD2 = 33,
  TC_STENCIL3 = 34, TC_REGRID_ZERO = 36, TC_REGRID_PIECE = 37,
  // kernels_lu.cpp
  TC_GETRF_NOPIV = 40, TC_LU_TRSM_L = 41, TC_LU_TRSM_U = 42, TC_LU_GEMM = 43,
  TC_LU_TRTRI = 44, TC_LU_TRSM_L_INV = 45, TC_LU_TRSM_U_INV = 46,
  // kernels_qr_bcgs.cpp
  TC_QR_GEMM_TN = 50, TC_QR_ZERO = 51, TC_QR_TRI_TT = 52, TC_QR_GEMM_NN = 53,
  // kernels_reshape.cpp
  TC_RESHAPE = 60,
  // kernels_blas.cpp (gemm_nn, trsm_solve), kernels_collections.cpp (advise)
  TC_GEMM_NN = 70, TC_ADVISE_PREFETCH = 71, TC_TRSM_SOLVE = 72,
  // kernels_inv.cpp
  TC_INV_TRSM_R = 80, TC_TRTRI_INPLACE = 81, TC_SYRK_T = 82, TC_GEMM_TN = 83,
  TC_TRMM_LLT = 84, TC_LAUUM = 85,
  // pybind.cpp
  TC_PY_TASK = 100,
};

// A task class with a CPU and a GPU incarnation, registered with the
// profiler under `id` (kernels_blas.cpp). Every kernels_*.cpp builds its
// classes through this; registering an id twice under different names is
// fatal. `blocking` runs the GPU chore on a worker thread (it may host-sync).
TaskClass make_tc(const char* name, TaskKind kind, void (*cpu)(Task&),
                  void (*gpu)(Task&, GpuTaskCtx&), TaskClassId id,
                  bool blocking = false);

// Registered once; ids stable.
TaskClass& tc_spd_fill();
TaskClass& tc_potrf();
TaskClass& tc_trsm();
TaskClass& tc_syrk();
TaskClass& tc_gemm();
TaskClass& tc_gemm_nn();
TaskClass& tc_trsm_solve();
// PARSEC_MCA_chore_gemm_nn=hip: C -= A B tasks take the hand NN kernel.
bool gemm_nn_hip();

TaskClass& tc_trtri();
TaskClass& tc_trsm_inv();
// The inversion loop of the CPU trtri chores: W's lower triangle <- L^-1
// for the n x n lower triangular L; nothing above W's diagonal is written.
void cpu_trtri_lower(int n, const double* L, int ldl, double* W, int ldw);
TaskClass& tc_geqrt();
TaskClass& tc_unmqr();
TaskClass& tc_tsqrt();
TaskClass& tc_tsmqr();

// Build the DAGs (DTD insertion; SPMD-safe: call on every rank).
void insert_spd_fill(Dtd& tp, TiledMatrix& A, uint32_t seed);
void insert_full_fill(Dtd& tp, TiledMatrix& A, uint32_t seed);
void insert_potrf(Dtd& tp, TiledMatrix& A);
// Householder tile QR, M >= N: R in the upper tiles, reflectors not kept.
void insert_geqrf(Dtd& tp, TiledMatrix& A);
// QR by block Gram-Schmidt with CholeskyQR2 panels (matrix-core rates;
// cond(A) <~ 1e7): A becomes the explicit orthonormal Q, R the upper
// tiles (kernels_qr_bcgs.cpp).
void insert_geqrf_bcgs(Dtd& tp, TiledMatrix& A, TiledMatrix& R);
void insert_getrf_nopiv(Dtd& tp, TiledMatrix& A);
void insert_fill_bf16(Dtd& tp, TiledMatrix& A, uint32_t seed);
void insert_gemm_bf16(Dtd& tp, TiledMatrix& At, TiledMatrix& B, TiledMatrix& C);
void insert_redistribute(Dtd& tp, TiledMatrix& Src, TiledMatrix& Dst);
void insert_reduce_axis(Dtd& tp, TiledMatrix& A, TiledMatrix& R, int axis);
void insert_band_to_rect(Dtd& tp, TiledMatrix& S, TiledMatrix& D);
void insert_subtile_extract(Dtd& tp, TiledMatrix& A, int tm, int tn,
                            TiledMatrix& S);
void insert_subtile_insert(Dtd& tp, TiledMatrix& S, TiledMatrix& A, int tm,
                           int tn);
void insert_apply_scale(Dtd& tp, TiledMatrix& A, double alpha, double beta);
// Tiled C = A*B, fp64 NN (idempotent DAG: k==0 overwrites C — the hipGraph
// capture/replay demo workload, and a plain library-GEMM DAG generally).
void insert_gemm_fp64(Dtd& tp, TiledMatrix& A, TiledMatrix& B, TiledMatrix& C);
// data_advise analog: prefetch one tile onto the device (no-op body).
void insert_advise_prefetch(Dtd& tp, Data* d);
// Cholesky solve / factor+solve (dplasma dpotrs/dposv analogs).
void insert_potrs(Dtd& tp, TiledMatrix& A, TiledMatrix& B);
void insert_posv(Dtd& tp, TiledMatrix& A, TiledMatrix& B);
// SPD inverse, in place on the lower tiles (dplasma dtrtri/dlauum/dpotri/
// dpoinv analogs): trtri turns L into W = L^-1, lauum turns W into the
// lower tiles of W^T W, potri = trtri + lauum on a factor from insert_potrf,
// poinv = potrf + potri in one taskpool.
void insert_trtri(Dtd& tp, TiledMatrix& A);
void insert_lauum(Dtd& tp, TiledMatrix& A);
void insert_potri(Dtd& tp, TiledMatrix& A);
void insert_poinv(Dtd& tp, TiledMatrix& A);
// LU solve / factor+solve, no pivoting (dgetrs/dgesv nopiv analogs).
void insert_getrs_nopiv(Dtd& tp, TiledMatrix& A, TiledMatrix& B);
void insert_gesv_nopiv(Dtd& tp, TiledMatrix& A, TiledMatrix& B);
// Least squares via BCGS QR (dgels analog): X = R^-1 Q^T B.
void insert_gels_bcgs(Dtd& tp, TiledMatrix& A, TiledMatrix& R,
                      TiledMatrix& B, TiledMatrix& X);
// Householder least squares / solve (dgels analog, M >= N, full column
// rank; a square A makes it the general solver): A's upper tiles get R as
// after insert_geqrf, rows [0, N) of B get X, rows [N, M) the residual part
// of Q^T B (kernels_qr.cpp).
void insert_gels(Dtd& tp, TiledMatrix& A, TiledMatrix& B);
void insert_reduce_sum(Dtd& tp, TiledMatrix& A, TiledMatrix& R);
// log-depth binary-tree variant (BT_reduction.jdf analog).
void insert_reduce_sum_tree(Dtd& tp, TiledMatrix& A, TiledMatrix& R);
void insert_stencil_1d(Dtd& tp, TiledMatrix& Src, TiledMatrix& Dst);

// One triangular sweep of a tiled solve (kernels_solve.cpp): for column tile
// j of B, solve op(F) Z = B over the first `rows` tile rows of B in place,
// with the triangular factor in F's leading rows x rows tiles. Each step k
// is one trsm_solve on the diagonal tile F(k,k) (upper, trans, unit as
// given) and then the gemm_nn updates B(i,j) -= op(F)(i,k) B(k,j) of the
// rows still to be solved. {lower, N} and {upper, T} sweep forward (k
// ascending, i = k+1..), the other two backward (k descending, i = k-1..0).
// Without trans the update reads tile F(i,k); with it, F(k,i) transposed.
void insert_tri_sweep(Dtd& tp, TiledMatrix& F, int rows, TiledMatrix& B, int j,
                      bool upper, bool trans, bool unit);
void insert_panel_fill(Dtd& tp, TiledMatrix& A, uint32_t seed);
void insert_potrf_panel(Dtd& tp, TiledMatrix& A);

// Most workgroups one panel-kernel launch may have. The kernel's workgroups
// spin on each other's counters, so all of them must be resident at once,
// and each takes a whole CU (about 150 KiB of LDS).
constexpr int QR_PANEL_MAX_WGS = 48;

// Test entry point of the QR panel factorization (kernels_qr.cpp): host
// buffers in, factored A and the k x k T out. impl: 0 hand kernels, 1
// rocSOLVER route, 2 CPU kernels.
void test_qr_factor_hip(double* A, size_t a_elems, int m, int k, int lda,
                        int ts_split, int impl, int wgs, int poolA,
                        const std::string& apply, int lookahead, double* T);

}  // namespace pa
