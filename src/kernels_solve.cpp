// Tiled triangular solves: the one tile sweep every solve is made of, and
// the solves built on it — Cholesky (potrs/posv), LU without pivoting
// (getrs/gesv), least squares through the BCGS QR (gels_bcgs). The
// Householder insert_gels (kernels_qr.cpp) uses the sweep too. The chores
// are the generic trsm_solve and gemm_nn of kernels_blas.cpp.
#include "kernels.hpp"

namespace pa {

void insert_tri_sweep(Dtd& tp, TiledMatrix& F, int rows, TiledMatrix& B, int j,
                      bool upper, bool trans, bool unit) {
  auto solve = [&](int k) {
    TrsmSolveArgs a{B.tile_rows(k), B.tile_cols(j), F.mb(), B.mb(), trans};
    a.upper = upper;
    a.unit = unit;
    Dtd::FlowSpec f[] = {{F.tile(k, k), ACCESS_IN},
                         {B.tile(k, j), ACCESS_INOUT}};
    tp.insert(&tc_trsm_solve(), &a, sizeof(a), f, 2, (1 << 20),
              B.rank_of(k, j));
  };
  auto update = [&](int i, int k) {
    GemmNNArgs a{B.tile_rows(i), B.tile_cols(j), B.tile_rows(k),
                 F.mb(),         B.mb(),         B.mb(),
                 -1.0,           1.0};
    a.transA = trans;
    Dtd::FlowSpec f[] = {{trans ? F.tile(k, i) : F.tile(i, k), ACCESS_IN},
                         {B.tile(k, j), ACCESS_IN},
                         {B.tile(i, j), ACCESS_INOUT}};
    tp.insert(&tc_gemm_nn(), &a, sizeof(a), f, 3, 0, B.rank_of(i, j));
  };
  if (upper == trans) {  // forward
    for (int k = 0; k < rows; k++) {
      solve(k);
      for (int i = k + 1; i < rows; i++) update(i, k);
    }
  } else {
    for (int k = rows - 1; k >= 0; k--) {
      solve(k);
      for (int i = k - 1; i >= 0; i--) update(i, k);
    }
  }
}

// Cholesky SOLVE (dplasma dpotrs/dposv analog): after insert_potrf left
// A's lower tiles holding L, solve A X = B for a block of right-hand
// sides: forward L Y = B, then backward L^T X = Y (the lower tile (k,i)
// transposed is the update's operand).
void insert_potrs(Dtd& tp, TiledMatrix& A, TiledMatrix& B) {
  PA_CHECK(A.mt() == A.nt() && A.mt() == B.mt(),
           "insert_potrs: A must be square with B.mt == A.mt");
  for (int j = 0; j < B.nt(); j++) {
    insert_tri_sweep(tp, A, A.mt(), B, j, /*upper=*/false, /*trans=*/false,
                     /*unit=*/false);
    insert_tri_sweep(tp, A, A.mt(), B, j, /*upper=*/false, /*trans=*/true,
                     /*unit=*/false);
  }
}

void insert_posv(Dtd& tp, TiledMatrix& A, TiledMatrix& B) {
  insert_potrf(tp, A);
  insert_potrs(tp, A, B);
}

// LU solve (dplasma dgetrs/dgesv nopiv analogs): after insert_getrf_nopiv
// left L (unit lower) and U (upper) packed in A's tiles, solve A X = B:
// forward L Y = B (unit diagonal), then backward U X = Y. Off-diagonal
// updates use A's tiles directly: forward uses the strictly-lower tiles
// (which hold L), backward the strictly-upper tiles (which hold U).
void insert_getrs_nopiv(Dtd& tp, TiledMatrix& A, TiledMatrix& B) {
  PA_CHECK(A.mt() == A.nt() && A.mt() == B.mt(),
           "insert_getrs_nopiv: A must be square with B.mt == A.mt");
  for (int j = 0; j < B.nt(); j++) {
    insert_tri_sweep(tp, A, A.mt(), B, j, /*upper=*/false, /*trans=*/false,
                     /*unit=*/true);
    insert_tri_sweep(tp, A, A.mt(), B, j, /*upper=*/true, /*trans=*/false,
                     /*unit=*/false);
  }
}

void insert_gesv_nopiv(Dtd& tp, TiledMatrix& A, TiledMatrix& B) {
  insert_getrf_nopiv(tp, A);
  insert_getrs_nopiv(tp, A, B);
}

// Least squares min ||A X - B|| via the BCGS QR (dgels analog, QR route):
// insert_geqrf_bcgs leaves Q explicit in A (m x n) and R (n x n upper) —
// X = R^{-1} Q^T B. Q^T B is a tiled TN GEMM chain; the triangular solve
// is a backward sweep with the upper-triangular trsm_solve. X must be
// A.nt x B.nt tiles. Inherits BCGS's cond(A) <~ 1e7 envelope.
void insert_gels_bcgs(Dtd& tp, TiledMatrix& A, TiledMatrix& R,
                      TiledMatrix& B, TiledMatrix& X) {
  insert_geqrf_bcgs(tp, A, R);
  PA_CHECK(X.mt() == A.nt() && X.nt() == B.nt() && B.mt() == A.mt(),
           "insert_gels_bcgs: X must be A.nt x B.nt tiles, B.mt == A.mt");
  // X[k,j] = sum_i Q[i,k]^T B[i,j]
  for (int k = 0; k < A.nt(); k++)
    for (int j = 0; j < B.nt(); j++)
      for (int i = 0; i < A.mt(); i++) {
        GemmNNArgs a{X.tile_rows(k), B.tile_cols(j), A.tile_rows(i),
                     A.mb(),         B.mb(),         X.mb(),
                     1.0,            i == 0 ? 0.0 : 1.0};
        a.transA = 1;
        Dtd::FlowSpec f[] = {{A.tile(i, k), ACCESS_IN},
                             {B.tile(i, j), ACCESS_IN},
                             {X.tile(k, j), i == 0 ? ACCESS_OUT
                                                   : ACCESS_INOUT}};
        tp.insert(&tc_gemm_nn(), &a, sizeof(a), f, 3, 0, X.rank_of(k, j));
      }
  // backward: R X = (Q^T B), R upper non-unit
  for (int j = 0; j < X.nt(); j++)
    insert_tri_sweep(tp, R, X.mt(), X, j, /*upper=*/true, /*trans=*/false,
                     /*unit=*/false);
}

}  // namespace pa
