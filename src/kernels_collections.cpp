// Collection operators: whole-collection data movement and elementwise /
// reduction DAGs over the tiles of a TiledMatrix — copy, scale, add, the
// three reduces, redistribute / regrid, band -> rect, subtile views, the 1-D
// stencil and the prefetch advice. None of them is linear algebra; each
// class has a plain HIP kernel (or a copy) as its GPU chore and a loop as
// its CPU chore.
#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include "device_gpu.hpp"

namespace pa {

// ---------------------------------------------------------- copy / apply
// Redistribution (data_dist/matrix/redistribute analog, same tile grid,
// any rank grids) and the generic elementwise operator (map_operator.c /
// apply.jdf analog; the scale op x = alpha*x + beta is the built-in).
__global__ void k_scale_tile(double* p, size_t n, double alpha, double beta) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = p[i] * alpha + beta;
}

static void cpu_copy_tile(Task& t) {
  Data* src = t.flows[0].data;
  Data* dst = t.flows[1].data;
  memcpy(dst->ensure_host(), src->pull_to_host(), src->bytes);
  dst->written_on(false);
}

static void gpu_copy_tile(Task& t, GpuTaskCtx& g) {
  Data* src = t.flows[0].data;
  PA_HIP_CHECK(hipMemcpyAsync(t.dev_ptr[1], t.dev_ptr[0], src->bytes,
                              hipMemcpyDeviceToDevice, g.stream));
}

static void cpu_scale(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  double alpha, beta;
  memcpy(&alpha, &a.i0, 8);
  memcpy(&beta, &a.j0, 8);
  Data* d = t.flows[0].data;
  double* p = (double*)d->pull_to_host();
  for (size_t i = 0; i < d->bytes / 8; i++) p[i] = p[i] * alpha + beta;
  d->written_on(false);
}

static void gpu_scale(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  double alpha, beta;
  memcpy(&alpha, &a.i0, 8);
  memcpy(&beta, &a.j0, 8);
  Data* d = t.flows[0].data;
  hipLaunchKernelGGL(k_scale_tile, dim3(2048), dim3(256), 0, g.stream,
                     (double*)t.dev_ptr[0], d->bytes / 8, alpha, beta);
}

static TaskClass& tc_copy_tile() {
  static TaskClass tc = make_tc("copy_tile", TaskKind::GPU, cpu_copy_tile,
                                gpu_copy_tile, TC_COPY_TILE);
  return tc;
}
static TaskClass& tc_scale() {
  static TaskClass tc =
      make_tc("scale", TaskKind::GPU, cpu_scale, gpu_scale, TC_SCALE);
  return tc;
}

__global__ void k_add_tile(double* dst, const double* src, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] += src[i];
}

static void cpu_add_tile(Task& t) {
  Data* a = t.flows[0].data;
  Data* c = t.flows[1].data;
  const double* p = (const double*)a->pull_to_host();
  double* q = (double*)c->pull_to_host();
  for (size_t i = 0; i < c->bytes / 8; i++) q[i] += p[i];
  c->written_on(false);
}

static void gpu_add_tile(Task& t, GpuTaskCtx& g) {
  Data* c = t.flows[1].data;
  hipLaunchKernelGGL(k_add_tile, dim3(2048), dim3(256), 0, g.stream,
                     (double*)t.dev_ptr[1], (const double*)t.dev_ptr[0],
                     c->bytes / 8);
}

static TaskClass& tc_add_tile() {
  static TaskClass tc = make_tc("add_tile", TaskKind::GPU, cpu_add_tile,
                                gpu_add_tile, TC_ADD_TILE);
  return tc;
}

// out = a + b (pure OUTPUT third flow — the tree-reduction combiner)
__global__ void k_add2(double* out, const double* a, const double* b,
                       size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = a[i] + b[i];
}

static void cpu_add2(Task& t) {
  const double* a = (const double*)t.flows[0].data->pull_to_host();
  const double* b = (const double*)t.flows[1].data->pull_to_host();
  Data* o = t.flows[2].data;
  double* q = (double*)o->ensure_host();
  for (size_t i = 0; i < o->bytes / 8; i++) q[i] = a[i] + b[i];
  o->written_on(false);
}

static void gpu_add2(Task& t, GpuTaskCtx& g) {
  Data* o = t.flows[2].data;
  hipLaunchKernelGGL(k_add2, dim3(2048), dim3(256), 0, g.stream,
                     (double*)t.dev_ptr[2], (const double*)t.dev_ptr[0],
                     (const double*)t.dev_ptr[1], o->bytes / 8);
}

static TaskClass& tc_add2() {
  static TaskClass tc =
      make_tc("add2", TaskKind::GPU, cpu_add2, gpu_add2, TC_ADD2);
  return tc;
}

// result += sum of all tiles of A (reduce.jdf / DTD reduce analog).
// The accumulation chains on `result`; contributions from each rank's
// tiles flow through the comm engine automatically.
// Binary-tree reduction (BT_reduction.jdf analog): log2(N) critical path
// instead of the flat chain's N. Internal workspace tiles are owned by
// the taskpool (the bcgs-style pattern); pair placement follows the left
// operand so cross-rank combines ride the normal dataflow.
void insert_reduce_sum_tree(Dtd& tp, TiledMatrix& A, TiledMatrix& R) {
  std::vector<Data*> level;
  std::vector<int> lrank;
  for (int m = 0; m < A.mt(); m++)
    for (int n = 0; n < (A.sym() ? m + 1 : A.nt()); n++) {
      level.push_back(A.tile(m, n));
      lrank.push_back(A.rank_of(m, n));
    }
  PA_CHECK(!level.empty(), "reduce_sum_tree: empty collection");
  auto* ctx = A.ctx();
  // one workspace strip holds every internal node (N-1 combines)
  int nw = (int)level.size();  // >= combines + final copy target
  auto W = std::make_shared<TiledMatrix>(ctx, (int64_t)A.mb() * nw, A.nb(),
                                         A.mb(), A.nb(), 1, 1);
  {
    std::vector<int> ranks((size_t)nw);
    for (int i = 0; i < nw; i++) ranks[i] = lrank[i % lrank.size()];
    W->set_rank_table(std::move(ranks));
  }
  tp.own(W);
  int wi = 0;
  while (level.size() > 1) {
    std::vector<Data*> next;
    std::vector<int> nrank;
    for (size_t i = 0; i + 1 < level.size(); i += 2) {
      bool last = level.size() == 2;
      Data* out = last ? R.tile(0, 0) : W->tile(wi, 0);
      int orank = last ? R.rank_of(0, 0) : lrank[i];
      if (!last) wi++;
      Dtd::FlowSpec f[] = {{level[i], ACCESS_IN},
                           {level[i + 1], ACCESS_IN},
                           {out, ACCESS_OUT}};
      tp.insert(&tc_add2(), nullptr, 0, f, 3, 0, orank);
      next.push_back(out);
      nrank.push_back(orank);
    }
    if (level.size() % 2) {  // odd leftover promotes unchanged
      next.push_back(level.back());
      nrank.push_back(lrank.back());
    }
    level.swap(next);
    lrank.swap(nrank);
  }
  if (level[0] != R.tile(0, 0)) {
    // single-tile collection: copy the lone input into R
    Dtd::FlowSpec f[] = {{level[0], ACCESS_IN}, {R.tile(0, 0), ACCESS_OUT}};
    tp.insert(&tc_copy_tile(), nullptr, 0, f, 2, 0, R.rank_of(0, 0));
  }
}

void insert_reduce_sum(Dtd& tp, TiledMatrix& A, TiledMatrix& R) {
  Data* r = R.tile(0, 0);
  for (int m = 0; m < A.mt(); m++)
    for (int n = 0; n < (A.sym() ? m + 1 : A.nt()); n++) {
      Dtd::FlowSpec f[] = {{A.tile(m, n), ACCESS_IN}, {r, ACCESS_INOUT}};
      tp.insert(&tc_add_tile(), nullptr, 0, f, 2, 0, R.rank_of(0, 0));
    }
}

// Reduce along one axis (reduce_col/reduce_row.jdf analogs): R's single
// tile row (axis=0: R is 1 x nt tiles, each = sum over the tile column)
// or tile column (axis=1) accumulates elementwise tile sums: the first
// addend copies (defining R's content), the rest add.
void insert_reduce_axis(Dtd& tp, TiledMatrix& A, TiledMatrix& R, int axis) {
  PA_CHECK(axis == 0 || axis == 1, "axis must be 0 (columns) or 1 (rows)");
  PA_CHECK(!A.sym(), "reduce_axis: dense collections only");
  const int outer = axis == 0 ? A.nt() : A.mt();
  const int inner = axis == 0 ? A.mt() : A.nt();
  PA_CHECK((axis == 0 ? R.nt() : R.mt()) == outer &&
               (axis == 0 ? R.mt() : R.nt()) == 1 &&
               R.tile_bytes() == A.tile_bytes(),
           "reduce_axis: R must be a single tile row/column matching A");
  for (int o = 0; o < outer; o++) {
    Data* r = axis == 0 ? R.tile(0, o) : R.tile(o, 0);
    const int rrank = axis == 0 ? R.rank_of(0, o) : R.rank_of(o, 0);
    for (int i = 0; i < inner; i++) {
      Data* a = axis == 0 ? A.tile(i, o) : A.tile(o, i);
      if (i == 0) {
        Dtd::FlowSpec f[] = {{a, ACCESS_IN}, {r, ACCESS_OUT}};
        tp.insert(&tc_copy_tile(), nullptr, 0, f, 2, 0, rrank);
      } else {
        Dtd::FlowSpec f[] = {{a, ACCESS_IN}, {r, ACCESS_INOUT}};
        tp.insert(&tc_add_tile(), nullptr, 0, f, 2, 0, rrank);
      }
    }
  }
}

// ---- general regridding (redistribute.jdf incl. non-matching tile grids,
// data_dist/matrix/redistribute/redistribute.jdf analog) ----
// One CPU piece-task per (dst tile, overlapping src tile): copies the
// intersection rectangle. Pieces of one dst tile serialize through INOUT
// chaining; cross-rank movement falls out of the normal protocol. A
// leading zero-task defines regions no src tile covers.
namespace {
struct RegridArgs {
  int r, c;        // rectangle extent (rows, cols)
  int si, sj;      // offset in src tile
  int di, dj;      // offset in dst tile
  int lds, ldd;    // column strides (elements)
  int elem;        // element size in bytes
};

void cpu_regrid_zero(Task& t) {
  Data* d = t.flows[0].data;
  memset(d->ensure_host(), 0, d->bytes);
  d->written_on(false);
}

void cpu_regrid_piece(Task& t) {
  const RegridArgs& a = t.arg<RegridArgs>();
  const char* s = (const char*)t.flows[0].data->pull_to_host();
  Data* dd = t.flows[1].data;
  char* d;
  if (t.flows[1].mode & ACCESS_IN) {
    d = (char*)dd->pull_to_host();
  } else {
    // OUT-only piece fully covers its destination (subtile extract)
    dd->begin_host_overwrite();
    d = (char*)dd->ensure_host();
  }
  const size_t rb = (size_t)a.r * a.elem;
  for (int j = 0; j < a.c; j++)
    memcpy(d + ((size_t)(a.dj + j) * a.ldd + a.di) * a.elem,
           s + ((size_t)(a.sj + j) * a.lds + a.si) * a.elem, rb);
  t.flows[1].data->written_on(false);
}

TaskClass& tc_regrid_zero() {
  static TaskClass tc = make_tc("regrid_zero", TaskKind::CPU, cpu_regrid_zero,
                                nullptr, TC_REGRID_ZERO);
  return tc;
}
TaskClass& tc_regrid_piece() {
  static TaskClass tc = make_tc("regrid_piece", TaskKind::CPU,
                                cpu_regrid_piece, nullptr, TC_REGRID_PIECE);
  return tc;
}
}  // namespace

void insert_redistribute(Dtd& tp, TiledMatrix& Src, TiledMatrix& Dst) {
  if (Src.mt() == Dst.mt() && Src.nt() == Dst.nt() &&
      Src.tile_bytes() == Dst.tile_bytes()) {
    // fast path: same tile grid — one (GPU-capable) whole-tile copy each
    for (int m = 0; m < Src.mt(); m++)
      for (int n = 0; n < (Src.sym() ? m + 1 : Src.nt()); n++) {
        Dtd::FlowSpec f[] = {{Src.tile(m, n), ACCESS_IN},
                             {Dst.tile(m, n), ACCESS_OUT}};
        tp.insert(&tc_copy_tile(), nullptr, 0, f, 2, 0, Dst.rank_of(m, n));
      }
    return;
  }
  PA_CHECK(Src.m() == Dst.m() && Src.n() == Dst.n() &&
           Src.elem_size() == Dst.elem_size() && !Src.sym() && !Dst.sym(),
           "redistribute: matrices must have equal global shape/dtype "
           "(sym storage regridding unsupported)");
  for (int dm = 0; dm < Dst.mt(); dm++)
    for (int dn = 0; dn < Dst.nt(); dn++) {
      const int rank = Dst.rank_of(dm, dn);
      {
        Dtd::FlowSpec f[] = {{Dst.tile(dm, dn), ACCESS_OUT}};
        tp.insert(&tc_regrid_zero(), nullptr, 0, f, 1, 0, rank);
      }
      const int64_t r0 = (int64_t)dm * Dst.mb(), r1 = r0 + Dst.tile_rows(dm);
      const int64_t c0 = (int64_t)dn * Dst.nb(), c1 = c0 + Dst.tile_cols(dn);
      for (int sm = (int)(r0 / Src.mb()); (int64_t)sm * Src.mb() < r1; sm++)
        for (int sn = (int)(c0 / Src.nb()); (int64_t)sn * Src.nb() < c1;
             sn++) {
          const int64_t sr0 = (int64_t)sm * Src.mb();
          const int64_t sc0 = (int64_t)sn * Src.nb();
          const int64_t ir0 = std::max(r0, sr0);
          const int64_t ir1 = std::min(r1, sr0 + Src.tile_rows(sm));
          const int64_t ic0 = std::max(c0, sc0);
          const int64_t ic1 = std::min(c1, sc0 + Src.tile_cols(sn));
          if (ir1 <= ir0 || ic1 <= ic0) continue;
          RegridArgs a;
          a.r = (int)(ir1 - ir0);
          a.c = (int)(ic1 - ic0);
          a.si = (int)(ir0 - sr0);
          a.sj = (int)(ic0 - sc0);
          a.di = (int)(ir0 - r0);
          a.dj = (int)(ic0 - c0);
          a.lds = Src.mb();
          a.ldd = Dst.mb();
          a.elem = (int)Src.elem_size();
          Dtd::FlowSpec f[] = {{Src.tile(sm, sn), ACCESS_IN},
                               {Dst.tile(dm, dn), ACCESS_INOUT}};
          tp.insert(&tc_regrid_piece(), &a, sizeof(a), f, 2, 0, rank);
        }
    }
}

// ---- band -> rectangular conversion (diag_band_to_rect.jdf analog) ----
// Copies a band-stored collection into a dense one; out-of-band tiles of
// the destination are zero-filled (they have no source).
void insert_band_to_rect(Dtd& tp, TiledMatrix& S, TiledMatrix& D) {
  PA_CHECK(S.mt() == D.mt() && S.nt() == D.nt() &&
           S.tile_bytes() == D.tile_bytes() && !D.sym(),
           "band_to_rect: matching tile grids required");
  for (int m = 0; m < S.mt(); m++)
    for (int n = 0; n < S.nt(); n++) {
      const int rank = D.rank_of(m, n);
      if (S.in_band(m, n)) {
        Dtd::FlowSpec f[] = {{S.tile(m, n), ACCESS_IN},
                             {D.tile(m, n), ACCESS_OUT}};
        tp.insert(&tc_copy_tile(), nullptr, 0, f, 2, 0, rank);
      } else {
        Dtd::FlowSpec f[] = {{D.tile(m, n), ACCESS_OUT}};
        tp.insert(&tc_regrid_zero(), nullptr, 0, f, 1, 0, rank);
      }
    }
}

// ---- recursive subtiling (subtile.c analog) ----
// View ONE tile of A as its own tiled collection S (same global shape as
// the tile, finer tiles), by copy: extract pieces tile->S, run any DAG on
// S (e.g. a recursive factorization of a diagonal block), insert back.
// The copies ride the normal dataflow, so extraction chains after the
// tile's last writer and write-back chains before its next reader —
// including across ranks.
void insert_subtile_extract(Dtd& tp, TiledMatrix& A, int tm, int tn,
                            TiledMatrix& S) {
  PA_CHECK(S.m() == A.tile_rows(tm) && S.n() == A.tile_cols(tn) &&
           S.elem_size() == A.elem_size() && !S.sym(),
           "subtile: S must have the tile's global shape");
  Data* src = A.tile(tm, tn);
  const int rank = A.rank_of(tm, tn);
  for (int i = 0; i < S.mt(); i++)
    for (int j = 0; j < S.nt(); j++) {
      RegridArgs a;
      a.r = S.tile_rows(i);
      a.c = S.tile_cols(j);
      a.si = i * S.mb();
      a.sj = j * S.nb();
      a.di = 0;
      a.dj = 0;
      a.lds = A.mb();
      a.ldd = S.mb();
      a.elem = (int)A.elem_size();
      Dtd::FlowSpec f[] = {{src, ACCESS_IN}, {S.tile(i, j), ACCESS_OUT}};
      tp.insert(&tc_regrid_piece(), &a, sizeof(a), f, 2, 0, rank);
    }
}

void insert_subtile_insert(Dtd& tp, TiledMatrix& S, TiledMatrix& A, int tm,
                           int tn) {
  PA_CHECK(S.m() == A.tile_rows(tm) && S.n() == A.tile_cols(tn) &&
           S.elem_size() == A.elem_size() && !S.sym(),
           "subtile: S must have the tile's global shape");
  Data* dst = A.tile(tm, tn);
  const int rank = A.rank_of(tm, tn);
  for (int i = 0; i < S.mt(); i++)
    for (int j = 0; j < S.nt(); j++) {
      RegridArgs a;
      a.r = S.tile_rows(i);
      a.c = S.tile_cols(j);
      a.si = 0;
      a.sj = 0;
      a.di = i * S.mb();
      a.dj = j * S.nb();
      a.lds = S.mb();
      a.ldd = A.mb();
      a.elem = (int)A.elem_size();
      Dtd::FlowSpec f[] = {{S.tile(i, j), ACCESS_IN}, {dst, ACCESS_INOUT}};
      tp.insert(&tc_regrid_piece(), &a, sizeof(a), f, 2, 0, rank);
    }
}

void insert_apply_scale(Dtd& tp, TiledMatrix& A, double alpha, double beta) {
  for (int m = 0; m < A.mt(); m++)
    for (int n = 0; n < (A.sym() ? m + 1 : A.nt()); n++) {
      TileArgs a;
      memcpy(&a.i0, &alpha, 8);
      memcpy(&a.j0, &beta, 8);
      Dtd::FlowSpec f[] = {{A.tile(m, n), ACCESS_INOUT}};
      tp.insert(&tc_scale(), &a, sizeof(a), f, 1, 0, A.rank_of(m, n));
    }
}

// ---------------------------------------------------------------- stencil
// 1-D 3-point stencil over a vector of tiles (tests/apps/stencil analog):
// dst[i] = (src[i-1] + src[i] + src[i+1]) / 3 with halos crossing tile
// boundaries through neighbor-tile flows (zero at domain edges).
__global__ void k_stencil3(double* dst, const double* left,
                           const double* mid, const double* right, int nbe) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < nbe; i += gridDim.x * blockDim.x) {
    double l = i > 0 ? mid[i - 1] : (left ? left[nbe - 1] : 0.0);
    double r = i < nbe - 1 ? mid[i + 1] : (right ? right[0] : 0.0);
    dst[i] = (l + mid[i] + r) / 3.0;
  }
}

static void cpu_stencil3(Task& t) {
  const TileArgs& a = t.arg<TileArgs>();
  const int nbe = a.m;
  const double* left =
      t.flows[1].data ? (const double*)t.flows[1].data->pull_to_host() : nullptr;
  const double* mid = (const double*)t.flows[0].data->pull_to_host();
  const double* right =
      t.flows[2].data ? (const double*)t.flows[2].data->pull_to_host() : nullptr;
  double* dst = (double*)t.flows[3].data->ensure_host();
  for (int i = 0; i < nbe; i++) {
    double l = i > 0 ? mid[i - 1] : (left ? left[nbe - 1] : 0.0);
    double r = i < nbe - 1 ? mid[i + 1] : (right ? right[0] : 0.0);
    dst[i] = (l + mid[i] + r) / 3.0;
  }
  t.flows[3].data->written_on(false);
}

static void gpu_stencil3(Task& t, GpuTaskCtx& g) {
  const TileArgs& a = t.arg<TileArgs>();
  hipLaunchKernelGGL(k_stencil3, dim3(64), dim3(256), 0, g.stream,
                     (double*)t.dev_ptr[3], (const double*)t.dev_ptr[1],
                     (const double*)t.dev_ptr[0], (const double*)t.dev_ptr[2],
                     a.m);
}

static TaskClass& tc_stencil3() {
  static TaskClass tc = make_tc("stencil3", TaskKind::GPU, cpu_stencil3,
                                gpu_stencil3, TC_STENCIL3);
  return tc;
}

// One stencil sweep Src -> Dst (tile vectors: mt x 1 tiles of mb x 1).
void insert_stencil_1d(Dtd& tp, TiledMatrix& Src, TiledMatrix& Dst) {
  PA_CHECK(Src.nt() == 1 && Dst.nt() == 1 && Src.mt() == Dst.mt());
  const int T = Src.mt();
  for (int t = 0; t < T; t++) {
    TileArgs a = tile_args(Src.tile_rows(t) * Src.tile_cols(0), 0, 0, 0);
    Dtd::FlowSpec f[4];
    f[0] = {Src.tile(t, 0), ACCESS_IN};
    f[1] = {t > 0 ? Src.tile(t - 1, 0) : nullptr, ACCESS_IN};
    f[2] = {t < T - 1 ? Src.tile(t + 1, 0) : nullptr, ACCESS_IN};
    f[3] = {Dst.tile(t, 0), ACCESS_OUT};
    tp.insert(&tc_stencil3(), &a, sizeof(a), f, 4, 0, Dst.rank_of(t, 0));
  }
}

// --------------------------------------------------------------- advise
// parsec_advise_data_on_device analog (device.h data_advise vtable row):
// a no-op GPU task with one READ flow — the engine's normal stage-in
// pulls the tile onto the device ahead of its first real consumer, on
// the h2d stream, overlapped with whatever is executing. On CPU-only
// contexts it degenerates to a no-op CPU task.
static void cpu_advise(Task&) {}
static void gpu_advise(Task&, GpuTaskCtx&) {}
static TaskClass& tc_advise() {
  static TaskClass tc = make_tc("advise_prefetch", TaskKind::GPU, cpu_advise,
                                gpu_advise, TC_ADVISE_PREFETCH);
  return tc;
}

void insert_advise_prefetch(Dtd& tp, Data* d) {
  Dtd::FlowSpec f[] = {{d, ACCESS_IN}};
  TileArgs a{};
  tp.insert(&tc_advise(), &a, sizeof(a), f, 1, 0, -1);
}

}  // namespace pa
