// libxde_hip.so — output rows of a sub-stepped fixed-grid solve (C ABI: include/xde_hip_grid.h; host:
// paddlexde_amd/solver/base_fixed_solver.py).
//
// HBM-bandwidth bound: one launch reads the step's operands once — y_a, y_b (linear) plus f_a, f_b (cubic) — and writes up to
// XDE_INTERP_MAX_ROWS rows straight into the solution's [..., T*L, D] layout.  Written like xde_combine.hip and
// xde_backprop.hip: 16 bytes per lane when every pointer is 16-byte aligned and the row geometry keeps vectors whole, a scalar
// path with the same bits otherwise, the operand count and G compile-time constants so that every operand load is issued before
// the first one is used, and a grid-stride loop over at most grid_cap() workgroups of kBlock.
// Built with -ffp-contract=off like the rest of the library.

#include "xde_common.hpp"
#include "xde_hip_grid.h"

using namespace xde;

namespace {

constexpr int kMaxRows = XDE_INTERP_MAX_ROWS;

struct InterpArgs {
  void* rows[kMaxRows];
  double w[kMaxRows][4];
  int kind[kMaxRows];
  const void* op[4];   // y_a, y_b, f_a, f_b
  int64_t n;           // elements per operand
  int64_t chunk;       // contiguous elements of a row between two jumps
  int64_t row_gap;     // row_stride - chunk (0: the rows are contiguous)
};

template <typename T, int NOP, int G, bool VEC>
__global__ __launch_bounds__(kBlock) void xde_interp_rows_kernel(InterpArgs a) {
  using P = Pack<T, VEC>;
  constexpr int W = P::W;
  const T* op[NOP];
#pragma unroll
  for (int j = 0; j < NOP; ++j) op[j] = static_cast<const T*>(a.op[j]);
  T wt[G][4];
#pragma unroll
  for (int r = 0; r < G; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) wt[r][k] = T(a.w[r][k]);
  const int64_t nvec = a.n / W;  // (the vector path is only taken when chunk, hence n, is a multiple of W)
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < nvec; i += stride) {
    P x[NOP];
#pragma unroll
    for (int j = 0; j < NOP; ++j) x[j] = P::load(op[j], i);
    int64_t d = i;
    if (a.row_gap) {
      const int64_t e = i * W;
      d = (e + (e / a.chunk) * a.row_gap) / W;
    }
#pragma unroll
    for (int r = 0; r < G; ++r) {
      P o;
      if (a.kind[r] == XDE_ROW_COPY_A) {
        o = x[0];
      } else if (a.kind[r] == XDE_ROW_COPY_B) {
        o = x[1];
      } else {
#pragma unroll
        for (int v = 0; v < W; ++v) {
          if (NOP == 2) {
            o.v[v] = x[0].v[v] + wt[r][0] * (x[1].v[v] - x[0].v[v]);
          } else {
            o.v[v] = ((wt[r][0] * x[0].v[v] + wt[r][1] * x[NOP > 2 ? 2 : 0].v[v]) + wt[r][2] * x[1].v[v]) +
                     wt[r][3] * x[NOP > 3 ? 3 : 0].v[v];
          }
        }
      }
      o.store_nt(static_cast<T*>(a.rows[r]), d);  // (solution rows: nobody re-reads them soon)
    }
  }
}

template <typename T, int NOP, bool VEC>
void launch_rows(const InterpArgs& a, int G, dim3 g, dim3 b, hipStream_t st, ProfScope& prof) {
  switch (G) {
#define XDE_ROWS_CASE(N) \
    case N: XDE_LAUNCH((xde_interp_rows_kernel<T, NOP, N, VEC>), g, b, st, prof, a); break;
    XDE_ROWS_CASE(1) XDE_ROWS_CASE(2) XDE_ROWS_CASE(3) XDE_ROWS_CASE(4) XDE_ROWS_CASE(5) XDE_ROWS_CASE(6) XDE_ROWS_CASE(7)
    XDE_ROWS_CASE(8)
#undef XDE_ROWS_CASE
    default: break;
  }
}
static_assert(kMaxRows == 8, "launch_rows instantiates row counts 1..8");

template <typename T>
void launch_typed(const InterpArgs& a, int nop, int G, bool vec, dim3 g, dim3 b, hipStream_t st, ProfScope& prof) {
  if (nop == 2) vec ? launch_rows<T, 2, true>(a, G, g, b, st, prof) : launch_rows<T, 2, false>(a, G, g, b, st, prof);
  else vec ? launch_rows<T, 4, true>(a, G, g, b, st, prof) : launch_rows<T, 4, false>(a, G, g, b, st, prof);
}

bool aligned_to(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

}  // namespace

extern "C" {

int xde_interp_rows(void* const* rows, const int* kinds, const double* w, int G, const void* y_a, const void* y_b, const void* f_a,
                    const void* f_b, int mode, int64_t outer, int64_t chunk, int64_t row_stride, int dtype, void* stream) {
  if (!rows || !kinds || !w || !y_a || !y_b) return fail(XDE_EBADARG, "xde_interp_rows: null pointer");
  if (G < 1 || G > kMaxRows) return fail(XDE_EBADARG, "xde_interp_rows: G out of range (1 .. XDE_INTERP_MAX_ROWS)");
  if (mode != XDE_INTERP_LINEAR && mode != XDE_INTERP_CUBIC) return fail(XDE_EBADARG, "xde_interp_rows: bad mode");
  if (mode == XDE_INTERP_CUBIC && (!f_a || !f_b)) return fail(XDE_EBADARG, "xde_interp_rows: null pointer (cubic needs f_a and f_b)");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, "xde_interp_rows: bad dtype");
  if (outer < 0 || chunk < 0) return fail(XDE_EBADARG, "xde_interp_rows: negative outer or chunk");
  if (outer > 1 && row_stride < chunk) return fail(XDE_EBADARG, "xde_interp_rows: row_stride < chunk");
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const int nop = mode == XDE_INTERP_CUBIC ? 4 : 2;
  InterpArgs a;
  memset(&a, 0, sizeof(a));
  a.op[0] = y_a;
  a.op[1] = y_b;
  a.op[2] = f_a;
  a.op[3] = f_b;
  for (int j = 0; j < nop; ++j)
    if (!aligned_to(a.op[j], esz)) return fail(XDE_EBADARG, "xde_interp_rows: operand not aligned to its element type");
  bool vec = true;
  for (int j = 0; j < nop; ++j) vec = vec && aligned16(a.op[j]);
  for (int r = 0; r < G; ++r) {
    if (!rows[r]) return fail(XDE_EBADARG, "xde_interp_rows: null row pointer");
    if (!aligned_to(rows[r], esz)) return fail(XDE_EBADARG, "xde_interp_rows: row not aligned to its element type");
    if (kinds[r] != XDE_ROW_INTERP && kinds[r] != XDE_ROW_COPY_A && kinds[r] != XDE_ROW_COPY_B)
      return fail(XDE_EBADARG, "xde_interp_rows: bad row kind");
    a.rows[r] = rows[r];
    a.kind[r] = kinds[r];
    for (int k = 0; k < 4; ++k) a.w[r][k] = w[r * 4 + k];
    vec = vec && aligned16(rows[r]);
  }
  const int64_t n = outer * chunk;
  if (n == 0) return XDE_OK;
  const int width = dtype == XDE_F32 ? 4 : 2;
  const bool strided = outer > 1 && row_stride != chunk;
  vec = vec && (chunk % width == 0) && (!strided || row_stride % width == 0);
  a.n = n;
  a.chunk = chunk;
  a.row_gap = strided ? row_stride - chunk : 0;
  const int64_t work = vec ? n / width : n;
  int64_t blocks = (work + kBlock - 1) / kBlock;
  if (blocks > grid_cap()) blocks = grid_cap();
  if (blocks < 1) blocks = 1;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // (profiled under the dense-output id: the kernel-id list of xde_hip.h is part of the frozen ABI, so these launches are counted
  // with xde_dense_eval's in xde_prof_collect — both write solution rows)
  ProfScope prof(XDE_KID_DENSE, double(nop + G) * double(n) * double(esz));
  dim3 g(static_cast<unsigned>(blocks)), b(kBlock);
  if (dtype == XDE_F32) launch_typed<float>(a, nop, G, vec, g, b, st, prof);
  else launch_typed<double>(a, nop, G, vec, g, b, st, prof);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"
