// libxde_hip.so — backward of the adaptive Runge–Kutta step for back-propagation through the accepted steps
// (C ABI: include/xde_hip_backprop.h; host: paddlexde_amd/solver/_rk_backprop.py).
//
// Both kernels are HBM-bandwidth bound element-wise linear combinations, written like the forward's combines
// (xde_combine.hip) and dense output (xde_dense.hip): 16 bytes per lane, the operand count a compile-time constant so
// that every stream of a vector is requested before the first one is used, a grid-stride loop over 2048 workgroups of
// 256 threads at most, and the last n % W elements done by the first workgroup with scalar loads.
// Built with -ffp-contract=off like the rest of the library.

#include "xde_common.hpp"
#include "xde_hip_backprop.h"

using namespace xde;

namespace {

// ------------------------------------------------------------------------------------------
// stage cotangent: out = sum_j x_j c_j  [, out2 = sum_j x_j c2_j]  — mu_i and (at stage 0) dL/dy_n from one set of reads
// ------------------------------------------------------------------------------------------
struct CotArgs {
  const void* x[XDE_BP_MAX_X];
  double c[XDE_BP_MAX_X];
  double c2[XDE_BP_MAX_X];
  void* out;
  void* out2;
  int64_t n;
};

template <typename T, int NX, bool TWO, bool VEC>
__global__ __launch_bounds__(kBlock) void xde_stage_cotangent_kernel(CotArgs a) {
  using P = Pack<T, VEC>;
  constexpr int W = P::W;
  const T* xp[NX];
  T c[NX], c2[NX];
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    xp[j] = static_cast<const T*>(a.x[j]);
    c[j] = T(a.c[j]);
    c2[j] = TWO ? T(a.c2[j]) : T(0);
  }
  T* __restrict__ out = static_cast<T*>(a.out);
  T* __restrict__ out2 = static_cast<T*>(a.out2);
  const int64_t nvec = a.n / W;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < nvec; i += stride) {
    P xv[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) xv[j] = P::load(xp[j], i);
    P o, o2;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      T s = xv[0].v[w] * c[0];
#pragma unroll
      for (int j = 1; j < NX; ++j) s = s + xv[j].v[w] * c[j];
      o.v[w] = s;
      if (TWO) {
        T s2 = xv[0].v[w] * c2[0];
#pragma unroll
        for (int j = 1; j < NX; ++j) s2 = s2 + xv[j].v[w] * c2[j];
        o2.v[w] = s2;
      }
    }
    o.store(out, i);
    if (TWO) o2.store(out2, i);
  }
  if (VEC) {
    const int64_t i = nvec * W + threadIdx.x;
    if (blockIdx.x == 0 && i < a.n) {
      T s = xp[0][i] * c[0], s2 = xp[0][i] * c2[0];
      for (int j = 1; j < NX; ++j) {
        s = s + xp[j][i] * c[j];
        s2 = s2 + xp[j][i] * c2[j];
      }
      out[i] = s;
      if (TWO) out2[i] = s2;
    }
  }
}

// ------------------------------------------------------------------------------------------
// dense cotangent: the quartic of one step is linear in (y0, y1, y_mid, f0, f1); G rows' cotangents -> five cotangents
// ------------------------------------------------------------------------------------------
constexpr int kDenseRows = 4;  // rows per launch (the caller's G is taken four at a time; later launches accumulate)
constexpr int kOuts = XDE_BP_DENSE_OUTS;

struct DenseCotArgs {
  void* out[kOuts];
  double w[kDenseRows][kOuts];
  const void* g;  // the first row of this launch
  int64_t n;      // elements per row (row r starts at g + r * n)
  uint32_t acc;   // bit k: outs[k] accumulates
};

template <typename T, int G, bool VEC>
__global__ __launch_bounds__(kBlock) void xde_dense_cotangent_kernel(DenseCotArgs a) {
  using P = Pack<T, VEC>;
  constexpr int W = P::W;
  const T* __restrict__ g = static_cast<const T*>(a.g);
  T wt[G][kOuts];
#pragma unroll
  for (int r = 0; r < G; ++r)
#pragma unroll
    for (int k = 0; k < kOuts; ++k) wt[r][k] = T(a.w[r][k]);
  // (no __restrict__ on the outputs: an accumulated output is read and written by the same lane)
  T* op[kOuts];
#pragma unroll
  for (int k = 0; k < kOuts; ++k) op[k] = static_cast<T*>(a.out[k]);
  const int64_t nvec = a.n / W;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < nvec; i += stride) {
    P gv[G];
#pragma unroll
    for (int r = 0; r < G; ++r) gv[r] = P::load(g + int64_t(r) * a.n, i);
    P old[kOuts];
#pragma unroll
    for (int k = 0; k < kOuts; ++k)
      if (op[k] && ((a.acc >> k) & 1u)) old[k] = P::load(op[k], i);
#pragma unroll
    for (int k = 0; k < kOuts; ++k) {
      if (!op[k]) continue;
      const bool acc = (a.acc >> k) & 1u;
      P o;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        T s = gv[0].v[w] * wt[0][k];
        if (acc) s = old[k].v[w] + s;
#pragma unroll
        for (int r = 1; r < G; ++r) s = s + gv[r].v[w] * wt[r][k];
        o.v[w] = s;
      }
      o.store(op[k], i);
    }
  }
  if (VEC) {
    const int64_t i = nvec * W + threadIdx.x;
    if (blockIdx.x == 0 && i < a.n) {
      for (int k = 0; k < kOuts; ++k) {
        if (!op[k]) continue;
        T s = g[i] * wt[0][k];
        if ((a.acc >> k) & 1u) s = op[k][i] + s;
        for (int r = 1; r < G; ++r) s = s + g[int64_t(r) * a.n + i] * wt[r][k];
        op[k][i] = s;
      }
    }
  }
}

int64_t grid_for(int64_t n, bool vec, int dtype) {
  const int width = dtype == XDE_F32 ? 4 : 2;
  const int64_t work = vec ? (n + width - 1) / width : n;
  int64_t blocks = (work + kBlock - 1) / kBlock;
  if (blocks > grid_cap()) blocks = grid_cap();
  return blocks < 1 ? 1 : blocks;
}

template <typename T, bool TWO, bool VEC>
void launch_cot(const CotArgs& a, int nx, dim3 g, dim3 b, hipStream_t st, ProfScope& prof) {
  switch (nx) {
#define XDE_COT_CASE(N) \
    case N: XDE_LAUNCH((xde_stage_cotangent_kernel<T, N, TWO, VEC>), g, b, st, prof, a); break;
    XDE_COT_CASE(1) XDE_COT_CASE(2) XDE_COT_CASE(3) XDE_COT_CASE(4) XDE_COT_CASE(5) XDE_COT_CASE(6) XDE_COT_CASE(7)
    XDE_COT_CASE(8) XDE_COT_CASE(9) XDE_COT_CASE(10) XDE_COT_CASE(11) XDE_COT_CASE(12) XDE_COT_CASE(13) XDE_COT_CASE(14)
    XDE_COT_CASE(15) XDE_COT_CASE(16)
#undef XDE_COT_CASE
    default: break;
  }
}
static_assert(XDE_BP_MAX_X == 16, "launch_cot instantiates operand counts 1..16");

template <typename T, bool VEC>
void launch_dense_cot(const DenseCotArgs& a, int G, dim3 g, dim3 b, hipStream_t st, ProfScope& prof) {
  switch (G) {
    case 1: XDE_LAUNCH((xde_dense_cotangent_kernel<T, 1, VEC>), g, b, st, prof, a); break;
    case 2: XDE_LAUNCH((xde_dense_cotangent_kernel<T, 2, VEC>), g, b, st, prof, a); break;
    case 3: XDE_LAUNCH((xde_dense_cotangent_kernel<T, 3, VEC>), g, b, st, prof, a); break;
    default: XDE_LAUNCH((xde_dense_cotangent_kernel<T, 4, VEC>), g, b, st, prof, a); break;
  }
}

}  // namespace

extern "C" {

int xde_stage_cotangent(void* out, void* out2, const void* const* x, const double* coef, const double* coef2, int nx, int64_t n,
                        int dtype, void* stream) {
  if (!out || !x || !coef) return fail(XDE_EBADARG, "xde_stage_cotangent: null pointer");
  if (out2 && !coef2) return fail(XDE_EBADARG, "xde_stage_cotangent: out2 needs coef2");
  if (nx < 1 || nx > XDE_BP_MAX_X) return fail(XDE_EBADARG, "xde_stage_cotangent: nx out of range");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, "xde_stage_cotangent: bad dtype");
  if (n < 0) return fail(XDE_EBADARG, "xde_stage_cotangent: negative n");
  CotArgs a;
  memset(&a, 0, sizeof(a));
  bool vec = aligned16(out) && (!out2 || aligned16(out2));
  for (int j = 0; j < nx; ++j) {
    if (!x[j]) return fail(XDE_EBADARG, "xde_stage_cotangent: null x[j]");
    if (x[j] == out || (out2 && x[j] == out2)) return fail(XDE_EBADARG, "xde_stage_cotangent: an output aliases an operand");
    a.x[j] = x[j];
    a.c[j] = coef[j];
    a.c2[j] = out2 ? coef2[j] : 0.0;
    vec = vec && aligned16(x[j]);
  }
  if (n == 0) return XDE_OK;
  a.out = out;
  a.out2 = out2;
  a.n = n;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double(nx + (out2 ? 2 : 1)) * double(n) * (dtype == XDE_F32 ? 4.0 : 8.0));
  dim3 g(static_cast<unsigned>(grid_for(n, vec, dtype))), b(kBlock);
  if (dtype == XDE_F32) {
    if (out2) vec ? launch_cot<float, true, true>(a, nx, g, b, st, prof) : launch_cot<float, true, false>(a, nx, g, b, st, prof);
    else vec ? launch_cot<float, false, true>(a, nx, g, b, st, prof) : launch_cot<float, false, false>(a, nx, g, b, st, prof);
  } else {
    if (out2) vec ? launch_cot<double, true, true>(a, nx, g, b, st, prof) : launch_cot<double, true, false>(a, nx, g, b, st, prof);
    else vec ? launch_cot<double, false, true>(a, nx, g, b, st, prof) : launch_cot<double, false, false>(a, nx, g, b, st, prof);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_dense_cotangent(void* const* outs, const void* g_rows, const double* w, int G, uint32_t acc_mask, int64_t n, int dtype,
                        void* stream) {
  if (!outs || !g_rows || !w) return fail(XDE_EBADARG, "xde_dense_cotangent: null pointer");
  if (G < 1) return fail(XDE_EBADARG, "xde_dense_cotangent: G must be >= 1");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, "xde_dense_cotangent: bad dtype");
  if (n < 0) return fail(XDE_EBADARG, "xde_dense_cotangent: negative n");
  int nout = 0;
  for (int k = 0; k < kOuts; ++k) nout += outs[k] ? 1 : 0;
  if (nout == 0) return fail(XDE_EBADARG, "xde_dense_cotangent: every output is null");
  if (n == 0) return XDE_OK;
  const int width = dtype == XDE_F32 ? 4 : 2;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  // every row starts at g_rows + r*n elements: rows stay 16-byte aligned only if n % width == 0
  bool vec = aligned16(g_rows) && (n % width == 0);
  for (int k = 0; k < kOuts; ++k) vec = vec && (!outs[k] || aligned16(outs[k]));
  hipStream_t st = static_cast<hipStream_t>(stream);
  dim3 g(static_cast<unsigned>(grid_for(n, vec, dtype))), b(kBlock);
  for (int r0 = 0; r0 < G; r0 += kDenseRows) {
    const int rows = G - r0 < kDenseRows ? G - r0 : kDenseRows;
    DenseCotArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < kOuts; ++k) a.out[k] = outs[k];
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < kOuts; ++k) a.w[r][k] = w[(r0 + r) * kOuts + k];
    a.g = static_cast<const char*>(g_rows) + size_t(r0) * size_t(n) * esz;
    a.n = n;
    a.acc = r0 == 0 ? acc_mask : 0x1Fu;  // (the rows after the first four add to what the first launch wrote)
    int nacc = 0;
    for (int k = 0; k < kOuts; ++k) nacc += (outs[k] && ((a.acc >> k) & 1u)) ? 1 : 0;
    ProfScope prof(XDE_KID_DENSE, double(rows + nacc + nout) * double(n) * double(esz));
    if (dtype == XDE_F32) vec ? launch_dense_cot<float, true>(a, rows, g, b, st, prof) : launch_dense_cot<float, false>(a, rows, g, b, st, prof);
    else vec ? launch_dense_cot<double, true>(a, rows, g, b, st, prof) : launch_dense_cot<double, false>(a, rows, g, b, st, prof);
    HIP_TRY(hipGetLastError());
  }
  return XDE_OK;
}

}  // extern "C"
