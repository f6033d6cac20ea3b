// libxde_hip.so — the natural cubic spline through a partly observed series on irregular knots (include/xde_hip_spline.h):
//
//   xde_spline_natural_coeffs   series[B, Tn, C] -> Y[B, Tn, C], M[B, Tn, C]: the end rule, the Thomas solve over the observed nodes
//                               and the fill of the missing rows.  Once per control, not per step: one lane per column, three serial
//                               sweeps over Tn with the predecessor node in registers; lanes along c read a time row coalesced.
//   xde_spline_natural_gather   value and derivative at L query times, in xde_history_gather's layout, with the device functions the
//                               CDE contraction builds dX from (xde_spline_device.hpp): the same bits.
//
// The two contraction entry points of the header are in xde_cde.hip, next to the kernels they launch.

#include "xde_hip_spline.h"

#include "xde_common.hpp"
#include "xde_control_host.hpp"
#include "xde_spline_device.hpp"

using namespace xde;

namespace {

constexpr int kNatMaxL = 128;  // query times per LAUNCH (the LDS table); more are served in tiles of this many

// One lane = one column e = b C + c.  During the sweeps Y[k] holds cp_k and M[k] holds dp_k at the nodes (the observed values are still
// readable from `series`); every element of Y and M is written before the lane returns.
template <typename T>
__global__ __launch_bounds__(kBlock) void xde_natural_coeffs_kernel(T* __restrict__ Y, T* __restrict__ M, const T* __restrict__ series,
                                                                    const T* __restrict__ ts, int64_t cols, int Tn, int C) {
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < cols; e += stride) {
    const int64_t b = e / C;
    const int64_t at = b * int64_t(Tn) * C + (e - b * C);  // element (b, 0, c); row k is C * k further
    const T* __restrict__ y = series + at;
    T* __restrict__ Yc = Y + at;
    T* __restrict__ Mc = M + at;
    // the end rule's first value
    int kf = 0;
    T yfirst = y[0];
    while (yfirst != yfirst && ++kf < Tn) yfirst = y[int64_t(kf) * C];
    if (kf == Tn) {  // nothing observed: all-NaN rows
      for (int k = 0; k < Tn; ++k) Yc[int64_t(k) * C] = yfirst, Mc[int64_t(k) * C] = yfirst;
      continue;
    }
    // 1. forward elimination, lagging one node: node i gets its cp, dp when the node b above it is met
    T ta = T(0), ya = T(0), cpa = T(0), dpa = T(0);
    bool have_a = false;
    T ti = ts[0], yi = yfirst, ylast = yfirst;
    int ki = 0;
    for (int k = 1; k < Tn; ++k) {
      T yb = y[int64_t(k) * C];
      const bool obs = yb == yb;
      if (obs) ylast = yb;
      if (!obs && k != Tn - 1) continue;
      if (!obs) yb = ylast;  // (the end rule's last value)
      const T tb = ts[k];
      T cp = T(0), dp = T(0);
      if (have_a) {
        const T hl = ti - ta, hr = tb - ti;
        const T sl = (yi - ya) / hl, sr = (yb - yi) / hr;
        const T rhs = T(6) * (sr - sl);
        const T den = T(2) * (hl + hr) - hl * cpa;
        cp = hr / den;
        dp = (rhs - hl * dpa) / den;
      }
      Yc[int64_t(ki) * C] = cp;
      Mc[int64_t(ki) * C] = dp;
      ta = ti, ya = yi, cpa = cp, dpa = dp, have_a = true;
      ti = tb, yi = yb, ki = k;
    }
    // 2. back substitution over the interior nodes (natural ends: M = 0 at the first and the last node)
    T Mb = T(0);
    Mc[int64_t(Tn - 1) * C] = T(0);
    for (int k = Tn - 2; k >= 1; --k) {
      const T yk = y[int64_t(k) * C];
      if (yk != yk) continue;
      const T Mk = Mc[int64_t(k) * C] - Yc[int64_t(k) * C] * Mb;
      Mc[int64_t(k) * C] = Mk;
      Mb = Mk;
    }
    Mc[0] = T(0);
    // 3. the values at the nodes, and each missing run once its right node is known
    int ka = 0;
    T Ma = T(0);
    ta = ts[0], ya = yfirst;
    Yc[0] = ya;
    for (int k = 1; k < Tn; ++k) {
      T yb = y[int64_t(k) * C];
      const bool obs = yb == yb;
      if (!obs && k != Tn - 1) continue;
      if (!obs) yb = ylast;
      const T tb = ts[k], Mk = Mc[int64_t(k) * C];
      Yc[int64_t(k) * C] = yb;
      if (k - ka > 1) {
        const T h = tb - ta;
        for (int j = ka + 1; j < k; ++j) {
          const T s = ts[j] - ta;
          const NaturalLag<T> r = make_natural_step<T>(ka, h, s);
          T val, der;
          natural_eval<T>(r, ya, yb, Ma, Mk, val, der);
          Mc[int64_t(j) * C] = Ma + (s / h) * (Mk - Ma);
          Yc[int64_t(j) * C] = val;
        }
      }
      ka = k, ta = tb, ya = yb, Ma = Mk;
    }
  }
}

// This launch serves the query times l0 .. l0 + Lt - 1 (Lt <= kNatMaxL) of the L the outputs hold, as xde_rows_gather_kernel does.
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void xde_natural_gather_kernel(T* __restrict__ val, T* __restrict__ der, const T* __restrict__ Y,
                                                                    const T* __restrict__ M, const T* __restrict__ ts,
                                                                    const T* __restrict__ tq, int64_t outer, int Tn, int D, int L, int l0,
                                                                    int Lt) {
  using P = Pack<T, VEC>;
  constexpr int W = P::W;
  __shared__ NaturalLag<T> tab[kNatMaxL];
  for (int l = threadIdx.x; l < Lt; l += kBlock) tab[l] = make_natural_lag<T>(ts, tq[l0 + l], Tn);
  __syncthreads();
  const int DV = D / W;
  const int64_t total = outer * int64_t(Lt) * DV;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  const int64_t rowv = int64_t(Tn) * DV;
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < total; e += stride) {
    const int dv = int(e % DV);
    const int l = int((e / DV) % Lt);
    const int64_t o = e / (int64_t(DV) * Lt);
    const NaturalLag<T>& r = tab[l];
    const int64_t at = e + (o * (L - Lt) + l0) * DV;  // ((o * L + l0 + l) * DV + dv)
    const int64_t base = o * rowv + int64_t(r.i) * DV + dv;
    const P y0 = P::load(Y, base), y1 = P::load(Y, base + DV), m0 = P::load(M, base), m1 = P::load(M, base + DV);
    P v, g;
#pragma unroll
    for (int x = 0; x < W; ++x) natural_eval<T>(r, y0.v[x], y1.v[x], m0.v[x], m1.v[x], v.v[x], g.v[x]);
    v.store_nt(val, at);
    if (der) g.store_nt(der, at);
  }
}

}  // namespace

extern "C" {

int xde_spline_natural_coeffs(void* Y, void* M, const void* series, const void* knots, int64_t B, int Tn, int C, int dtype, void* stream) {
  if (int rc = check_rows({"xde_spline_natural_coeffs"}, {Y, M, series, knots}, {}, "B, C", {B, C}, Tn, dtype)) return rc;
  const int64_t cols = B * int64_t(C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_DENSE, 3.0 * double(cols) * Tn * elem_size(dtype));
  dim3 g(grid_for(cols)), blk(kBlock);
  with_dtype(dtype, [&](auto ty) {
    using T = typename decltype(ty)::type;
    XDE_LAUNCH((xde_natural_coeffs_kernel<T>), g, blk, st, prof, static_cast<T*>(Y), static_cast<T*>(M), static_cast<const T*>(series),
               static_cast<const T*>(knots), cols, Tn, C);
  });
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_spline_natural_gather(void* val, void* der, const void* Y, const void* M, const void* knots, const void* tq, int64_t outer, int Tn,
                              int L, int D, int dtype, void* stream) {
  // (`der` may be null)
  if (int rc = check_rows({"xde_spline_natural_gather"}, {val, Y, M, knots, tq}, {der}, "outer, L, D", {outer, L, D}, Tn, dtype))
    return rc;
  const int width = vec_width(dtype);
  const bool vec = (D % width) == 0 && aligned16(val) && aligned16(der) && aligned16(Y) && aligned16(M);
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int l0 = 0; l0 < L; l0 += kNatMaxL) {
    const int Lt = L - l0 < kNatMaxL ? L - l0 : kNatMaxL;
    ProfScope prof(XDE_KID_DENSE, (der ? 6.0 : 5.0) * double(outer) * Lt * D * elem_size(dtype));
    dim3 g(grid_for(outer * int64_t(Lt) * (vec ? D / width : D))), b(kBlock);
    with_dtype(dtype, [&](auto ty) {
      using T = typename decltype(ty)::type;
      with_flag(vec, [&](auto v) {
        XDE_LAUNCH((xde_natural_gather_kernel<T, decltype(v)::value>), g, b, st, prof, static_cast<T*>(val), static_cast<T*>(der),
                   static_cast<const T*>(Y), static_cast<const T*>(M), static_cast<const T*>(knots), static_cast<const T*>(tq), outer, Tn,
                   D, L, l0, Lt);
      });
    });
    HIP_TRY(hipGetLastError());
  }
  return XDE_OK;
}

}  // extern "C"
