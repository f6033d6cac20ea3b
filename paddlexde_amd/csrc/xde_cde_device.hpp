// The control derivative dX[b, c] of the CDE kernels, on chip: the launch's argument block, the query's table entry and the one device
// function that evaluates a channel.  Shared by the contraction (xde_cde.hip) and the fused last layer (xde_cdehead.hip): both build
// the same bits from the same code.
#pragma once

#include "xde_hip_cde.h"

#include "xde_common.hpp"
#include "xde_control_host.hpp"
#include "xde_spline_device.hpp"

namespace xde {

struct CdeArgs {
  void* out;         // out[B, H]   | gF[B, H, C]
  const void* in;    // F[B, H, C]  | gout[B, H]
  const void* series;  // natural control: Y
  const void* coef;    // natural control: M (else `series` again, never read)
  const void* knots;
  const void* t_dev;
  double t_host;
  int64_t B;
  int H, C, Tn;
  int method;
  int time_f64;
  int R, r_log;  // lanes per row team, log2 of it
  int S, Hc;     // slices of H per batch row, rows per slice
  int Gb;        // batch rows per work item (S == 1): short rows H are grouped until one pass of the workgroup is full
  int lds;       // dX rows live in LDS (C <= kCdeMaxC)
  int nt;        // stream F (it is read once, and larger than the caches)
};

// (NAT: the natural control, an instantiation of its own — the linear / cubic ones carry none of its code or registers)
template <typename T, bool NAT>
struct CdeTab {
  RowsLag<T> lin;
  RowsScale<T> sc;
  HermiteLag<T> cub;
};
template <typename T>
struct CdeTab<T, true> {
  NaturalLag<T> nat;
};

// the launch's time -> the query's table entry (one thread per workgroup)
template <typename T, bool NAT>
__device__ __forceinline__ void cde_make_tab(CdeTab<T, NAT>* tb, const CdeArgs& a) {
  const T tau = T(launch_time(a.t_dev, a.time_f64, a.t_host));  // the time in the series dtype first (InterpolationBase._gather)
  const T* ts = static_cast<const T*>(a.knots);
  if constexpr (NAT) {
    tb->nat = make_natural_lag<T>(ts, tau, a.Tn);
  } else if (a.method == XDE_HISTORY_LINEAR) {
    tb->lin = make_lag<T, 2>(ts, tau, a.Tn);
    tb->sc = make_scales<T, 2>(ts, tb->lin.row[0], a.Tn);
  } else {
    tb->cub = make_hermite_lag<T>(ts, tau, a.Tn);
  }
}

// dX[b, c]: `sb` = series[b], `mb` = coef[b]
template <typename T, bool NAT>
__device__ __forceinline__ T cde_dx(const CdeTab<T, NAT>& tb, int method, const T* __restrict__ sb, const T* __restrict__ mb, int c, int C,
                                    int Tn) {
  T val, der;
  if constexpr (NAT) {
    const int64_t at = int64_t(tb.nat.i) * C + c;  // (i <= Tn - 2: row i + 1 exists)
    natural_eval<T>(tb.nat, sb[at], sb[at + C], mb[at], mb[at + C], val, der);
  } else if (method == XDE_HISTORY_LINEAR) {
    const T x[2] = {sb[int64_t(tb.lin.row[0]) * C + c], sb[int64_t(tb.lin.row[1]) * C + c]};
    rows_eval<T, 2>(tb.lin, tb.sc, x, val, der);
  } else {
    const int i = tb.cub.i, i1 = i + 1 < Tn ? i + 1 : Tn - 1;
    hermite_eval<T>(tb.cub, sb[int64_t(i) * C + c], sb[int64_t(i1) * C + c], sb[int64_t(tb.cub.zrow) * C + c], val, der);
  }
  return der;
}

}  // namespace xde
