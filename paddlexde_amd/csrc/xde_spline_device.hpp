// The per-query device functions of the series splines (interpolation/interpolate_base.py:50-107 over interpolate.py): ONE statement
// of each formula, shared by the history gathers (xde_history.hip, xde_dense.hip: value and derivative rows written out) and the CDE
// contraction (xde_cde.hip: the derivative row kept on chip).  What depends on the query time alone — the interval index
// i = clip(bucketize(tau) - 1, 0, T-1), the basis weights, the scales — is a small table entry a workgroup builds once; what depends on
// the series is a handful of ops per element.  The scale conventions are the reference's `_make_series`, as written.  The natural cubic
// spline at the end is the project's own (include/xde_hip_spline.h): its gather (xde_spline.hip) and the CDE contraction share it.
#pragma once

#include "xde_common.hpp"

namespace xde {

// the time of a launch that takes one: the float64 (`time_f64`) or float32 element `t_dev` points at, else the host's number
__device__ __forceinline__ double launch_time(const void* t_dev, int time_f64, double t_host) {
  if (!t_dev) return t_host;
  return time_f64 ? *static_cast<const double*>(t_dev) : double(*static_cast<const float*>(t_dev));
}

// ------------------------------------------------------------------------------------------
// "weighted rows": LinearInterpolation (M = 2) and BezierSpline (M = 4)
// ------------------------------------------------------------------------------------------
template <typename T>
struct RowsLag {
  int row[4];      // his rows min(i + k, T - 1)
  T wv[4], wd[4];  // weight of row k (of `his[row] / scale{k+1}`: the reference divides the SERIES, then weights it) in value / derivative
  T h1;            // scale1_i
};

// the per-lag table entry (one thread per lag)
template <typename T, int M>
__device__ __forceinline__ RowsLag<T> make_lag(const T* __restrict__ ts, T tau, int Tn) {
  constexpr int SPAN = M == 2 ? 1 : 3;  // scale = t[j + SPAN] - t[j], j < T - SPAN
  int lo = 0, hi = Tn;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (ts[mid] < tau) lo = mid + 1; else hi = mid;
  }
  int i = lo - 1;  // bucketize(tau, t) - 1 with right=False: #{t_j < tau} - 1
  i = i < 0 ? 0 : (i > Tn - 1 ? Tn - 1 : i);
  auto scale1 = [&](int j) -> T {  // concat(scale, scale[-1:] * SPAN)[j]
    int jj = j < Tn - SPAN ? j : Tn - SPAN - 1;
    return ts[jj + SPAN] - ts[jj];
  };
  RowsLag<T> r;
  r.h1 = scale1(i);
  const T s = (tau - ts[i]) / r.h1;
  T w[4] = {T(0), T(0), T(0), T(0)}, g[4] = {T(0), T(0), T(0), T(0)};
  if (M == 2) {
    // [s, 1] @ [[-1, 1], [1, 0]] = [-s + 1, s];  [1, 0] @ H = [-1, 1]
    w[0] = -s + T(1);
    w[1] = s;
    g[0] = T(-1);
    g[1] = T(1);
  } else {
    // [s^3, s^2, s, 1] @ H,  [3 s^2, 2 s, 1, 0] @ H  with H = [[-1,3,-3,1],[3,-6,3,0],[-3,3,0,0],[1,0,0,0]]
    const T s2 = s * s, s3 = s2 * s;
    w[0] = ((-s3 + T(3) * s2) - T(3) * s) + T(1);
    w[1] = (T(3) * s3 - T(6) * s2) + T(3) * s;
    w[2] = T(-3) * s3 + T(3) * s2;
    w[3] = s3;
    const T a = T(3) * s2, b = T(2) * s;
    g[0] = (-a + T(3) * b) - T(3);
    g[1] = (T(3) * a - T(6) * b) + T(3);
    g[2] = T(-3) * a + T(3) * b;
    g[3] = a;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r.row[k] = i + k < Tn ? i + k : Tn - 1;
    r.wv[k] = w[k];
    r.wd[k] = g[k];
  }
  return r;
}

template <typename T>
struct RowsScale {
  T sc[4];
};

template <typename T, int M>
__device__ __forceinline__ RowsScale<T> make_scales(const T* __restrict__ ts, int i, int Tn) {
  constexpr int SPAN = M == 2 ? 1 : 3;
  auto scale1 = [&](int j) -> T {
    int jj = j < Tn - SPAN ? j : Tn - SPAN - 1;
    return ts[jj + SPAN] - ts[jj];
  };
  RowsScale<T> q;
#pragma unroll
  for (int k = 0; k < 4; ++k) q.sc[k] = scale1(i - k < 0 ? 0 : i - k);
  return q;
}

// one element: x[k] = his[row[k]] of this column  ->  value and derivative
template <typename T, int M>
__device__ __forceinline__ void rows_eval(const RowsLag<T>& r, const RowsScale<T>& q, const T* x, T& val, T& der) {
  T av = r.wv[0] * (x[0] / q.sc[0]);
  T ad = r.wd[0] * (x[0] / q.sc[0]);
#pragma unroll
  for (int k = 1; k < M; ++k) {
    const T p = x[k] / q.sc[k];
    av = av + r.wv[k] * p;
    ad = ad + r.wd[k] * p;
  }
  val = av * r.h1;  // evaluate(): result *= scale
  der = ad;         // derivative(): no scale factor
}

// ------------------------------------------------------------------------------------------
// CubicHermiteSpline (one-sided node differences, the last one repeated)
// ------------------------------------------------------------------------------------------
template <typename T>
struct HermiteLag {
  int i, mode, zrow, pad;  // mode 0: interior; 1: i == T-2 (d1 repeats d0's rows); 2: i == T-1 (both use rows T-2, T-1)
  T h1, h2, ha, hb, c0, c1, c2, c3, g0, g1, g2, g3;
};

template <typename T>
__device__ __forceinline__ HermiteLag<T> make_hermite_lag(const T* __restrict__ ts, T tau, int Tn) {
  int lo = 0, hi = Tn;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (ts[mid] < tau) lo = mid + 1; else hi = mid;
  }
  int i = lo - 1;
  i = i < 0 ? 0 : (i > Tn - 1 ? Tn - 1 : i);
  auto h_at = [&](int j) -> T {
    int jj = j < Tn - 1 ? j : Tn - 2;
    return ts[jj + 1] - ts[jj];
  };
  HermiteLag<T> r;
  r.i = i;
  r.mode = i <= Tn - 3 ? 0 : (i == Tn - 2 ? 1 : 2);
  r.zrow = r.mode == 0 ? i + 2 : Tn - 2;
  r.pad = 0;
  r.h1 = h_at(i);
  r.h2 = i == 0 ? h_at(0) : h_at(i - 1);
  r.ha = h_at(i);
  r.hb = h_at(i + 1);
  const T sx = (tau - ts[i]) / r.h1;
  const T s2 = sx * sx, s3 = s2 * sx;
  r.c0 = T(2) * s3 - T(3) * s2 + T(1);
  r.c1 = T(-2) * s3 + T(3) * s2;
  r.c2 = s3 - T(2) * s2 + sx;
  r.c3 = s3 - s2;
  r.g0 = T(6) * s2 - T(6) * sx;
  r.g1 = T(-6) * s2 + T(6) * sx;
  r.g2 = T(3) * s2 - T(4) * sx + T(1);
  r.g3 = T(3) * s2 - T(2) * sx;
  return r;
}

// one element: X = his[i], Y = his[min(i + 1, T - 1)], Z = his[zrow] of this column  ->  value and derivative
template <typename T>
__device__ __forceinline__ void hermite_eval(const HermiteLag<T>& r, T X, T Y, T Z, T& val, T& der) {
  const T p0 = X / r.h1, p1 = Y / r.h2;
  const T n0 = r.mode == 2 ? X - Z : Y - X;
  const T n1 = r.mode == 0 ? Z - Y : n0;
  const T d0 = n0 / r.ha, d1 = n1 / r.hb;
  val = (((r.c0 * p0 + r.c1 * p1) + r.c2 * d0) + r.c3 * d1) * r.h1;
  der = ((r.g0 * p0 + r.g1 * p1) + r.g2 * d0) + r.g3 * d1;
}

// ------------------------------------------------------------------------------------------
// NaturalCubicSpline (include/xde_hip_spline.h): the C2 cubic through Y with second derivatives M, both dense on the knot grid
// ------------------------------------------------------------------------------------------
template <typename T>
struct NaturalLag {
  int i, pad;          // i = clip(#{k : t_k <= tau} - 1, 0, Tn - 2): the rows are i and i + 1
  T h, s, h6, s2, s6;  // h = t_{i+1} - t_i, s = tau - t_i, h / 6, s / 2, s / 6
};

// the table entry of a step s into an interval of length h (the coefficient build's fill calls this with the interval between two
// observed nodes)
template <typename T>
__device__ __forceinline__ NaturalLag<T> make_natural_step(int i, T h, T s) {
  NaturalLag<T> r;
  r.i = i;
  r.pad = 0;
  r.h = h;
  r.s = s;
  r.h6 = h / T(6);
  r.s2 = s / T(2);
  r.s6 = s / T(6);
  return r;
}

template <typename T>
__device__ __forceinline__ NaturalLag<T> make_natural_lag(const T* __restrict__ ts, T tau, int Tn) {
  int lo = 0, hi = Tn;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (ts[mid] <= tau) lo = mid + 1; else hi = mid;
  }
  int i = lo - 1;  // #{t_k <= tau} - 1: a query on a knot starts that knot's interval (s = 0, the value is Y_i exactly)
  i = i < 0 ? 0 : (i > Tn - 2 ? Tn - 2 : i);
  return make_natural_step<T>(i, ts[i + 1] - ts[i], tau - ts[i]);
}

// one element: Y0 = Y[i], Y1 = Y[i + 1], M0 = M[i], M1 = M[i + 1] of this column  ->  value and derivative
template <typename T>
__device__ __forceinline__ void natural_eval(const NaturalLag<T>& r, T Y0, T Y1, T M0, T M1, T& val, T& der) {
  const T sl = (Y1 - Y0) / r.h;
  const T d0 = sl - r.h6 * (T(2) * M0 + M1);
  const T e = (M1 - M0) / r.h;
  val = Y0 + r.s * (d0 + r.s * (M0 / T(2) + r.s6 * e));
  der = d0 + r.s * (M0 + r.s2 * e);
}

}  // namespace xde
