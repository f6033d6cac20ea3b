// libxde_hip.so — per-sample output times of a joint adaptive solve (C ABI: include/xde_hip_teval.h, the specification, op by op;
// host: paddlexde_amd/solver/_rk_teval.py).
//
// Both kernels own ROWS the way xde_rows.hip's do: G = min(256, pow2 >= ceil(D / W)) lanes work on a row — several rows per wave at
// small D, a workgroup per row at large D, D beyond one workgroup's stride as a loop in that workgroup.  Every lane of a row finds the
// row's range [b, e) of queries inside the step by two binary searches over the row's leading cnt[r] times (the lanes of a row read
// the same addresses: one transaction per wave and probe), so there is no cursor, no LDS and no barrier, and a row without a query in
// the step leaves after those reads.  A lane walks the chunks g, g + G, ... of its row: one 16-byte load per operand where the row
// starts on a 16-byte boundary, single elements else, the same arithmetic.  The dense kernel forms y_mid once per chunk and writes one
// chunk per query; the cotangent kernel forms the five float64 weights of a query from its fraction and folds the queries in
// increasing q.  No atomics.  Built with -ffp-contract=off like the rest of the library.

#include "xde_common.hpp"
#include "xde_hip_teval.h"

using namespace xde;

namespace {

constexpr int64_t kTevalMaxElems = int64_t(1) << 40;
constexpr int64_t kTevalMaxOut = int64_t(1) << 48;
constexpr int kOuts = XDE_TEVAL_OUTS;

struct TevalMap {
  int32_t G, rpb;  // lanes of a row; rows of a workgroup
  int32_t C;       // chunks of a row
  int32_t vec;     // every state operand pointer is 16-byte aligned
  int32_t out_vec;  // so is the Q x rows x D array (out / g)
  int64_t rows, D, Q, nrb;
};

struct TevalStep {
  const double* tq;
  const int32_t* cnt;
  double t0, t1, dt;
  int32_t direction, time_dtype;
};

template <typename T> __device__ __forceinline__ void tv_load(const T* p, int64_t o, int n, bool vec, T (&x)[VecOf<T>::W]) {
  constexpr int W = VecOf<T>::W;
  if (vec) {
    const Pack<T, true> q = Pack<T, true>::load(p + o, 0);
#pragma unroll
    for (int w = 0; w < W; ++w) x[w] = q.v[w];
  } else {
#pragma unroll
    for (int w = 0; w < W; ++w) x[w] = w < n ? p[o + w] : T(0);
  }
}

template <typename T> __device__ __forceinline__ void tv_store(T* p, int64_t o, int n, bool vec, const T (&x)[VecOf<T>::W]) {
  constexpr int W = VecOf<T>::W;
  if (vec) {
    Pack<T, true> q;
#pragma unroll
    for (int w = 0; w < W; ++w) q.v[w] = x[w];
    q.store(p + o, 0);
  } else {
#pragma unroll
    for (int w = 0; w < W; ++w)
      if (w < n) p[o + w] = x[w];
  }
}

// dir * TT(v) as a double (a TT value widened is exact; so is the sign)
__device__ __forceinline__ double tv_key(double v, bool t32, int dir) {
  const double x = t32 ? double(float(v)) : v;
  return dir < 0 ? -x : x;
}

// the first q < n of the row whose time is later than `key` (the row is monotone in the direction of integration)
__device__ __forceinline__ int tv_upper(const double* row, int n, double key, bool t32, int dir) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (tv_key(row[mid], t32, dir) > key) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// MEMBERSHIP of the header: the range [b, e) of row r inside the step
__device__ __forceinline__ void tv_range(const TevalStep& s, int64_t r, int64_t Q, int& b, int& e) {
  const bool t32 = s.time_dtype == XDE_F32;
  const int32_t c = s.cnt[r];
  const int n = c < 0 ? 0 : (int64_t(c) > Q ? int(Q) : int(c));  // (0 <= cnt[r] <= Q is the caller's statement: never read past the row)
  const double* row = s.tq + r * Q;
  b = tv_upper(row, n, tv_key(s.t0, t32, s.direction), t32, s.direction);
  e = b < n ? tv_upper(row, n, tv_key(s.t1, t32, s.direction), t32, s.direction) : b;
}

template <typename T> __device__ __forceinline__ T tv_frac(double tq, double t0, double t1, bool t32) {
  return t32 ? T((float(tq) - float(t0)) / (float(t1) - float(t0))) : T((tq - t0) / (t1 - t0));
}

// interp_fit (utils/ode_utils.py:44-49) + interp_evaluate (:69-77), xde_dense.hip's op order
template <typename T> __device__ __forceinline__ T tv_quartic(T y0v, T y1v, T f0v, T f1v, T ymid, T x, T dt) {
  T ca = T(2) * dt * (f1v - f0v) - T(8) * (y1v + y0v) + T(16) * ymid;
  T cb = dt * (T(5) * f0v - T(3) * f1v) + T(18) * y0v + T(14) * y1v - T(32) * ymid;
  T cc = dt * (f1v - T(4) * f0v) - T(11) * y0v - T(5) * y1v + T(16) * ymid;
  T cd = dt * f0v;
  T total = y0v + x * cd;
  T xp = x;
  xp = xp * x;
  total = total + xp * cc;
  xp = xp * x;
  total = total + xp * cb;
  xp = xp * x;
  total = total + xp * ca;
  return total;
}

// ------------------------------------------------------------------------------------------
// 1: dense output at every row's own times
// ------------------------------------------------------------------------------------------
struct TevalDenseArgs {
  void* out;
  const void* k[XDE_MAX_K];
  double mid[XDE_MAX_K];
  const void* y0;
  const void* y1;
  const void* f0;
  const void* f1;
  TevalStep s;
  int32_t nk;
  int32_t k0_is_f0, klast_is_f1;  // an operand given twice is read once
  TevalMap m;
};

// NK > 0: the operand count is a compile-time constant and every stream of a chunk is requested before the first is used.
// NK == 0: the loop over a.nk operands (Dopri8's midpoint weights take more than seven).
template <typename T, int NK> __global__ __launch_bounds__(kBlock) void xde_teval_dense_kernel(TevalDenseArgs a) {
  constexpr int W = VecOf<T>::W;
  constexpr int MAXK = NK > 0 ? NK : 1;
  const TevalMap& m = a.m;
  const T* y0 = static_cast<const T*>(a.y0);
  const T* y1 = static_cast<const T*>(a.y1);
  const T* f0 = static_cast<const T*>(a.f0);
  const T* f1 = static_cast<const T*>(a.f1);
  T* out = static_cast<T*>(a.out);
  const bool t32 = a.s.time_dtype == XDE_F32;
  const T dt = t32 ? T(float(a.s.dt)) : T(a.s.dt);  // `dt.astype(y0.dtype)`
  const int nk = NK > 0 ? NK : a.nk;
  const T* kp[MAXK];
  T cm[MAXK];
  if (NK > 0) {
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
      kp[j] = static_cast<const T*>(a.k[j]);
      cm[j] = dt * T(a.mid[j]);  // `dt * self.mid`
    }
  }
  const int g = threadIdx.x & (m.G - 1);
  for (int64_t rb = blockIdx.x; rb < m.nrb; rb += gridDim.x) {
    const int64_t r = rb * m.rpb + threadIdx.x / m.G;
    if (r >= m.rows) continue;
    int b, e;
    tv_range(a.s, r, m.Q, b, e);
    if (e <= b) continue;
    const double* trow = a.s.tq + r * m.Q;
    const int64_t base = r * m.D;
    const bool rowvec = m.vec && (base % W) == 0;
    for (int ch = g; ch < m.C; ch += m.G) {
      const int64_t o = base + int64_t(ch) * W;
      const int64_t left = m.D - int64_t(ch) * W;
      const int n = left < W ? int(left) : W;
      const bool vec = rowvec && n == W;
      T a0[W], a1[W], b0[W], b1[W], ym[W];
      tv_load<T>(y1, o, n, vec, a1);
      tv_load<T>(f1, o, n, vec, b1);
      tv_load<T>(y0, o, n, vec, a0);
      tv_load<T>(f0, o, n, vec, b0);
      if (NK > 0) {
        T kk[MAXK][W];
#pragma unroll
        for (int j = 0; j < MAXK; ++j) {
          if (j == 0 && a.k0_is_f0) {
#pragma unroll
            for (int w = 0; w < W; ++w) kk[j][w] = b0[w];
          } else if (j == MAXK - 1 && a.klast_is_f1) {
#pragma unroll
            for (int w = 0; w < W; ++w) kk[j][w] = b1[w];
          } else {
            tv_load<T>(kp[j], o, n, vec, kk[j]);
          }
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
          T acc = kk[0][w] * cm[0];
#pragma unroll
          for (int j = 1; j < MAXK; ++j) acc = acc + kk[j][w] * cm[j];
          ym[w] = a0[w] + acc;
        }
      } else {
        T acc[W];
        for (int j = 0; j < nk; ++j) {
          T kj[W];
          tv_load<T>(static_cast<const T*>(a.k[j]), o, n, vec, kj);
          const T cj = dt * T(a.mid[j]);
#pragma unroll
          for (int w = 0; w < W; ++w) acc[w] = j == 0 ? kj[w] * cj : acc[w] + kj[w] * cj;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) ym[w] = a0[w] + acc[w];
      }
      for (int q = b; q < e; ++q) {
        const T x = tv_frac<T>(trow[q], a.s.t0, a.s.t1, t32);
        T v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) v[w] = tv_quartic<T>(a0[w], a1[w], b0[w], b1[w], ym[w], x, dt);
        const int64_t oo = (int64_t(q) * m.rows + r) * m.D + int64_t(ch) * W;
        tv_store<T>(out, oo, n, m.out_vec && n == W && (oo % W) == 0, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// 2: the cotangent of 1
// ------------------------------------------------------------------------------------------
struct TevalCotArgs {
  void* out[kOuts];
  const void* g;
  TevalStep s;
  uint32_t acc;  // bit j: outs[j] accumulates
  TevalMap m;
};

// (p0 + pm, p1, pm, q0, q1) of solver/_rk_backprop.py: quartic_weights, in float64 in its written order
__device__ __forceinline__ void tv_weights(double x, double dts, double (&w)[kOuts]) {
  const double x2 = x * x;
  const double x3 = x2 * x;
  const double x4 = x3 * x;
  const double p0 = 1.0 - 11.0 * x2 + 18.0 * x3 - 8.0 * x4;
  const double p1 = -5.0 * x2 + 14.0 * x3 - 8.0 * x4;
  const double pm = 16.0 * x2 - 32.0 * x3 + 16.0 * x4;
  const double q0 = dts * (x - 4.0 * x2 + 5.0 * x3 - 2.0 * x4);
  const double q1 = dts * (x2 - 3.0 * x3 + 2.0 * x4);
  w[0] = p0 + pm;
  w[1] = p1;
  w[2] = pm;
  w[3] = q0;
  w[4] = q1;
}

template <typename T> __global__ __launch_bounds__(kBlock) void xde_teval_cotangent_kernel(TevalCotArgs a) {
  constexpr int W = VecOf<T>::W;
  const TevalMap& m = a.m;
  const T* gp = static_cast<const T*>(a.g);
  // (no __restrict__ on the outputs: an accumulated output is read and written by the same lane)
  T* op[kOuts];
#pragma unroll
  for (int j = 0; j < kOuts; ++j) op[j] = static_cast<T*>(a.out[j]);
  const bool t32 = a.s.time_dtype == XDE_F32;
  const double dts = double(t32 ? T(float(a.s.dt)) : T(a.s.dt));
  const int g = threadIdx.x & (m.G - 1);
  for (int64_t rb = blockIdx.x; rb < m.nrb; rb += gridDim.x) {
    const int64_t r = rb * m.rpb + threadIdx.x / m.G;
    if (r >= m.rows) continue;
    int b, e;
    tv_range(a.s, r, m.Q, b, e);
    const double* trow = a.s.tq + r * m.Q;
    const int64_t base = r * m.D;
    const bool rowvec = m.vec && (base % W) == 0;
    for (int ch = g; ch < m.C; ch += m.G) {
      const int64_t o = base + int64_t(ch) * W;
      const int64_t left = m.D - int64_t(ch) * W;
      const int n = left < W ? int(left) : W;
      const bool vec = rowvec && n == W;
      if (e <= b) {  // an empty range: 0, or the value kept
        T z[W];
#pragma unroll
        for (int w = 0; w < W; ++w) z[w] = T(0);
#pragma unroll
        for (int j = 0; j < kOuts; ++j)
          if (op[j] && !((a.acc >> j) & 1u)) tv_store<T>(op[j], o, n, vec, z);
        continue;
      }
      T s[kOuts][W];
      for (int q = b; q < e; ++q) {
        const T x = tv_frac<T>(trow[q], a.s.t0, a.s.t1, t32);
        double wd[kOuts];
        tv_weights(double(x), dts, wd);
        T gq[W];
        const int64_t oo = (int64_t(q) * m.rows + r) * m.D + int64_t(ch) * W;
        tv_load<T>(gp, oo, n, m.out_vec && n == W && (oo % W) == 0, gq);
        if (q == b) {
#pragma unroll
          for (int j = 0; j < kOuts; ++j) {
            const T wj = T(wd[j]);
#pragma unroll
            for (int w = 0; w < W; ++w) s[j][w] = gq[w] * wj;
            if (op[j] && ((a.acc >> j) & 1u)) {
              T old[W];
              tv_load<T>(op[j], o, n, vec, old);
#pragma unroll
              for (int w = 0; w < W; ++w) s[j][w] = old[w] + s[j][w];
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < kOuts; ++j) {
            const T wj = T(wd[j]);
#pragma unroll
            for (int w = 0; w < W; ++w) s[j][w] = s[j][w] + gq[w] * wj;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kOuts; ++j)
        if (op[j]) tv_store<T>(op[j], o, n, vec, s[j]);
    }
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
bool tv_aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

bool tv_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

int tv_check_shape(const std::string& who, int64_t rows, int64_t D, int64_t Q, int dtype, int time_dtype, int direction, double t0,
                   double t1, double dt) {
  if (rows < 1) return fail(XDE_EBADARG, who + ": rows < 1");
  if (D < 1) return fail(XDE_EBADARG, who + ": D < 1");
  if (D > (int64_t(1) << 31)) return fail(XDE_EBADARG, who + ": D is too large (D <= 2^31)");
  if (rows > kTevalMaxElems / D) return fail(XDE_EBADARG, who + ": rows * D is too large (> 2^40)");
  if (Q < 1 || Q > int64_t(2147483647)) return fail(XDE_EBADARG, who + ": Q out of range (1 <= Q <= 2^31 - 1)");
  if (Q > kTevalMaxOut / (rows * D)) return fail(XDE_EBADARG, who + ": Q * rows * D is too large (> 2^48)");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, who + ": bad dtype");
  if (time_dtype != XDE_F32 && time_dtype != XDE_F64) return fail(XDE_EBADARG, who + ": bad time_dtype");
  if (direction != 1 && direction != -1) return fail(XDE_EBADARG, who + ": direction must be +1 or -1");
  if (!((t0 - t0) == 0.0) || !((t1 - t1) == 0.0) || !((dt - dt) == 0.0)) return fail(XDE_EBADARG, who + ": t0, t1 and dt must be finite");
  if (!(double(direction) * (t1 - t0) > 0.0)) return fail(XDE_EBADARG, who + ": the step (t0, t1] must run in the direction of integration");
  return XDE_OK;
}

int tv_check_times(const std::string& who, const double* tq, const int32_t* cnt) {
  if (!tq || !cnt) return fail(XDE_EBADARG, who + ": null pointer");
  if (!tv_aligned(tq, 8)) return fail(XDE_EBADARG, who + ": tq not aligned to its element type");
  if (!tv_aligned(cnt, 4)) return fail(XDE_EBADARG, who + ": cnt not aligned to its element type");
  return XDE_OK;
}

TevalMap tv_map(int64_t rows, int64_t D, int64_t Q, int dtype, bool vec, bool out_vec) {
  TevalMap m;
  const int W = dtype == XDE_F32 ? 4 : 2;
  const int64_t C = (D + W - 1) / W;
  int G = 1;
  while (G < kBlock && G < C) G <<= 1;
  m.G = G;
  m.rpb = kBlock / G;
  m.C = int32_t(C);  // (D <= 2^31: C fits 32 bits)
  m.vec = vec ? 1 : 0;
  m.out_vec = out_vec ? 1 : 0;
  m.rows = rows;
  m.D = D;
  m.Q = Q;
  m.nrb = (rows + m.rpb - 1) / m.rpb;
  return m;
}

dim3 tv_grid(const TevalMap& m) {
  int64_t blocks = m.nrb;
  if (blocks > grid_cap()) blocks = grid_cap();
  return dim3(static_cast<unsigned>(blocks));
}

}  // namespace

extern "C" {

// (profiled under the id of the launch they stand for: the kernel-id list of xde_hip.h is part of the frozen ABI)
int xde_teval_dense(void* out, const double* tq, const int32_t* cnt, const void* const* k, const double* mid, int nk, const void* y0,
                    const void* y1, const void* f0, const void* f1, double t0, double t1, double dt, int direction, int time_dtype,
                    int64_t rows, int64_t D, int64_t Q, int dtype, void* stream) {
  const std::string who = "xde_teval_dense";
  if (!out || !y0 || !y1 || !f0 || !f1 || !k || !mid) return fail(XDE_EBADARG, who + ": null pointer");
  if (int rc = tv_check_times(who, tq, cnt)) return rc;
  if (int rc = tv_check_shape(who, rows, D, Q, dtype, time_dtype, direction, t0, t1, dt)) return rc;
  if (nk < 1 || nk > XDE_MAX_K) return fail(XDE_EBADARG, who + ": nk out of range (1 <= nk <= 14)");
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const size_t nbytes = size_t(rows) * size_t(D) * esz;
  const size_t obytes = nbytes * size_t(Q);
  TevalDenseArgs a;
  memset(&a, 0, sizeof(a));
  bool vec = aligned16(y0) && aligned16(y1) && aligned16(f0) && aligned16(f1);
  for (const void* p : {static_cast<const void*>(out), y0, y1, f0, f1})
    if (!tv_aligned(p, esz)) return fail(XDE_EBADARG, who + ": operand not aligned to its element type");
  bool clash = tv_overlap(out, obytes, y0, nbytes) || tv_overlap(out, obytes, y1, nbytes) || tv_overlap(out, obytes, f0, nbytes) ||
               tv_overlap(out, obytes, f1, nbytes);
  for (int j = 0; j < nk; ++j) {
    if (!k[j]) return fail(XDE_EBADARG, who + ": null k[j]");
    if (!tv_aligned(k[j], esz)) return fail(XDE_EBADARG, who + ": operand not aligned to its element type");
    clash = clash || tv_overlap(out, obytes, k[j], nbytes);
    a.k[j] = k[j];
    a.mid[j] = mid[j];
    vec = vec && aligned16(k[j]);
  }
  if (clash) return fail(XDE_EBADARG, who + ": out overlaps a state operand");
  a.out = out;
  a.y0 = y0;
  a.y1 = y1;
  a.f0 = f0;
  a.f1 = f1;
  a.s = TevalStep{tq, cnt, t0, t1, dt, direction, time_dtype};
  a.nk = nk;
  a.k0_is_f0 = k[0] == f0 ? 1 : 0;
  a.klast_is_f1 = (nk > 1 && k[nk - 1] == f1) ? 1 : 0;
  a.m = tv_map(rows, D, Q, dtype, vec, aligned16(out));
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_DENSE, double(nk + 5) * double(nbytes));
  const dim3 gr = tv_grid(a.m), b(kBlock);
#define TEVAL_D(T)                                                                            \
  switch (nk) {                                                                               \
    case 1: XDE_LAUNCH((xde_teval_dense_kernel<T, 1>), gr, b, st, prof, a); break;            \
    case 2: XDE_LAUNCH((xde_teval_dense_kernel<T, 2>), gr, b, st, prof, a); break;            \
    case 3: XDE_LAUNCH((xde_teval_dense_kernel<T, 3>), gr, b, st, prof, a); break;            \
    case 4: XDE_LAUNCH((xde_teval_dense_kernel<T, 4>), gr, b, st, prof, a); break;            \
    case 5: XDE_LAUNCH((xde_teval_dense_kernel<T, 5>), gr, b, st, prof, a); break;            \
    case 6: XDE_LAUNCH((xde_teval_dense_kernel<T, 6>), gr, b, st, prof, a); break;            \
    case 7: XDE_LAUNCH((xde_teval_dense_kernel<T, 7>), gr, b, st, prof, a); break;            \
    default: XDE_LAUNCH((xde_teval_dense_kernel<T, 0>), gr, b, st, prof, a); break;           \
  }
  if (dtype == XDE_F32) TEVAL_D(float)
  else TEVAL_D(double)
#undef TEVAL_D
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_teval_cotangent(void* const* outs, const void* g, const double* tq, const int32_t* cnt, double t0, double t1, double dt,
                        int direction, int time_dtype, uint32_t acc_mask, int64_t rows, int64_t D, int64_t Q, int dtype, void* stream) {
  const std::string who = "xde_teval_cotangent";
  if (!outs || !g) return fail(XDE_EBADARG, who + ": null pointer");
  if (int rc = tv_check_times(who, tq, cnt)) return rc;
  if (int rc = tv_check_shape(who, rows, D, Q, dtype, time_dtype, direction, t0, t1, dt)) return rc;
  if (acc_mask >> kOuts) return fail(XDE_EBADARG, who + ": acc_mask has a bit beyond the five outputs");
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const size_t nbytes = size_t(rows) * size_t(D) * esz;
  const size_t gbytes = nbytes * size_t(Q);
  if (!tv_aligned(g, esz)) return fail(XDE_EBADARG, who + ": operand not aligned to its element type");
  TevalCotArgs a;
  memset(&a, 0, sizeof(a));
  int nout = 0, nacc = 0;
  bool vec = true;
  for (int j = 0; j < kOuts; ++j) {
    if (!outs[j]) continue;
    if (!tv_aligned(outs[j], esz)) return fail(XDE_EBADARG, who + ": operand not aligned to its element type");
    if (tv_overlap(outs[j], nbytes, g, gbytes)) return fail(XDE_EBADARG, who + ": an output overlaps g");
    for (int i = 0; i < j; ++i)
      if (tv_overlap(outs[j], nbytes, outs[i], nbytes)) return fail(XDE_EBADARG, who + ": two outputs overlap");
    a.out[j] = outs[j];
    vec = vec && aligned16(outs[j]);
    ++nout;
    nacc += (acc_mask >> j) & 1u;
  }
  if (nout == 0) return fail(XDE_EBADARG, who + ": every output is null");
  a.g = g;
  a.s = TevalStep{tq, cnt, t0, t1, dt, direction, time_dtype};
  a.acc = acc_mask;
  a.m = tv_map(rows, D, Q, dtype, vec, aligned16(g));
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_DENSE, double(1 + nout + nacc) * double(nbytes));
  const dim3 gr = tv_grid(a.m), b(kBlock);
  if (dtype == XDE_F32) XDE_LAUNCH((xde_teval_cotangent_kernel<float>), gr, b, st, prof, a);
  else XDE_LAUNCH((xde_teval_cotangent_kernel<double>), gr, b, st, prof, a);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"
