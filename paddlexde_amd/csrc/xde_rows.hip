// libxde_hip.so — per-sample adaptive stepping: every row of the batch its own step (C ABI: include/xde_hip_rows.h, the
// specification, op by op; host: paddlexde_amd/solver/_rk_rows.py).
//
// All four kernels are streams over rows x D operands with a [rows] control block beside them.
//
// xde_rows_stage_combine is FLAT: a lane owns 16-byte vectors of the rows x D array whatever D is.  The kernel finds the aligned part
// of the array from the pointers' own bits (all operands share one phase, else the element-wise instantiation runs), so an
// element-aligned pointer and a vector that straddles two rows take the same path: the row of a vector's first element comes from one
// division per lane, advanced by the grid stride's quotient and remainder from then on, and a carry moves to the next row inside a
// vector.  A row's coefficients c_j = T(coef_j) * T(h_r) are formed where the row changes.
//
// The other three kernels own ROWS: G lanes work on a row, G = min(256, pow2 >= ceil(D / W)) a function of D alone — several rows per
// wave at small D, a workgroup per row at large D, D beyond one workgroup's stride as a loop in that workgroup.  A lane walks the
// chunks g, g + G, ... of its row (one 16-byte load per operand where the row starts on a 16-byte boundary, single elements else:
// the same arithmetic), sums float64 squares sequentially, and the lanes' sums meet in a butterfly of ascending offsets (in the wave by
// cross-lane moves, across the waves of a workgroup through LDS): the pairwise tree the header states, the same for every launch
// shape.  No atomics, no scratch.  One lane per row then runs control_step of xde_control_device.hpp on a block built from the row's
// planes: xde_rows_norm_control takes its rows in batches, the batch's sums first, then its controllers side by side.  Built with
// -ffp-contract=off like the rest of the library.

#include "xde_common.hpp"
#include "xde_control_device.hpp"
#include "xde_hip_rows.h"

using namespace xde;

namespace {

constexpr int64_t kRowsMaxElems = int64_t(1) << 40;
constexpr int64_t kRowsMaxOut = int64_t(1) << 48;
constexpr int64_t kRowsFillBlocks = 1024;  // workgroups that fill the device: 256 CUs, four workgroups of 256 lanes each

struct RowsCtl {  // xde_rows_ctl_t's planes
  double *t, *t_prev, *h, *h_used, *ratio, *nonfinite;
  int32_t *accept, *done, *status, *next_out, *n_accept, *n_reject, *steps_in_interval;
  void* t_stage;
};

// ------------------------------------------------------------------------------------------
// 1: the stage combine, flat
// ------------------------------------------------------------------------------------------
struct RowsCombineArgs {
  void* out;
  void* out2;
  const void* y0;
  const void* k[XDE_ROWS_MAX_K];
  double coef[XDE_ROWS_MAX_K];
  double coef2[XDE_ROWS_MAX_K];
  const double* h;
  const int32_t* done;
  int64_t N, D;
  int64_t head, nvec;      // single elements in front of the first vector; whole vectors
  int64_t step_q, step_r;  // divmod(grid stride in elements, D)
};

template <typename T, int NK, bool OUT2> struct RowCoef {
  T c[NK], c2[NK];
  bool done;
  __device__ __forceinline__ void of(const RowsCombineArgs& a, int64_t r) {
    const T dt = T(a.h[r]);
    done = a.done[r] != 0;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      c[j] = T(a.coef[j]) * dt;
      c2[j] = OUT2 ? dt * T(a.coef2[j]) : T(0);
    }
  }
};

template <typename T, int NK, bool OUT2, bool VEC>
__global__ __launch_bounds__(kBlock) void xde_rows_combine_kernel(RowsCombineArgs a) {
  using P = Pack<T, VEC>;
  constexpr int W = P::W;
  const T* kp[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) kp[j] = static_cast<const T*>(a.k[j]);
  const T* y0 = static_cast<const T*>(a.y0);
  T* out = static_cast<T*>(a.out);
  T* out2 = static_cast<T*>(a.out2);
  const int64_t D = a.D;
  RowCoef<T, NK, OUT2> rc;
  int64_t v = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (v < a.nvec) {
    const int64_t e0 = a.head + v * W;
    int64_t r = e0 / D, rem = e0 - r * D;  // the one division of this lane
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (; v < a.nvec; v += stride) {
      P kk[NK];
#pragma unroll
      for (int j = 0; j < NK; ++j) kk[j] = P::load(kp[j] + a.head, v);
      const P y = P::load(y0 + a.head, v);
      rc.of(a, r);
      int64_t rr = r, rm = rem;
      P o, o2;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        T acc = kk[0].v[w] * rc.c[0];
#pragma unroll
        for (int j = 1; j < NK; ++j) acc = acc + kk[j].v[w] * rc.c[j];
        o.v[w] = rc.done ? y.v[w] : y.v[w] + acc;
        if (OUT2) {
          T e = kk[0].v[w] * rc.c2[0];
#pragma unroll
          for (int j = 1; j < NK; ++j) e = e + kk[j].v[w] * rc.c2[j];
          o2.v[w] = e;
        }
        if (w + 1 < W && ++rm == D) {  // the carry: the vector goes on in the next row
          rm = 0;
          ++rr;
          rc.of(a, rr);
        }
      }
      o.store(out + a.head, v);
      if (OUT2) o2.store(out2 + a.head, v);
      r += a.step_q;
      rem += a.step_r;
      if (rem >= D) {
        rem -= D;
        ++r;
      }
    }
  }
  // the single elements at either end of the aligned part (at most 2 (W - 1))
  const int64_t tail0 = a.head + a.nvec * W;
  const int64_t edge = a.head + (a.N - tail0);
  if (VEC && blockIdx.x == 0 && int64_t(threadIdx.x) < edge) {
    const int64_t i = int64_t(threadIdx.x) < a.head ? int64_t(threadIdx.x) : tail0 + (threadIdx.x - a.head);
    rc.of(a, i / D);
    T acc = kp[0][i] * rc.c[0];
#pragma unroll
    for (int j = 1; j < NK; ++j) acc = acc + kp[j][i] * rc.c[j];
    if (OUT2) {
      T e = kp[0][i] * rc.c2[0];
#pragma unroll
      for (int j = 1; j < NK; ++j) e = e + kp[j][i] * rc.c2[j];
      out2[i] = e;
    }
    const T yv = y0[i];
    out[i] = rc.done ? yv : yv + acc;
  }
}

// ------------------------------------------------------------------------------------------
// rows owned by groups of G lanes
// ------------------------------------------------------------------------------------------
struct RowMap {
  int32_t G, rpb;  // lanes of a row; rows of a workgroup
  int32_t C;       // chunks of a row
  int32_t vec;     // every operand pointer is 16-byte aligned
  int32_t batch;   // rows a workgroup of xde_rows_norm_control takes before it runs their controllers: a multiple of rpb
  int64_t rows, D, nrb;
};

template <typename T> __device__ __forceinline__ void load_chunk(const T* p, int64_t o, int n, bool vec, T (&x)[VecOf<T>::W]) {
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

template <typename T> __device__ __forceinline__ void store_chunk(T* p, int64_t o, int n, bool vec, const T (&x)[VecOf<T>::W]) {
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

// THE ROW SUM's tree over the lanes' sums (ascending offsets: (S_0 + S_1), (S_2 + S_3), ... then pairs of pairs); every lane of the
// group ends with the row's values.  Reached by all threads of the workgroup (G > 64 is uniform over it).
__device__ __forceinline__ void group_sum(double& s, int& nf, int G) {
  __shared__ double ls[kWaves];
  __shared__ int ln[kWaves];
  for (int off = 1; off < G && off < 64; off <<= 1) {
    s = s + __shfl_xor(s, off, 64);
    nf += __shfl_xor(nf, off, 64);
  }
  if (G > 64) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      ls[wave] = s;
      ln[wave] = nf;
    }
    __syncthreads();
    if (G == 128) {
      const int w0 = wave & ~1;
      s = ls[w0] + ls[w0 + 1];
      nf = ln[w0] + ln[w0 + 1];
    } else {
      s = (ls[0] + ls[1]) + (ls[2] + ls[3]);
      nf = (ln[0] + ln[1]) + (ln[2] + ln[3]);
    }
    __syncthreads();  // (the next row of this workgroup writes ls again)
  }
}

// ------------------------------------------------------------------------------------------
// 2: error norm + controller
// ------------------------------------------------------------------------------------------
struct RowsNormArgs {
  const void* k[XDE_ROWS_MAX_K];
  double coef[XDE_ROWS_MAX_K];
  const void* e_pre;
  const void* y0;
  const void* y1;
  RowsCtl ctl;
  xde_ctrl_params_t p;  // n_stage = 0: control_step writes no stage times
  const double* t_span;
  int32_t n_out, n_stage;
  RowMap m;
};

template <typename T> __device__ __forceinline__ void rows_control(const RowsNormArgs& a, int64_t r, double sum, int nf) {
  const RowsCtl& c = a.ctl;
  const double cnt = double(a.m.D);
  const double ratio = norm_from_sums(&sum, &cnt, 1, XDE_NORM_RMS, a.p.state_dtype, nullptr);
  // the row's planes as a control block of xde_rk_control's (only scalar fields are touched: it lives in registers)
  xde_ctrl_t z;
  z.t1 = c.t[r];
  z.dt = c.h[r];
  z.t_plan = a.p.time_dtype == XDE_F32 ? double(float(z.t1) + float(z.dt)) : z.t1 + z.dt;
  z.ratio_prev = 0.0;
  z.n_steps = 0;
  z.n_accept = c.n_accept[r];
  z.n_reject = c.n_reject[r];
  z.steps_in_interval = c.steps_in_interval[r];
  z.accept = 0;
  z.status = c.status[r];
  z.next_out = c.next_out[r];
  z.n_out = a.n_out;
  z.done = 0;
  z.next_step_index = 0;
  z.on_step_t = 0;
  // (a.p.n_stage is 0: the stage times are written below, in the [stage][rows] layout)
  if (a.p.time_dtype == XDE_F32) control_step<float>(&z, a.p, ratio, double(nf), a.t_span, nullptr, nullptr);
  else control_step<double>(&z, a.p, ratio, double(nf), a.t_span, nullptr, nullptr);
  c.t_prev[r] = z.t0;
  c.t[r] = z.t1;
  c.h_used[r] = z.dt_last;
  c.h[r] = z.dt;
  c.ratio[r] = z.ratio;
  c.nonfinite[r] = z.nonfinite;
  c.accept[r] = z.accept;
  c.status[r] = z.status;
  c.n_accept[r] = int32_t(z.n_accept);
  c.n_reject[r] = int32_t(z.n_reject);
  c.steps_in_interval[r] = int32_t(z.steps_in_interval);
  T* ts = static_cast<T*>(c.t_stage);
  for (int i = 0; i < a.n_stage; ++i) {
    const T al = T(a.p.alpha[i]);
    ts[int64_t(i) * a.m.rows + r] = z.done ? T(z.t1) : (al == T(1) ? T(z.t_plan) : T(z.t1) + al * T(z.dt));
  }
}

template <typename T, int NK, bool PRE> __global__ __launch_bounds__(kBlock) void xde_rows_norm_control_kernel(RowsNormArgs a) {
  constexpr int W = VecOf<T>::W;
  const RowMap& m = a.m;
  const T* kp[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) kp[j] = static_cast<const T*>(a.k[j]);
  const T* epre = static_cast<const T*>(a.e_pre);
  const T* y0 = static_cast<const T*>(a.y0);
  const T* y1 = static_cast<const T*>(a.y1);
  const T rtol = T(a.p.rtol), atol = T(a.p.atol);
  const int g = threadIdx.x & (m.G - 1);
  // A workgroup takes a BATCH of m.batch consecutive rows (rows_map: one pass of rpb rows, up to 64 rows while the grid still fills
  // the device): their sums first, group by group, into LDS; then one lane per row runs the controller, all rows
  // of the batch side by side (the controller is some hundred dependent instructions and a float64 pow: run by
  // one lane of a group after its own row it would hold the whole wave for two rows' worth of traffic).
  __shared__ double bs[kBlock];
  __shared__ int bn[kBlock];
  const int64_t nbatch = (m.rows + m.batch - 1) / m.batch;
  for (int64_t bb = blockIdx.x; bb < nbatch; bb += gridDim.x) {  // (workgroup-uniform: every barrier below is reached by all)
    for (int it = 0; it < m.batch / m.rpb; ++it) {
      const int rl = it * m.rpb + int(threadIdx.x) / m.G;
      const int64_t r = bb * m.batch + rl;
      const bool live = r < m.rows;
      bool frozen = true;
      T c[NK];
      if (live) {
        frozen = a.ctl.done[r] != 0 || a.ctl.status[r] != XDE_STATUS_OK;
        const T dt = T(a.ctl.h[r]);
#pragma unroll
        for (int j = 0; j < NK; ++j) c[j] = dt * T(a.coef[j]);  // `dt * tableau.c_error`
      }
      double s = 0.0;
      int nf = 0;
      if (!frozen) {
        const int64_t base = r * m.D;
        const bool rowvec = m.vec && (base % W) == 0;
        for (int ch = g; ch < m.C; ch += m.G) {
          const int64_t o = base + int64_t(ch) * W;
          const int64_t left = m.D - int64_t(ch) * W;
          const int n = left < W ? int(left) : W;
          const bool vec = rowvec && n == W;
          T kk[NK][W], ep[W], a0[W], a1[W];
          load_chunk<T>(y1, o, n, vec, a1);
          if (PRE) load_chunk<T>(epre, o, n, vec, ep);
#pragma unroll
          for (int j = 0; j < NK; ++j) load_chunk<T>(kp[j], o, n, vec, kk[j]);
          load_chunk<T>(y0, o, n, vec, a0);
#pragma unroll
          for (int w = 0; w < W; ++w) {
            if (w < n) {
              T e = PRE ? ep[w] + kk[0][w] * c[0] : kk[0][w] * c[0];
#pragma unroll
              for (int j = 1; j < NK; ++j) e = e + kk[j][w] * c[j];
              const T tol = atol + rtol * fmax_(abs_(a0[w]), abs_(a1[w]));
              const T q = e / tol;
              s = s + double(q) * double(q);
              nf += finite_(a0[w]) ? 0 : 1;
            }
          }
        }
      }
      group_sum(s, nf, m.G);
      if (live && g == 0) {
        bs[rl] = s;
        bn[rl] = nf;
      }
    }
    __syncthreads();
    const int64_t r = bb * m.batch + threadIdx.x;
    if (int(threadIdx.x) < m.batch && r < m.rows) {
      if (a.ctl.done[r] != 0 || a.ctl.status[r] != XDE_STATUS_OK) a.ctl.accept[r] = 0;
      else rows_control<T>(a, r, bs[threadIdx.x], bn[threadIdx.x]);
    }
    __syncthreads();  // (the next batch writes bs again)
  }
}

// ------------------------------------------------------------------------------------------
// 3: dense output + commit
// ------------------------------------------------------------------------------------------
struct RowsDenseArgs {
  void* out;
  const void* k[XDE_ROWS_MAX_K];
  double mid[XDE_ROWS_MAX_K];
  void* y0;
  const void* y1;
  void* f0;
  const void* f1;
  RowsCtl ctl;
  const double* t_span;
  int32_t n_out, direction, time_dtype;
  RowMap m;
};

// interp_fit (utils/ode_utils.py:44-49) + interp_evaluate (:69-77), xde_dense.hip's op order
template <typename T> __device__ __forceinline__ T rows_quartic(T y0v, T y1v, T f0v, T f1v, T ymid, T x, T dt) {
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

template <typename TT> __device__ __forceinline__ bool rows_covers(double ts, double t1, int dir) { return TT(dir) * TT(ts) <= TT(dir) * TT(t1); }
template <typename T, typename TT> __device__ __forceinline__ T rows_frac(double ts, double t0, double t1) {
  return T((TT(ts) - TT(t0)) / (TT(t1) - TT(t0)));
}

template <typename T, int NK> __global__ __launch_bounds__(kBlock) void xde_rows_dense_commit_kernel(RowsDenseArgs a) {
  constexpr int W = VecOf<T>::W;
  const RowMap& m = a.m;
  const T* kp[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) kp[j] = static_cast<const T*>(a.k[j]);
  T* y0 = static_cast<T*>(a.y0);
  T* f0 = static_cast<T*>(a.f0);
  const T* y1 = static_cast<const T*>(a.y1);
  const T* f1 = static_cast<const T*>(a.f1);
  T* out = static_cast<T*>(a.out);
  const bool t32 = a.time_dtype == XDE_F32;
  const int g = threadIdx.x & (m.G - 1);
  for (int64_t rb = blockIdx.x; rb < m.nrb; rb += gridDim.x) {  // (workgroup-uniform: the barrier below is reached by all)
    const int64_t r = rb * m.rpb + threadIdx.x / m.G;
    const bool on = r < m.rows && a.ctl.accept[r] != 0;
    int ob = 0, oe = 0;
    if (on) {
      const double t0 = a.ctl.t_prev[r], t1 = a.ctl.t[r];
      const T dt = t32 ? T(float(a.ctl.h_used[r])) : T(a.ctl.h_used[r]);  // `dt.astype(y0.dtype)`
      ob = oe = a.ctl.next_out[r];
      while (oe < a.n_out && (t32 ? rows_covers<float>(a.t_span[oe], t1, a.direction) : rows_covers<double>(a.t_span[oe], t1, a.direction))) ++oe;
      T cm[NK];
#pragma unroll
      for (int j = 0; j < NK; ++j) cm[j] = dt * T(a.mid[j]);  // `dt * self.mid`
      const int64_t base = r * m.D;
      const bool rowvec = m.vec && (base % W) == 0;
      for (int ch = g; ch < m.C; ch += m.G) {
        const int64_t o = base + int64_t(ch) * W;
        const int64_t left = m.D - int64_t(ch) * W;
        const int n = left < W ? int(left) : W;
        const bool vec = rowvec && n == W;
        T a1[W], b1[W];
        load_chunk<T>(y1, o, n, vec, a1);
        load_chunk<T>(f1, o, n, vec, b1);
        if (oe > ob) {
          T kk[NK][W], a0[W], ym[W];
#pragma unroll
          for (int j = 0; j < NK; ++j) load_chunk<T>(kp[j], o, n, vec, kk[j]);
          load_chunk<T>(y0, o, n, vec, a0);
#pragma unroll
          for (int w = 0; w < W; ++w) {
            T acc = kk[0][w] * cm[0];
#pragma unroll
            for (int j = 1; j < NK; ++j) acc = acc + kk[j][w] * cm[j];
            ym[w] = a0[w] + acc;
          }
          for (int j = ob; j < oe; ++j) {
            const T x = t32 ? rows_frac<T, float>(a.t_span[j], t0, t1) : rows_frac<T, double>(a.t_span[j], t0, t1);
            T q[W];
#pragma unroll
            for (int w = 0; w < W; ++w) q[w] = rows_quartic<T>(a0[w], a1[w], kk[0][w], b1[w], ym[w], x, dt);
            const int64_t oo = (int64_t(j) * m.rows + r) * m.D + int64_t(ch) * W;
            store_chunk<T>(out, oo, n, m.vec && n == W && (oo % W) == 0, q);
          }
        }
        store_chunk<T>(y0, o, n, vec, a1);
        store_chunk<T>(f0, o, n, vec, b1);
      }
    }
    if (m.G > 64) __syncthreads();  // every wave of the row has read the cursor
    if (on && g == 0) {
      a.ctl.next_out[r] = oe;
      a.ctl.done[r] = oe >= a.n_out ? 1 : 0;
    }
  }
}

// ------------------------------------------------------------------------------------------
// 4: the scaled norms of the initial-step heuristic
// ------------------------------------------------------------------------------------------
struct RowsScaledArgs {
  double* out;
  const void* a;
  const void* b;
  const void* y0;
  double rtol, atol;
  int32_t state_dtype;
  RowMap m;
};

template <typename T, bool DIFF> __global__ __launch_bounds__(kBlock) void xde_rows_scaled_norm_kernel(RowsScaledArgs a) {
  constexpr int W = VecOf<T>::W;
  const RowMap& m = a.m;
  const T* pa = static_cast<const T*>(a.a);
  const T* pb = static_cast<const T*>(a.b);
  const T* y0 = static_cast<const T*>(a.y0);
  const T rtol = T(a.rtol), atol = T(a.atol);
  const int g = threadIdx.x & (m.G - 1);
  for (int64_t rb = blockIdx.x; rb < m.nrb; rb += gridDim.x) {
    const int64_t r = rb * m.rpb + threadIdx.x / m.G;
    const bool live = r < m.rows;
    double s = 0.0;
    int nf = 0;
    if (live) {
      const int64_t base = r * m.D;
      const bool rowvec = m.vec && (base % W) == 0;
      for (int ch = g; ch < m.C; ch += m.G) {
        const int64_t o = base + int64_t(ch) * W;
        const int64_t left = m.D - int64_t(ch) * W;
        const int n = left < W ? int(left) : W;
        const bool vec = rowvec && n == W;
        T xa[W], xb[W], yy[W];
        load_chunk<T>(pa, o, n, vec, xa);
        if (DIFF) load_chunk<T>(pb, o, n, vec, xb);
        load_chunk<T>(y0, o, n, vec, yy);
#pragma unroll
        for (int w = 0; w < W; ++w) {
          if (w < n) {
            const T scale = atol + abs_(yy[w]) * rtol;
            const T q = (DIFF ? xa[w] - xb[w] : xa[w]) / scale;
            s = s + double(q) * double(q);
          }
        }
      }
    }
    group_sum(s, nf, m.G);
    if (live && g == 0) {
      const double cnt = double(m.D);
      a.out[r] = norm_from_sums(&s, &cnt, 1, XDE_NORM_RMS, a.state_dtype, nullptr);
    }
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
bool rows_aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

bool rows_overlap(const void* a, const void* b, size_t n) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + n && y < x + n;
}

int rows_check_shape(const std::string& who, int64_t rows, int64_t D, int dtype) {
  if (rows < 1) return fail(XDE_EBADARG, who + ": rows < 1");
  if (D < 1) return fail(XDE_EBADARG, who + ": D < 1");
  if (rows > kRowsMaxElems / D) return fail(XDE_EBADARG, who + ": rows * D is too large (> 2^40)");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, who + ": bad dtype");
  return XDE_OK;
}

int rows_check_out(const std::string& who, int32_t n_out, int64_t rows, int64_t D) {
  if (n_out < 1) return fail(XDE_EBADARG, who + ": n_out out of range (1 <= n_out <= 2^31 - 1)");
  if (int64_t(n_out) > kRowsMaxOut / (rows * D)) return fail(XDE_EBADARG, who + ": n_out * rows * D is too large (> 2^48)");
  return XDE_OK;
}

int rows_check_nk(const std::string& who, const void* const* k, const double* coef, int nk, size_t esz) {
  if (!k || !coef) return fail(XDE_EBADARG, who + ": null pointer");
  if (nk < 1 || nk > XDE_ROWS_MAX_K) return fail(XDE_EBADARG, who + ": nk out of range (1 <= nk <= 7)");
  for (int j = 0; j < nk; ++j) {
    if (!k[j]) return fail(XDE_EBADARG, who + ": null k[j]");
    if (!rows_aligned(k[j], esz)) return fail(XDE_EBADARG, who + ": operand not aligned to its element type");
  }
  return XDE_OK;
}

int rows_check_ctl(const std::string& who, const xde_rows_ctl_t* ctl, size_t esz, bool need_stage, RowsCtl* out) {
  if (!ctl) return fail(XDE_EBADARG, who + ": null ctl");
  if (ctl->struct_size != sizeof(xde_rows_ctl_t))
    return fail(XDE_EBADARG, who + ": xde_rows_ctl_t layout mismatch: the caller says struct_size=" + std::to_string(ctl->struct_size) +
                                 ", this library has sizeof=" + std::to_string(sizeof(xde_rows_ctl_t)));
  for (const void* p : {static_cast<const void*>(ctl->t), static_cast<const void*>(ctl->t_prev), static_cast<const void*>(ctl->h),
                        static_cast<const void*>(ctl->h_used), static_cast<const void*>(ctl->ratio), static_cast<const void*>(ctl->nonfinite)}) {
    if (!p) return fail(XDE_EBADARG, who + ": null plane in ctl");
    if (!rows_aligned(p, 8)) return fail(XDE_EBADARG, who + ": plane of ctl not aligned to its element type");
  }
  for (const void* p : {static_cast<const void*>(ctl->accept), static_cast<const void*>(ctl->done), static_cast<const void*>(ctl->status),
                        static_cast<const void*>(ctl->next_out), static_cast<const void*>(ctl->n_accept), static_cast<const void*>(ctl->n_reject),
                        static_cast<const void*>(ctl->steps_in_interval)}) {
    if (!p) return fail(XDE_EBADARG, who + ": null plane in ctl");
    if (!rows_aligned(p, 4)) return fail(XDE_EBADARG, who + ": plane of ctl not aligned to its element type");
  }
  if (need_stage && !ctl->t_stage) return fail(XDE_EBADARG, who + ": null plane in ctl (t_stage)");
  if (ctl->t_stage && !rows_aligned(ctl->t_stage, esz)) return fail(XDE_EBADARG, who + ": plane of ctl not aligned to its element type");
  *out = RowsCtl{ctl->t, ctl->t_prev, ctl->h, ctl->h_used, ctl->ratio, ctl->nonfinite, ctl->accept, ctl->done, ctl->status, ctl->next_out,
                 ctl->n_accept, ctl->n_reject, ctl->steps_in_interval, ctl->t_stage};
  return XDE_OK;
}

// what the row kernels need of the controller's parameters
int rows_check_params(const std::string& who, const xde_ctrl_params_t* p, int dtype) {
  if (int rc = check_params(p, who.c_str())) return rc;
  if (p->state_dtype != dtype) return fail(XDE_EBADARG, who + ": params->state_dtype is not the operands' dtype");
  if (p->n_step_t != 0 || p->replay || p->pi_controller)
    return fail(XDE_EBADARG, who + ": step_t, a prescribed step sequence and the PI controller are not served per row");
  if (p->norm_kind != XDE_NORM_RMS) return fail(XDE_EBADARG, who + ": the row norm is the RMS norm");
  return XDE_OK;
}

RowMap rows_map(int64_t rows, int64_t D, int dtype, bool vec) {
  RowMap m;
  const int W = dtype == XDE_F32 ? 4 : 2;
  const int64_t C = (D + W - 1) / W;
  int G = 1;
  while (G < kBlock && G < C) G <<= 1;
  m.G = G;
  m.rpb = kBlock / G;
  m.C = int32_t(C);  // (D <= 2^40 / rows; C fits 32 bits for D < 2^32: checked by the callers through rows_check_map)
  m.vec = vec ? 1 : 0;
  m.rows = rows;
  m.D = D;
  m.nrb = (rows + m.rpb - 1) / m.rpb;
  // xde_rows_norm_control's batch: the rows of one pass (rpb), doubled up to 64 only while the launch still has kRowsFillBlocks
  // workgroups — so a batch never takes workgroups that a small batch of samples needs to fill the device, and at large D with few
  // rows the launch is a workgroup per row, the controller's cost spread over the row's own traffic
  m.batch = m.rpb;
  while (m.batch < 64 && rows >= int64_t(2) * m.batch * kRowsFillBlocks) m.batch *= 2;
  return m;
}

int rows_check_map(const std::string& who, int64_t D) {
  if (D > (int64_t(1) << 31)) return fail(XDE_EBADARG, who + ": D is too large for a row-owning launch (D <= 2^31)");
  return XDE_OK;
}

dim3 rows_grid(const RowMap& m) {
  int64_t blocks = m.nrb;
  if (blocks > grid_cap()) blocks = grid_cap();
  return dim3(static_cast<unsigned>(blocks));
}

}  // namespace

extern "C" {

// (profiled under the ids of the launches they stand for: the kernel-id list of xde_hip.h is part of the frozen ABI)
int xde_rows_stage_combine(void* out, void* out2, const void* y0, const void* const* k, const double* coef, const double* coef2, int nk,
                           const xde_rows_ctl_t* ctl, int64_t rows, int64_t D, int dtype, void* stream) {
  const std::string who = "xde_rows_stage_combine";
  if (!out || !y0) return fail(XDE_EBADARG, who + ": null pointer");
  if ((out2 == nullptr) != (coef2 == nullptr)) return fail(XDE_EBADARG, who + ": out2 and coef2 come together");
  if (int rc = rows_check_shape(who, rows, D, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  if (int rc = rows_check_nk(who, k, coef, nk, esz)) return rc;
  for (const void* p : {static_cast<const void*>(out), static_cast<const void*>(out2), y0})
    if (p && !rows_aligned(p, esz)) return fail(XDE_EBADARG, who + ": operand not aligned to its element type");
  RowsCtl c;
  if (int rc = rows_check_ctl(who, ctl, esz, false, &c)) return rc;
  const int64_t N = rows * D;
  const size_t nbytes = size_t(N) * esz;
  bool clash = rows_overlap(out, y0, nbytes) || rows_overlap(out2, y0, nbytes) || rows_overlap(out, out2, nbytes);
  for (int j = 0; j < nk; ++j) clash = clash || rows_overlap(out, k[j], nbytes) || rows_overlap(out2, k[j], nbytes);
  if (clash) return fail(XDE_EBADARG, who + ": an output overlaps another operand");
  RowsCombineArgs a;
  memset(&a, 0, sizeof(a));
  a.out = out;
  a.out2 = out2;
  a.y0 = y0;
  const int W = dtype == XDE_F32 ? 4 : 2;
  const auto phase = [&](const void* p) { return int((reinterpret_cast<uintptr_t>(p) / esz) % W); };
  bool vec = phase(out) == phase(y0) && (!out2 || phase(out2) == phase(y0));
  for (int j = 0; j < nk; ++j) {
    a.k[j] = k[j];
    a.coef[j] = coef[j];
    if (coef2) a.coef2[j] = coef2[j];
    vec = vec && phase(k[j]) == phase(y0);
  }
  a.h = c.h;
  a.done = c.done;
  a.N = N;
  a.D = D;
  if (vec) {
    a.head = (W - phase(y0)) % W;
    if (a.head > N) a.head = N;
    a.nvec = (N - a.head) / W;
  } else {
    a.head = 0;
    a.nvec = N;
  }
  int64_t blocks = (a.nvec + kBlock - 1) / kBlock;
  if (blocks > grid_cap()) blocks = grid_cap();
  if (blocks < 1) blocks = 1;
  const int64_t stride = blocks * kBlock * (vec ? W : 1);
  a.step_q = stride / D;
  a.step_r = stride % D;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double(nk + 2 + (out2 ? 1 : 0)) * double(nbytes));
  const dim3 gr(static_cast<unsigned>(blocks)), b(kBlock);
#define ROWS_L4(T, NK)                                                                                   \
  do {                                                                                                   \
    if (out2 && vec) XDE_LAUNCH((xde_rows_combine_kernel<T, NK, true, true>), gr, b, st, prof, a);       \
    else if (out2) XDE_LAUNCH((xde_rows_combine_kernel<T, NK, true, false>), gr, b, st, prof, a);        \
    else if (vec) XDE_LAUNCH((xde_rows_combine_kernel<T, NK, false, true>), gr, b, st, prof, a);         \
    else XDE_LAUNCH((xde_rows_combine_kernel<T, NK, false, false>), gr, b, st, prof, a);                 \
  } while (0)
#define ROWS_NK(T)                  \
  switch (nk) {                     \
    case 1: ROWS_L4(T, 1); break;   \
    case 2: ROWS_L4(T, 2); break;   \
    case 3: ROWS_L4(T, 3); break;   \
    case 4: ROWS_L4(T, 4); break;   \
    case 5: ROWS_L4(T, 5); break;   \
    case 6: ROWS_L4(T, 6); break;   \
    default: ROWS_L4(T, 7); break;  \
  }
  if (dtype == XDE_F32) ROWS_NK(float)
  else ROWS_NK(double)
#undef ROWS_L4
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_rows_norm_control(const void* const* k, const double* c_err, int nk, const void* e_pre, const void* y0, const void* y1,
                          const xde_rows_ctl_t* ctl, const xde_ctrl_params_t* params, const double* t_span, int32_t n_out, int64_t rows,
                          int64_t D, int dtype, void* stream) {
  const std::string who = "xde_rows_norm_control";
  if (!y0 || !y1 || !t_span) return fail(XDE_EBADARG, who + ": null pointer");
  if (int rc = rows_check_shape(who, rows, D, dtype)) return rc;
  if (int rc = rows_check_map(who, D)) return rc;
  if (int rc = rows_check_out(who, n_out, rows, D)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  if (int rc = rows_check_nk(who, k, c_err, nk, esz)) return rc;
  if (e_pre && nk != 1) return fail(XDE_EBADARG, who + ": e_pre takes exactly one remaining operand");
  for (const void* p : {e_pre, y0, y1})
    if (p && !rows_aligned(p, esz)) return fail(XDE_EBADARG, who + ": operand not aligned to its element type");
  if (!rows_aligned(t_span, 8)) return fail(XDE_EBADARG, who + ": t_span not aligned to its element type");
  if (int rc = rows_check_params(who, params, dtype)) return rc;
  RowsNormArgs a;
  memset(&a, 0, sizeof(a));
  if (int rc = rows_check_ctl(who, ctl, esz, true, &a.ctl)) return rc;
  bool vec = aligned16(y0) && aligned16(y1) && (!e_pre || aligned16(e_pre));
  for (int j = 0; j < nk; ++j) {
    a.k[j] = k[j];
    a.coef[j] = c_err[j];
    vec = vec && aligned16(k[j]);
  }
  a.e_pre = e_pre;
  a.y0 = y0;
  a.y1 = y1;
  a.p = *params;
  a.n_stage = params->n_stage;
  a.p.n_stage = 0;
  a.t_span = t_span;
  a.n_out = n_out;
  a.m = rows_map(rows, D, dtype, vec);
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_ERRNORM, double(nk + 2 + (e_pre ? 1 : 0)) * double(rows) * double(D) * double(esz));
  int64_t nbatch = (rows + a.m.batch - 1) / a.m.batch;
  if (nbatch > grid_cap()) nbatch = grid_cap();
  const dim3 gr(static_cast<unsigned>(nbatch)), b(kBlock);
#define ROWS_NC(T)                                                                                             \
  do {                                                                                                         \
    if (e_pre) XDE_LAUNCH((xde_rows_norm_control_kernel<T, 1, true>), gr, b, st, prof, a);                     \
    else switch (nk) {                                                                                         \
      case 1: XDE_LAUNCH((xde_rows_norm_control_kernel<T, 1, false>), gr, b, st, prof, a); break;              \
      case 2: XDE_LAUNCH((xde_rows_norm_control_kernel<T, 2, false>), gr, b, st, prof, a); break;              \
      case 3: XDE_LAUNCH((xde_rows_norm_control_kernel<T, 3, false>), gr, b, st, prof, a); break;              \
      case 4: XDE_LAUNCH((xde_rows_norm_control_kernel<T, 4, false>), gr, b, st, prof, a); break;              \
      case 5: XDE_LAUNCH((xde_rows_norm_control_kernel<T, 5, false>), gr, b, st, prof, a); break;              \
      case 6: XDE_LAUNCH((xde_rows_norm_control_kernel<T, 6, false>), gr, b, st, prof, a); break;              \
      default: XDE_LAUNCH((xde_rows_norm_control_kernel<T, 7, false>), gr, b, st, prof, a); break;             \
    }                                                                                                          \
  } while (0)
  if (dtype == XDE_F32) ROWS_NC(float);
  else ROWS_NC(double);
#undef ROWS_NC
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_rows_dense_commit(void* out, const void* const* k, const double* mid, int nk, void* y0, const void* y1, void* f0, const void* f1,
                          const xde_rows_ctl_t* ctl, const xde_ctrl_params_t* params, const double* t_span, int32_t n_out, int64_t rows,
                          int64_t D, int dtype, void* stream) {
  const std::string who = "xde_rows_dense_commit";
  if (!out || !y0 || !y1 || !f0 || !f1 || !t_span) return fail(XDE_EBADARG, who + ": null pointer");
  if (int rc = rows_check_shape(who, rows, D, dtype)) return rc;
  if (int rc = rows_check_map(who, D)) return rc;
  if (int rc = rows_check_out(who, n_out, rows, D)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  if (int rc = rows_check_nk(who, k, mid, nk, esz)) return rc;
  if (k[0] != f0) return fail(XDE_EBADARG, who + ": k[0] must be f0 (the derivative at the step's start)");
  for (const void* p : {static_cast<const void*>(out), static_cast<const void*>(y0), y1, static_cast<const void*>(f0), f1})
    if (!rows_aligned(p, esz)) return fail(XDE_EBADARG, who + ": operand not aligned to its element type");
  if (!rows_aligned(t_span, 8)) return fail(XDE_EBADARG, who + ": t_span not aligned to its element type");
  if (int rc = rows_check_params(who, params, dtype)) return rc;
  const size_t nbytes = size_t(rows) * size_t(D) * esz;
  bool clash = rows_overlap(y0, y1, nbytes) || rows_overlap(y0, f0, nbytes) || rows_overlap(y0, f1, nbytes) || rows_overlap(f0, y1, nbytes) ||
               rows_overlap(f0, f1, nbytes);
  for (int j = 1; j < nk; ++j) clash = clash || rows_overlap(y0, k[j], nbytes) || rows_overlap(f0, k[j], nbytes);
  if (clash) return fail(XDE_EBADARG, who + ": y0 / f0 overlap another operand");
  RowsDenseArgs a;
  memset(&a, 0, sizeof(a));
  if (int rc = rows_check_ctl(who, ctl, esz, false, &a.ctl)) return rc;
  bool vec = aligned16(out) && aligned16(y0) && aligned16(y1) && aligned16(f0) && aligned16(f1);
  for (int j = 0; j < nk; ++j) {
    a.k[j] = k[j];
    a.mid[j] = mid[j];
    vec = vec && aligned16(k[j]);
  }
  a.out = out;
  a.y0 = y0;
  a.y1 = y1;
  a.f0 = f0;
  a.f1 = f1;
  a.t_span = t_span;
  a.n_out = n_out;
  a.direction = params->direction;
  a.time_dtype = params->time_dtype;
  a.m = rows_map(rows, D, dtype, vec);
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_DENSE, 4.0 * double(nbytes));
  const dim3 gr = rows_grid(a.m), b(kBlock);
#define ROWS_DC(T)                                                                                   \
  switch (nk) {                                                                                      \
    case 1: XDE_LAUNCH((xde_rows_dense_commit_kernel<T, 1>), gr, b, st, prof, a); break;             \
    case 2: XDE_LAUNCH((xde_rows_dense_commit_kernel<T, 2>), gr, b, st, prof, a); break;             \
    case 3: XDE_LAUNCH((xde_rows_dense_commit_kernel<T, 3>), gr, b, st, prof, a); break;             \
    case 4: XDE_LAUNCH((xde_rows_dense_commit_kernel<T, 4>), gr, b, st, prof, a); break;             \
    case 5: XDE_LAUNCH((xde_rows_dense_commit_kernel<T, 5>), gr, b, st, prof, a); break;             \
    case 6: XDE_LAUNCH((xde_rows_dense_commit_kernel<T, 6>), gr, b, st, prof, a); break;             \
    default: XDE_LAUNCH((xde_rows_dense_commit_kernel<T, 7>), gr, b, st, prof, a); break;            \
  }
  if (dtype == XDE_F32) ROWS_DC(float)
  else ROWS_DC(double)
#undef ROWS_DC
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_rows_scaled_norm(double* out, const void* a_, const void* b_, const void* y0, double rtol, double atol, int64_t rows, int64_t D,
                         int dtype, void* stream) {
  const std::string who = "xde_rows_scaled_norm";
  if (!out || !a_ || !y0) return fail(XDE_EBADARG, who + ": null pointer");
  if (int rc = rows_check_shape(who, rows, D, dtype)) return rc;
  if (int rc = rows_check_map(who, D)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  for (const void* p : {a_, b_, y0})
    if (p && !rows_aligned(p, esz)) return fail(XDE_EBADARG, who + ": operand not aligned to its element type");
  if (!rows_aligned(out, 8)) return fail(XDE_EBADARG, who + ": out not aligned to its element type");
  RowsScaledArgs a;
  memset(&a, 0, sizeof(a));
  a.out = out;
  a.a = a_;
  a.b = b_;
  a.y0 = y0;
  a.rtol = rtol;
  a.atol = atol;
  a.state_dtype = dtype;
  a.m = rows_map(rows, D, dtype, aligned16(a_) && aligned16(y0) && (!b_ || aligned16(b_)));
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_SCALEDNORM, double(b_ ? 3 : 2) * double(rows) * double(D) * double(esz));
  const dim3 gr = rows_grid(a.m), b(kBlock);
  if (dtype == XDE_F32) {
    if (b_) XDE_LAUNCH((xde_rows_scaled_norm_kernel<float, true>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_rows_scaled_norm_kernel<float, false>), gr, b, st, prof, a);
  } else {
    if (b_) XDE_LAUNCH((xde_rows_scaled_norm_kernel<double, true>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_rows_scaled_norm_kernel<double, false>), gr, b, st, prof, a);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"
