// libxde_hip.so — the gradient of cdeint with respect to its control path (include/xde_hip_cdegrad.h):
//
//   xde_cde_control_grad / _natural           gdX[b, c] = sum_h gout[b, h] * F[b, h, c], scattered to the rows X'(t) was built from
//   xde_spline_natural_coeffs_backward        the transpose of xde_spline_natural_coeffs (once per backward pass)
//   xde_spline_natural_gather_backward        the transpose of xde_spline_natural_gather
//
// (a) One workgroup = one batch row b at a time.  Its 256 lanes are P x CL: P partial sums over h (a function of H alone, so the
// summation order is), CL lanes along c that hold W consecutive channels each; a row longer than CL * W is walked in chunks.  A chunk's
// partials meet in LDS (the header's tree), and its gdX is written out at once to all Tn rows — weight times gdX on the rows X'(t)
// read, +0 elsewhere — so gdX needs no table, C has no limit, and the dense output is written exactly once with no memset.

#include "xde_hip_cdegrad.h"

#include "xde_common.hpp"
#include "xde_control_host.hpp"
#include "xde_spline_device.hpp"

using namespace xde;

namespace {

constexpr int kGradMaxP = 32;   // partial sums over h per channel
constexpr int kGradEntries = 6;  // (row, weight) entries of dX's transpose: 2 linear, 6 cubic, 2 + 2 natural
constexpr int kGatherTile = 128;  // query times per table of the gather's transpose

struct GradArgs {
  void* out0;  // gSeries | gY
  void* out1;  // gM (natural control), else null
  const void* gout;
  const void* F;
  const void* knots;
  const void* t_dev;
  double t_host;
  int64_t B;
  int H, C, Tn;
  int method;
  int time_f64;
  int P, p_log;
  int ovec;  // the outputs take 16-byte stores (vec, and they are 16-byte aligned too)
};

template <typename T>
struct GradTab {
  int n[2];                     // entries of out0, of out1
  int row[2][kGradEntries];
  T w[2][kGradEntries];
};

// the weights of the natural spline's `der` (header (a)) and `val` (header FOLD) with respect to Y_i, Y_{i+1}, M_i, M_{i+1}
template <typename T>
__device__ __forceinline__ void natural_der_weights(T h, T s, T* w) {
  const T rh = T(1) / h;
  const T q = (s * s) / (T(2) * h);
  w[0] = -rh;
  w[1] = rh;
  w[2] = (s - h / T(3)) - q;
  w[3] = q - h / T(6);
}
template <typename T>
__device__ __forceinline__ void natural_val_weights(T h, T s, T* w) {
  const T r = s / h;
  const T s2 = s * s, s3 = s2 * s;
  w[0] = T(1) - r;
  w[1] = r;
  w[2] = (-(s * h) / T(3) + s2 / T(2)) - s3 / (T(6) * h);
  w[3] = -(s * h) / T(6) + s3 / (T(6) * h);
}

// the launch's time -> the entries of dX's transpose (one thread per workgroup)
template <typename T, bool NAT>
__device__ __forceinline__ void grad_make_tab(GradTab<T>* tb, const GradArgs& a) {
  const T tau = T(launch_time(a.t_dev, a.time_f64, a.t_host));
  const T* ts = static_cast<const T*>(a.knots);
  const int Tn = a.Tn;
  tb->n[0] = tb->n[1] = 0;
  auto put = [&](int o, int row, T w) {
    tb->row[o][tb->n[o]] = row;
    tb->w[o][tb->n[o]] = w;
    ++tb->n[o];
  };
  if constexpr (NAT) {
    const NaturalLag<T> r = make_natural_lag<T>(ts, tau, Tn);
    T w[4];
    natural_der_weights<T>(r.h, r.s, w);
    put(0, r.i, w[0]);
    put(0, r.i + 1, w[1]);
    put(1, r.i, w[2]);
    put(1, r.i + 1, w[3]);
  } else if (a.method == XDE_HISTORY_LINEAR) {
    const RowsLag<T> r = make_lag<T, 2>(ts, tau, Tn);
    const RowsScale<T> sc = make_scales<T, 2>(ts, r.row[0], Tn);
    put(0, r.row[0], T(-1) / sc.sc[0]);
    put(0, r.row[1], T(1) / sc.sc[1]);
  } else {
    const HermiteLag<T> r = make_hermite_lag<T>(ts, tau, Tn);
    const int i = r.i, i1 = i + 1 < Tn ? i + 1 : Tn - 1;
    const T a0 = r.g0 / r.h1, a1 = r.g1 / r.h2, b0 = r.g2 / r.ha, b1 = r.g3 / r.hb;
    put(0, i, a0);
    put(0, i1, a1);
    if (r.mode == 0) {
      put(0, i1, b0), put(0, i, -b0), put(0, i + 2, b1), put(0, i1, -b1);
    } else if (r.mode == 1) {
      put(0, i1, b0), put(0, i, -b0), put(0, i1, b1), put(0, i, -b1);
    } else {
      put(0, i, b0), put(0, Tn - 2, -b0), put(0, i, b1), put(0, Tn - 2, -b1);
    }
  }
}

template <typename T>
__device__ __forceinline__ T grad_row_value(const GradTab<T>& tb, int o, int k, T g) {
  T v = T(0);
  const int n = tb.n[o];
  for (int j = 0; j < n; ++j)
    if (tb.row[o][j] == k) v = v + tb.w[o][j] * g;
  return v;
}

// all Tn rows of one chunk of channels: `per` vectors (OV: the outputs take 16-byte stores) or elements of a row, from `base` on;
// s_gdx holds the chunk's gdX
template <typename T, bool OV, bool NAT>
__device__ __forceinline__ void grad_write_chunk(const GradTab<T>& tb, const T* s_gdx, T* __restrict__ out0, T* __restrict__ out1,
                                                 int64_t base, int per, int Tn, int C) {
  using PV = Pack<T, OV>;
  for (int e = threadIdx.x; e < Tn * per; e += kBlock) {
    const int k = e / per, x = e - k * per;
    PV o0, o1;
#pragma unroll
    for (int m = 0; m < PV::W; ++m) {
      const T g = s_gdx[x * PV::W + m];
      o0.v[m] = grad_row_value<T>(tb, 0, k, g);
      if (NAT) o1.v[m] = grad_row_value<T>(tb, 1, k, g);
    }
    const int64_t at = (base + int64_t(k) * C) / PV::W + x;  // (OV: C % W == 0, so every row of the chunk starts on a vector)
    o0.store(out0, at);
    if (NAT) o1.store(out1, at);
  }
}

template <typename T, bool VEC, bool NAT>
__global__ __launch_bounds__(kBlock) void xde_cde_control_grad_kernel(GradArgs a) {
  constexpr int W = VecOf<T>::W;
  __shared__ GradTab<T> tb;
  __shared__ T s_part[kBlock * W];
  // (no barrier of its own: the table is read in phase 2 only, behind the barrier that ends the first chunk's tree — the other waves
  // request their rows of F while this lane walks the knots)
  if (threadIdx.x == 0) grad_make_tab<T, NAT>(&tb, a);
  const T* __restrict__ F = static_cast<const T*>(a.F);
  const T* __restrict__ gout = static_cast<const T*>(a.gout);
  T* __restrict__ out0 = static_cast<T*>(a.out0);
  T* __restrict__ out1 = static_cast<T*>(a.out1);
  const int C = a.C, H = a.H, Tn = a.Tn, P = a.P;
  const int CL = kBlock >> a.p_log;
  const int NV = (C + W - 1) / W;
  const int cl = threadIdx.x & (CL - 1), p = threadIdx.x / CL;
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    const T* __restrict__ gb = gout + b * H;
    for (int q0 = 0; q0 < NV; q0 += CL) {
      // phase 1: this lane's partial p of the channels q W .. q W + W - 1
      const int q = q0 + cl;
      T v[W];
#pragma unroll
      for (int k = 0; k < W; ++k) v[k] = T(0);
      if (q < NV) {
#pragma unroll 4
        for (int h = p; h < H; h += P) {
          const T g = gb[h];
          const int64_t at = (b * H + h) * int64_t(C);
          if (VEC) {
            const Pack<T, true> x = Pack<T, true>::load(F, at / W + q);  // (C % W == 0: every row starts on a vector)
#pragma unroll
            for (int k = 0; k < W; ++k) v[k] = v[k] + g * x.v[k];
          } else {
#pragma unroll
            for (int k = 0; k < W; ++k) {
              const int c = q * W + k;
              if (c < C) v[k] = v[k] + g * F[at + c];
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < W; ++k) s_part[threadIdx.x * W + k] = v[k];
      // the header's tree over the partials: lane (p, cl) sits CL lanes after (p - 1, cl)
      for (int off = P >> 1; off > 0; off >>= 1) {
        __syncthreads();
        if (p < off) {
#pragma unroll
          for (int k = 0; k < W; ++k) s_part[threadIdx.x * W + k] = s_part[threadIdx.x * W + k] + s_part[(threadIdx.x + off * CL) * W + k];
        }
      }
      __syncthreads();
      // phase 2: s_part[0 .. nv W) is gdX of this chunk's channels; all Tn rows of them are written here, once
      const int nv = NV - q0 < CL ? NV - q0 : CL;  // vectors of this chunk
      const int64_t base = b * int64_t(Tn) * C + int64_t(q0) * W;  // element (b, 0, q0 W)
      if (VEC && a.ovec) grad_write_chunk<T, true, NAT>(tb, s_part, out0, out1, base, nv, Tn, C);
      else grad_write_chunk<T, false, NAT>(tb, s_part, out0, out1, base, C - q0 * W < nv * W ? C - q0 * W : nv * W, Tn, C);
      __syncthreads();  // (the next chunk overwrites s_part)
    }
  }
}

// One lane = one column e = b C + c (header (b)).  ws0[k] holds cp_k and ws1[k] holds GY_k at the nodes; gS[k] holds dl_k until the
// descending sweep replaces it.
template <typename T>
__global__ __launch_bounds__(kBlock) void xde_natural_coeffs_backward_kernel(T* __restrict__ gS, const T* __restrict__ gY,
                                                                             const T* __restrict__ gM, const T* __restrict__ series,
                                                                             const T* __restrict__ ts, T* __restrict__ ws0,
                                                                             T* __restrict__ ws1, int64_t cols, int Tn, int C) {
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < cols; e += stride) {
    const int64_t b = e / C;
    const int64_t at = b * int64_t(Tn) * C + (e - b * C);  // element (b, 0, c); row k is C * k further
    const T* __restrict__ y = series + at;
    const T* __restrict__ gy = gY + at;
    const T* __restrict__ gm = gM + at;
    T* __restrict__ o = gS + at;
    T* __restrict__ cpw = ws0 + at;
    T* __restrict__ gyw = ws1 + at;
    int kf = 0;
    while (kf < Tn && y[int64_t(kf) * C] != y[int64_t(kf) * C]) ++kf;
    if (kf == Tn) {  // nothing observed
      for (int k = 0; k < Tn; ++k) o[int64_t(k) * C] = T(0);
      continue;
    }
    // 1. the fold and the forward elimination, lagging one node
    T ta = T(0), cpa = T(0), dla = T(0);
    bool have_a = false;
    int ki = 0, kl = kf;
    T ti = ts[0], accY = gy[0], accM = gm[0];
    for (int k = 1; k < Tn; ++k) {
      const T yk = y[int64_t(k) * C];
      const bool obs = yk == yk;
      if (obs) kl = k;
      if (!obs && k != Tn - 1) continue;
      const T tb = ts[k];
      T bY = gy[int64_t(k) * C], bM = gm[int64_t(k) * C];
      if (k - ki > 1) {
        const T h = tb - ti;
        for (int j = ki + 1; j < k; ++j) {
          T w[4];
          natural_val_weights<T>(h, ts[j] - ti, w);
          const T gyj = gy[int64_t(j) * C], gmj = gm[int64_t(j) * C];
          accY = accY + w[0] * gyj;
          bY = bY + w[1] * gyj;
          accM = (accM + w[2] * gyj) + w[0] * gmj;
          bM = (bM + w[3] * gyj) + w[1] * gmj;
        }
      }
      T cp = T(0), dl = T(0);
      if (have_a) {
        const T hl = ti - ta, hr = tb - ti;
        const T den = T(2) * (hl + hr) - hl * cpa;
        cp = hr / den;
        dl = (accM - hl * dla) / den;
      }
      cpw[int64_t(ki) * C] = cp;
      gyw[int64_t(ki) * C] = accY;
      o[int64_t(ki) * C] = dl;
      ta = ti, cpa = cp, dla = dl, have_a = true;
      ti = tb, ki = k, accY = bY, accM = bM;
    }
    gyw[int64_t(Tn - 1) * C] = accY;
    // 2. back substitution and the transposed right-hand side, lagging one node: node kb is final once the node below it has its lam
    T lamB = T(0), tb = ts[Tn - 1], uAbove = T(0);
    int kb = Tn - 1;
    bool have_above = false;
    for (int k = Tn - 2; k >= 0; --k) {
      const T yk = y[int64_t(k) * C];
      if (k != 0 && yk != yk) {
        o[int64_t(k) * C] = T(0);
        continue;
      }
      const T tk = ts[k];
      const T lam = k == 0 ? T(0) : o[int64_t(k) * C] - cpw[int64_t(k) * C] * lamB;
      const T u = (T(6) * (lam - lamB)) / (tb - tk);
      T G = gyw[int64_t(kb) * C] + u;
      if (have_above) G = G - uAbove;
      o[int64_t(kb) * C] = G;
      lamB = lam, tb = tk, kb = k, uAbove = u, have_above = true;
    }
    o[0] = gyw[0] - uAbove;
    // 3. the end rule
    if (kf > 0) {
      o[int64_t(kf) * C] = o[int64_t(kf) * C] + o[0];
      o[0] = T(0);
    }
    if (kl < Tn - 1) {
      o[int64_t(kl) * C] = o[int64_t(kl) * C] + o[int64_t(Tn - 1) * C];
      o[int64_t(Tn - 1) * C] = T(0);
    }
  }
}

template <typename T>
struct GatherGradLag {
  int i, pad;
  T wv[4], wd[4];  // weights of val / der with respect to Y_i, Y_{i+1}, M_i, M_{i+1}
};

// One lane = one column e = o D + d (header (c)); the queries are served in tiles of kGatherTile through an LDS table.
template <typename T>
__global__ __launch_bounds__(kBlock) void xde_natural_gather_backward_kernel(T* __restrict__ gY, T* __restrict__ gM,
                                                                             const T* __restrict__ gval, const T* __restrict__ gder,
                                                                             const T* __restrict__ ts, const T* __restrict__ tq,
                                                                             int64_t cols, int Tn, int D, int L) {
  __shared__ GatherGradLag<T> tab[kGatherTile];
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int l0 = 0; l0 < L; l0 += kGatherTile) {
    const int Lt = L - l0 < kGatherTile ? L - l0 : kGatherTile;
    if (l0) __syncthreads();  // (the previous tile's readers are done)
    for (int l = threadIdx.x; l < Lt; l += kBlock) {
      const NaturalLag<T> r = make_natural_lag<T>(ts, tq[l0 + l], Tn);
      tab[l].i = r.i;
      tab[l].pad = 0;
      natural_val_weights<T>(r.h, r.s, tab[l].wv);
      natural_der_weights<T>(r.h, r.s, tab[l].wd);
    }
    __syncthreads();
    for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < cols; e += stride) {
      const int64_t o = e / D;
      const int64_t d = e - o * D;
      const int64_t out_at = o * int64_t(Tn) * D + d;
      const int64_t in_at = (o * int64_t(L) + l0) * D + d;
      for (int k = 0; k < Tn; ++k) {
        T yv = T(0), mv = T(0);
        if (l0) yv = gY[out_at + int64_t(k) * D], mv = gM[out_at + int64_t(k) * D];
        for (int l = 0; l < Lt; ++l) {
          const int i = tab[l].i;
          if (i != k && i + 1 != k) continue;
          const int x = i == k ? 0 : 1;
          if (gval) {
            const T gv = gval[in_at + int64_t(l) * D];
            yv = yv + tab[l].wv[x] * gv;
            mv = mv + tab[l].wv[2 + x] * gv;
          }
          if (gder) {
            const T gd = gder[in_at + int64_t(l) * D];
            yv = yv + tab[l].wd[x] * gd;
            mv = mv + tab[l].wd[2 + x] * gd;
          }
        }
        gY[out_at + int64_t(k) * D] = yv;
        gM[out_at + int64_t(k) * D] = mv;
      }
    }
  }
}

// everything the host decides about a launch of (a): the ONE statement of it — the launcher runs it, the plan query reports it
xde_cdegrad_plan_t grad_plan(const void* F, int64_t B, int H, int C, int dtype) {
  const int width = vec_width(dtype);
  xde_cdegrad_plan_t p;
  memset(&p, 0, sizeof(p));
  p.vec = (C % width) == 0 && aligned16(F);
  p.P = H < kGradMaxP ? pow2ceil(H) : kGradMaxP;
  p.CL = kBlock / p.P;
  const int NV = (C + width - 1) / width;
  p.chunks = (NV + p.CL - 1) / p.CL;
  p.rows = (H + p.P - 1) / p.P;
  p.blocks = B > grid_cap() ? grid_cap() : B;
  p.strided = B > p.blocks;
  return p;
}

void grad_args(GradArgs* a, const xde_cdegrad_plan_t& p, void* out0, void* out1, const void* gout, const void* F, const void* knots,
               const TimedCall& c) {
  memset(a, 0, sizeof(*a));
  a->out0 = out0, a->out1 = out1, a->gout = gout, a->F = F, a->knots = knots, a->t_dev = c.t_dev, a->t_host = c.t_host;
  a->B = c.B, a->H = c.H, a->C = c.C, a->Tn = c.Tn, a->method = c.method, a->time_f64 = c.time_dtype == XDE_F64;
  a->P = p.P;
  for (a->p_log = 0; (1 << a->p_log) < a->P; ++a->p_log) {}
  a->ovec = p.vec && aligned16(out0) && aligned16(out1);
}

// the one launcher of both controls: the arguments have passed check_timed (`out1`: gM of the natural control, else null)
int grad_launch(void* out0, void* out1, const void* gout, const void* F, const void* knots, const TimedCall& c) {
  const xde_cdegrad_plan_t p = grad_plan(F, c.B, c.H, c.C, c.dtype);
  GradArgs a;
  grad_args(&a, p, out0, out1, gout, F, knots, c);
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  const bool natural = c.method == kMethodNatural;
  const double outs = natural ? 2.0 : 1.0;  // dense outputs written
  ProfScope prof(XDE_KID_DENSE, (double(c.B) * c.H * c.C + double(c.B) * c.H + outs * double(c.B) * c.Tn * c.C) * elem_size(c.dtype));
  dim3 g(static_cast<unsigned>(p.blocks)), blk(kBlock);
  with_dtype(c.dtype, [&](auto ty) {
    using T = typename decltype(ty)::type;
    with_flag(natural, [&](auto nat) {
      with_flag(p.vec != 0, [&](auto vec) {
        XDE_LAUNCH((xde_cde_control_grad_kernel<T, decltype(vec)::value, decltype(nat)::value>), g, blk, st, prof, a);
      });
    });
  });
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // namespace

extern "C" {

int xde_cde_control_grad(void* gSeries, const void* gout, const void* F, const void* knots, const void* t_dev, double t_host,
                         int time_dtype, int64_t B, int H, int C, int Tn, int method, int dtype, void* stream) {
  const TimedCall c{t_dev, t_host, time_dtype, B, H, C, Tn, method, dtype, stream};
  if (int rc = check_timed(ArgCheck{"xde_cde_control_grad"}.public_method(method), {gSeries, gout, F, knots}, c)) return rc;
  return grad_launch(gSeries, nullptr, gout, F, knots, c);
}

int xde_cde_control_grad_natural(void* gY, void* gM, const void* gout, const void* F, const void* knots, const void* t_dev, double t_host,
                                 int time_dtype, int64_t B, int H, int C, int Tn, int dtype, void* stream) {
  const TimedCall c{t_dev, t_host, time_dtype, B, H, C, Tn, kMethodNatural, dtype, stream};
  if (int rc = check_timed({"xde_cde_control_grad_natural"}, {gY, gM, gout, F, knots}, c)) return rc;
  return grad_launch(gY, gM, gout, F, knots, c);
}

int xde_cde_control_grad_plan(const void* F, int64_t B, int H, int C, int dtype, xde_cdegrad_plan_t* plan) {
  const int rc = ArgCheck{"xde_cde_control_grad_plan"}.not_null({plan}).sizes("B, H, C", {B, H, C}).dtype(dtype).aligned({F}, dtype).rc;
  if (rc) return rc;
  *plan = grad_plan(F, B, H, C, dtype);
  return XDE_OK;
}

int64_t xde_spline_natural_coeffs_backward_workspace_bytes(int64_t B, int Tn, int C, int dtype) {
  if (B < 1 || C < 1 || Tn < 2 || (dtype != XDE_F32 && dtype != XDE_F64)) return -1;
  return 2 * B * int64_t(Tn) * C * elem_size(dtype);
}

int xde_spline_natural_coeffs_backward(void* gSeries, const void* gY, const void* gM, const void* series, const void* knots,
                                       void* workspace, int64_t B, int Tn, int C, int dtype, void* stream) {
  const Ptrs operands = {gSeries, gY, gM, series, knots, workspace};
  if (int rc = check_rows({"xde_spline_natural_coeffs_backward"}, operands, {}, "B, C", {B, C}, Tn, dtype)) return rc;
  const int64_t cols = B * int64_t(C), n = cols * Tn;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_DENSE, 8.0 * double(n) * elem_size(dtype));
  dim3 g(grid_for(cols)), blk(kBlock);
  with_dtype(dtype, [&](auto ty) {
    using T = typename decltype(ty)::type;
    XDE_LAUNCH((xde_natural_coeffs_backward_kernel<T>), g, blk, st, prof, static_cast<T*>(gSeries), static_cast<const T*>(gY),
               static_cast<const T*>(gM), static_cast<const T*>(series), static_cast<const T*>(knots), static_cast<T*>(workspace),
               static_cast<T*>(workspace) + n, cols, Tn, C);
  });
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_spline_natural_gather_backward(void* gY, void* gM, const void* gval, const void* gder, const void* knots, const void* tq,
                                       int64_t outer, int Tn, int L, int D, int dtype, void* stream) {
  const ArgCheck no = ArgCheck{"xde_spline_natural_gather_backward"}.either(gval, gder);
  if (int rc = check_rows(no, {gY, gM, knots, tq}, {gval, gder}, "outer, L, D", {outer, L, D}, Tn, dtype)) return rc;
  const int64_t cols = outer * int64_t(D);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double cotangents = (gval ? 1.0 : 0.0) + (gder ? 1.0 : 0.0);
  ProfScope prof(XDE_KID_DENSE, (2.0 * double(cols) * Tn + cotangents * double(cols) * L) * elem_size(dtype));
  dim3 g(grid_for(cols)), blk(kBlock);
  with_dtype(dtype, [&](auto ty) {
    using T = typename decltype(ty)::type;
    XDE_LAUNCH((xde_natural_gather_backward_kernel<T>), g, blk, st, prof, static_cast<T*>(gY), static_cast<T*>(gM),
               static_cast<const T*>(gval), static_cast<const T*>(gder), static_cast<const T*>(knots), static_cast<const T*>(tq), cols,
               Tn, D, L);
  });
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"
