// libxde_hip.so — the vector field of a neural CDE dz = F(t, z) dX(t) (include/xde_hip_cde.h):
//
//   xde_cde_contract            out[b, h]   = sum_c F[b, h, c] * dX[b, c]
//   xde_cde_contract_backward   gF[b, h, c] = gout[b, h] * dX[b, c]
//
//   xde_cde_contract_natural / _backward   the same two on the natural cubic spline (Y, M) of include/xde_hip_spline.h: dX from four rows
//
// dX[b, :] is the time derivative of the control spline through series[b] at the launch's time: the `der` of xde_history_gather for
// one query, from the same device functions (xde_spline_device.hpp), kept in LDS / registers and never written out.  F (or gF) is the
// only large operand and crosses HBM once, in 16-byte vectors; as framework ops this was a spline launch (value AND derivative
// written), a batched [H, C] x [C] product and, on the way back, a broadcast multiply over a materialised dX.
//
// One work item = one batch row b (or, when B alone cannot fill the chip, one slice of its H rows; or, when H is short and B large,
// a few consecutive batch rows that fill one pass of the workgroup): the workgroup builds dX[b, :] once and walks h.  A (b, h) row belongs to a TEAM of R lanes (R = min(64, pow2ceil(ceil(C / W))), a function of C and the dtype only);
// the summation order inside a team is the header's, whatever the grid, the slicing or the alignment.

#include "xde_hip_cde.h"
#include "xde_hip_spline.h"

#include "xde_common.hpp"
#include "xde_control_host.hpp"
#include "xde_spline_device.hpp"

using namespace xde;

namespace {

constexpr int kCdeMaxC = 2048;  // channels of dX[b, :] a workgroup keeps in LDS (16 KiB of fp64); a longer row is recomputed per use
constexpr int kCdeRows = 4;     // rows of F a team has in flight (independent 16-byte loads per lane)

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

// s_dx[g C + c] <- dX[b0 + g, c], g < nb  (between two barriers: the previous item's readers are done, this item's readers see it);
// `sb` = series[b0], `mb` = coef[b0]
template <typename T, bool NAT>
__device__ __forceinline__ void cde_fill_dx(T* s_dx, const CdeTab<T, NAT>& tb, int method, const T* __restrict__ sb, const T* __restrict__ mb,
                                            int nb, int C, int Tn, bool first) {
  if (!first) __syncthreads();
  if (nb == 1) {
    for (int c = threadIdx.x; c < C; c += kBlock) s_dx[c] = cde_dx<T, NAT>(tb, method, sb, mb, c, C, Tn);
  } else {
    for (int e = threadIdx.x; e < nb * C; e += kBlock) {
      const int g = e / C;
      s_dx[e] = cde_dx<T, NAT>(tb, method, sb + int64_t(g) * Tn * C, mb + int64_t(g) * Tn * C, e - g * C, C, Tn);
    }
  }
  __syncthreads();
}

// work item -> its first batch row b0, its batch rows nb and its rows [r0, r1) counted from row b0 * H of F (rows of consecutive batch
// rows are contiguous): a slice of one batch row's H rows (S > 1), or Gb whole batch rows (S == 1)
struct CdeItem {
  int64_t b0;
  int nb, r0, r1;
};
__device__ __forceinline__ CdeItem cde_item(const CdeArgs& a, int64_t it) {
  CdeItem w;
  if (a.S > 1) {
    w.b0 = it / a.S;
    const int part = int(it - w.b0 * a.S);
    w.nb = 1;
    w.r0 = part * a.Hc;
    w.r1 = a.H - w.r0 < a.Hc ? a.H : w.r0 + a.Hc;
  } else {
    w.b0 = it * a.Gb;
    w.nb = a.B - w.b0 < a.Gb ? int(a.B - w.b0) : a.Gb;
    w.r0 = 0;
    w.r1 = w.nb * a.H;
  }
  return w;
}

// vector q of the row that starts at element `at` of F: W elements (those past C are not loaded and not used)
template <typename T, bool VEC>
__device__ __forceinline__ void cde_load(T* x, const T* __restrict__ F, int64_t at, int q, int C, bool nt) {
  constexpr int W = VecOf<T>::W;
  if (VEC) {
    using P = Pack<T, true>;
    const P p = load_sel<P>(F, at / W + q, nt);  // (C % W == 0: every row starts on a vector)
#pragma unroll
    for (int k = 0; k < W; ++k) x[k] = p.v[k];
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int c = q * W + k;
      x[k] = c < C ? F[at + c] : T(0);
    }
  }
}

template <typename T, bool VEC, bool LDSDX, bool GRP, bool NAT>
__global__ __launch_bounds__(kBlock) void xde_cde_contract_kernel(CdeArgs a) {
  constexpr int W = VecOf<T>::W;
  constexpr int U = kCdeRows;
  __shared__ CdeTab<T, NAT> tb;
  __shared__ T s_dx[LDSDX ? kCdeMaxC : 1];
  if (threadIdx.x == 0) cde_make_tab<T, NAT>(&tb, a);
  __syncthreads();
  const T* __restrict__ F = static_cast<const T*>(a.in);
  const T* __restrict__ series = static_cast<const T*>(a.series);
  const T* __restrict__ coef = static_cast<const T*>(a.coef);
  T* __restrict__ out = static_cast<T*>(a.out);
  const int C = a.C, H = a.H, Tn = a.Tn, R = a.R, method = a.method;
  const int NV = (C + W - 1) / W;
  const int j = threadIdx.x & (R - 1), team = threadIdx.x >> a.r_log, TPB = kBlock >> a.r_log;
  const bool nt = a.nt != 0;
  const bool single = NV <= R;  // a lane holds at most one vector of a row: the common case (C <= 64 W)
  const int64_t items = a.S > 1 ? a.B * a.S : (a.B + a.Gb - 1) / a.Gb;
  bool first = true;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x, first = false) {
    const CdeItem w = cde_item(a, it);
    const int r1 = w.r1;
    const T* __restrict__ sb = series + w.b0 * int64_t(Tn) * C;
    const T* __restrict__ mb = NAT ? coef + w.b0 * int64_t(Tn) * C : sb;
    const int64_t row0 = w.b0 * H;
    if (single) {
      // the first rows of F are requested BEFORE dX is built: they do not depend on it
      T x[U][W];
      auto load_rows = [&](int rb) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int r = rb + u * TPB + team;
          if (r < r1 && j < NV) cde_load<T, VEC>(x[u], F, (row0 + r) * C, j, C, nt);
        }
      };
      load_rows(w.r0);
      if (LDSDX) cde_fill_dx<T, NAT>(s_dx, tb, method, sb, mb, GRP ? w.nb : 1, C, Tn, first);
      // this lane's channels of dX, per row slot (slots of a grouped item may sit in different batch rows; a grouped item is one pass)
      T dx[U][W];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int r = w.r0 + u * TPB + team;
        const int g = (GRP && r < r1) ? r / H : 0;  // (GRP: the launch groups batch rows, Gb > 1)
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const int c = j * W + k;
          dx[u][k] = c < C ? (LDSDX ? s_dx[g * C + c] : cde_dx<T, NAT>(tb, method, sb + int64_t(g) * Tn * C, mb + int64_t(g) * Tn * C, c, C, Tn)) : T(0);
        }
      }
      for (int rb = w.r0;;) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int r = rb + u * TPB + team;
          T v = T(0);
          if (r < r1 && j < NV) {
#pragma unroll
            for (int k = 0; k < W; ++k)
              if (VEC || j * W + k < C) v = v + x[u][k] * dx[u][k];
          }
          for (int off = R >> 1; off > 0; off >>= 1) v = v + __shfl_down(v, off, R);
          if (j == 0 && r < r1) out[row0 + r] = v;
        }
        rb += U * TPB;
        if (rb >= r1) break;
        load_rows(rb);
      }
    } else {
      // (rows longer than a team's reach are not grouped: nb == 1)
      if (LDSDX) cde_fill_dx<T, NAT>(s_dx, tb, method, sb, mb, 1, C, Tn, first);
      for (int rb = w.r0; rb < r1; rb += TPB) {
        const int r = rb + team;
        T v = T(0);
        if (r < r1) {
          for (int q = j; q < NV; q += R) {
            T x[W];
            cde_load<T, VEC>(x, F, (row0 + r) * C, q, C, nt);
#pragma unroll
            for (int k = 0; k < W; ++k) {
              const int c = q * W + k;
              if (VEC || c < C) v = v + x[k] * (LDSDX ? s_dx[c] : cde_dx<T, NAT>(tb, method, sb, mb, c, C, Tn));
            }
          }
        }
        for (int off = R >> 1; off > 0; off >>= 1) v = v + __shfl_down(v, off, R);
        if (j == 0 && r < r1) out[row0 + r] = v;
      }
    }
  }
}

template <typename T, bool VEC, bool LDSDX, bool GRP, bool NAT>
__global__ __launch_bounds__(kBlock) void xde_cde_backward_kernel(CdeArgs a) {
  using P = Pack<T, VEC>;
  constexpr int W = P::W;
  __shared__ CdeTab<T, NAT> tb;
  __shared__ T s_dx[LDSDX ? kCdeMaxC : 1];
  if (threadIdx.x == 0) cde_make_tab<T, NAT>(&tb, a);
  __syncthreads();
  const T* __restrict__ gout = static_cast<const T*>(a.in);
  const T* __restrict__ series = static_cast<const T*>(a.series);
  const T* __restrict__ coef = static_cast<const T*>(a.coef);
  T* __restrict__ gF = static_cast<T*>(a.out);
  const int C = a.C, H = a.H, Tn = a.Tn, method = a.method;
  const int per = C / W;  // vectors (VEC: C % W == 0) or elements (W == 1) of a row
  // lanes that share one row; a longer row is walked in strides of them
  const int row_lanes = per < kBlock ? per : kBlock;
  const int rows_per_pass = kBlock / row_lanes;
  const int my_row = threadIdx.x / row_lanes, q0 = threadIdx.x % row_lanes;
  const int64_t items = a.S > 1 ? a.B * a.S : (a.B + a.Gb - 1) / a.Gb;
  bool first = true;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x, first = false) {
    const CdeItem w = cde_item(a, it);
    const T* __restrict__ sb = series + w.b0 * int64_t(Tn) * C;
    const T* __restrict__ mb = NAT ? coef + w.b0 * int64_t(Tn) * C : sb;
    if (LDSDX) cde_fill_dx<T, NAT>(s_dx, tb, method, sb, mb, GRP ? w.nb : 1, C, Tn, first);
    if (my_row >= rows_per_pass) continue;  // (no barrier below this point of the item)
    for (int r = w.r0 + my_row; r < w.r1; r += rows_per_pass) {
      const int64_t row = w.b0 * H + r;
      const int g = GRP ? r / H : 0;
      const T gv = gout[row];
      for (int q = q0; q < per; q += row_lanes) {
        P o;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const int c = q * W + k;
          o.v[k] = gv * (LDSDX ? s_dx[g * C + c] : cde_dx<T, NAT>(tb, method, sb + int64_t(g) * Tn * C, mb + int64_t(g) * Tn * C, c, C, Tn));
        }
        o.store(gF, row * per + q);
      }
    }
  }
}

// slices of H per batch row: one (a workgroup reads series[b] once) unless B alone leaves most of the chip idle
void cde_slices(xde_cde_plan_t* p, int64_t B, int H, int C, int64_t rows_per_pass, int64_t full_pass) {
  constexpr int64_t kWant = 1024;  // work items that fill the chip
  int64_t S = (kWant + B - 1) / B;
  const int64_t most = (int64_t(H) + rows_per_pass - 1) / rows_per_pass;  // a slice is at least one pass of the workgroup
  if (S > most) S = most;
  if (S < 1) S = 1;
  p->Hc = int((int64_t(H) + S - 1) / S);
  p->S = (H + p->Hc - 1) / p->Hc;
  // batch rows per item: where a batch row's H rows leave most of the workgroup's pass idle, consecutive batch rows share an item (more
  // independent loads in flight per workgroup, fewer barriers) — as long as their dX rows fit the LDS table and the chip stays full
  p->Gb = 1;
  if (p->S == 1 && p->lds) {
    int64_t G = full_pass / H;
    if (G > kCdeMaxC / C) G = kCdeMaxC / C;
    if (G > B / kWant) G = B / kWant;
    if (G > 1) p->Gb = int(G);
  }
}

// everything the host decides about a launch, from the direction, the sizes, the dtype and the big operand's alignment: the ONE
// statement of it — the launchers run what it returns, xde_cde_plan reports it
xde_cde_plan_t cde_plan(bool backward, const void* big, int64_t B, int H, int C, int dtype) {
  const int width = vec_width(dtype);
  xde_cde_plan_t p;
  memset(&p, 0, sizeof(p));
  p.vec = (C % width) == 0 && aligned16(big);
  p.lds = C <= kCdeMaxC;
  if (!backward) {
    const int NV = (C + width - 1) / width;
    p.R = NV < 64 ? pow2ceil(NV) : 64;
    p.single = NV <= p.R;
    const int TPB = kBlock / p.R;  // row teams of a workgroup
    p.rows_per_pass = p.single ? kCdeRows * TPB : TPB;
    cde_slices(&p, B, H, C, TPB, p.single ? int64_t(kCdeRows) * TPB : 0);
    p.nt = big_operand(B * int64_t(H) * C, dtype) ? 1 : 0;
  } else {
    p.R = 1;
    const int per = p.vec ? C / width : C;
    p.rows_per_pass = per < kBlock ? kBlock / per : 1;
    cde_slices(&p, B, H, C, p.rows_per_pass, per < kBlock ? int64_t(kCdeRows) * p.rows_per_pass : 0);
  }
  p.grouped = p.Gb > 1;
  p.items = p.S > 1 ? B * p.S : (B + p.Gb - 1) / p.Gb;
  p.blocks = p.items > grid_cap() ? grid_cap() : p.items;
  return p;
}

void cde_args(CdeArgs* a, const xde_cde_plan_t& p, void* out, const void* in, const void* series, const void* coef, const void* knots,
              const TimedCall& c) {
  memset(a, 0, sizeof(*a));
  a->out = out, a->in = in, a->series = series, a->coef = coef, a->knots = knots, a->t_dev = c.t_dev, a->t_host = c.t_host;
  a->B = c.B, a->H = c.H, a->C = c.C, a->Tn = c.Tn, a->method = c.method, a->time_f64 = c.time_dtype == XDE_F64;
  a->R = p.R;
  for (a->r_log = 0; (1 << a->r_log) < a->R; ++a->r_log) {}
  a->S = p.S, a->Hc = p.Hc, a->Gb = p.Gb, a->lds = p.lds, a->nt = p.nt;
}

// the one launcher of both directions and every control: the arguments have passed check_timed (`coef`: M of the natural control,
// method kMethodNatural; else `series` again, never read)
int cde_launch(bool backward, void* out, const void* in, const void* series, const void* coef, const void* knots, const TimedCall& c) {
  const xde_cde_plan_t p = cde_plan(backward, backward ? out : in, c.B, c.H, c.C, c.dtype);
  CdeArgs a;
  cde_args(&a, p, out, in, series, coef, knots, c);
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  const bool natural = c.method == kMethodNatural;
  const double rows = natural ? 4.0 : 3.0;  // control rows read per batch row
  ProfScope prof(XDE_KID_DENSE, (double(c.B) * c.H * c.C + double(c.B) * c.H + rows * double(c.B) * c.C) * elem_size(c.dtype));
  dim3 g(static_cast<unsigned>(p.blocks)), blk(kBlock);
  with_flag(!backward, [&](auto forward) {
    with_dtype(c.dtype, [&](auto ty) {
      using T = typename decltype(ty)::type;
      with_flag(natural, [&](auto nat) {
        with_flag(p.vec != 0, [&](auto vec) {
          auto launch = [&](auto ldsdx, auto grp) {
            constexpr bool VEC = decltype(vec)::value, LDSDX = decltype(ldsdx)::value, GRP = decltype(grp)::value;
            constexpr bool NAT = decltype(nat)::value;
            if constexpr (decltype(forward)::value) XDE_LAUNCH((xde_cde_contract_kernel<T, VEC, LDSDX, GRP, NAT>), g, blk, st, prof, a);
            else XDE_LAUNCH((xde_cde_backward_kernel<T, VEC, LDSDX, GRP, NAT>), g, blk, st, prof, a);
          };
          // (a launch that groups batch rows keeps their dX rows in LDS: GRP implies LDSDX, so <LDSDX = false, GRP = true> does not exist)
          if (p.grouped) launch(std::true_type{}, std::true_type{});
          else if (p.lds) launch(std::true_type{}, std::false_type{});
          else launch(std::false_type{}, std::false_type{});
        });
      });
    });
  });
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // namespace

extern "C" {

int xde_cde_contract(void* out, const void* F, const void* series, const void* knots, const void* t_dev, double t_host, int time_dtype,
                     int64_t B, int H, int C, int Tn, int method, int dtype, void* stream) {
  const TimedCall c{t_dev, t_host, time_dtype, B, H, C, Tn, method, dtype, stream};
  if (int rc = check_timed(ArgCheck{"xde_cde_contract"}.public_method(method), {out, F, series, knots}, c)) return rc;
  return cde_launch(false, out, F, series, series, knots, c);
}

int xde_cde_contract_backward(void* gF, const void* gout, const void* series, const void* knots, const void* t_dev, double t_host,
                              int time_dtype, int64_t B, int H, int C, int Tn, int method, int dtype, void* stream) {
  const TimedCall c{t_dev, t_host, time_dtype, B, H, C, Tn, method, dtype, stream};
  if (int rc = check_timed(ArgCheck{"xde_cde_contract_backward"}.public_method(method), {gF, gout, series, knots}, c)) return rc;
  return cde_launch(true, gF, gout, series, series, knots, c);
}

int xde_cde_contract_natural(void* out, const void* F, const void* Y, const void* M, const void* knots, const void* t_dev, double t_host,
                             int time_dtype, int64_t B, int H, int C, int Tn, int dtype, void* stream) {
  const TimedCall c{t_dev, t_host, time_dtype, B, H, C, Tn, kMethodNatural, dtype, stream};
  if (int rc = check_timed({"xde_cde_contract_natural"}, {out, F, Y, M, knots}, c)) return rc;
  return cde_launch(false, out, F, Y, M, knots, c);
}

int xde_cde_contract_natural_backward(void* gF, const void* gout, const void* Y, const void* M, const void* knots, const void* t_dev,
                                      double t_host, int time_dtype, int64_t B, int H, int C, int Tn, int dtype, void* stream) {
  const TimedCall c{t_dev, t_host, time_dtype, B, H, C, Tn, kMethodNatural, dtype, stream};
  if (int rc = check_timed({"xde_cde_contract_natural_backward"}, {gF, gout, Y, M, knots}, c)) return rc;
  return cde_launch(true, gF, gout, Y, M, knots, c);
}

int xde_cde_plan(int backward, const void* big, int64_t B, int H, int C, int dtype, xde_cde_plan_t* plan) {
  if (int rc = ArgCheck{"xde_cde_plan"}.not_null({plan}).sizes("B, H, C", {B, H, C}).dtype(dtype).aligned({big}, dtype).rc) return rc;
  *plan = cde_plan(backward != 0, big, B, H, C, dtype);
  return XDE_OK;
}

}  // extern "C"
