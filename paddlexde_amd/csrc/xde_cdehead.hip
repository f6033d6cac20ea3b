// libxde_hip.so — the last layer of a neural CDE's field fused into the contraction with the control's derivative
// (include/xde_hip_cdehead.h):
//
//   xde_cdehead_forward    out[b, h] = sum_c act(sum_k a[b, k] W[h C + c, k] + bias[h C + c]) * dX[b, c]
//   xde_cdehead_backward   s[b, n]   = gout[b, h] * dX[b, c] * act'(pre[b, n])
//
// F = act(pre) [B, H, C] exists only as accumulator tiles: the pre-activations are produced by v_mfma_f32_32x32x2_f32, the activation
// is applied in registers, the product with dX[b, c] (built on chip by the contraction's own device functions, xde_cde_device.hpp)
// goes through an LDS tile and is summed over c.  fp32 matrix peak equals fp32 vector peak on this part: the matrix cores are used so
// that the VALU is free for tanhf and the epilogue while the products run, and so that F never crosses HBM — not for a higher flop rate.
//
// OPERAND PLACEMENT.  Rows n = h C + c of W sit on the instruction's M axis, batch rows on its N axis: lane l of a wave supplies
// A = W[n0 + l % 32][k], B = a[b0 + l % 32][k] with k from the half l / 32 of the row, and receives D[i][l % 32] for the 16 rows
// i = 8 (r / 4) + 4 (l / 32) + r % 4, r = 0..15 — 16 pre-activations of ITS batch row.  The sum over k is order-free between the two
// operands, so lane half 0 takes k in [0, KH) and lane half 1 takes [KH, K) (KH = 4 ceil(K / 8)), each contiguous in memory: 16-byte
// loads, no LDS for the product.  The a tile [32 x K] stays in registers (K / 2 per lane, the cap on K) for the walk over n; W is read
// per batch tile from L2.
//
// WORK.  One item = 32 batch rows x one slice of whole rows h (slices only where B alone cannot fill the chip).  The four waves of the
// workgroup take consecutive chunks of 32 n: a PASS is 128 n.  Forward: every wave writes its 32 x 32 products p = act(pre) * dX to
// an LDS tile; after one barrier, thread (b, slot) adds the runs of c of the rows h = first + slot, first + slot + 8, ... that the
// pass holds, sequentially in ascending c; a run that the pass cuts leaves its running sum in s_carry[b] and is taken up by the next
// pass.  Tiles and carries are double buffered: one barrier per pass.  out[b, h] is written once, by one thread; no atomics.
// Backward: no LDS tile and no barrier after the dX tile — each lane stores its 16 values of s (16-byte stores where aligned).
//
// The accumulation order that can be stated is in the header; the order inside one matrix instruction cannot.

#include "xde_hip_cdehead.h"

#include "xde_cde_device.hpp"
#include "xde_common.hpp"
#include "xde_control_host.hpp"
#include "xde_spline_device.hpp"

using namespace xde;

namespace {

constexpr int kHeadTile = 32;                   // batch rows of an item = rows of W of a chunk: the instruction is 32 x 32
constexpr int kHeadPass = kHeadTile * kWaves;   // rows of W between two barriers
constexpr int kHeadMaxC = 192;                  // channels of the dX tile [C][32] in LDS (24 KiB); a longer row is evaluated per use
constexpr int kHeadSlots = kBlock / kHeadTile;  // rows h summed side by side in the forward's reduction
static_assert(int64_t(XDE_CDEHEAD_MAX_HC) + kHeadPass <= int64_t(INT32_MAX), "the pass walk must stay inside an int");
constexpr int kHeadQB = 4;                      // 16-byte vectors of a W row requested ahead of the instructions that use them

typedef float v16f_t __attribute__((ext_vector_type(16)));

struct HeadArgs {
  CdeArgs ctl;  // the control, the time and B, H, C, Tn, method as the contraction takes them (its out / in and plan fields unused)
  void* out;    // out[B, H] | s[B, H C]
  const float* gout;
  const float* a;
  const float* W;
  const float* bias;
  int K, KH, kq;
  int S, Hc;
  int act;
  int avec, wvec, svec;  // 16-byte access of a, W, s
  int lds;               // the dX tile is in LDS
};

// four consecutive k of one row from `at` (k0 = the first one's index): those at or past `kend` — and all of a null row — are +0
__device__ __forceinline__ void head_load4(float* x, const float* __restrict__ row, int k0, int kend, bool vec) {
  if (row && vec && k0 < kend) {  // (vec: K % 4 == 0, KH % 4 == 0, the operand 16-byte aligned — the vector is inside the half)
    const v4f_t v = *reinterpret_cast<const v4f_t*>(row + k0);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = (row && k0 + j < kend) ? row[k0 + j] : 0.0f;
  }
}

// the 32 x 32 pre-activation tile (without bias) of the rows `wrow` (this lane's row of W, null past the slice) against the batch tile in
// `ar`: lane half's k from `k0` to `kend`, ascending, kq vectors; the next kHeadQB vectors of W are requested before the current ones are used
template <int KQ>
__device__ __forceinline__ v16f_t head_tile(const float (&ar)[4 * KQ], const float* __restrict__ wrow, int k0, int kend, bool wvec, int kq) {
  constexpr int QB = KQ < kHeadQB ? KQ : kHeadQB;
  v16f_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float cur[QB][4], nxt[QB][4];
#pragma unroll
  for (int u = 0; u < QB; ++u) head_load4(cur[u], wrow, k0 + 4 * u, kend, wvec);
#pragma unroll
  for (int qb = 0; qb < KQ; qb += QB) {
    if (qb + QB < KQ) {
#pragma unroll
      for (int u = 0; u < QB; ++u) head_load4(nxt[u], wrow, k0 + 4 * (qb + QB + u), kend, wvec);
    }
#pragma unroll
    for (int u = 0; u < QB; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[u][j], ar[4 * (qb + u) + j], acc, 0, 0, 0);
    }
    if (qb + QB >= kq) break;  // (uniform: the vectors past kq are all +0)
    if (qb + QB < KQ) {
#pragma unroll
      for (int u = 0; u < QB; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[u][j] = nxt[u][j];
    }
  }
  return acc;
}

template <int KQ, bool NAT, bool BWD>
__global__ __launch_bounds__(kBlock) void xde_cdehead_kernel(HeadArgs a) {
  __shared__ CdeTab<float, NAT> tb;
  __shared__ float s_dx[kHeadMaxC * kHeadTile];                  // [c][b]
  __shared__ float s_tile[BWD ? 1 : 2 * kHeadPass * kHeadTile];  // [parity][n - pass start][b]
  __shared__ float s_carry[BWD ? 1 : 2 * kHeadTile];             // [parity][b]
  if (threadIdx.x == 0) cde_make_tab<float, NAT>(&tb, a.ctl);
  __syncthreads();
  const float* __restrict__ series = static_cast<const float*>(a.ctl.series);
  const float* __restrict__ coef = static_cast<const float*>(a.ctl.coef);
  const int C = a.ctl.C, H = a.ctl.H, Tn = a.ctl.Tn, method = a.ctl.method, K = a.K;
  const int64_t B = a.ctl.B, HC = int64_t(H) * C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, bl = lane & 31;
  const int k0 = half ? a.KH : 0, kend = half ? K : (a.KH < K ? a.KH : K);
  const bool lds = a.lds != 0, tanh_act = a.act == XDE_CDEHEAD_ACT_TANH;
  const int64_t items = ((B + kHeadTile - 1) / kHeadTile) * a.S;
  int parity = 0;
  bool first = true;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x, first = false) {
    const int64_t bt = it / a.S;
    const int part = int(it - bt * a.S);
    const int64_t b0 = bt * kHeadTile;
    const int h0 = part * a.Hc, h1 = H - h0 < a.Hc ? H : h0 + a.Hc;
    const int ns = h0 * C, ne = h1 * C;  // (H C <= XDE_CDEHEAD_MAX_HC, checked on the host: every n the walk forms is below ne + kHeadPass, an int)
    const bool brow = b0 + bl < B;       // this lane's batch row exists
    const float* __restrict__ sb = series + (b0 + bl) * int64_t(Tn) * C;
    const float* __restrict__ mb = NAT ? coef + (b0 + bl) * int64_t(Tn) * C : sb;

    // this lane's half of its row of a, for the whole item (a missing row is +0: its results are never stored)
    float ar[4 * KQ];
    {
      const float* arow = brow ? a.a + (b0 + bl) * int64_t(K) : nullptr;
#pragma unroll
      for (int q = 0; q < KQ; ++q) head_load4(ar + 4 * q, arow, k0 + 4 * q, kend, a.avec != 0);
    }
    // the dX tile (between two barriers: the previous item's readers are done, this item's readers see it)
    if (lds) {
      if (!first) __syncthreads();
      for (int e = threadIdx.x; e < kHeadTile * C; e += kBlock) {
        const int g = e / C, c = e - g * C;
        float v = 0.0f;
        if (b0 + g < B) {
          const float* __restrict__ sg = series + (b0 + g) * int64_t(Tn) * C;
          v = cde_dx<float, NAT>(tb, method, sg, NAT ? coef + (b0 + g) * int64_t(Tn) * C : sg, c, C, Tn);
        }
        s_dx[c * kHeadTile + g] = v;
      }
      __syncthreads();
    }
    auto dx_of = [&](int c) -> float {
      if (lds) return s_dx[c * kHeadTile + bl];
      return brow ? cde_dx<float, NAT>(tb, method, sb, mb, c, C, Tn) : 0.0f;
    };

    for (int p0 = ns; p0 < ne; p0 += kHeadPass) {
      const int nc0 = p0 + wave * kHeadTile;  // this wave's chunk (wave-uniform)
      if (nc0 < ne) {
        const int nrow = nc0 + bl;
        const v16f_t acc = head_tile<KQ>(ar, nrow < ne ? a.W + int64_t(nrow) * K : nullptr, k0, kend, a.wvec != 0, a.kq);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ng = nc0 + 8 * g + 4 * half;  // this lane's rows ng .. ng + 3
          if (ng >= ne) continue;
          int h = ng / C, c = ng - h * C;
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int n = ng + j;
            v[j] = 0.0f;
            if (n < ne) {
              const float pre = a.bias ? acc[4 * g + j] + a.bias[n] : acc[4 * g + j];
              const float y = tanh_act ? tanhf(pre) : pre;
              const float dx = dx_of(c);
              if constexpr (BWD) {
                const float gd = (brow ? a.gout[(b0 + bl) * int64_t(H) + h] : 0.0f) * dx;
                v[j] = tanh_act ? gd * (1.0f - y * y) : gd;
              } else {
                v[j] = y * dx;
              }
            }
            if (++c == C) c = 0, ++h;
          }
          if constexpr (BWD) {
            if (brow) {
              float* __restrict__ srow = static_cast<float*>(a.out) + (b0 + bl) * HC;
              if (a.svec && (ng & 3) == 0 && ng + 3 < ne) {
                v4f_t o;
                o.x = v[0], o.y = v[1], o.z = v[2], o.w = v[3];
                *reinterpret_cast<v4f_t*>(srow + ng) = o;
              } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  if (ng + j < ne) srow[ng + j] = v[j];
              }
            }
          } else {
            float* __restrict__ tile = s_tile + parity * (kHeadPass * kHeadTile);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (ng + j < ne) tile[(ng + j - p0) * kHeadTile + bl] = v[j];
          }
        }
      }
      if constexpr (!BWD) {
        __syncthreads();
        // the runs of c this pass holds, [p0, p1): thread (b, slot) takes rows h = hf + slot, hf + slot + kHeadSlots, ...
        const float* __restrict__ tile = s_tile + parity * (kHeadPass * kHeadTile);
        const int p1 = ne - p0 < kHeadPass ? ne : p0 + kHeadPass;
        const int b = threadIdx.x & (kHeadTile - 1), slot = threadIdx.x / kHeadTile;
        const int hf = p0 / C, hl = (p1 - 1) / C;
        for (int h = hf + slot; h <= hl; h += kHeadSlots) {
          const int r0 = h * C, r1 = r0 + C;
          const int lo = r0 > p0 ? r0 : p0, hi = r1 < p1 ? r1 : p1;
          float v = lo > r0 ? s_carry[(parity ^ 1) * kHeadTile + b] : 0.0f;
          for (int n = lo; n < hi; ++n) v = v + tile[(n - p0) * kHeadTile + b];
          if (hi < r1) s_carry[parity * kHeadTile + b] = v;  // (only the pass's last row can be cut at its end)
          else if (b0 + b < B) static_cast<float*>(a.out)[(b0 + b) * int64_t(H) + h] = v;
        }
        parity ^= 1;
      }
    }
  }
}

// everything the host decides about a launch from the sizes, the dtype and the activation: the launcher runs what it returns,
// xde_cdehead_plan reports it
xde_cdehead_plan_t head_plan(int64_t B, int H, int C, int K, int dtype, int act) {
  xde_cdehead_plan_t p;
  memset(&p, 0, sizeof(p));
  p.k_cap = XDE_CDEHEAD_MAX_K;
  p.served = dtype == XDE_F32 && K <= XDE_CDEHEAD_MAX_K && (act == XDE_CDEHEAD_ACT_IDENTITY || act == XDE_CDEHEAD_ACT_TANH);
  p.tile_b = kHeadTile, p.tile_n = kHeadTile, p.pass_n = kHeadPass;
  p.kq = int((int64_t(K) + 7) / 8);
  p.kh = 4 * p.kq;
  p.kq_regs = pow2ceil(p.kq < 32 ? p.kq : 32);
  const int64_t tiles = (B + kHeadTile - 1) / kHeadTile;
  // slices of H per batch tile: one unless the batch tiles alone leave most of the chip idle; a slice is whole rows h, so that no run
  // of c is ever split between workgroups
  constexpr int64_t kWant = 1024;
  int64_t S = (kWant + tiles - 1) / tiles;
  if (S > H) S = H;
  p.Hc = int((int64_t(H) + S - 1) / S);
  p.S = (H + p.Hc - 1) / p.Hc;
  p.lds_dx = C <= kHeadMaxC;
  p.lds_bytes = int(sizeof(float)) * (kHeadMaxC * kHeadTile + 2 * kHeadPass * kHeadTile + 2 * kHeadTile) +
                int(sizeof(CdeTab<float, false>) > sizeof(CdeTab<float, true>) ? sizeof(CdeTab<float, false>) : sizeof(CdeTab<float, true>));  // (the larger table)
  p.items = tiles * p.S;
  p.blocks = p.items > grid_cap() ? grid_cap() : p.items;
  return p;
}

struct HeadCall {
  const void *a, *W, *bias, *series, *coef, *knots;
  int K, act;
};

int head_check(ArgCheck no, Ptrs required, const HeadCall& o, const TimedCall& c) {
  no.not_null(required).sizes("B, H, C, K", {c.B, c.H, c.C, o.K});
  // (the kernel walks n = h C + c in int, a pass of kHeadPass at a time: the last pass may step that far past H C)
  if (!no.rc && int64_t(c.H) * c.C > int64_t(XDE_CDEHEAD_MAX_HC)) no.refuse(": bad sizes (need H * C <= 2^31 - 256)");
  no.knots(c.Tn).dtype(c.dtype).time_dtype(c.time_dtype).control_method(c.method);
  if (!no.rc && o.act != XDE_CDEHEAD_ACT_IDENTITY && o.act != XDE_CDEHEAD_ACT_TANH) no.refuse(": unknown act");
  if (!no.rc && c.dtype != XDE_F32) no.refuse(": not served: the fused head is fp32 only (take the unfused route)");
  if (!no.rc && o.K > XDE_CDEHEAD_MAX_K)
    no.refuse(": not served: K = " + std::to_string(o.K) + " is beyond XDE_CDEHEAD_MAX_K = " + std::to_string(XDE_CDEHEAD_MAX_K));
  return no.aligned(required, c.dtype).aligned({o.bias, o.coef}, c.dtype).time_aligned(c.t_dev, c.time_dtype).rc;
}

// the one launcher of both directions and every control: `big` = out | s, `gout` null for the forward
int head_launch(bool backward, void* big, const void* gout, const HeadCall& o, const TimedCall& c) {
  const xde_cdehead_plan_t p = head_plan(c.B, c.H, c.C, o.K, c.dtype, o.act);
  const bool natural = c.method == kMethodNatural;
  HeadArgs h;
  memset(&h, 0, sizeof(h));
  h.ctl.series = o.series, h.ctl.coef = natural ? o.coef : o.series, h.ctl.knots = o.knots, h.ctl.t_dev = c.t_dev, h.ctl.t_host = c.t_host;
  h.ctl.B = c.B, h.ctl.H = c.H, h.ctl.C = c.C, h.ctl.Tn = c.Tn, h.ctl.method = c.method, h.ctl.time_f64 = c.time_dtype == XDE_F64;
  h.out = big, h.gout = static_cast<const float*>(gout), h.a = static_cast<const float*>(o.a), h.W = static_cast<const float*>(o.W);
  h.bias = static_cast<const float*>(o.bias);
  h.K = o.K, h.KH = p.kh, h.kq = p.kq, h.S = p.S, h.Hc = p.Hc, h.act = o.act, h.lds = p.lds_dx;
  h.avec = (o.K % 4) == 0 && aligned16(o.a);
  h.wvec = (o.K % 4) == 0 && aligned16(o.W);
  h.svec = backward && ((int64_t(c.H) * c.C) % 4) == 0 && aligned16(big);
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  const double rows = natural ? 4.0 : 3.0;  // control rows read per batch row
  const double hc = double(c.H) * c.C, tiles = double((c.B + kHeadTile - 1) / kHeadTile);
  // a, the control rows and out (or gout and s) once; W once per batch tile (from L2)
  ProfScope prof(XDE_KID_DENSE, (double(c.B) * o.K + rows * double(c.B) * c.C + double(c.B) * c.H + tiles * hc * o.K + (backward ? double(c.B) * hc : 0.0)) * 4.0);
  dim3 g(static_cast<unsigned>(p.blocks)), blk(kBlock);
  auto with_kq = [&](auto&& fn) {
    switch (p.kq_regs) {
      case 1: fn(std::integral_constant<int, 1>{}); break;
      case 2: fn(std::integral_constant<int, 2>{}); break;
      case 4: fn(std::integral_constant<int, 4>{}); break;
      case 8: fn(std::integral_constant<int, 8>{}); break;
      case 16: fn(std::integral_constant<int, 16>{}); break;
      default: fn(std::integral_constant<int, 32>{}); break;
    }
  };
  with_kq([&](auto kq) {
    with_flag(natural, [&](auto nat) {
      with_flag(backward, [&](auto bwd) {
        XDE_LAUNCH((xde_cdehead_kernel<decltype(kq)::value, decltype(nat)::value, decltype(bwd)::value>), g, blk, st, prof, h);
      });
    });
  });
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // namespace

extern "C" {

int xde_cdehead_forward(void* out, const void* a, const void* W, const void* bias, const void* series, const void* coef, const void* knots,
                        const void* t_dev, double t_host, int time_dtype, int64_t B, int H, int C, int K, int Tn, int method, int act,
                        int dtype, void* stream) {
  ArgCheck no{"xde_cdehead_forward"};
  if (!coef) no.public_method(method);
  const TimedCall c{t_dev, t_host, time_dtype, B, H, C, Tn, coef ? kMethodNatural : method, dtype, stream};
  const HeadCall o{a, W, bias, series, coef, knots, K, act};
  if (int rc = head_check(no, {out, a, W, series, knots}, o, c)) return rc;
  return head_launch(false, out, nullptr, o, c);
}

int xde_cdehead_backward(void* s, const void* gout, const void* a, const void* W, const void* bias, const void* series, const void* coef,
                         const void* knots, const void* t_dev, double t_host, int time_dtype, int64_t B, int H, int C, int K, int Tn,
                         int method, int act, int dtype, void* stream) {
  ArgCheck no{"xde_cdehead_backward"};
  if (!coef) no.public_method(method);
  const TimedCall c{t_dev, t_host, time_dtype, B, H, C, Tn, coef ? kMethodNatural : method, dtype, stream};
  const HeadCall o{a, W, bias, series, coef, knots, K, act};
  if (int rc = head_check(no, {s, gout, a, W, series, knots}, o, c)) return rc;
  return head_launch(true, s, gout, o, c);
}

int xde_cdehead_plan(int64_t B, int H, int C, int K, int dtype, int act, xde_cdehead_plan_t* plan) {
  if (int rc = ArgCheck{"xde_cdehead_plan"}.not_null({plan}).sizes("B, H, C, K", {B, H, C, K}).dtype(dtype).rc) return rc;
  *plan = head_plan(B, H, C, K, dtype, act);
  return XDE_OK;
}

}  // extern "C"
