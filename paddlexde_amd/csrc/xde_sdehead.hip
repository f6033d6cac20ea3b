// libxde_hip.so — the last layer of an SDE's matrix diffusion fused into the Euler-Maruyama step (include/xde_hip_sdehead.h):
//
//   xde_sdehead_step       y1[r, d]  = (y0 + f dt)[r, d] + sum_m act(sum_k a[r, k] W[d M + m, k] + bias[d M + m]) * w[r, m]
//   xde_sdehead_backward   s[r, n]   = (gy1[r, d] * w[r, m]) * act'(pre[r, n]),  gf = gy1 dt
//
// g = act(pre) [rows, D, M] exists only as accumulator tiles: the pre-activations are produced by v_mfma_f32_32x32x2_f32, the activation
// is applied in registers, the product with the increment w[r, m] = s Z[r M + m] (generated on chip by the generator of the general
// noise kernels, xde_sde_device.hpp: the same bits) goes through an LDS tile and is summed over m, and the thread that finishes (r, d)
// reads y0 and f and writes y1.
//
// OPERAND PLACEMENT.  Rows n = d M + m of W sit on the instruction's M axis, state rows on its N axis: lane l of a wave supplies
// A = W[n0 + l % 32][k], B = a[r0 + l % 32][k] with k from the half l / 32 of the row, and receives D[i][l % 32] for the 16 rows
// i = 8 (q / 4) + 4 (l / 32) + q % 4, q = 0..15 — 16 pre-activations of ITS state row.  Lane half 0 takes k in [0, KH) and lane half 1
// [KH, K) (KH = 4 ceil(K / 8)), each contiguous in memory: 16-byte loads, no LDS for the product.
//
// TWO TILES PER WAVE.  W is read per work item from L2, and with one 32-row tile per item every 16-byte load of W feeds four
// instructions.  Here a wave keeps TWO tiles of a in registers (rows r0 .. r0 + 31 and r0 + 32 .. r0 + 63: K / 2 registers per lane and
// tile) and issues the two tiles' instructions on each W value back to back: eight instructions per load, two independent accumulator
// chains, half the L2 traffic per flop.  That is K registers per lane for a, so it is done where K <= 128; beyond (to the cap 256) a wave
// holds one tile.  The chain of one (r, n) is the same instructions in the same order in both plans.
//
// WORK.  One item = 32 TILES state rows x one slice of whole d (slices only where the rows alone cannot fill the chip).  The four waves
// of the workgroup take consecutive chunks of 32 n: a PASS is 128 n.  The increments of the item's rows are the contiguous flat span
// [r0 M, (r0 + 32 TILES) M), which starts on a Philox block (r0 % 4 == 0): one block per lane and round, scaled by s, into LDS as
// [m][row] — once per item.  Beyond kSdeHeadMaxM the span does not fit and a lane generates the block of each increment it needs.
//
// FORWARD.  Every wave writes its 32 x 32 TILES products p = act(pre) * w to an LDS tile [row][n - pass start] (row stride 129: the
// writers of a chunk, consecutive rows, fall on consecutive banks).  After ONE barrier the outputs (r, d) the pass touches are dealt to
// the threads d fastest — consecutive lanes take consecutive d of a row, then the next row — so that the three state arrays y0, f and
// y1 are met in runs of consecutive addresses (with one slice, D <= a pass and M small, whole rows back to back).  A thread adds its run
// of m sequentially in ascending m; a run that the pass cuts leaves its running sum in s_carry[row] and is taken up by the next pass
// (a run longer than a pass goes through the carry more than once).  Tiles and carries are double buffered: one barrier per pass.
// y1[r, d] is written once, by the thread that finished the run; no atomics.
// BACKWARD.  No LDS tile and no barrier after the increments: each lane stores its 4-groups of s (16-byte stores where aligned); gf is
// written by the threads that own (r, d) in the same d-fastest order.
//
// The accumulation order that can be stated is in the header; the order inside one matrix instruction cannot.

#include "xde_hip_sdehead.h"

#include "xde_common.hpp"
#include "xde_control_host.hpp"
#include "xde_sde_device.hpp"

using namespace xde;

namespace {

constexpr int kSdeHeadTile = 32;                     // state rows of a tile = rows of W of a chunk: the instruction is 32 x 32
constexpr int kSdeHeadPass = kSdeHeadTile * kWaves;  // rows of W between two barriers
constexpr int kSdeHeadStride = kSdeHeadPass + 1;     // floats between two rows of the product tile (odd: see above)
constexpr int kSdeHeadMaxM = 48;                     // M up to which the increments [M][64] are kept in LDS (12 KiB)
constexpr int kSdeHeadQB = 4;                        // 16-byte vectors of a W row requested ahead of the instructions that use them
constexpr int64_t kSdeHeadWant = 1024;               // work items wanted before D is left unsliced
static_assert(int64_t(XDE_SDEHEAD_MAX_DM) + kSdeHeadPass <= int64_t(INT32_MAX), "the pass walk must stay inside an int");
static_assert(XDE_SDEHEAD_PAIR_K * 2 == XDE_SDEHEAD_MAX_K, "two tiles at the pair cap cost the registers of one at the cap");

typedef float v16f_t __attribute__((ext_vector_type(16)));

struct SdeHeadArgs {
  float* big;        // y1[rows, D] | s[rows, D M]
  float* gf;         // backward, or null
  const float* y0;   // forward | gy1
  const float* f;    // forward
  const float* a;
  const float* W;
  const float* bias;
  int64_t rows;
  int D, M, K, KH, kq;
  int S, Dc;
  int act;
  int avec, wvec, svec;  // 16-byte access of a, W, s
  int lds;               // the increments are in LDS
  float dt, s;
  uint32_t key0, key1, k;
};

// four consecutive k of one row from `at` (k0 = the first one's index): those at or past `kend` — and all of a null row — are +0
__device__ __forceinline__ void sdehead_load4(float* x, const float* __restrict__ row, int k0, int kend, bool vec) {
  if (row && vec && k0 < kend) {  // (vec: K % 4 == 0, KH % 4 == 0, the operand 16-byte aligned — the vector is inside the half)
    const v4f_t v = *reinterpret_cast<const v4f_t*>(row + k0);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = (row && k0 + j < kend) ? row[k0 + j] : 0.0f;
  }
}

// the 32 x 32 pre-activation tiles (without bias) of the rows `wrow` (this lane's row of W, null past the slice) against the TILES state
// tiles in `ar`: lane half's k from `k0` to `kend`, ascending, kq vectors.  Each W value meets every tile before the next one is taken;
// the next kSdeHeadQB vectors of W are requested before the current ones are used.
template <int KQ, int TILES>
__device__ __forceinline__ void sdehead_tiles(v16f_t (&acc)[TILES], const float (&ar)[TILES][4 * KQ], const float* __restrict__ wrow, int k0,
                                              int kend, bool wvec, int kq) {
  constexpr int QB = KQ < kSdeHeadQB ? KQ : kSdeHeadQB;
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
  float cur[QB][4], nxt[QB][4];
#pragma unroll
  for (int u = 0; u < QB; ++u) sdehead_load4(cur[u], wrow, k0 + 4 * u, kend, wvec);
#pragma unroll
  for (int qb = 0; qb < KQ; qb += QB) {
    if (qb + QB < KQ) {
#pragma unroll
      for (int u = 0; u < QB; ++u) sdehead_load4(nxt[u], wrow, k0 + 4 * (qb + QB + u), kend, wvec);
    }
#pragma unroll
    for (int u = 0; u < QB; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int t = 0; t < TILES; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[u][j], ar[t][4 * (qb + u) + j], acc[t], 0, 0, 0);
      }
    }
    if (qb + QB >= kq) break;  // (uniform: the vectors past kq are all +0)
    if (qb + QB < KQ) {
#pragma unroll
      for (int u = 0; u < QB; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[u][j] = nxt[u][j];
    }
  }
}

template <int KQ, int TILES, bool BWD>
__global__ __launch_bounds__(kBlock) void xde_sdehead_kernel(SdeHeadArgs a) {
  constexpr int ROWS = kSdeHeadTile * TILES;
  __shared__ float s_w[kSdeHeadMaxM * ROWS];                 // [m][row]
  __shared__ float s_tile[BWD ? 1 : 2 * ROWS * kSdeHeadStride];  // [parity][row][n - pass start]
  __shared__ float s_carry[BWD ? 1 : 2 * ROWS];              // [parity][row]
  const int D = a.D, M = a.M, K = a.K;
  const int64_t rows = a.rows, DM = int64_t(D) * M;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, bl = lane & 31;
  const int k0 = half ? a.KH : 0, kend = half ? K : (a.KH < K ? a.KH : K);
  const bool lds = a.lds != 0, tanh_act = a.act == XDE_SDEHEAD_ACT_TANH;
  const float s = a.s, dt = a.dt;
  const int64_t items = ((rows + ROWS - 1) / ROWS) * a.S;
  int parity = 0;
  bool first = true;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x, first = false) {  // (workgroup-uniform: every barrier below is reached by all)
    const int64_t rt = it / a.S;
    const int part = int(it - rt * a.S);
    const int64_t r0 = rt * ROWS;
    const int nrows = rows - r0 < ROWS ? int(rows - r0) : ROWS;  // rows of the item that exist
    const int d0 = part * a.Dc, d1 = D - d0 < a.Dc ? D : d0 + a.Dc;
    const int ns = d0 * M, ne = d1 * M;  // (D M <= XDE_SDEHEAD_MAX_DM, checked on the host: every n the walk forms is below ne + kSdeHeadPass, an int)

    // this lane's half of its rows of a, one per tile, for the whole item (a missing row is +0: its results are never stored)
    float ar[TILES][4 * KQ];
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      const int rl = t * kSdeHeadTile + bl;
      const float* arow = rl < nrows ? a.a + (r0 + rl) * int64_t(K) : nullptr;
#pragma unroll
      for (int q = 0; q < KQ; ++q) sdehead_load4(ar[t] + 4 * q, arow, k0 + 4 * q, kend, a.avec != 0);
    }
    // the increments of the item's rows (between two barriers: the previous item's readers are done, this item's readers see them).
    // The span starts at element r0 M, a multiple of 4: block b of the span is Philox block r0 M / 4 + b, and only the array's last
    // block is cut.
    if (lds) {
      if (!first) __syncthreads();
      const int len = nrows * M;
      const uint64_t j0 = uint64_t(r0) * uint64_t(M) / 4u;
      for (int b = threadIdx.x; 4 * b < len; b += kBlock) {
        float z[4];
        normals(j0 + uint64_t(b), a.k, a.key0, a.key1, 0u, z);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int e = 4 * b + v;
          if (e < len) {
            const int rl = e / M;
            s_w[(e - rl * M) * ROWS + rl] = s * z[v];
          }
        }
      }
      __syncthreads();
    }
    // w[r0 + rl, m]; without the LDS span, from the block that holds element (r0 + rl) M + m (kept while the next m stays inside it)
    uint64_t jc = ~uint64_t(0);
    float zc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    auto w_of = [&](int rl, int m) -> float {
      if (lds) return s_w[m * ROWS + rl];
      if (rl >= nrows) return 0.0f;
      const uint64_t e = uint64_t(r0 + rl) * uint64_t(M) + uint64_t(m);
      if ((e >> 2) != jc) {
        jc = e >> 2;
        normals(jc, a.k, a.key0, a.key1, 0u, zc);
      }
      const int v = int(e & 3u);
      return s * (v == 0 ? zc[0] : v == 1 ? zc[1] : v == 2 ? zc[2] : zc[3]);
    };

    for (int p0 = ns; p0 < ne; p0 += kSdeHeadPass) {
      const int nc0 = p0 + wave * kSdeHeadTile;  // this wave's chunk (wave-uniform)
      if (nc0 < ne) {
        const int nrow = nc0 + bl;
        v16f_t acc[TILES];
        sdehead_tiles<KQ, TILES>(acc, ar, nrow < ne ? a.W + int64_t(nrow) * K : nullptr, k0, kend, a.wvec != 0, a.kq);
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
          const int rl = t * kSdeHeadTile + bl;
          const bool brow = rl < nrows;  // this lane's state row of the tile exists
          if constexpr (BWD) {
            if (!lds && !brow) continue;  // (nothing to store, and no generator to run for it)
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int ng = nc0 + 8 * g + 4 * half;  // this lane's rows ng .. ng + 3
            if (ng >= ne) continue;
            int d = ng / M, m = ng - d * M;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int n = ng + j;
              v[j] = 0.0f;
              if (n < ne) {
                const float pre = a.bias ? acc[t][4 * g + j] + a.bias[n] : acc[t][4 * g + j];
                const float y = tanh_act ? tanhf(pre) : pre;
                const float w = w_of(rl, m);
                if constexpr (BWD) {
                  const float gw = (brow ? a.y0[(r0 + rl) * int64_t(D) + d] : 0.0f) * w;
                  v[j] = tanh_act ? gw * (1.0f - y * y) : gw;
                } else {
                  v[j] = y * w;
                }
              }
              if (++m == M) m = 0, ++d;
            }
            if constexpr (BWD) {
              if (brow) {
                float* __restrict__ srow = a.big + (r0 + rl) * DM;
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
              float* __restrict__ trow = s_tile + parity * (ROWS * kSdeHeadStride) + rl * kSdeHeadStride + (ng - p0);
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (ng + j < ne) trow[j] = v[j];
            }
          }
        }
      }
      if constexpr (!BWD) {
        __syncthreads();
        // the runs of m this pass holds, [p0, p1): output q = rl * nd + (d - df) goes to thread q % kBlock — d fastest
        const float* __restrict__ tile = s_tile + parity * (ROWS * kSdeHeadStride);
        const int p1 = ne - p0 < kSdeHeadPass ? ne : p0 + kSdeHeadPass;
        const int df = p0 / M, dl = (p1 - 1) / M, nd = dl - df + 1;
        for (int q = threadIdx.x; q < nrows * nd; q += kBlock) {
          const int rl = q / nd, d = df + (q - rl * nd);
          const int n0 = d * M, n1 = n0 + M;
          const int lo = n0 > p0 ? n0 : p0, hi = n1 < p1 ? n1 : p1;
          const float* __restrict__ trow = tile + rl * kSdeHeadStride - p0;
          float v;
          int n = lo;
          if (lo > n0) v = s_carry[(parity ^ 1) * ROWS + rl];
          else v = trow[n++];  // (the sum starts from the first product, not from +0)
          for (; n < hi; ++n) v = v + trow[n];
          if (hi < n1) {
            s_carry[parity * ROWS + rl] = v;  // (only the pass's last d can be cut at its end)
          } else {
            const int64_t o = (r0 + rl) * int64_t(D) + d;
            a.big[o] = (a.y0[o] + a.f[o] * dt) + v;
          }
        }
        parity ^= 1;
      }
    }
    if constexpr (BWD) {
      if (a.gf) {
        const int nd = d1 - d0;
        for (int64_t q = threadIdx.x; q < int64_t(nrows) * nd; q += kBlock) {
          const int rl = int(q / nd), d = d0 + int(q - int64_t(rl) * nd);
          const int64_t o = (r0 + rl) * int64_t(D) + d;
          a.gf[o] = a.y0[o] * dt;
        }
      }
    }
  }
}

constexpr int sdehead_lds_bytes(int tiles) {
  return int(sizeof(float)) * (kSdeHeadMaxM + 2 * kSdeHeadStride + 2) * kSdeHeadTile * tiles;
}

// everything the host decides about a launch from the sizes, the dtype and the activation: the launcher runs what it returns,
// xde_sdehead_plan reports it
xde_sdehead_plan_t sdehead_plan(int64_t rows, int D, int M, int K, int dtype, int act) {
  xde_sdehead_plan_t p;
  memset(&p, 0, sizeof(p));
  p.k_cap = XDE_SDEHEAD_MAX_K;
  p.served = dtype == XDE_F32 && K <= XDE_SDEHEAD_MAX_K && (act == XDE_SDEHEAD_ACT_IDENTITY || act == XDE_SDEHEAD_ACT_TANH);
  p.tiles = K <= XDE_SDEHEAD_PAIR_K ? 2 : 1;
  p.tile_r = kSdeHeadTile * p.tiles, p.tile_n = kSdeHeadTile, p.pass_n = kSdeHeadPass;
  p.kq = int((int64_t(K) + 7) / 8);
  p.kh = 4 * p.kq;
  p.kq_regs = p.kq <= 2 ? 2 : p.kq <= 8 ? 8 : p.kq <= 16 ? 16 : 32;
  const int64_t tiles = (rows + p.tile_r - 1) / p.tile_r;
  // slices of D per row tile: one unless the row tiles alone leave most of the chip idle; a slice is whole d, so that no run of m is
  // ever split between workgroups, and at least a chunk of n where D has that many
  int64_t S = (kSdeHeadWant + tiles - 1) / tiles;
  const int64_t dmin = (kSdeHeadTile + int64_t(M) - 1) / M;
  if (S > D / dmin) S = D / dmin;
  if (S < 1) S = 1;
  p.Dc = int((int64_t(D) + S - 1) / S);
  p.S = (D + p.Dc - 1) / p.Dc;
  p.lds_w = M <= kSdeHeadMaxM;
  p.lds_bytes = sdehead_lds_bytes(p.tiles);
  p.items = tiles * p.S;
  p.blocks = p.items > grid_cap() ? grid_cap() : p.items;
  return p;
}

struct SdeHeadCall {
  const void *a, *W, *bias;
  int64_t rows;
  int D, M, K, act;
  double dt, s;
  uint64_t seed;
  int64_t k;
  int dtype;
  void* stream;
};

int sdehead_check(ArgCheck no, Ptrs required, Ptrs optional, const SdeHeadCall& c) {
  no.not_null(required).sizes("rows, D, M, K", {c.rows, c.D, c.M, c.K});
  // (the kernel walks n = d M + m in int, a pass of kSdeHeadPass at a time: the last pass may step that far past D M)
  if (!no.rc && int64_t(c.D) * c.M > int64_t(XDE_SDEHEAD_MAX_DM)) no.refuse(": bad sizes (need D * M <= 2^31 - 256)");
  if (!no.rc && (c.k < 0 || c.k > int64_t(0xffffffffLL))) no.refuse(": k out of range (0 <= k < 2^32)");
  no.dtype(c.dtype);
  if (!no.rc && c.act != XDE_SDEHEAD_ACT_IDENTITY && c.act != XDE_SDEHEAD_ACT_TANH) no.refuse(": unknown act");
  if (!no.rc && c.dtype != XDE_F32) no.refuse(": not served: the fused head is fp32 only (take the unfused route)");
  if (!no.rc && c.K > XDE_SDEHEAD_MAX_K)
    no.refuse(": not served: K = " + std::to_string(c.K) + " is beyond XDE_SDEHEAD_MAX_K = " + std::to_string(XDE_SDEHEAD_MAX_K));
  return no.aligned(required, c.dtype).aligned(optional, c.dtype).rc;
}

// the one launcher of both directions: `big` = y1 | s, `src` = y0 | gy1, `f` the drift (forward), `gf` its cotangent (backward, or null)
int sdehead_launch(bool backward, void* big, void* gf, const void* src, const void* f, const SdeHeadCall& c) {
  const xde_sdehead_plan_t p = sdehead_plan(c.rows, c.D, c.M, c.K, c.dtype, c.act);
  SdeHeadArgs h;
  memset(&h, 0, sizeof(h));
  h.big = static_cast<float*>(big), h.gf = static_cast<float*>(gf), h.y0 = static_cast<const float*>(src), h.f = static_cast<const float*>(f);
  h.a = static_cast<const float*>(c.a), h.W = static_cast<const float*>(c.W), h.bias = static_cast<const float*>(c.bias);
  h.rows = c.rows, h.D = c.D, h.M = c.M, h.K = c.K, h.KH = p.kh, h.kq = p.kq, h.S = p.S, h.Dc = p.Dc, h.act = c.act, h.lds = p.lds_w;
  h.avec = (c.K % 4) == 0 && aligned16(c.a);
  h.wvec = (c.K % 4) == 0 && aligned16(c.W);
  h.svec = backward && ((int64_t(c.D) * c.M) % 4) == 0 && aligned16(big);
  h.dt = float(c.dt), h.s = float(c.s);
  h.key0 = uint32_t(c.seed), h.key1 = uint32_t(c.seed >> 32), h.k = uint32_t(c.k);
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  const double n = double(c.rows) * c.D, dm = double(c.D) * c.M, tiles = double((c.rows + p.tile_r - 1) / p.tile_r);
  // a once per slice; y0, f and y1 (or gy1, gf and s) once; W once per row tile (from L2)
  ProfScope prof(backward ? XDE_KID_COMBINE : XDE_KID_COMBINE_FUSE,
                 (double(c.rows) * c.K * p.S + tiles * dm * c.K + (backward ? (gf ? 2.0 : 1.0) * n + double(c.rows) * dm : 3.0 * n)) * 4.0);
  dim3 g(static_cast<unsigned>(p.blocks)), blk(kBlock);
  auto with_kq = [&](auto&& fn) {  // (the two-tile instantiations end at the pair cap: kq_regs 32 is the one-tile plan)
    switch (p.kq_regs) {
      case 2: fn(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{}); break;
      case 8: fn(std::integral_constant<int, 8>{}, std::integral_constant<int, 2>{}); break;
      case 16: fn(std::integral_constant<int, 16>{}, std::integral_constant<int, 2>{}); break;
      default: fn(std::integral_constant<int, 32>{}, std::integral_constant<int, 1>{}); break;
    }
  };
  with_kq([&](auto kq, auto tiles_c) {
    with_flag(backward, [&](auto bwd) {
      XDE_LAUNCH((xde_sdehead_kernel<decltype(kq)::value, decltype(tiles_c)::value, decltype(bwd)::value>), g, blk, st, prof, h);
    });
  });
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // namespace

extern "C" {

int xde_sdehead_step(void* y1, const void* y0, const void* f, const void* a, const void* W, const void* bias, int64_t rows, int D, int M,
                     int K, int act, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  const SdeHeadCall c{a, W, bias, rows, D, M, K, act, dt, s, seed, k, dtype, stream};
  if (int rc = sdehead_check(ArgCheck{"xde_sdehead_step"}, {y1, y0, f, a, W}, {bias}, c)) return rc;
  return sdehead_launch(false, y1, nullptr, y0, f, c);
}

int xde_sdehead_backward(void* s_out, void* gf, const void* gy1, const void* a, const void* W, const void* bias, int64_t rows, int D, int M,
                         int K, int act, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  const SdeHeadCall c{a, W, bias, rows, D, M, K, act, dt, s, seed, k, dtype, stream};
  if (int rc = sdehead_check(ArgCheck{"xde_sdehead_backward"}, {s_out, gy1, a, W}, {bias, gf}, c)) return rc;
  return sdehead_launch(true, s_out, gf, gy1, nullptr, c);
}

int xde_sdehead_plan(int64_t rows, int D, int M, int K, int dtype, int act, xde_sdehead_plan_t* plan) {
  if (int rc = ArgCheck{"xde_sdehead_plan"}.not_null({plan}).sizes("rows, D, M, K", {rows, D, M, K}).dtype(dtype).rc) return rc;
  *plan = sdehead_plan(rows, D, M, K, dtype, act);
  return XDE_OK;
}

}  // extern "C"
