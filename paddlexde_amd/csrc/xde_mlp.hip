// libxde_hip.so — a neural ODE's whole vector field, a small multi-layer perceptron, as one launch (include/xde_hip_mlp.h):
//
//   xde_mlp_field   out = L_n(act(L_{n-1}(... act(L_1(x)) ...))),  L_l(h) = h W_l^T + bias_l  (+ t_r * the time column in L_1)
//
// The hidden activations exist only in LDS.  A solve of a neural ODE is launch-bound: every evaluation of the field costs two to three
// launches per layer when it is composed of library calls, and one here.
//
// WORK.  One item = 32 TILES consecutive state rows, TILES = 1 or 2 (the plan).  A workgroup of four waves takes items blockIdx.x,
// blockIdx.x + gridDim.x, ...  Per item: the rows of x are read once (16-byte loads where widths[0] % 4 == 0 and x is aligned) into LDS
// buffer 0; layer l reads buffer l % 2 and writes buffer (l + 1) % 2, the last layer writes out; one barrier per layer boundary.
//
// LDS.  Two buffers of kMlpBufFloats floats, each an activation matrix TRANSPOSED: h[k][row], ROWS = 32 TILES floats per k.  The lanes
// of a wave read 32 consecutive rows of one k (lane half 1: of another k): consecutive banks, no conflict, and the same for the
// writes of a finished chunk (a lane writes neuron n of ITS row).  Widths up to 256 with one tile and up to 128 with two fill a buffer
// exactly: 2 x 32 KiB.
//
// OPERAND PLACEMENT (that of the fused heads).  Neurons n on the instruction's M axis, state rows on its N axis: lane l of a wave
// supplies A = W[n0 + l % 32][k], B = h[k][l % 32] with k from the half l / 32 of the row, and receives D[i][l % 32] for the 16 neurons
// i = 8 (q / 4) + 4 (l / 32) + q % 4, q = 0..15 — 16 pre-activations of ITS state row.  Lane half 0 takes k in [0, KH) and lane half 1
// [KH, K) (KH = 4 ceil(K / 8)), each contiguous in a row of W: 16-byte loads, the next vector requested before the current one is
// used.  With two tiles every value of W meets both tiles' B operands back to back: two independent accumulator chains per load.  The
// chain of one (r, n) is the same instructions in the same order in both plans.
//
// The four waves take the chunks nc0 = 32 wave, 32 wave + 128, ... of a layer: the layers of a small field (50 neurons) occupy two
// waves, and a layer of 256 gives each wave two chunks.
//
// The accumulation order that can be stated is in the header; the order inside one matrix instruction cannot.

#include "xde_hip_mlp.h"

#include "xde_common.hpp"
#include "xde_control_host.hpp"

using namespace xde;

namespace {

constexpr int kMlpTile = 32;                                    // state rows of a tile = neurons of a chunk: the instruction is 32 x 32
constexpr int kMlpPass = kMlpTile * kWaves;                     // neurons the waves of a workgroup cover side by side
constexpr int kMlpBufFloats = XDE_MLP_MAX_WIDTH * kMlpTile;     // one activation buffer: [256][32] or [128][64]
constexpr int64_t kMlpPairTiles = 512;                          // single tiles beyond which two are paired: two workgroups on each of 256 CUs
static_assert(XDE_MLP_PAIR_WIDTH * 2 * kMlpTile == kMlpBufFloats, "two tiles at the pair width fill the buffer of one at the cap");
static_assert(2 * kMlpBufFloats * sizeof(float) <= 64 * 1024, "both buffers are static LDS");

typedef float v16f_t __attribute__((ext_vector_type(16)));

struct MlpArgs {
  float* out;
  const float* x;
  const float* t_rows;  // or null: t
  const float* W[XDE_MLP_MAX_LAYERS];
  const float* bias[XDE_MLP_MAX_LAYERS];  // null: none
  int32_t widths[XDE_MLP_MAX_LAYERS + 1];
  int32_t wvec[XDE_MLP_MAX_LAYERS];  // 16-byte loads of W_l
  int64_t rows;
  int n_layers, tanh_act, time, xvec, ovec;
  float t;
};

// four consecutive k of one row of W from k0: those at or past `kend` — and all of a null row — are +0
__device__ __forceinline__ void mlp_load4(float* w, const float* __restrict__ row, int k0, int kend, bool vec) {
  if (row && vec && k0 < kend) {  // (vec: K % 4 == 0, KH % 4 == 0, the row stride % 4 == 0, W 16-byte aligned — the vector is inside the half)
    const v4f_t v = *reinterpret_cast<const v4f_t*>(row + k0);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (row && k0 + j < kend) ? row[k0 + j] : 0.0f;
  }
}

template <int TILES>
__global__ __launch_bounds__(kBlock) void xde_mlp_kernel(MlpArgs a) {
  constexpr int ROWS = kMlpTile * TILES;
  __shared__ float s_act[2][kMlpBufFloats];  // [parity][k][row]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, bl = lane & 31;
  const int64_t rows = a.rows, items = (rows + ROWS - 1) / ROWS;
  const int L = a.n_layers, K0 = a.widths[0], NL = a.widths[L];
  bool first = true;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x, first = false) {  // (workgroup-uniform: every barrier below is reached by all)
    const int64_t r0 = it * ROWS;
    const int nrows = rows - r0 < ROWS ? int(rows - r0) : ROWS;  // rows of the item that exist
    if (!first) __syncthreads();  // the previous item's last layer has read buffer (L - 1) % 2, which may be buffer 0

    // x -> buffer 0, transposed; a missing row is +0 (its results are never stored).  Consecutive threads take consecutive addresses.
    if (a.xvec) {
      const int kv = K0 >> 2;
      for (int e = threadIdx.x; e < ROWS * kv; e += kBlock) {
        const int rl = e / kv, k = 4 * (e - rl * kv);
        v4f_t v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (rl < nrows) v = *reinterpret_cast<const v4f_t*>(a.x + (r0 + rl) * int64_t(K0) + k);
        s_act[0][(k + 0) * ROWS + rl] = v.x, s_act[0][(k + 1) * ROWS + rl] = v.y;
        s_act[0][(k + 2) * ROWS + rl] = v.z, s_act[0][(k + 3) * ROWS + rl] = v.w;
      }
    } else {
      for (int e = threadIdx.x; e < ROWS * K0; e += kBlock) {
        const int rl = e / K0, k = e - rl * K0;
        s_act[0][k * ROWS + rl] = rl < nrows ? a.x[(r0 + rl) * int64_t(K0) + k] : 0.0f;
      }
    }
    // this lane's time, one per tile
    float tr[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      const int rl = t * kMlpTile + bl;
      tr[t] = !a.time ? 0.0f : !a.t_rows ? a.t : rl < nrows ? a.t_rows[r0 + rl] : 0.0f;
    }
    __syncthreads();

#pragma unroll 1
    for (int l = 0; l < L; ++l) {
      const int K = a.widths[l], N = a.widths[l + 1];
      const bool last = l == L - 1, timed = l == 0 && a.time != 0, wvec = a.wvec[l] != 0;
      const int ld = K + (timed ? 1 : 0);  // floats between two rows of W
      const int kq = (K + 7) >> 3, KH = 4 * kq;
      const int k0 = half ? KH : 0, kend = half ? K : (KH < K ? KH : K);
      const float* __restrict__ W = a.W[l];
      const float* __restrict__ bias = a.bias[l];
      const float* __restrict__ in = s_act[l & 1];
      float* __restrict__ nxt_act = s_act[(l + 1) & 1];

      for (int nc0 = wave * kMlpTile; nc0 < N; nc0 += kMlpPass) {  // this wave's chunks (wave-uniform)
        const int nrow = nc0 + bl;
        const float* __restrict__ wrow = nrow < N ? W + int64_t(nrow) * ld : nullptr;
        v16f_t acc[TILES];
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
        float cur[4], nxt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        mlp_load4(cur, wrow, k0, kend, wvec);
        for (int q = 0; q < kq; ++q) {  // (uniform: both halves walk kq vectors, the tail of the shorter one is +0 * +0)
          if (q + 1 < kq) mlp_load4(nxt, wrow, k0 + 4 * (q + 1), kend, wvec);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * q + j;
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
              const float b = k < kend ? in[k * ROWS + t * kMlpTile + bl] : 0.0f;
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j], b, acc[t], 0, 0, 0);
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
        }
        // the layer's tail: this lane's 16 neurons of its state row in each tile
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ng = nc0 + 8 * g + 4 * half;  // neurons ng .. ng + 3
          if (ng >= N) continue;
          float bv[4], tw[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool live = ng + j < N;
            bv[j] = (bias && live) ? bias[ng + j] : 0.0f;
            tw[j] = (timed && live) ? W[int64_t(ng + j) * ld + K] : 0.0f;
          }
#pragma unroll
          for (int t = 0; t < TILES; ++t) {
            const int rl = t * kMlpTile + bl;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float pre = acc[t][4 * g + j];
              if (bias) pre = pre + bv[j];
              if (timed) pre = pre + tr[t] * tw[j];
              v[j] = (a.tanh_act && !last) ? tanhf(pre) : pre;
            }
            if (!last) {
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (ng + j < N) nxt_act[(ng + j) * ROWS + rl] = v[j];
            } else if (rl < nrows) {
              float* __restrict__ orow = a.out + (r0 + rl) * int64_t(NL);
              if (a.ovec) {  // (N % 4 == 0 and ng % 4 == 0: the four are inside the row)
                v4f_t o;
                o.x = v[0], o.y = v[1], o.z = v[2], o.w = v[3];
                *reinterpret_cast<v4f_t*>(orow + ng) = o;
              } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  if (ng + j < N) orow[ng + j] = v[j];
              }
            }
          }
        }
      }
      if (!last) __syncthreads();
    }
  }
}

// everything the host decides about a launch from the sizes, the dtype and the activation: the launcher runs what it returns,
// xde_mlp_plan reports it.  `widths` has been checked: min(n_layers, XDE_MLP_MAX_LAYERS) + 1 entries >= 1 are read.
xde_mlp_plan_t mlp_plan(int64_t rows, const int32_t* widths, int n_layers, int dtype, int act) {
  xde_mlp_plan_t p;
  memset(&p, 0, sizeof(p));
  const int L = n_layers < XDE_MLP_MAX_LAYERS ? n_layers : XDE_MLP_MAX_LAYERS;
  p.width_cap = XDE_MLP_MAX_WIDTH;
  p.served = dtype == XDE_F32 && n_layers <= XDE_MLP_MAX_LAYERS && (act == XDE_MLP_ACT_IDENTITY || act == XDE_MLP_ACT_TANH);
  for (int l = 0; l <= L; ++l) {
    if (widths[l] > XDE_MLP_MAX_WIDTH) p.served = 0;
    if (l < L && widths[l] > p.max_width) p.max_width = widths[l];
  }
  const int64_t singles = (rows + kMlpTile - 1) / kMlpTile;
  p.tiles = (p.max_width <= XDE_MLP_PAIR_WIDTH && singles > kMlpPairTiles) ? 2 : 1;
  p.tile_r = kMlpTile * p.tiles, p.tile_n = kMlpTile, p.pass_n = kMlpPass;
  p.x_vec = (widths[0] % 4) == 0;
  p.out_vec = (widths[L] % 4) == 0;
  p.lds_bytes = 2 * kMlpBufFloats * int(sizeof(float));
  p.items = (rows + p.tile_r - 1) / p.tile_r;
  p.blocks = p.items > grid_cap() ? grid_cap() : p.items;
  return p;
}

// the checks the plan query and the launch share, after their null pointers: the sizes (n_layers first: it says how much of widths is read)
ArgCheck& mlp_sizes(ArgCheck& no, int64_t rows, const int32_t* widths, int n_layers, int dtype) {
  no.sizes("rows, n_layers", {rows, int64_t(n_layers)});
  if (!no.rc)
    for (int l = 0; l <= (n_layers < XDE_MLP_MAX_LAYERS ? n_layers : XDE_MLP_MAX_LAYERS); ++l) no.sizes("every width", {int64_t(widths[l])});
  return no.dtype(dtype);
}

}  // namespace

extern "C" {

int xde_mlp_field(void* out, const void* x, const void* t_rows, double t, const void* const* W, const void* const* bias,
                  const int32_t* widths, int n_layers, int64_t rows, int act, int time, int dtype, void* stream) {
  ArgCheck no{"xde_mlp_field"};
  no.not_null({out, x, W, widths});
  mlp_sizes(no, rows, widths, n_layers, dtype);
  if (!no.rc && act != XDE_MLP_ACT_IDENTITY && act != XDE_MLP_ACT_TANH) no.refuse(": unknown act");
  if (!no.rc && dtype != XDE_F32) no.refuse(": not served: the fused field is fp32 only (take the plain composition)");
  if (!no.rc && n_layers > XDE_MLP_MAX_LAYERS)
    no.refuse(": not served: n_layers = " + std::to_string(n_layers) + " is beyond XDE_MLP_MAX_LAYERS = " + std::to_string(XDE_MLP_MAX_LAYERS));
  if (no.rc) return no.rc;
  const xde_mlp_plan_t p = mlp_plan(rows, widths, n_layers, dtype, act);
  if (!p.served) return no.refuse(": not served: a width is beyond XDE_MLP_MAX_WIDTH = " + std::to_string(XDE_MLP_MAX_WIDTH)).rc;
  no.aligned({out, x, t_rows}, dtype);
  for (int l = 0; l < n_layers; ++l) no.not_null({W[l]}).aligned({W[l], bias ? bias[l] : nullptr}, dtype);
  if (no.rc) return no.rc;

  MlpArgs h;
  memset(&h, 0, sizeof(h));
  h.out = static_cast<float*>(out), h.x = static_cast<const float*>(x), h.t_rows = static_cast<const float*>(t_rows);
  h.rows = rows, h.n_layers = n_layers, h.tanh_act = act == XDE_MLP_ACT_TANH, h.time = time != 0, h.t = float(t);
  double wbytes = 0.0;
  for (int l = 0; l <= n_layers; ++l) h.widths[l] = widths[l];
  for (int l = 0; l < n_layers; ++l) {
    const int ld = widths[l] + (l == 0 && time ? 1 : 0);
    h.W[l] = static_cast<const float*>(W[l]), h.bias[l] = bias ? static_cast<const float*>(bias[l]) : nullptr;
    h.wvec[l] = (widths[l] % 4) == 0 && (ld % 4) == 0 && aligned16(W[l]);
    wbytes += 4.0 * widths[l + 1] * (ld + 1);
  }
  h.xvec = p.x_vec && aligned16(x);
  h.ovec = p.out_vec && aligned16(out);
  // x and out once; the weights once per work item (from L2)
  ProfScope prof(XDE_KID_COMBINE_FUSE, 4.0 * double(rows) * (widths[0] + widths[n_layers] + (time && t_rows ? 1 : 0)) + double(p.items) * wbytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  dim3 g(static_cast<unsigned>(p.blocks)), blk(kBlock);
  with_flag(p.tiles == 2, [&](auto pair) { XDE_LAUNCH((xde_mlp_kernel<decltype(pair)::value ? 2 : 1>), g, blk, st, prof, h); });
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_mlp_plan(int64_t rows, const int32_t* widths, int n_layers, int dtype, int act, int time, xde_mlp_plan_t* plan) {
  (void)time;  // (the time column is a rank-one add in the first layer's tail: it moves nothing in the plan)
  ArgCheck no{"xde_mlp_plan"};
  no.not_null({plan, widths});
  if (mlp_sizes(no, rows, widths, n_layers, dtype).rc) return no.rc;
  *plan = mlp_plan(rows, widths, n_layers, dtype, act);
  return XDE_OK;
}

}  // extern "C"
