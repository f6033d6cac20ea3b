// libxde_hip.so — the vector-Jacobian product of the fused MLP field (include/xde_hip_mlp.h): what one stage of the adjoint's backward
// solve needs of a neural ODE's field, in two launches:
//
//   xde_mlp_field_vjp   f = field(x, t),   gx = a^T df/dx,   gW_l = a^T df/dW_l,   gb_l = a^T df/dbias_l,   gt = a^T df/dt
//
// The field is recomputed, the cotangent `a` walks back through every layer, and neither a hidden activation nor a hidden cotangent
// is ever written to device memory.  Composed of library calls the same work is a taped forward and an autograd walk of 25 to 30
// small launches for three layers.
//
// WORK.  One item = a tile of 32 consecutive state rows.  A workgroup of four waves takes items blockIdx.x, blockIdx.x + gridDim.x, ...
//
// LDS.  One buffer per layer boundary, h_0 .. h_{L-1}, and one for the cotangent: sum(widths[0 .. L]) x 32 floats, all live at once,
// each a matrix TRANSPOSED, [k][row], at a row pitch of exactly 32 floats: element (k, row) sits at 32 k + (row ^ (k & 31)).  Two read
// patterns meet these buffers.  The forward and the transposed product read the 32 rows of one k: row ^ c is a permutation of the 32
// banks.  The outer product reads ONE row across 32 consecutive k (or n): k & 31 takes every value once, so row ^ (k & 31) does too —
// no conflict either way, and no padding: at a pitch of 33 the field 128-128-128-128 (512 x 33 x 4 B = 66 KiB) would not fit the 64 KiB
// a workgroup takes here, with the swizzle it fills them exactly.
//
// PER ITEM.
//   load      x -> h_0, a -> the cotangent's buffer (a row past `rows` is +0 in both), this lane's time t_r.
//   forward   layer by layer the instructions of xde_mlp.hip's single-tile walk, operand for operand: h_{l+1} = act(pre_l) into ITS
//             buffer, the last layer's pre to f.  One barrier per layer boundary.
//   backward  for l = L - 1 .. 0, with D = dpre_l [n][row] (the cotangent's buffer for the last layer, else the buffer of h_{l+1},
//             overwritten in place) and H = h_l [k][row]:
//     sums    thread n: the row sum of D[n][.] over the tile's rows (gb_l) and, in layer 0 with time, of D[n][r] * t_r (the time column
//             of gW_0), both pairwise — neighbours first, then those sums two by two, five levels — into the workgroup's slab.
//     outer   gW_l chunk (32 n) x (32 k): n on the instruction's M axis, k on its N axis, contraction over the tile's 32 rows, lane half
//             0 rows 0..15 and lane half 1 rows 16..31: 16 instructions.  The chunks of a layer are dealt round-robin to the four
//             waves; a lane ends with gW[n0 + i][k0 + lane % 32] for 16 i and adds them into the slab (consecutive lanes, consecutive
//             addresses).
//     ---- barrier: H is about to be overwritten
//     transposed  dh_l chunk of 32 k: k on the M axis, state rows on N, contraction over n: lane half 0 walks n in [0, min(NH, N)),
//             lane half 1 [NH, N), NH = 4 ceil(N / 8) — the forward's split, over n.  Lanes read consecutive k of one row of W_l
//             (coalesced, from L2), four rows ahead.  The lane that receives dh_l[r][k] reads h_l[r][k] from LDS, forms dpre_{l-1} and
//             stores it over that very element: no other lane touches it.  Layer 0 writes gx instead (16-byte stores where it may).
//     ---- barrier
//
// THE REDUCTION OVER ITEMS.  Workgroup b owns slab b of the workspace: P floats, per layer gW_l [N][ld] and then the row sums [N].  Its
// first item STORES every element, each later item loads, adds and stores; an element is always touched by the same lane, so program
// order is all the ordering it needs — no atomics, no memset.  Every workgroup has at least one item (blocks <= items): every slab is
// whole.  The second launch sums the slabs in ascending b, one thread per element, into gW_l and gb_l; one more workgroup forms gt from
// the row sums of dpre_0: gt = sum over ascending n of (sum over ascending b of slab_b's row sum n) * W_0[n][w0].

#include "xde_hip_mlp.h"

#include "xde_common.hpp"
#include "xde_control_host.hpp"

using namespace xde;

namespace {

constexpr int kVjpTile = 32;                  // state rows of a tile = an edge of a chunk: the instruction is 32 x 32
constexpr int kVjpPass = kVjpTile * kWaves;   // k the waves of a workgroup cover side by side in the transposed product
constexpr int kVjpLdsFloats = XDE_MLP_VJP_LDS_BYTES / 4;
static_assert(XDE_MLP_VJP_LDS_BYTES <= 64 * 1024, "the buffers are static LDS");
static_assert(XDE_MLP_MAX_WIDTH <= kBlock, "the row sums take one thread per neuron");

typedef float v16f_t __attribute__((ext_vector_type(16)));

struct VjpArgs {
  float* f;
  float* gx;
  const float* x;
  const float* a;
  const float* t_rows;  // or null: t
  const float* W[XDE_MLP_MAX_LAYERS];
  const float* bias[XDE_MLP_MAX_LAYERS];  // null: none
  float* slabs;                           // [blocks][P]
  int32_t widths[XDE_MLP_MAX_LAYERS + 1];
  int32_t wvec[XDE_MLP_MAX_LAYERS];   // 16-byte loads of W_l in the forward
  int32_t buf[XDE_MLP_MAX_LAYERS + 1];  // first float of h_l's buffer; [L]: of the cotangent's
  int32_t offW[XDE_MLP_MAX_LAYERS];   // gW_l in a slab; the row sums follow it
  int64_t rows;
  int32_t P;
  int n_layers, tanh_act, time, xvec, avec, fvec, gxvec;
  float t;
};

struct VjpSumArgs {
  const float* slabs;
  const float* W0;  // the time column is read for gt
  float* gW[XDE_MLP_MAX_LAYERS];
  float* gb[XDE_MLP_MAX_LAYERS];  // null: not wanted
  float* gt;                      // null: time == 0
  int32_t widths[XDE_MLP_MAX_LAYERS + 1];
  int32_t offW[XDE_MLP_MAX_LAYERS];
  int32_t P, blocks, n_layers, time;
};

// element (k, row) of a [k][row] buffer: see LDS above
__device__ __forceinline__ int sw(int k, int row) { return (k << 5) + (row ^ (k & 31)); }

// four consecutive k of one row of W from k0, as in the forward kernel: those at or past `kend` — and all of a null row — are +0
__device__ __forceinline__ void vjp_load4(float* w, const float* __restrict__ row, int k0, int kend, bool vec) {
  if (row && vec && k0 < kend) {
    const v4f_t v = *reinterpret_cast<const v4f_t*>(row + k0);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (row && k0 + j < kend) ? row[k0 + j] : 0.0f;
  }
}

// column k of four consecutive rows of W from n0 (row stride ld): rows at or past `nend` — and every row of a null column — are +0
__device__ __forceinline__ void vjp_col4(float* w, const float* __restrict__ col, int n0, int nend, int ld) {
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = (col && n0 + j < nend) ? col[int64_t(n0 + j) * ld] : 0.0f;
}

// rows [r0, r0 + nrows) of src[rows][width] into a [k][row] buffer, a missing row +0; consecutive threads, consecutive addresses
__device__ __forceinline__ void vjp_stage(float* __restrict__ dst, const float* __restrict__ src, int64_t r0, int nrows, int width, bool vec) {
  if (vec) {
    const int kv = width >> 2;
    for (int e = threadIdx.x; e < kVjpTile * kv; e += kBlock) {
      const int rl = e / kv, k = 4 * (e - rl * kv);
      v4f_t v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (rl < nrows) v = *reinterpret_cast<const v4f_t*>(src + (r0 + rl) * int64_t(width) + k);
      dst[sw(k + 0, rl)] = v.x, dst[sw(k + 1, rl)] = v.y, dst[sw(k + 2, rl)] = v.z, dst[sw(k + 3, rl)] = v.w;
    }
  } else {
    for (int e = threadIdx.x; e < kVjpTile * width; e += kBlock) {
      const int rl = e / width, k = e - rl * width;
      dst[sw(k, rl)] = rl < nrows ? src[(r0 + rl) * int64_t(width) + k] : 0.0f;
    }
  }
}

__global__ __launch_bounds__(kBlock) void xde_mlp_vjp_kernel(VjpArgs by_value) {
  // the per-layer tables are indexed by a run-time l: read where the dispatch put them (the kernel's only argument starts its argument
  // segment), each entry by a scalar load when it is needed, they do not crowd the scalar registers for the whole kernel
#if defined(__HIP_DEVICE_COMPILE__)
  (void)by_value;
  const VjpArgs& a = *(const VjpArgs*)__builtin_amdgcn_kernarg_segment_ptr();
#else
  const VjpArgs& a = by_value;  // (the host pass only parses the body)
#endif
  __shared__ float s_lds[kVjpLdsFloats];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, bl = lane & 31;
  const int64_t rows = a.rows, items = (rows + kVjpTile - 1) / kVjpTile;
  const int L = a.n_layers, K0 = a.widths[0], NL = a.widths[L];
  float* __restrict__ slab = a.slabs + int64_t(blockIdx.x) * a.P;
  bool first = true;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x, first = false) {  // (workgroup-uniform: every barrier below is reached by all)
    const int64_t r0 = it * kVjpTile;
    const int nrows = rows - r0 < kVjpTile ? int(rows - r0) : kVjpTile;  // rows of the item that exist
    if (!first) __syncthreads();  // the previous item's layer 0 has read the buffers of h_0 and h_1

    vjp_stage(s_lds + a.buf[0], a.x, r0, nrows, K0, a.xvec != 0);
    vjp_stage(s_lds + a.buf[L], a.a, r0, nrows, NL, a.avec != 0);
    const float tr = !a.time ? 0.0f : !a.t_rows ? a.t : bl < nrows ? a.t_rows[r0 + bl] : 0.0f;  // this lane's time
    __syncthreads();

    // ---- forward: xde_mlp.hip's walk of one tile, instruction for instruction; h_{l+1} into its own buffer
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
      const int K = a.widths[l], N = a.widths[l + 1];
      const bool last = l == L - 1, timed = l == 0 && a.time != 0, wvec = a.wvec[l] != 0;
      const int ld = K + (timed ? 1 : 0);  // floats between two rows of W
      const int kq = (K + 7) >> 3, KH = 4 * kq;
      const int k0 = half ? KH : 0, kend = half ? K : (KH < K ? KH : K);
      const float* __restrict__ W = a.W[l];
      const float* __restrict__ bias = a.bias[l];
      const float* __restrict__ in = s_lds + a.buf[l];
      float* __restrict__ nxt_act = s_lds + a.buf[last ? l : l + 1];  // (the last layer stores to f only)

      for (int nc0 = wave * kVjpTile; nc0 < N; nc0 += kVjpPass) {  // this wave's chunks (wave-uniform)
        const int nrow = nc0 + bl;
        const float* __restrict__ wrow = nrow < N ? W + int64_t(nrow) * ld : nullptr;
        v16f_t acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        float cur[4], nxt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        vjp_load4(cur, wrow, k0, kend, wvec);
        for (int q = 0; q < kq; ++q) {  // (uniform: both halves walk kq vectors, the tail of the shorter one is +0 * +0)
          if (q + 1 < kq) vjp_load4(nxt, wrow, k0 + 4 * (q + 1), kend, wvec);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * q + j;
            const float b = k < kend ? in[sw(k, bl)] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j], b, acc, 0, 0, 0);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
        }
        // the layer's tail: this lane's 16 neurons of its state row
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ng = nc0 + 8 * g + 4 * half;  // neurons ng .. ng + 3
          if (ng >= N) continue;
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool live = ng + j < N;
            const float bv = (bias && live) ? bias[ng + j] : 0.0f;
            const float tw = (timed && live) ? W[int64_t(ng + j) * ld + K] : 0.0f;
            float pre = acc[4 * g + j];
            if (bias) pre = pre + bv;
            if (timed) pre = pre + tr * tw;
            v[j] = (a.tanh_act && !last) ? tanhf(pre) : pre;
          }
          if (!last) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (ng + j < N) nxt_act[sw(ng + j, bl)] = v[j];
          } else if (bl < nrows) {
            float* __restrict__ orow = a.f + (r0 + bl) * int64_t(NL);
            if (a.fvec) {  // (N % 4 == 0 and ng % 4 == 0: the four are inside the row)
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
      if (!last) __syncthreads();
    }

    // ---- backward
#pragma unroll 1
    for (int l = L - 1; l >= 0; --l) {
      const int K = a.widths[l], N = a.widths[l + 1];
      const bool timed = l == 0 && a.time != 0;
      const int ld = K + (timed ? 1 : 0);
      const float* __restrict__ W = a.W[l];
      const float* __restrict__ D = s_lds + a.buf[l + 1];  // dpre_l [n][row]
      float* __restrict__ H = s_lds + a.buf[l];            // h_l [k][row]; dpre_{l-1} after this layer
      float* __restrict__ sW = slab + a.offW[l];
      float* __restrict__ sB = sW + int64_t(N) * ld;

      // the row sums: thread n (a row past `rows` holds +0)
      if (int(threadIdx.x) < N) {
        const int n = threadIdx.x;
        float v[kVjpTile], vt[kVjpTile];
#pragma unroll
        for (int r = 0; r < kVjpTile; ++r) {
          v[r] = D[sw(n, r)];
          vt[r] = timed ? v[r] * (!a.t_rows ? a.t : r < nrows ? a.t_rows[r0 + r] : 0.0f) : 0.0f;
        }
        // pairwise: rows 2i and 2i + 1, then those sums two by two, ...: five levels, the rounding of a tree, not of a chain of 32
#pragma unroll
        for (int w = 1; w < kVjpTile; w <<= 1)
#pragma unroll
          for (int r = 0; r < kVjpTile; r += 2 * w) v[r] = v[r] + v[r + w], vt[r] = vt[r] + vt[r + w];
        float s = v[0], st = vt[0];
        if (!first) s = sB[n] + s;
        sB[n] = s;
        if (timed) {
          if (!first) st = sW[int64_t(n) * ld + K] + st;
          sW[int64_t(n) * ld + K] = st;
        }
      }

      // the outer product: this wave's chunks of gW_l
      const int ck = (K + kVjpTile - 1) / kVjpTile, chunks = ck * ((N + kVjpTile - 1) / kVjpTile);
      for (int c = wave; c < chunks; c += kWaves) {  // (wave-uniform)
        const int n0 = (c / ck) * kVjpTile, k0 = (c % ck) * kVjpTile;
        const bool nlive = n0 + bl < N, klive = k0 + bl < K;
        v16f_t acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int r = 16 * half + j;
          const float da = nlive ? D[sw(n0 + bl, r)] : 0.0f;
          const float hb = klive ? H[sw(k0 + bl, r)] : 0.0f;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(da, hb, acc, 0, 0, 0);
        }
        if (klive) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int n = n0 + 8 * (q >> 2) + 4 * half + (q & 3);
            if (n < N) {
              float* __restrict__ p = sW + int64_t(n) * ld + k0 + bl;
              *p = first ? acc[q] : *p + acc[q];
            }
          }
        }
      }
      __syncthreads();  // every read of h_l is done: the transposed product's tail overwrites it

      // the transposed product: dh_l, then dpre_{l-1} in place over h_l, or gx
      const int nq = (N + 7) >> 3, NH = 4 * nq;
      const int nb = half ? NH : 0, nend = half ? N : (NH < N ? NH : N);
      for (int kc0 = wave * kVjpTile; kc0 < K; kc0 += kVjpPass) {  // this wave's chunks (wave-uniform)
        const float* __restrict__ wcol = kc0 + bl < K ? W + kc0 + bl : nullptr;
        v16f_t acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        float cur[4], nxt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        vjp_col4(cur, wcol, nb, nend, ld);
        for (int q = 0; q < nq; ++q) {  // (uniform: both halves walk nq fours, the tail of the shorter one is +0 * +0)
          if (q + 1 < nq) vjp_col4(nxt, wcol, nb + 4 * (q + 1), nend, ld);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int n = nb + 4 * q + j;
            const float b = n < nend ? D[sw(n, bl)] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j], b, acc, 0, 0, 0);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int kg = kc0 + 8 * g + 4 * half;  // k = kg .. kg + 3 of this lane's state row
          if (kg >= K) continue;
          if (l > 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (kg + j >= K) continue;
              float* __restrict__ p = H + sw(kg + j, bl);
              float d = acc[4 * g + j];
              if (a.tanh_act) {
                const float h = *p, hh = h * h;
                d = d * (1.0f - hh);
              }
              *p = d;
            }
          } else if (bl < nrows) {
            float* __restrict__ grow = a.gx + (r0 + bl) * int64_t(K0);
            if (a.gxvec) {  // (K % 4 == 0 and kg % 4 == 0: the four are inside the row)
              v4f_t o;
              o.x = acc[4 * g + 0], o.y = acc[4 * g + 1], o.z = acc[4 * g + 2], o.w = acc[4 * g + 3];
              *reinterpret_cast<v4f_t*>(grow + kg) = o;
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (kg + j < K) grow[kg + j] = acc[4 * g + j];
            }
          }
        }
      }
      if (l > 0) __syncthreads();
    }
  }
}

// the slabs summed in ascending block order: one thread per element of gW_l and gb_l; the workgroup after them forms gt
__global__ __launch_bounds__(kBlock) void xde_mlp_vjp_sum_kernel(VjpSumArgs a) {
  __shared__ float s_gt[kBlock];
  const int64_t P = a.P;
  const int sum_blocks = (a.P + kBlock - 1) / kBlock;
  if (int(blockIdx.x) < sum_blocks) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.P) return;
    float s = a.slabs[p];
    for (int b = 1; b < a.blocks; ++b) s = s + a.slabs[b * P + p];
    for (int l = 0; l < a.n_layers; ++l) {
      const int N = a.widths[l + 1], ld = a.widths[l] + (l == 0 && a.time ? 1 : 0);
      const int q = p - a.offW[l];
      if (q < 0 || q >= N * (ld + 1)) continue;
      if (q < N * ld) a.gW[l][q] = s;
      else if (a.gb[l]) a.gb[l][q - N * ld] = s;
    }
    return;
  }
  // gt (launched with time only): thread n the product of neuron n, thread 0 their sum in ascending n
  const int N = a.widths[1], ld = a.widths[0] + 1, n = threadIdx.x;
  float v = 0.0f;
  if (n < N) {
    const int64_t p = a.offW[0] + int64_t(N) * ld + n;
    float s = a.slabs[p];
    for (int b = 1; b < a.blocks; ++b) s = s + a.slabs[b * P + p];
    v = s * a.W0[int64_t(n) * ld + a.widths[0]];
  }
  s_gt[n] = v;
  __syncthreads();
  if (n == 0) {
    float g = 0.0f;
    for (int i = 0; i < N; ++i) g = g + s_gt[i];
    *a.gt = g;
  }
}

// everything the host decides about a call from the sizes, the dtype, the activation and the caller's limit on workgroups: the
// launcher runs what it returns, xde_mlp_vjp_plan reports it.  `widths` has been checked as mlp_sizes (xde_mlp.hip) checks it.
xde_mlp_vjp_plan_t vjp_plan(int64_t rows, const int32_t* widths, int n_layers, int dtype, int act, int time, int max_blocks) {
  xde_mlp_vjp_plan_t p;
  memset(&p, 0, sizeof(p));
  const int L = n_layers < XDE_MLP_MAX_LAYERS ? n_layers : XDE_MLP_MAX_LAYERS;
  p.served = dtype == XDE_F32 && n_layers <= XDE_MLP_MAX_LAYERS && (act == XDE_MLP_ACT_IDENTITY || act == XDE_MLP_ACT_TANH);
  p.tile_r = kVjpTile, p.pitch = kVjpTile, p.lds_cap = XDE_MLP_VJP_LDS_BYTES, p.grid_cap = XDE_MLP_VJP_MAX_BLOCKS;
  int64_t sum = 0;
  for (int l = 0; l <= L; ++l) {
    if (widths[l] > XDE_MLP_MAX_WIDTH) p.served = 0;
    sum += widths[l];
    if (l < L) p.params += int64_t(widths[l + 1]) * (widths[l] + (l == 0 && time ? 1 : 0) + 1);
  }
  p.sum_widths = int32_t(sum < INT32_MAX ? sum : INT32_MAX);
  const int64_t lds = sum * p.pitch * 4;
  p.lds_bytes = int32_t(lds < INT32_MAX ? lds : INT32_MAX);
  if (lds > p.lds_cap) p.served = 0;
  p.gx_vec = (widths[0] % 4) == 0;
  p.items = (rows + p.tile_r - 1) / p.tile_r;
  const int64_t cap = max_blocks > 0 && max_blocks < p.grid_cap ? max_blocks : p.grid_cap;
  p.blocks = p.items > cap ? cap : p.items;
  p.workspace_bytes = p.blocks * p.params * 4;
  return p;
}

ArgCheck& vjp_sizes(ArgCheck& no, int64_t rows, const int32_t* widths, int n_layers, int dtype, int max_blocks) {
  no.sizes("rows, n_layers", {rows, int64_t(n_layers)});
  if (!no.rc)
    for (int l = 0; l <= (n_layers < XDE_MLP_MAX_LAYERS ? n_layers : XDE_MLP_MAX_LAYERS); ++l) no.sizes("every width", {int64_t(widths[l])});
  no.dtype(dtype);
  if (!no.rc && max_blocks < 0) no.refuse(": bad max_blocks (need max_blocks >= 0)");
  return no;
}

}  // namespace

extern "C" {

int xde_mlp_field_vjp(void* f, void* gx, void* const* gW, void* const* gb, void* gt, const void* x, const void* a, const void* t_rows,
                      double t, const void* const* W, const void* const* bias, const int32_t* widths, int n_layers, int64_t rows, int act,
                      int time, int dtype, void* workspace, int64_t workspace_bytes, int max_blocks, void* stream) {
  ArgCheck no{"xde_mlp_field_vjp"};
  no.not_null({f, gx, gW, x, a, W, widths, workspace});
  if (time) no.not_null({gt});
  vjp_sizes(no, rows, widths, n_layers, dtype, max_blocks);
  if (!no.rc && act != XDE_MLP_ACT_IDENTITY && act != XDE_MLP_ACT_TANH) no.refuse(": unknown act");
  if (!no.rc && dtype != XDE_F32) no.refuse(": not served: the fused vjp is fp32 only (take the plain composition)");
  if (!no.rc && n_layers > XDE_MLP_MAX_LAYERS)
    no.refuse(": not served: n_layers = " + std::to_string(n_layers) + " is beyond XDE_MLP_MAX_LAYERS = " + std::to_string(XDE_MLP_MAX_LAYERS));
  if (no.rc) return no.rc;
  const xde_mlp_vjp_plan_t p = vjp_plan(rows, widths, n_layers, dtype, act, time, max_blocks);
  for (int l = 0; l <= n_layers && !no.rc; ++l)
    if (widths[l] > XDE_MLP_MAX_WIDTH) no.refuse(": not served: a width is beyond XDE_MLP_MAX_WIDTH = " + std::to_string(XDE_MLP_MAX_WIDTH));
  if (!no.rc && !p.served)
    no.refuse(": not served: the widths sum to " + std::to_string(p.sum_widths) + ", beyond the LDS bound of " +
              std::to_string(p.lds_cap / (4 * p.pitch)) + " (" + std::to_string(p.lds_cap) + " bytes at " + std::to_string(4 * p.pitch) +
              " per unit of width)");
  if (!no.rc && workspace_bytes < p.workspace_bytes)
    no.refuse(": workspace too small: " + std::to_string(workspace_bytes) + " bytes, the plan needs " + std::to_string(p.workspace_bytes));
  no.aligned({f, gx, gt, x, a, t_rows, workspace}, dtype);
  for (int l = 0; l < n_layers; ++l)
    no.not_null({W[l], gW[l]}).aligned({W[l], gW[l], bias ? bias[l] : nullptr, gb ? gb[l] : nullptr}, dtype);
  if (no.rc) return no.rc;

  VjpArgs h;
  VjpSumArgs s;
  memset(&h, 0, sizeof(h));
  memset(&s, 0, sizeof(s));
  h.f = static_cast<float*>(f), h.gx = static_cast<float*>(gx), h.x = static_cast<const float*>(x), h.a = static_cast<const float*>(a);
  h.t_rows = static_cast<const float*>(t_rows), h.slabs = static_cast<float*>(workspace);
  h.rows = rows, h.n_layers = n_layers, h.tanh_act = act == XDE_MLP_ACT_TANH, h.time = time != 0, h.t = float(t), h.P = int32_t(p.params);
  s.slabs = h.slabs, s.W0 = static_cast<const float*>(W[0]), s.gt = static_cast<float*>(gt);
  s.P = h.P, s.blocks = int32_t(p.blocks), s.n_layers = n_layers, s.time = h.time;
  double wbytes = 0.0;
  int32_t buf = 0, off = 0;
  for (int l = 0; l <= n_layers; ++l) {
    h.widths[l] = s.widths[l] = widths[l];
    h.buf[l] = buf, buf += widths[l] * kVjpTile;
  }
  for (int l = 0; l < n_layers; ++l) {
    const int ld = widths[l] + (l == 0 && time ? 1 : 0);
    h.W[l] = static_cast<const float*>(W[l]), h.bias[l] = bias ? static_cast<const float*>(bias[l]) : nullptr;
    h.wvec[l] = (widths[l] % 4) == 0 && (ld % 4) == 0 && aligned16(W[l]);
    h.offW[l] = s.offW[l] = off, off += widths[l + 1] * (ld + 1);
    s.gW[l] = static_cast<float*>(gW[l]), s.gb[l] = gb ? static_cast<float*>(gb[l]) : nullptr;
    wbytes += 4.0 * widths[l + 1] * (ld + 1);
  }
  h.xvec = p.gx_vec && aligned16(x);
  h.gxvec = p.gx_vec && aligned16(gx);
  h.avec = (widths[n_layers] % 4) == 0 && aligned16(a);
  h.fvec = (widths[n_layers] % 4) == 0 && aligned16(f);
  hipStream_t st = static_cast<hipStream_t>(stream);
  {  // x, a, f and gx once; per work item the weights twice (from L2) and the slab read and written
    ProfScope prof(XDE_KID_COMBINE_FUSE, 4.0 * double(rows) * (2 * widths[0] + 2 * widths[n_layers] + (time && t_rows ? 1 : 0)) +
                                             double(p.items) * 4.0 * wbytes);
    dim3 g(static_cast<unsigned>(p.blocks)), blk(kBlock);
    XDE_LAUNCH(xde_mlp_vjp_kernel, g, blk, st, prof, h);
  }
  {
    ProfScope prof(XDE_KID_COMBINE_FUSE, double(p.blocks + 1) * wbytes);
    dim3 g(static_cast<unsigned>((p.params + kBlock - 1) / kBlock + (time ? 1 : 0))), blk(kBlock);
    XDE_LAUNCH(xde_mlp_vjp_sum_kernel, g, blk, st, prof, s);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_mlp_vjp_plan(int64_t rows, const int32_t* widths, int n_layers, int dtype, int act, int time, int max_blocks,
                     xde_mlp_vjp_plan_t* plan) {
  ArgCheck no{"xde_mlp_vjp_plan"};
  no.not_null({plan, widths});
  if (vjp_sizes(no, rows, widths, n_layers, dtype, max_blocks).rc) return no.rc;
  *plan = vjp_plan(rows, widths, n_layers, dtype, act, time, max_blocks);
  return XDE_OK;
}

}  // extern "C"
