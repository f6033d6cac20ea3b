// libxde_hip.so — the Ito Euler-Maruyama step with general (and scalar) noise, and its cotangents (C ABI: include/xde_hip_gn.h; host:
// paddlexde_amd/solver/base_fixed_solver.py, sdeint's option noise_type).
//
// The traffic is g: M elements per output against three for y0, f and y1.  A workgroup owns a TILE of TO consecutive outputs
// o = r * D + d and with them the contiguous span [o_lo * M, o_hi * M) of g, at most kGnTile elements: TO = kGnTile / min(M, kGnChunk),
// 256 outputs at M = 8 (one per lane: the OUT = 1 instantiation, fewer registers) and up to 2048 at M = 1 (kGnOut per lane), so the
// fixed cost of a tile — two barriers and the generator's latency — is spread over the same number of bytes for every M.  The span is
// read with coalesced 16-byte loads — the kernel finds the 16-byte aligned part of the span from the pointer's own bits, so a pointer
// that is only element-aligned, a span that starts inside a vector and a last partial tile take the same path with up to W - 1 single
// elements at either end — into registers, and the NEXT tile's span is requested before this tile is summed.  In LDS the span lies one
// output per row of stride (M | 1) elements: an odd stride, so the lanes of a wave, each reading its own row at the same m, fall on
// different banks (ds_read_b32: 32 banks, 32-lane groups; ds_read_b64 with an odd stride in 8-byte units: 32 distinct bank pairs of 64
// banks).  Each lane then sums its rows against the increments of their state rows in m order: the sum is sequential in m whatever the
// launch shape.
//
// The increments w[r, m] = s * Z[r * M + m] of the rows a tile meets are generated ONCE per workgroup, one Philox block per lane and
// pass, into LDS (D outputs share a row's M increments; with D = 32, M = 8 a tile of 256 outputs needs 16 fp32 blocks).
//
// M is taken in chunks of kGnChunk, which keeps a chunk of the tile (<= kGnTile elements of g, and as many increments at most) in LDS.
// With M <= kGnChunk the chunk is the whole span (the vector path above); beyond it, a chunk is mc consecutive elements of every
// output's row (runs of mc elements at stride M, read element-wise, coalesced over a run), and the lane's running sum goes on across
// chunks in a register: still the sequential order.
//
// The backward is the same tiling turned round: gy1 (the next tile's requested ahead) and each output's state row go to LDS, the
// increments are staged as in the forward, and the span of gg is written with 16-byte stores (element-wise runs when M is chunked).
// NOISE = false (gg not wanted) compiles the generator and the LDS out.  No atomics, one launch.  Built with -ffp-contract=off like the
// rest of the library.

#include "xde_common.hpp"
#include "xde_hip_gn.h"
#include "xde_sde_device.hpp"

using namespace xde;

namespace {

constexpr int kGnChunk = 32;               // elements of M a chunk holds at most
constexpr int kGnTile = 2048;              // elements of g (and of w) a chunk of a tile holds at most
constexpr int kGnOut = kGnTile / kBlock;   // outputs of a tile a lane owns at most (M == 1: the tile is kGnTile outputs)
// TO rows of stride (mc | 1): mc == 1 gives stride 1 (TO = kGnTile rows), mc >= 2 at most TO * mc + TO <= kGnTile + kGnTile / 2
constexpr int kGnGBuf = kGnTile + kGnTile / 2;
constexpr int64_t kGnMaxDim = int64_t(1) << 30;
constexpr int64_t kGnMaxElems = int64_t(1) << 48;

struct GnArgs {
  void* out[2];       // y1 | gf, gg
  const void* in[3];  // y0, f, g | gy1
  int64_t N;          // rows * D
  int32_t D, M, TO;
  double dt, s;
  uint32_t key0, key1, k;
};

// a tile of the outputs: its first output, how many it holds, the first state row it meets and its first output's place in that row
struct GnTileAt {
  int64_t o_lo, r_lo;
  int cnt, rel0;
};

__device__ __forceinline__ GnTileAt gn_tile(int64_t tile, const GnArgs& a) {
  GnTileAt x;
  x.o_lo = tile * a.TO;
  const int64_t left = a.N - x.o_lo;
  x.cnt = left < a.TO ? int(left) : a.TO;
  x.r_lo = x.o_lo / a.D;
  x.rel0 = int(x.o_lo - x.r_lo * a.D);
  return x;
}

// the aligned part of a span of `len` elements at p: `head` single elements, then `nvec` 16-byte vectors, then the rest from `tail0`
struct GnSpan {
  int head, nvec, tail0;
};

template <typename T> __device__ __forceinline__ GnSpan gn_span(const T* p, int len) {
  constexpr int W = Block<T>::W;
  const int phase = int((reinterpret_cast<uintptr_t>(p) / sizeof(T)) % W);
  GnSpan sp;
  sp.head = (W - phase) % W;
  if (sp.head > len) sp.head = len;
  sp.nvec = (len - sp.head) / W;
  sp.tail0 = sp.head + sp.nvec * W;
  return sp;
}

// w[i * mc + (m - m0)] = s * Z[(r_lo + i) * M + m] for the tile's rows i < nrows and the chunk's m0 <= m < m0 + mc.  `whole` (the chunk
// is all of M): the rows' increments are one contiguous run of Z, walked block by block; else one run of mc elements per row.
template <typename T>
__device__ __forceinline__ void gn_stage_noise(T* wbuf, int64_t r_lo, int nrows, int M, int m0, int mc, bool whole, T s, const GnArgs& a) {
  constexpr int W = Block<T>::W;
  const int runs = whole ? 1 : nrows;
  const int len = whole ? nrows * mc : mc;
  const int nb = (len + W - 1) / W + 1;  // blocks a run can touch (one more where it starts inside a block)
  for (int it = threadIdx.x; it < runs * nb; it += kBlock) {
    const int i = it / nb, b = it - i * nb;
    const int64_t start = (r_lo + i) * int64_t(M) + m0;
    const int64_t j = start / W + b;
    if (j * W >= start + len) continue;
    T z[W];
    normals(uint64_t(j), a.k, a.key0, a.key1, 0u, z);
#pragma unroll
    for (int v = 0; v < W; ++v) {
      const int64_t e = j * W + v;
      if (e >= start && e < start + len) wbuf[i * mc + int(e - start)] = s * z[v];
    }
  }
}

// the span of g a tile owns, from global memory into registers: a lane's whole vectors (NV at most) and its one edge element
template <typename T, int NV>
__device__ __forceinline__ void gn_fetch(const T* g, const GnTileAt& x, int M, Pack<T, true> (&regs)[NV], T& edge) {
  const int t = threadIdx.x;
  const int len = x.cnt * M;
  const T* gp = g + x.o_lo * int64_t(M);
  const GnSpan sp = gn_span(gp, len);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = t + i * kBlock;
    if (v < sp.nvec) regs[i] = Pack<T, true>::load(gp + sp.head, v);
  }
  if (t < sp.head + (len - sp.tail0)) edge = gp[t < sp.head ? t : sp.tail0 + (t - sp.head)];
}

// ... and from the registers into LDS, one output per row of stride ldp
template <typename T, int NV>
__device__ __forceinline__ void gn_spill(T* gbuf, const T* g, const GnTileAt& x, int M, int ldp, const Pack<T, true> (&regs)[NV], T edge) {
  constexpr int W = Block<T>::W;
  const int t = threadIdx.x;
  const int len = x.cnt * M;
  const GnSpan sp = gn_span(g + x.o_lo * int64_t(M), len);
  if (t < sp.head + (len - sp.tail0)) {
    const int q = t < sp.head ? t : sp.tail0 + (t - sp.head);
    const int ol = q / M;
    gbuf[ol * ldp + (q - ol * M)] = edge;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = t + i * kBlock;
    if (v < sp.nvec) {
      const int q = sp.head + v * W;
      int ol = q / M, m = q - ol * M;
#pragma unroll
      for (int u = 0; u < W; ++u) {
        gbuf[ol * ldp + m] = regs[i].v[u];
        if (++m == M) {
          m = 0;
          ++ol;
        }
      }
    }
  }
}

// OUT: the outputs of a tile a lane owns at most, 1 (TO <= 256: M >= 8) or kGnOut (the instantiation for smaller M: more registers)
template <typename T, int OUT>
__global__ __launch_bounds__(kBlock) void xde_sde_gn_step_kernel(GnArgs a) {
  constexpr int W = Block<T>::W;
  constexpr int NV = kGnTile / W / kBlock;  // vectors of a span a lane moves at most
  using Pk = Pack<T, true>;
  __shared__ T gbuf[OUT == 1 ? kGnTile + kBlock : kGnGBuf];
  __shared__ T wbuf[kGnTile];
  const int t = threadIdx.x;
  const int D = a.D, M = a.M, TO = a.TO;
  const T dt = T(a.dt), s = T(a.s);
  const T* y0 = static_cast<const T*>(a.in[0]);
  const T* f = static_cast<const T*>(a.in[1]);
  const T* g = static_cast<const T*>(a.in[2]);
  T* y1 = static_cast<T*>(a.out[0]);
  const bool whole = M <= kGnChunk;
  const int64_t ntiles = (a.N + TO - 1) / TO;
  Pk regs[NV];
  T edge = T(0);
  if (whole && int64_t(blockIdx.x) < ntiles) gn_fetch<T, NV>(g, gn_tile(blockIdx.x, a), M, regs, edge);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (workgroup-uniform: the barriers below are reached by all)
    const GnTileAt x = gn_tile(tile, a);
    const int nrows = (x.rel0 + x.cnt - 1) / D + 1;
    T base[OUT], acc[OUT];
#pragma unroll
    for (int j = 0; j < OUT; ++j) {
      const int ol = t + j * kBlock;
      base[j] = acc[j] = T(0);
      if (ol < x.cnt) base[j] = y0[x.o_lo + ol] + f[x.o_lo + ol] * dt;
    }
    for (int m0 = 0; m0 < M; m0 += kGnChunk) {
      const int mc = M - m0 < kGnChunk ? M - m0 : kGnChunk;
      const int ldp = mc | 1;
      __syncthreads();  // the chunk before has been read
      if (whole) {
        gn_spill<T, NV>(gbuf, g, x, M, ldp, regs, edge);
      } else {
        for (int i = t; i < x.cnt * mc; i += kBlock) {
          const int ol = i / mc, m = i - ol * mc;
          gbuf[ol * ldp + m] = g[(x.o_lo + ol) * int64_t(M) + m0 + m];
        }
      }
      gn_stage_noise<T>(wbuf, x.r_lo, nrows, M, m0, mc, whole, s, a);
      __syncthreads();
      // the next tile's span is on its way while this one is summed
      if (whole && tile + gridDim.x < ntiles) gn_fetch<T, NV>(g, gn_tile(tile + gridDim.x, a), M, regs, edge);
#pragma unroll
      for (int j = 0; j < OUT; ++j) {
        const int ol = t + j * kBlock;
        if (ol < x.cnt) {
          const T* gr = gbuf + ol * ldp;
          const T* wr = wbuf + ((x.rel0 + ol) / D) * mc;
          T sum = acc[j];
          int m = 0;
          if (m0 == 0) {
            sum = gr[0] * wr[0];
            m = 1;
          }
          for (; m < mc; ++m) sum = sum + gr[m] * wr[m];
          acc[j] = sum;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < OUT; ++j) {
      const int ol = t + j * kBlock;
      if (ol < x.cnt) y1[x.o_lo + ol] = base[j] + acc[j];
    }
  }
}

// NOISE: gg is wanted (else gf alone: no generator, no LDS)
template <typename T, bool NOISE, int OUT>
__global__ __launch_bounds__(kBlock) void xde_sde_gn_backward_kernel(GnArgs a) {
  constexpr int W = Block<T>::W;
  constexpr int NV = kGnTile / W / kBlock;
  using Pk = Pack<T, true>;
  __shared__ T wbuf[NOISE ? kGnTile : 1];
  __shared__ T ybuf[NOISE ? OUT * kBlock : 1];
  __shared__ int rbuf[NOISE ? OUT * kBlock : 1];
  const int t = threadIdx.x;
  const int D = a.D, M = a.M, TO = a.TO;
  const T dt = T(a.dt), s = T(a.s);
  const T* gy1 = static_cast<const T*>(a.in[0]);
  T* gf = static_cast<T*>(a.out[0]);
  T* gg = static_cast<T*>(a.out[1]);
  const bool whole = M <= kGnChunk;
  const int64_t ntiles = (a.N + TO - 1) / TO;
  T gy[OUT];
  if (int64_t(blockIdx.x) < ntiles) {
    const GnTileAt x = gn_tile(blockIdx.x, a);
#pragma unroll
    for (int j = 0; j < OUT; ++j) gy[j] = t + j * kBlock < x.cnt ? gy1[x.o_lo + t + j * kBlock] : T(0);
  }
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const GnTileAt x = gn_tile(tile, a);
    if (gf) {
#pragma unroll
      for (int j = 0; j < OUT; ++j)
        if (t + j * kBlock < x.cnt) gf[x.o_lo + t + j * kBlock] = gy[j] * dt;
    }
    const int nrows = (x.rel0 + x.cnt - 1) / D + 1;
    for (int m0 = 0; NOISE && m0 < M; m0 += kGnChunk) {
      const int mc = M - m0 < kGnChunk ? M - m0 : kGnChunk;
      __syncthreads();  // the chunk (and the tile) before has been read
      if (m0 == 0) {
#pragma unroll
        for (int j = 0; j < OUT; ++j) {
          const int ol = t + j * kBlock;
          if (ol < x.cnt) {
            ybuf[ol] = gy[j];
            rbuf[ol] = (x.rel0 + ol) / D;
          }
        }
      }
      gn_stage_noise<T>(wbuf, x.r_lo, nrows, M, m0, mc, whole, s, a);
      __syncthreads();
      if (whole) {
        const int len = x.cnt * M;
        T* gp = gg + x.o_lo * int64_t(M);
        const GnSpan sp = gn_span(gp, len);
        if (t < sp.head + (len - sp.tail0)) {
          const int q = t < sp.head ? t : sp.tail0 + (t - sp.head);
          const int ol = q / M;
          gp[q] = ybuf[ol] * wbuf[rbuf[ol] * mc + (q - ol * M)];
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int v = t + i * kBlock;
          if (v < sp.nvec) {
            const int q = sp.head + v * W;
            int ol = q / M, m = q - ol * M;
            Pk o;
#pragma unroll
            for (int u = 0; u < W; ++u) {
              o.v[u] = ybuf[ol] * wbuf[rbuf[ol] * mc + m];
              if (++m == M) {
                m = 0;
                ++ol;
              }
            }
            o.store(gp + sp.head, v);
          }
        }
      } else {
        for (int i = t; i < x.cnt * mc; i += kBlock) {
          const int ol = i / mc, m = i - ol * mc;
          gg[(x.o_lo + ol) * int64_t(M) + m0 + m] = ybuf[ol] * wbuf[rbuf[ol] * mc + m];
        }
      }
    }
    // the next tile's cotangents (this tile's are in LDS, or were only needed for gf)
    if (tile + gridDim.x < ntiles) {
      const GnTileAt nx = gn_tile(tile + gridDim.x, a);
#pragma unroll
      for (int j = 0; j < OUT; ++j) gy[j] = t + j * kBlock < nx.cnt ? gy1[nx.o_lo + t + j * kBlock] : T(0);
    }
  }
}

bool gn_elem_aligned(const void* p, size_t esz) { return (reinterpret_cast<uintptr_t>(p) % esz) == 0; }

bool gn_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

// rows, D, M, their product, k and the dtype
int gn_check_shape(const char* who, int64_t rows, int64_t D, int64_t M, int64_t k, int dtype) {
  if (rows < 1) return fail(XDE_EBADARG, std::string(who) + ": rows < 1");
  if (D < 1 || D > kGnMaxDim) return fail(XDE_EBADARG, std::string(who) + ": D out of range (1 <= D <= 2^30)");
  if (M < 1 || M > kGnMaxDim) return fail(XDE_EBADARG, std::string(who) + ": M out of range (1 <= M <= 2^30)");
  if (rows > kGnMaxElems / D || rows * D > kGnMaxElems / M) return fail(XDE_EBADARG, std::string(who) + ": rows * D * M is too large (> 2^48)");
  if (k < 0 || k > int64_t(0xffffffffLL)) return fail(XDE_EBADARG, std::string(who) + ": k out of range (0 <= k < 2^32)");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, std::string(who) + ": bad dtype");
  return XDE_OK;
}

void gn_fill(GnArgs& a, int64_t rows, int64_t D, int64_t M, double dt, double s, uint64_t seed, int64_t k) {
  memset(&a, 0, sizeof(a));
  a.N = rows * D;
  a.D = int32_t(D);
  a.M = int32_t(M);
  const int64_t mc = M < kGnChunk ? M : kGnChunk;
  a.TO = int32_t(kGnTile / mc);
  a.dt = dt;
  a.s = s;
  a.key0 = uint32_t(seed);
  a.key1 = uint32_t(seed >> 32);
  a.k = uint32_t(k);
}

dim3 gn_grid(const GnArgs& a) {
  int64_t blocks = (a.N + a.TO - 1) / a.TO;
  if (blocks > grid_cap()) blocks = grid_cap();
  return dim3(static_cast<unsigned>(blocks));
}

}  // namespace

extern "C" {

// (profiled under the fixed-step fuse id, as xde_sde_em_step: the kernel-id list of xde_hip.h is part of the frozen ABI)
int xde_sde_gn_step(void* y1, const void* y0, const void* f, const void* g, int64_t rows, int64_t D, int64_t M, double dt, double s,
                    uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_gn_step";
  if (!y1 || !y0 || !f || !g) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  if (int rc = gn_check_shape(who, rows, D, M, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  for (const void* p : {static_cast<const void*>(y1), y0, f, g})
    if (!gn_elem_aligned(p, esz)) return fail(XDE_EBADARG, std::string(who) + ": operand not aligned to its element type");
  const size_t nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if ((y1 != y0 && gn_overlap(y1, nbytes, y0, nbytes)) || gn_overlap(y1, nbytes, f, nbytes) || gn_overlap(y1, nbytes, g, gbytes))
    return fail(XDE_EBADARG, std::string(who) + ": operands overlap (y1 may be y0; no other overlap)");
  GnArgs a;
  gn_fill(a, rows, D, M, dt, s, seed, k);
  a.out[0] = y1;
  a.in[0] = y0;
  a.in[1] = f;
  a.in[2] = g;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE_FUSE, double(4 + M) * double(nbytes));
  const dim3 gr = gn_grid(a), b(kBlock);
  const bool one = a.TO <= kBlock;  // a lane owns one output of a tile
  if (dtype == XDE_F32) {
    if (one) XDE_LAUNCH((xde_sde_gn_step_kernel<float, 1>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_gn_step_kernel<float, kGnOut>), gr, b, st, prof, a);
  } else {
    if (one) XDE_LAUNCH((xde_sde_gn_step_kernel<double, 1>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_gn_step_kernel<double, kGnOut>), gr, b, st, prof, a);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_sde_gn_backward(void* gf, void* gg, const void* gy1, int64_t rows, int64_t D, int64_t M, double dt, double s, uint64_t seed,
                        int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_gn_backward";
  if (!gy1) return fail(XDE_EBADARG, std::string(who) + ": null pointer (gy1)");
  if (int rc = gn_check_shape(who, rows, D, M, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  for (const void* p : {static_cast<const void*>(gf), static_cast<const void*>(gg), gy1})
    if (p && !gn_elem_aligned(p, esz)) return fail(XDE_EBADARG, std::string(who) + ": operand not aligned to its element type");
  const size_t nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if (gn_overlap(gf, nbytes, gy1, nbytes) || gn_overlap(gg, gbytes, gy1, nbytes) || gn_overlap(gf, nbytes, gg, gbytes))
    return fail(XDE_EBADARG, std::string(who) + ": an output overlaps another operand");
  if (!gf && !gg) return XDE_OK;
  GnArgs a;
  gn_fill(a, rows, D, M, dt, s, seed, k);
  a.out[0] = gf;
  a.out[1] = gg;
  a.in[0] = gy1;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double(1 + (gf ? 1 : 0)) * double(nbytes) + (gg ? double(gbytes) : 0.0));
  const dim3 gr = gn_grid(a), b(kBlock);
  const bool one = a.TO <= kBlock;
  if (dtype == XDE_F32) {
    if (gg && one) XDE_LAUNCH((xde_sde_gn_backward_kernel<float, true, 1>), gr, b, st, prof, a);
    else if (gg) XDE_LAUNCH((xde_sde_gn_backward_kernel<float, true, kGnOut>), gr, b, st, prof, a);
    else if (one) XDE_LAUNCH((xde_sde_gn_backward_kernel<float, false, 1>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_gn_backward_kernel<float, false, kGnOut>), gr, b, st, prof, a);
  } else {
    if (gg && one) XDE_LAUNCH((xde_sde_gn_backward_kernel<double, true, 1>), gr, b, st, prof, a);
    else if (gg) XDE_LAUNCH((xde_sde_gn_backward_kernel<double, true, kGnOut>), gr, b, st, prof, a);
    else if (one) XDE_LAUNCH((xde_sde_gn_backward_kernel<double, false, 1>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_gn_backward_kernel<double, false, kGnOut>), gr, b, st, prof, a);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"
