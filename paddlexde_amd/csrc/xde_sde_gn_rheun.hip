// libxde_hip.so — the reversible Heun step with general (and scalar) noise and the launches of its constant-memory cotangent sweep
// (C ABI: include/xde_hip_gn.h; host: FixedSolver._rheun_step under a [D, M] diffusion, solver=GeneralReversibleHeun, and
// sdeint_adjoint's matrix-noise sweep).
//
// The predictor is the step kernel of xde_sde_gn_device.hpp in one more mode (kGnRPredict); the corrector is Heun's, as it stands.  What
// is new here follows from two facts about the scheme under matrix noise.
//
// THE SEAM.  The diffusion gh1 = diffusion(t1, yh1) meets two increments: step k's corrector takes gh1 w_k, step k + 1's predictor
// gh1 w_{k+1}.  The seam kernel is the step kernel's tiling — the span of g through registers into LDS rows of odd stride, the next
// tile's span requested before this one is summed — with TWO staged increment arrays in LDS and two running sums per output, both in m
// order.  One pass over the M N elements of gh1 serves both formulas; the corrector's y1 goes from the register into the predictor's
// base.  LDS: the span (kGnGBuf elements at most) and 2 kGnTile increments, 28 KiB in fp32 and 56 KiB in fp64.
//
// THE STAGE.  The cotangent of gh1 is rank two per output: c1[o] w_{k1}[r, :] from the step after and (ay1[o] / 2) w_{k0}[r, :] from this
// step's corrector.  The stage kernel is the backward kernel's tiling with both increment arrays and both N-vectors in LDS and writes
// the span of bg with 16-byte stores: 3 N elements read, (1 + M) N written, no M N cotangent carried from step to step.  Its tile is
// kGnTile * 4 / sizeof(T) elements, 8 KiB of either dtype, which keeps two increment arrays, two vectors and the row table in 40 KiB.
//
// THE STEP of the sweep has neither a generator nor a matrix: one lane per 16-byte vector of its seven state arrays (the lane loop of
// the diagonal kernels, restated for this formula because this source is built without packed fp32 math and xde_sde.hip is not).

#include "xde_sde_gn_device.hpp"

using namespace xde;
using namespace xde::gn;

namespace {

struct SeamArgs {
  GnArgs g;         // out: y1, yh2, a1; in: y0, f0, g1, f1, a0; dt, s, k: the corrector's (step k0)
  const void* yh1;
  double dt1, s1;   // the predictor's (step k1)
  uint32_t k1;
};

template <typename T, int OUT>
__global__ __launch_bounds__(kBlock) void xde_sde_gn_seam_kernel(SeamArgs sa) {
  constexpr int W = Block<T>::W;
  constexpr int NV = kGnTile / W / kBlock;
  using Pk = Pack<T, true>;
  __shared__ T gbuf[OUT == 1 ? kGnTile + kBlock : kGnGBuf];
  __shared__ T wbuf[2][kGnTile];
  const GnArgs& a = sa.g;
  const int t = threadIdx.x;
  const int D = a.D, M = a.M, TO = a.TO;
  const T dt1 = T(sa.dt1), s0 = T(a.s), s1 = T(sa.s1);
  const T half = T(0.5), hdt0 = half * T(a.dt);
  const T* y0 = static_cast<const T*>(a.in[0]);
  const T* f0 = static_cast<const T*>(a.in[1]);
  const T* g = static_cast<const T*>(a.in[2]);
  const T* f1 = static_cast<const T*>(a.in[3]);
  const T* a0 = static_cast<const T*>(a.in[4]);
  const T* yh1 = static_cast<const T*>(sa.yh1);
  T* y1 = static_cast<T*>(a.out[0]);
  T* yh2 = static_cast<T*>(a.out[1]);
  T* a1 = static_cast<T*>(a.out[2]);
  const bool whole = M <= kGnChunk;
  const int64_t ntiles = (a.N + TO - 1) / TO;
  Pk regs[NV];
  T edge = T(0);
  if (whole && int64_t(blockIdx.x) < ntiles) gn_fetch<T, NV>(g, gn_tile(blockIdx.x, a), M, regs, edge);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (workgroup-uniform: the barriers below are reached by all)
    const GnTileAt x = gn_tile(tile, a);
    const int nrows = (x.rel0 + x.cnt - 1) / D + 1;
    T base[OUT], prev[OUT], acc0[OUT], acc1[OUT];
#pragma unroll
    for (int j = 0; j < OUT; ++j) {
      const int ol = t + j * kBlock;
      base[j] = prev[j] = acc0[j] = acc1[j] = T(0);
      if (ol < x.cnt) {
        base[j] = y0[x.o_lo + ol] + (f0[x.o_lo + ol] + f1[x.o_lo + ol]) * hdt0;
        prev[j] = a0[x.o_lo + ol];
      }
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
      gn_stage_noise<T>(wbuf[0], x.r_lo, nrows, M, m0, mc, whole, s0, a.k, a);
      gn_stage_noise<T>(wbuf[1], x.r_lo, nrows, M, m0, mc, whole, s1, sa.k1, a);
      __syncthreads();
      if (whole && tile + gridDim.x < ntiles) gn_fetch<T, NV>(g, gn_tile(tile + gridDim.x, a), M, regs, edge);
#pragma unroll
      for (int j = 0; j < OUT; ++j) {
        const int ol = t + j * kBlock;
        if (ol < x.cnt) {
          const T* gr = gbuf + ol * ldp;
          const int wr = ((x.rel0 + ol) / D) * mc;
          T b = acc0[j], p = acc1[j];
          int m = 0;
          if (m0 == 0) {
            b = gr[0] * wbuf[0][wr];
            p = gr[0] * wbuf[1][wr];
            m = 1;
          }
          for (; m < mc; ++m) {  // one read of g[o, m] for both sums, each sequential in m
            const T gv = gr[m];
            b = b + gv * wbuf[0][wr + m];
            p = p + gv * wbuf[1][wr + m];
          }
          acc0[j] = b;
          acc1[j] = p;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < OUT; ++j) {
      const int ol = t + j * kBlock;
      if (ol < x.cnt) {
        const int64_t o = x.o_lo + ol;
        const T y = base[j] + (prev[j] + acc0[j]) * half;  // the corrector's y1, kept for the predictor
        const T pb = ((y + y) - yh1[o]) + f1[o] * dt1;
        y1[o] = y;
        a1[o] = acc1[j];
        yh2[o] = pb + acc1[j];
      }
    }
  }
}

struct StageArgs {
  GnArgs g;    // out: bf, bg; in: ay1, c1, af1; dt; s, k: step k0's (the increment that meets ay1 / 2)
  double s1;   // step k1's (the increment that meets c1)
  uint32_t k1;
};

template <typename T> struct StageTile {
  static constexpr int TILE = kGnTile * 4 / int(sizeof(T));  // elements of bg (and of each increment array) a chunk of a tile holds at most
  static constexpr int OUT = TILE / kBlock;
};

// OUT: the outputs of a tile a lane owns at most, 1 or StageTile<T>::OUT.  ay1 null: bg = c1 (x) w1; c1 null: bg = (ay1 / 2) (x) w0.
template <typename T, int OUT>
__global__ __launch_bounds__(kBlock) void xde_sde_gn_rstage_kernel(StageArgs sa) {
  constexpr int W = Block<T>::W;
  constexpr int TILE = StageTile<T>::TILE;
  constexpr int NV = TILE / W / kBlock;
  using Pk = Pack<T, true>;
  __shared__ T wbuf[2][TILE];
  __shared__ T cbuf[OUT * kBlock];
  __shared__ T pbuf[OUT * kBlock];
  __shared__ int rbuf[OUT * kBlock];
  const GnArgs& a = sa.g;
  const int t = threadIdx.x;
  const int D = a.D, M = a.M, TO = a.TO;
  const T half = T(0.5), hdt = half * T(a.dt), s0 = T(a.s), s1 = T(sa.s1);
  T* bf = static_cast<T*>(a.out[0]);
  T* bg = static_cast<T*>(a.out[1]);
  const T* ay1 = static_cast<const T*>(a.in[0]);
  const T* c1 = static_cast<const T*>(a.in[1]);
  const T* af1 = static_cast<const T*>(a.in[2]);
  const bool has_p = ay1 != nullptr, has_c = c1 != nullptr;
  const bool whole = M <= kGnChunk;
  const int64_t ntiles = (a.N + TO - 1) / TO;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (workgroup-uniform)
    const GnTileAt x = gn_tile(tile, a);
    const int nrows = (x.rel0 + x.cnt - 1) / D + 1;
    __syncthreads();  // the tile before has been read
#pragma unroll
    for (int j = 0; j < OUT; ++j) {
      const int ol = t + j * kBlock;
      if (ol < x.cnt) {
        const int64_t o = x.o_lo + ol;
        const T ay = has_p ? ay1[o] : T(0);
        cbuf[ol] = has_c ? c1[o] : T(0);
        pbuf[ol] = ay * half;
        rbuf[ol] = (x.rel0 + ol) / D;
        if (bf) bf[o] = af1 ? af1[o] + ay * hdt : ay * hdt;  // (bf may be af1: this lane's element, read first)
      }
    }
    for (int m0 = 0; m0 < M; m0 += kGnChunk) {
      const int mc = M - m0 < kGnChunk ? M - m0 : kGnChunk;
      if (m0) __syncthreads();  // the chunk before has been read
      if (has_p) gn_stage_noise<T>(wbuf[0], x.r_lo, nrows, M, m0, mc, whole, s0, a.k, a);
      if (has_c) gn_stage_noise<T>(wbuf[1], x.r_lo, nrows, M, m0, mc, whole, s1, sa.k1, a);
      __syncthreads();
      // bg[o, m] = c1[o] * w1[r, m] + (ay1[o] / 2) * w0[r, m]; one term alone where the other operand is null
      auto value = [&](int ol, int m) -> T {
        const int wi = rbuf[ol] * mc + m;
        if (has_c && has_p) return cbuf[ol] * wbuf[1][wi] + pbuf[ol] * wbuf[0][wi];
        return has_c ? cbuf[ol] * wbuf[1][wi] : pbuf[ol] * wbuf[0][wi];
      };
      if (whole) {
        const int len = x.cnt * M;
        T* gp = bg + x.o_lo * int64_t(M);
        const GnSpan sp = gn_span(gp, len);
        if (t < sp.head + (len - sp.tail0)) {
          const int q = t < sp.head ? t : sp.tail0 + (t - sp.head);
          const int ol = q / M;
          gp[q] = value(ol, q - ol * M);
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
              o.v[u] = value(ol, m);
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
          bg[(x.o_lo + ol) * int64_t(M) + m0 + m] = value(ol, m);
        }
      }
    }
  }
}

struct StepArgs {
  void* out[4];       // ay0, ayh0, af0, c0
  const void* in[3];  // ay1, v, ayh1
  int64_t n, nblk;
  double dt;
};

// A = ayh1 + v (FIRST: A = v), ay0 = ay1 + (A + A), ayh0 = -A, af0 = ay1 * (0.5 * dt) + A * dt, c0 = ay1 * 0.5 + A
template <typename T, bool FIRST> __device__ __forceinline__ void rstep_apply(T ay, T v, T ayh, T dt, T (&o)[4]) {
  const T A = FIRST ? v : ayh + v;
  o[0] = ay + (A + A);
  o[1] = -A;
  o[2] = ay * (T(0.5) * dt) + A * dt;
  o[3] = ay * T(0.5) + A;
}

// One lane per 16-byte vector; a lane loads all its operands before it stores, so ay0 may be ay1 and ayh0 may be ayh1.  VEC false (a
// pointer that is not 16-byte aligned) and the last partial vector take the scalar path with the same bits.
template <typename T, bool VEC, bool FIRST>
__global__ __launch_bounds__(kBlock) void xde_sde_gn_rstep_kernel(StepArgs a) {
  constexpr int W = Block<T>::W;
  using P = Pack<T, true>;
  const T dt = T(a.dt);
  const T* ay1 = static_cast<const T*>(a.in[0]);
  const T* vv = static_cast<const T*>(a.in[1]);
  const T* ayh1 = static_cast<const T*>(a.in[2]);
  T* out[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = static_cast<T*>(a.out[i]);
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < a.nblk; j += stride) {
    const int64_t e0 = j * W;
    if (VEC && e0 + W <= a.n) {
      const P AY = P::load(ay1, j), V = P::load(vv, j);
      P H = V;
      if constexpr (!FIRST) H = P::load(ayh1, j);
      P O[4];
#pragma unroll
      for (int u = 0; u < W; ++u) {
        T o[4];
        rstep_apply<T, FIRST>(AY.v[u], V.v[u], H.v[u], dt, o);
#pragma unroll
        for (int i = 0; i < 4; ++i) O[i].v[u] = o[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) O[i].store(out[i], j);
    } else {
      for (int64_t e = e0; e < e0 + W && e < a.n; ++e) {
        T o[4];
        rstep_apply<T, FIRST>(ay1[e], vv[e], FIRST ? vv[e] : ayh1[e], dt, o);
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i][e] = o[i];
      }
    }
  }
}

template <typename T, bool VEC> void rstep_launch(const StepArgs& a, dim3 gr, hipStream_t st, ProfScope& prof) {
  if (a.in[2]) XDE_LAUNCH((xde_sde_gn_rstep_kernel<T, VEC, false>), gr, dim3(kBlock), st, prof, a);
  else XDE_LAUNCH((xde_sde_gn_rstep_kernel<T, VEC, true>), gr, dim3(kBlock), st, prof, a);
}

int check_k(const char* who, const char* name, int64_t k) {
  if (k < 0 || k > int64_t(0xffffffffLL)) return fail(XDE_EBADARG, std::string(who) + ": " + name + " out of range (0 <= k < 2^32)");
  return XDE_OK;
}

}  // namespace

extern "C" {

// (the prediction is a stage input: the stage combines' id)
int xde_sde_gn_rheun_predict(void* yh1, void* a, const void* y, const void* yh0, const void* f, const void* g, int64_t rows, int64_t D,
                             int64_t M, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_gn_rheun_predict";
  if (!yh1 || !a || !y || !yh0 || !f || !g) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  if (int rc = gn_check_shape(who, rows, D, M, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8, nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if (int rc = gn_check_operands(who, {yh1, a}, nullptr, {y, yh0, f}, g, false, nbytes, gbytes, esz, "operands overlap (no output may overlap another operand)"))
    return rc;
  GnArgs ga;
  gn_fill(ga, rows, D, M, dt, s, seed, k);
  ga.out[0] = yh1;
  ga.out[1] = a;
  ga.in[0] = y;
  ga.in[1] = f;
  ga.in[2] = g;
  ga.in[3] = yh0;
  ProfScope prof(XDE_KID_COMBINE, double(6 + M) * double(nbytes));
  return gn_launch_step<kGnRPredict>(ga, dtype, static_cast<hipStream_t>(stream), prof);
}

// (the SDE's fuse, as the correctors)
int xde_sde_gn_rheun_seam(void* y1, void* yh2, void* a1, const void* y0, const void* f0, const void* f1, const void* a0, const void* yh1,
                          const void* g1, int64_t rows, int64_t D, int64_t M, double dt0, double s0, int64_t k0, double dt1, double s1,
                          int64_t k1, uint64_t seed, int dtype, void* stream) {
  const char* who = "xde_sde_gn_rheun_seam";
  if (!y1 || !yh2 || !a1 || !y0 || !f0 || !f1 || !a0 || !yh1 || !g1) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  if (int rc = gn_check_shape(who, rows, D, M, k0, dtype)) return rc;
  if (int rc = check_k(who, "k1", k1)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8, nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if (int rc = gn_check_operands(who, {y1, yh2, a1}, nullptr, {y0, f0, f1, a0, yh1}, g1, true, nbytes, gbytes, esz,
                                 "operands overlap (y1 may be y0; no other overlap: yh2 may not be yh1)"))
    return rc;
  SeamArgs sa;
  gn_fill(sa.g, rows, D, M, dt0, s0, seed, k0);
  sa.g.out[0] = y1;
  sa.g.out[1] = yh2;
  sa.g.out[2] = a1;
  sa.g.in[0] = y0;
  sa.g.in[1] = f0;
  sa.g.in[2] = g1;
  sa.g.in[3] = f1;
  sa.g.in[4] = a0;
  sa.yh1 = yh1;
  sa.dt1 = dt1;
  sa.s1 = s1;
  sa.k1 = uint32_t(k1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE_FUSE, double(8 + M) * double(nbytes));
  const dim3 gr = gn_grid(sa.g), b(kBlock);
  const bool one = sa.g.TO <= kBlock;
  if (dtype == XDE_F32) {
    if (one) XDE_LAUNCH((xde_sde_gn_seam_kernel<float, 1>), gr, b, st, prof, sa);
    else XDE_LAUNCH((xde_sde_gn_seam_kernel<float, kGnOut>), gr, b, st, prof, sa);
  } else {
    if (one) XDE_LAUNCH((xde_sde_gn_seam_kernel<double, 1>), gr, b, st, prof, sa);
    else XDE_LAUNCH((xde_sde_gn_seam_kernel<double, kGnOut>), gr, b, st, prof, sa);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_sde_gn_rheun_adjoint_stage(void* bf, void* bg, const void* af1, const void* c1, const void* ay1, int64_t rows, int64_t D, int64_t M,
                                   double dt, double s0, int64_t k0, double s1, int64_t k1, uint64_t seed, int dtype, void* stream) {
  const char* who = "xde_sde_gn_rheun_adjoint_stage";
  if (!bg) return fail(XDE_EBADARG, std::string(who) + ": null pointer (bg)");
  if (!ay1 && !c1) return fail(XDE_EBADARG, std::string(who) + ": null pointer (ay1 and c1: one of them must be given)");
  if (!ay1 && (bf || af1)) return fail(XDE_EBADARG, std::string(who) + ": bf is af1 plus a multiple of ay1: with ay1 null, bf and af1 must be null");
  if (ay1 && !bf) return fail(XDE_EBADARG, std::string(who) + ": null pointer (bf)");
  if (ay1 && (af1 == nullptr) != (c1 == nullptr))
    return fail(XDE_EBADARG, std::string(who) + ": null pointer (af1 and c1 are given or null together)");
  if (int rc = gn_check_shape(who, rows, D, M, k0, dtype)) return rc;
  if (int rc = check_k(who, "k1", k1)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8, nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if (int rc = gn_check_operands(who, {bf}, bg, {af1, c1, ay1}, nullptr, true, nbytes, gbytes, esz, "operands overlap (bf may be af1; no other overlap)"))
    return rc;
  StageArgs sa;
  gn_fill(sa.g, rows, D, M, dt, s0, seed, k0);
  const int64_t tile = dtype == XDE_F32 ? StageTile<float>::TILE : StageTile<double>::TILE;
  sa.g.TO = int32_t(tile / (M < kGnChunk ? M : kGnChunk));
  sa.g.out[0] = bf;
  sa.g.out[1] = bg;
  sa.g.in[0] = ay1;
  sa.g.in[1] = c1;
  sa.g.in[2] = af1;
  sa.s1 = s1;
  sa.k1 = uint32_t(k1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double((ay1 ? 1 : 0) + (c1 ? 1 : 0) + (af1 ? 1 : 0) + (bf ? 1 : 0)) * double(nbytes) + double(gbytes));
  const dim3 gr = gn_grid(sa.g), b(kBlock);
  const bool one = sa.g.TO <= kBlock;
  if (dtype == XDE_F32) {
    if (one) XDE_LAUNCH((xde_sde_gn_rstage_kernel<float, 1>), gr, b, st, prof, sa);
    else XDE_LAUNCH((xde_sde_gn_rstage_kernel<float, StageTile<float>::OUT>), gr, b, st, prof, sa);
  } else {
    if (one) XDE_LAUNCH((xde_sde_gn_rstage_kernel<double, 1>), gr, b, st, prof, sa);
    else XDE_LAUNCH((xde_sde_gn_rstage_kernel<double, StageTile<double>::OUT>), gr, b, st, prof, sa);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

// (ayh1 null: the first backward step)
int xde_sde_gn_rheun_adjoint_step(void* ay0, void* ayh0, void* af0, void* c0, const void* ay1, const void* ayh1, const void* v, int64_t n,
                                  double dt, int dtype, void* stream) {
  const char* who = "xde_sde_gn_rheun_adjoint_step";
  if (!ay0 || !ayh0 || !af0 || !c0 || !ay1 || !v) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  if (n < 0) return fail(XDE_EBADARG, std::string(who) + ": n < 0");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, std::string(who) + ": bad dtype");
  const size_t esz = dtype == XDE_F32 ? 4 : 8, nbytes = size_t(n) * esz;
  const void* ptrs[7] = {ay0, ayh0, af0, c0, ay1, ayh1, v};
  bool vec = true;
  for (const void* p : ptrs) {
    if (p && !gn_elem_aligned(p, esz)) return fail(XDE_EBADARG, std::string(who) + ": operand not aligned to its element type");
    vec = vec && aligned16(p);
  }
  for (int o = 0; o < 4; ++o)
    for (int x = o + 1; x < 7; ++x) {
      if ((o == 0 && x == 4 && ay0 == ay1) || (o == 1 && x == 5 && ayh0 == ayh1)) continue;  // in place
      if (gn_overlap(ptrs[o], nbytes, ptrs[x], nbytes))
        return fail(XDE_EBADARG, std::string(who) + ": operands overlap (ay0 may be ay1 and ayh0 may be ayh1; no other overlap)");
    }
  if (n == 0) return XDE_OK;
  StepArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < 4; ++i) a.out[i] = const_cast<void*>(ptrs[i]);
  a.in[0] = ay1;
  a.in[1] = v;
  a.in[2] = ayh1;
  a.n = n;
  const int W = dtype == XDE_F32 ? 4 : 2;
  a.nblk = (n + W - 1) / W;
  a.dt = dt;
  int64_t blocks = (a.nblk + kBlock - 1) / kBlock;
  if (blocks > grid_cap()) blocks = grid_cap();
  const dim3 gr(static_cast<unsigned>(blocks));
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double(ayh1 ? 7 : 6) * double(nbytes));
  if (dtype == XDE_F32) vec ? rstep_launch<float, true>(a, gr, st, prof) : rstep_launch<float, false>(a, gr, st, prof);
  else vec ? rstep_launch<double, true>(a, gr, st, prof) : rstep_launch<double, false>(a, gr, st, prof);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"
