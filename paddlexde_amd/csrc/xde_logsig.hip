// libxde_hip.so — logsignature windows: the depth-2 log-ODE control of cdeint, and its cotangent (C ABI: include/xde_hip_logsig.h;
// host: paddlexde_amd/interpolation/__init__.py, logsig_windows / logsig_path).
//
// FORWARD.  An item is a window (b, w); a TEAM of G lanes (a power of two, 256 / G items to a workgroup, so a small K packs many items
// into one workgroup) works on it.  The pairs (i, j), i < j, are cut into TS x TS register tiles over the blocks bi <= bj of TS
// channels, one tile to a lane: per step k the lane reads the 2 TS entries of p_{k+1} its tile needs from LDS once (p_k stays in
// registers from the step before, p_0 from the item's start) and feeds 2 TS^2 float64 products from them.  TS = 2 up to C = 16
// (10 tiles at C = 8), 4 beyond (36 tiles at C = 32, 136 at C = 64).  Beyond 256 tiles (C > 88) the tiles are taken in batches of
// 256 and a UNIT of work is (item, batch).  The window's points are staged in LDS in chunks of k: a team's slot holds kLds / (items per
// workgroup) elements, i.e. slot / C points at a time (12 at the least), so L is not bounded by LDS; the accumulators stay in
// registers across chunks and the sum over k is sequential whatever the plan.  The chunk is fetched with 16-byte loads: the slot is
// shifted by the span's own phase so that the aligned part of the global span is the aligned part of the slot.
//
// The K outputs of a workgroup's items are one contiguous span of out: where a unit is a whole item (C <= 88) they are gathered in LDS
// (the points' buffer, done with) and stored with 16-byte stores, up to W - 1 single elements at either end; the batched units write
// their runs of TS elements directly.
//
// BACKWARD.  A unit is again a window; it OWNS its points m = 0 .. n - 1 (and the series' last point, for the last window), so every
// element of gx is written once, by the lane that owns it, without atomics.  A window's first point is also the last point of the
// window before: the unit stages the cotangents of both windows (one contiguous span of gout, 2 K elements) in LDS once, and the
// polygon differences d[m][j] = nxt[j] - prv[j] of its points in chunks of rows; each lane then sums its row of the antisymmetric G
// against d[m] in j order.  Where 2 K elements do not fit a team's slot (C > 76) the lanes read G from global memory instead (gout
// is small and stays in L2).
//
// No MFMA (its accumulation order is not the stated one), no atomics, one launch each.  Built with -ffp-contract=off like the rest
// of the library.

#include "xde_common.hpp"
#include "xde_hip_logsig.h"

using namespace xde;

namespace {

constexpr int kLsLds = 6144;                 // elements of LDS the teams of a workgroup share (24 per lane)
constexpr int kLsPad = kBlock * 4;           // the slots' phase shifts: at most W - 1 elements per team
constexpr int kLsMaxC = 512;
constexpr int64_t kLsMaxElems = int64_t(1) << 48;

struct LsArgs {
  void* out;         // out | gx
  const void* in[2]; // x | gout, x
  int64_t T, W, L;   // L <= T - 1
  int64_t nunits;    // B * W * nbatch
  int32_t C, K, pairs;  // pairs: level 2 is wanted and C > 1
  int32_t G, slot;      // lanes of a team, elements of its LDS slot
  int32_t nb, ntiles, nbatch;  // forward: blocks of TS channels, tiles, batches of G tiles
  int32_t rows, glds;          // backward: rows of d a chunk holds, G staged in LDS
};

__device__ __forceinline__ int ls_pair(int C, int i, int j) { return C + i * (2 * C - i - 1) / 2 + (j - i - 1); }

// the points of window w of its batch row: the first point's index in time and n
__device__ __forceinline__ void ls_window(const LsArgs& a, int64_t w, int64_t& t0, int64_t& n) {
  t0 = w * a.L;
  const int64_t left = a.T - 1 - t0;
  n = left < a.L ? left : a.L;
}

template <typename T, int TS>
__global__ __launch_bounds__(kBlock) void xde_logsig_windows_kernel(LsArgs a) {
  constexpr int W = VecOf<T>::W;
  using Pk = Pack<T, true>;
  __shared__ __attribute__((aligned(16))) T buf[kLsLds + kLsPad];
  const int C = a.C, K = a.K, G = a.G;
  const int ipw = kBlock / G;
  const int team = threadIdx.x / G, tl = threadIdx.x - team * G;
  const T* x = static_cast<const T*>(a.in[0]);
  T* out = static_cast<T*>(a.out);
  const int pc = a.slot / C;                 // points a chunk holds (>= 2 where there are pairs)
  const int S = pc - 1;                      // steps of a chunk
  const int64_t nchunks = (a.pairs && a.L > 1) ? (a.L - 1 + S - 1) / S : 0;
  T* slot = buf + team * (a.slot + W);
  const bool gathered = a.nbatch == 1;       // a unit is a whole item: its K outputs go through LDS
  for (int64_t unit0 = int64_t(blockIdx.x) * ipw; unit0 < a.nunits; unit0 += int64_t(gridDim.x) * ipw) {  // (workgroup-uniform)
    const int64_t unit = unit0 + team;
    const bool live = unit < a.nunits;
    const int64_t item = live ? unit / a.nbatch : 0;
    const int batch = live ? int(unit - item * a.nbatch) : 0;
    const int64_t b = item / a.W, w = item - b * a.W;
    int64_t t0, n;
    ls_window(a, w, t0, n);
    const T* p0 = x + (b * a.T + t0) * C;    // the window's first point
    // the lane's tile
    const int tile = batch * G + tl;
    const bool work = live && a.pairs && tile < a.ntiles;
    int i0 = 0, j0 = 0;
    if (work) {
      int bi = 0, rem = tile, len = a.nb;
      while (rem >= len) {
        rem -= len;
        --len;
        ++bi;
      }
      i0 = bi * TS;
      j0 = (bi + rem) * TS;
    }
    int ci[TS], cj[TS];                      // the tile's channels (clamped: the results past C are dropped)
    T pi0[TS], pj0[TS], pi[TS], pj[TS];
    double acc[TS][TS];
#pragma unroll
    for (int u = 0; u < TS; ++u) {
      ci[u] = i0 + u < C ? i0 + u : C - 1;
      cj[u] = j0 + u < C ? j0 + u : C - 1;
      pi0[u] = pj0[u] = pi[u] = pj[u] = T(0);
      if (work) {
        pi0[u] = p0[ci[u]];
        pj0[u] = p0[cj[u]];
      }
#pragma unroll
      for (int v = 0; v < TS; ++v) acc[u][v] = 0.0;
    }
    for (int64_t ch = 0; ch < nchunks; ++ch) {
      const int64_t k0 = 1 + ch * S;
      const int64_t leftk = n - k0;
      const int cnt = leftk <= 0 ? 0 : (leftk < S ? int(leftk) : S);  // steps k0 .. k0 + cnt - 1 on the points p_k0 .. p_{k0 + cnt}
      const T* gp = p0 + k0 * C;
      const int len = (live && cnt > 0) ? (cnt + 1) * C : 0;
      const int phase = int((reinterpret_cast<uintptr_t>(gp) / sizeof(T)) % W);
      __syncthreads();  // the chunk (or the outputs) before has been read
      if (len > 0) {
        int head = (W - phase) % W;
        if (head > len) head = len;
        const int nvec = (len - head) / W, tail0 = head + nvec * W;
        for (int v = tl; v < nvec; v += G) {
          const Pk r = Pk::load(gp + head, v);
#pragma unroll
          for (int u = 0; u < W; ++u) slot[phase + head + v * W + u] = r.v[u];
        }
        for (int e = tl; e < head + (len - tail0); e += G) {
          const int q = e < head ? e : tail0 + (e - head);
          slot[phase + q] = gp[q];
        }
      }
      __syncthreads();
      if (work && cnt > 0) {
        const T* row = slot + phase;
#pragma unroll
        for (int u = 0; u < TS; ++u) {
          pi[u] = row[ci[u]];
          pj[u] = row[cj[u]];
        }
        for (int s = 0; s < cnt; ++s) {
          row += C;
          double ui[TS], uj[TS], di[TS], dj[TS];
#pragma unroll
          for (int u = 0; u < TS; ++u) {
            const T ni = row[ci[u]], nj = row[cj[u]];
            ui[u] = double(T(pi[u] - pi0[u]));
            uj[u] = double(T(pj[u] - pj0[u]));
            di[u] = double(T(ni - pi[u]));
            dj[u] = double(T(nj - pj[u]));
            pi[u] = ni;
            pj[u] = nj;
          }
#pragma unroll
          for (int u = 0; u < TS; ++u)
#pragma unroll
            for (int v = 0; v < TS; ++v) acc[u][v] = acc[u][v] + (ui[u] * dj[v] - uj[v] * di[u]);
        }
      }
    }
    T* dst;  // where this unit's outputs go: its K elements of out, or of the workgroup's gathered span
    if (gathered) {
      __syncthreads();  // the last chunk has been read: the buffer now gathers the outputs
      dst = buf + team * K;
    } else {
      dst = out + item * K;
    }
    if (live && batch == 0) {
      const T* pn = p0 + n * C;
      for (int c = tl; c < C; c += G) dst[c] = pn[c] - p0[c];
    }
    if (work) {
#pragma unroll
      for (int u = 0; u < TS; ++u)
#pragma unroll
        for (int v = 0; v < TS; ++v) {
          const int i = i0 + u, j = j0 + v;
          if (i < j && j < C) dst[ls_pair(C, i, j)] = T(0.5 * acc[u][v]);
        }
    }
    if (gathered) {
      __syncthreads();
      const int64_t left = a.nunits - unit0;
      const int len = int(left < ipw ? left : ipw) * K;  // (<= 4096: 16 outputs per tile, at most 256 tiles to a workgroup)
      T* op = out + unit0 * K;
      const int phase = int((reinterpret_cast<uintptr_t>(op) / sizeof(T)) % W);
      int head = (W - phase) % W;
      if (head > len) head = len;
      const int nvec = (len - head) / W, tail0 = head + nvec * W;
      const int t = threadIdx.x;
      for (int v = t; v < nvec; v += kBlock) {
        Pk r;
#pragma unroll
        for (int u = 0; u < W; ++u) r.v[u] = buf[head + v * W + u];
        r.store(op + head, v);
      }
      if (t < head + (len - tail0)) {
        const int q = t < head ? t : tail0 + (t - head);
        op[q] = buf[q];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void xde_logsig_windows_backward_kernel(LsArgs a) {
  __shared__ T buf[kLsLds];
  const int C = a.C, K = a.K, G = a.G;
  const int ipw = kBlock / G;
  const int team = threadIdx.x / G, tl = threadIdx.x - team * G;
  const T* gout = static_cast<const T*>(a.in[0]);
  const T* x = static_cast<const T*>(a.in[1]);
  T* gx = static_cast<T*>(a.out);
  const int R = a.rows;                       // rows of d a chunk holds (>= 1)
  const int64_t nchunks = (a.L + 1 + R - 1) / R;  // (the last window owns n + 1 <= L + 1 points)
  T* slot = buf + team * a.slot;
  T* gl = slot;                               // the cotangents of the window before and of this window: 2 K elements
  T* de = slot + (a.glds ? 2 * K : 0);        // d of the shared first point in the window before: C elements
  T* dl = de + C;                             // d of this chunk's rows: R * C elements
  for (int64_t unit = int64_t(blockIdx.x) * ipw + team, unit0 = int64_t(blockIdx.x) * ipw; unit0 < a.nunits;
       unit0 += int64_t(gridDim.x) * ipw, unit += int64_t(gridDim.x) * ipw) {  // (workgroup-uniform)
    const bool live = unit < a.nunits;
    const int64_t b = live ? unit / a.W : 0, w = live ? unit - b * a.W : 0;
    int64_t t0, n;
    ls_window(a, w, t0, n);
    const int64_t owned = live ? n + (w == a.W - 1 ? 1 : 0) : 0;  // the points m < owned are this unit's
    const T* p0 = x + (b * a.T + t0) * C;
    const T* g_e = gout + ((b * a.W + w) - 1) * K;  // the window before (read only where w > 0)
    const T* g_l = g_e + K;
    for (int64_t ch = 0; ch < nchunks; ++ch) {
      const int64_t m0 = ch * R;
      const int64_t leftm = owned - m0;
      const int cnt = leftm <= 0 ? 0 : (leftm < R ? int(leftm) : R);  // the rows m0 .. m0 + cnt - 1
      __syncthreads();  // the chunk before has been read
      if (ch == 0 && live) {
        if (a.glds)
          for (int e = tl + (w > 0 ? 0 : K); e < 2 * K; e += G) gl[e] = g_e[e];
        if (a.pairs && w > 0)  // the window before: nxt of its last point is its first point, prv the point before the last
          for (int j = tl; j < C; j += G) de[j] = p0[j - a.L * C] - p0[j - C];
      }
      if (a.pairs)
        for (int e = tl; e < cnt * C; e += G) {
          const int r = e / C, j = e - r * C;
          const int64_t m = m0 + r;
          const int64_t nx = m < n ? m + 1 : 0, pv = m > 0 ? m - 1 : n;
          dl[e] = p0[nx * C + j] - p0[pv * C + j];
        }
      __syncthreads();
      const T* ge = a.glds ? gl : g_e;
      const T* gw = a.glds ? gl + K : g_l;
      for (int e = tl; e < cnt * C; e += G) {
        const int r = e / C, c = e - r * C;
        const int64_t m = m0 + r;
        double s = 0.0, se = 0.0;
        const bool shared = m == 0 && w > 0;
        if (a.pairs) {
          // row c of G in the triangle: column c above the diagonal (pair(j + 1, c) - pair(j, c) = C - j - 2), then the run pair(c, .)
          const T* d = dl + r * C;
          const int row = ls_pair(C, c, c + 1) - (c + 1);
          for (int j = 0, at = C + c - 1; j < c; at += C - j - 2, ++j) s = s + double(-gw[at]) * double(d[j]);
          for (int j = c + 1; j < C; ++j) s = s + double(gw[row + j]) * double(d[j]);
          if (shared) {
            for (int j = 0, at = C + c - 1; j < c; at += C - j - 2, ++j) se = se + double(-ge[at]) * double(de[j]);
            for (int j = c + 1; j < C; ++j) se = se + double(ge[row + j]) * double(de[j]);
          }
        }
        double q = 0.5 * s;
        if (m == n) q = q + double(gw[c]);
        if (m == 0) q = q - double(gw[c]);
        if (shared) q = (0.5 * se + double(ge[c])) + q;
        gx[(b * a.T + t0 + m) * C + c] = T(q);
      }
    }
  }
}

bool ls_elem_aligned(const void* p, size_t esz) { return (reinterpret_cast<uintptr_t>(p) % esz) == 0; }

bool ls_overlap(const void* a, double na, const void* b, double nb) {
  const double x = double(reinterpret_cast<uintptr_t>(a)), y = double(reinterpret_cast<uintptr_t>(b));
  return x < y + nb && y < x + na;
}

int ls_pow2ceil(int64_t v) {
  int p = 1;
  while (p < v && p < kBlock) p *= 2;
  return p;
}

int64_t ls_channels(int64_t C, int depth) { return depth == 1 ? C : C + C * (C - 1) / 2; }

// B, T, C, L, depth, their products and the dtype; fills what both launches share
int ls_check_fill(const char* who, LsArgs& a, int64_t B, int64_t T, int64_t C, int64_t L, int depth, int dtype) {
  if (B < 1) return fail(XDE_EBADARG, std::string(who) + ": B < 1");
  if (T < 2) return fail(XDE_EBADARG, std::string(who) + ": T < 2 (a window needs two points)");
  if (C < 1 || C > kLsMaxC) return fail(XDE_EBADARG, std::string(who) + ": C out of range (1 <= C <= 512)");
  if (L < 1) return fail(XDE_EBADARG, std::string(who) + ": L < 1");
  if (depth < 1 || depth > 2)
    return fail(XDE_EBADARG, std::string(who) + ": depth " + std::to_string(depth) + " is not built: depth 1 and depth 2 (increments and Levy areas) are");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, std::string(who) + ": bad dtype");
  if (L > T - 1) L = T - 1;
  const int64_t W = (T - 1 + L - 1) / L, K = ls_channels(C, depth);
  if (T > kLsMaxElems / C || B > kLsMaxElems / (T * C)) return fail(XDE_EBADARG, std::string(who) + ": B * T * C is too large (> 2^48)");
  if (W > kLsMaxElems / K || B > kLsMaxElems / (W * K)) return fail(XDE_EBADARG, std::string(who) + ": B * W * K is too large (> 2^48)");
  memset(&a, 0, sizeof(a));
  a.T = T;
  a.W = W;
  a.L = L;
  a.C = int32_t(C);
  a.K = int32_t(K);
  a.pairs = depth == 2 && C > 1;
  return XDE_OK;
}

dim3 ls_grid(const LsArgs& a) {
  const int ipw = kBlock / a.G;
  int64_t blocks = (a.nunits + ipw - 1) / ipw;
  if (blocks > grid_cap()) blocks = grid_cap();
  return dim3(static_cast<unsigned>(blocks));
}

}  // namespace

extern "C" {

int64_t xde_logsig_channels(int64_t C, int depth) {
  if (C < 1 || C > kLsMaxC || depth < 1 || depth > 2) {
    fail(XDE_EBADARG, "xde_logsig_channels: 1 <= C <= 512 and depth 1 or 2 (deeper levels are not built)");
    return -1;
  }
  return ls_channels(C, depth);
}

int xde_logsig_windows(void* out, const void* x, int64_t B, int64_t T, int64_t C, int64_t L, int depth, int dtype, void* stream) {
  const char* who = "xde_logsig_windows";
  if (!out || !x) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  LsArgs a;
  if (int rc = ls_check_fill(who, a, B, T, C, L, depth, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  if (!ls_elem_aligned(out, esz) || !ls_elem_aligned(x, esz)) return fail(XDE_EBADARG, std::string(who) + ": operand not aligned to its element type");
  const double xbytes = double(B) * double(T) * double(C) * double(esz), obytes = double(B) * double(a.W) * double(a.K) * double(esz);
  if (ls_overlap(out, obytes, x, xbytes)) return fail(XDE_EBADARG, std::string(who) + ": out overlaps x");
  a.out = out;
  a.in[0] = x;
  const int TS = C <= 16 ? 2 : 4;
  a.nb = int32_t((C + TS - 1) / TS);
  a.ntiles = a.pairs ? a.nb * (a.nb + 1) / 2 : 0;
  a.G = ls_pow2ceil(a.pairs ? a.ntiles : C);
  a.nbatch = a.pairs ? (a.ntiles + a.G - 1) / a.G : 1;
  a.slot = kLsLds / (kBlock / a.G);
  a.nunits = B * a.W * a.nbatch;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, xbytes + obytes);
  const dim3 gr = ls_grid(a), b(kBlock);
  if (dtype == XDE_F32) {
    if (TS == 2) XDE_LAUNCH((xde_logsig_windows_kernel<float, 2>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_logsig_windows_kernel<float, 4>), gr, b, st, prof, a);
  } else {
    if (TS == 2) XDE_LAUNCH((xde_logsig_windows_kernel<double, 2>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_logsig_windows_kernel<double, 4>), gr, b, st, prof, a);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_logsig_windows_backward(void* gx, const void* gout, const void* x, int64_t B, int64_t T, int64_t C, int64_t L, int depth,
                                int dtype, void* stream) {
  const char* who = "xde_logsig_windows_backward";
  if (!gx || !gout || !x) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  LsArgs a;
  if (int rc = ls_check_fill(who, a, B, T, C, L, depth, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  if (!ls_elem_aligned(gx, esz) || !ls_elem_aligned(gout, esz) || !ls_elem_aligned(x, esz))
    return fail(XDE_EBADARG, std::string(who) + ": operand not aligned to its element type");
  const double xbytes = double(B) * double(T) * double(C) * double(esz), obytes = double(B) * double(a.W) * double(a.K) * double(esz);
  if (ls_overlap(gx, xbytes, x, xbytes) || ls_overlap(gx, xbytes, gout, obytes)) return fail(XDE_EBADARG, std::string(who) + ": gx overlaps another operand");
  a.out = gx;
  a.in[0] = gout;
  a.in[1] = x;
  // a team's slot holds (2 K cotangents, where they fit) + the row of the window before + at least one row of this window
  const int64_t lanes = C * a.L < kBlock ? C * a.L : kBlock;
  const int64_t need = ((2 * int64_t(a.K) + 2 * C) * kBlock + kLsLds - 1) / kLsLds;  // lanes whose share of LDS holds that
  a.glds = need <= kBlock;
  a.G = ls_pow2ceil(a.glds && need > lanes ? need : lanes);
  a.slot = kLsLds / (kBlock / a.G);
  a.rows = int32_t((a.slot - (a.glds ? 2 * a.K : 0)) / C - 1);
  if (a.rows > a.L + 1) a.rows = int32_t(a.L + 1);
  a.nunits = B * a.W;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, 2.0 * xbytes + obytes);
  const dim3 gr = ls_grid(a), b(kBlock);
  if (dtype == XDE_F32) XDE_LAUNCH((xde_logsig_windows_backward_kernel<float>), gr, b, st, prof, a);
  else XDE_LAUNCH((xde_logsig_windows_backward_kernel<double>), gr, b, st, prof, a);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"
