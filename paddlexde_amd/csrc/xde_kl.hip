// libxde_hip.so — the KL term of a latent SDE fused into the Ito Euler-Maruyama step (C ABI: include/xde_hip_kl.h; host:
// paddlexde_amd/solver/base_fixed_solver.py, sdeint's options logqp / prior_drift).
//
// The first kernels of the library where a group of lanes owns a ROW (the last axis of the state: D elements).  A row is served by P
// lanes, P a power of two <= 64 chosen on the host from D, so a wave holds 64 / P rows and a wave's lanes read consecutive 16-byte
// vectors of consecutive rows.  The unit of a lane's work is one Philox block j = e / W of the FLAT array (W = 4 fp32, 2 fp64: one
// 16-byte vector of every operand, and the normals of xde_sde_em_step's lane j): lane p of a row takes the blocks j_lo + p,
// j_lo + p + P, ... that hold elements of its row, so rows longer than P blocks loop.  Where D % W == 0 and every state pointer is
// 16-byte aligned (VEC) a block lies inside one row and is moved as vectors; otherwise rows straddle blocks, the lane masks the block's
// elements to its row and moves them one by one — the same Z[e] either way, and each element is touched by exactly one lane.
//
// The forward keeps a double partial per lane (elements in index order), finishes the row with an xor-shuffle tree over its P lanes
// (no LDS, no atomics, no second launch), and lane 0 of the row writes acc1[r].  The order of the sum depends on (D, dtype, VEC, the
// row's offset in its first block) only: a launch repeats its bits, and the accumulate-only mode (STEP = false: no y0 / y1, no
// generator) runs the same loop and gives the same bits.  The shuffles sit in wave-uniform control flow: a wave walks its rows
// together, lanes of rows past the end carry a zero partial.
//
// The backward is element-wise on the same mapping (so no lane divides e by D): one double per row, gacc[r], is read by the row's
// lanes and rounded to the state dtype once.  Built with -ffp-contract=off like the rest of the library.

#include "xde_common.hpp"
#include "xde_hip_kl.h"
#include "xde_sde_device.hpp"

using namespace xde;

namespace {

struct KlArgs {
  void* out[3];       // y1 | gf, gg, gh
  const void* in[5];  // y0, f, g, h | gy1, f, g, h
  double* acc1;
  const double* acc0;  // the backward's gacc
  int64_t rows, D;
  double dt, s;
  uint32_t key0, key1, k;
  int P;  // lanes per row: a power of two, 1 .. 64
};

// the rows of a wave's pass and a lane's place in its row
struct RowLane {
  int64_t rb, step;  // the wave's first row, and the rows all waves advance by
  int sub, p;        // the lane's row within the wave's pass, and its lane within the row
};

__device__ __forceinline__ RowLane row_lane(int P) {
  const int lane = threadIdx.x & 63;
  const int G = 64 / P;  // rows per wave
  const int64_t wave = int64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  return RowLane{wave * G, int64_t(gridDim.x) * kWaves * G, lane / P, lane & (P - 1)};
}

// STEP: y1 = (y0 + f * dt) + g * (s * Z) as well as the row sums; else the row sums alone (no y0, y1, generator)
template <typename T, bool VEC, bool STEP>
__global__ __launch_bounds__(kBlock) void xde_sde_kl_step_kernel(KlArgs a) {
  constexpr int W = Block<T>::W;
  using Pk = Pack<T, true>;
  const int64_t rows = a.rows, D = a.D;
  const int P = a.P;
  const T dt = T(a.dt), s = T(a.s);
  const double half_dt = 0.5 * double(dt);
  const T* y0 = static_cast<const T*>(a.in[0]);
  const T* f = static_cast<const T*>(a.in[1]);
  const T* g = static_cast<const T*>(a.in[2]);
  const T* h = static_cast<const T*>(a.in[3]);
  T* y1 = static_cast<T*>(a.out[0]);
  const RowLane rl = row_lane(P);
  for (int64_t rb = rl.rb; rb < rows; rb += rl.step) {  // (wave-uniform: the shuffles below are reached by all 64 lanes)
    const int64_t r = rb + rl.sub;
    const bool active = r < rows;
    double part = 0.0;
    if (active) {
      const int64_t e_lo = r * D, e_hi = e_lo + D;
      const int64_t j_hi = (e_hi + W - 1) / W;
      for (int64_t j = e_lo / W + rl.p; j < j_hi; j += P) {
        T z[W] = {};
        if (VEC) {
          Pk F = Pk::load(f, j), G = Pk::load(g, j), H = Pk::load(h, j), Y, O;
          if (STEP) {
            Y = Pk::load(y0, j);
            normals(uint64_t(j), a.k, a.key0, a.key1, 0u, z);
          }
#pragma unroll
          for (int v = 0; v < W; ++v) {
            if (STEP) O.v[v] = (Y.v[v] + F.v[v] * dt) + G.v[v] * (s * z[v]);
            const T u = (F.v[v] - H.v[v]) / G.v[v];
            const T t = u * u;
            part += double(t);
          }
          if (STEP) O.store(y1, j);
        } else {
          if (STEP) normals(uint64_t(j), a.k, a.key0, a.key1, 0u, z);
#pragma unroll
          for (int v = 0; v < W; ++v) {
            const int64_t e = j * W + v;
            if (e >= e_lo && e < e_hi) {
              const T fe = f[e], ge = g[e];
              if (STEP) y1[e] = (y0[e] + fe * dt) + ge * (s * z[v]);
              const T u = (fe - h[e]) / ge;
              const T t = u * u;
              part += double(t);
            }
          }
        }
      }
    }
    for (int off = P >> 1; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if (active && rl.p == 0) a.acc1[r] = (a.acc0 ? a.acc0[r] : 0.0) + part * half_dt;
  }
}

// GY: the cotangent of y1 is given (the fused step's backward); else the accumulate-only mode's.  Null outputs are skipped.
template <typename T, bool VEC, bool GY>
__global__ __launch_bounds__(kBlock) void xde_sde_kl_backward_kernel(KlArgs a) {
  constexpr int W = Block<T>::W;
  using Pk = Pack<T, true>;
  const int64_t rows = a.rows, D = a.D;
  const int P = a.P;
  const T dt = T(a.dt), s = T(a.s);
  const T* gy = static_cast<const T*>(a.in[0]);
  const T* f = static_cast<const T*>(a.in[1]);
  const T* g = static_cast<const T*>(a.in[2]);
  const T* h = static_cast<const T*>(a.in[3]);
  T* gf = static_cast<T*>(a.out[0]);
  T* gg = static_cast<T*>(a.out[1]);
  T* gh = static_cast<T*>(a.out[2]);
  const bool noise = GY && gg != nullptr;
  const RowLane rl = row_lane(P);
  for (int64_t rb = rl.rb; rb < rows; rb += rl.step) {
    const int64_t r = rb + rl.sub;
    if (r >= rows) continue;
    const T ar = T(a.acc0[r] * double(dt));
    const int64_t e_lo = r * D, e_hi = e_lo + D;
    const int64_t j_hi = (e_hi + W - 1) / W;
    for (int64_t j = e_lo / W + rl.p; j < j_hi; j += P) {
      T z[W] = {};
      if (VEC) {
        Pk F = Pk::load(f, j), G = Pk::load(g, j), H = Pk::load(h, j), Y, OF, OG, OH;
        if (GY) Y = Pk::load(gy, j);
        if (noise) normals(uint64_t(j), a.k, a.key0, a.key1, 0u, z);
#pragma unroll
        for (int v = 0; v < W; ++v) {
          const T u = (F.v[v] - H.v[v]) / G.v[v];
          const T c = ar * (u / G.v[v]);
          if (GY) {
            OF.v[v] = Y.v[v] * dt + c;
            OG.v[v] = Y.v[v] * (s * z[v]) - c * u;
          } else {
            OF.v[v] = c;
            OG.v[v] = -(c * u);
          }
          OH.v[v] = -c;
        }
        if (gf) OF.store(gf, j);
        if (gg) OG.store(gg, j);
        if (gh) OH.store(gh, j);
      } else {
        if (noise) normals(uint64_t(j), a.k, a.key0, a.key1, 0u, z);
#pragma unroll
        for (int v = 0; v < W; ++v) {
          const int64_t e = j * W + v;
          if (e >= e_lo && e < e_hi) {
            const T ge = g[e];
            const T u = (f[e] - h[e]) / ge;
            const T c = ar * (u / ge);
            T of, og;
            if (GY) {
              const T y = gy[e];
              of = y * dt + c;
              og = y * (s * z[v]) - c * u;
            } else {
              of = c;
              og = -(c * u);
            }
            if (gf) gf[e] = of;
            if (gg) gg[e] = og;
            if (gh) gh[e] = -c;
          }
        }
      }
    }
  }
}

bool aligned_to(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

struct Operand {
  const void* p;
  size_t bytes;
  bool out;
};

// no output may overlap another operand, but for the pairs (i, j) in `same`, which may be the same array (then the same pointer)
bool any_overlap(const Operand* ops, int count, const int (*same)[2], int nsame) {
  for (int i = 0; i < count; ++i) {
    if (!ops[i].out) continue;
    for (int j = 0; j < count; ++j) {
      if (j == i || (ops[j].out && j < i)) continue;
      bool allowed = false;
      for (int m = 0; m < nsame; ++m)
        if (((same[m][0] == i && same[m][1] == j) || (same[m][0] == j && same[m][1] == i)) && ops[i].p == ops[j].p) allowed = true;
      if (!allowed && overlap(ops[i].p, ops[i].bytes, ops[j].p, ops[j].bytes)) return true;
    }
  }
  return false;
}

// rows, D, dtype, and k where a generator runs
int check_shape(const char* who, int64_t rows, int64_t D, int64_t k, bool uses_k, int dtype) {
  if (rows < 0) return fail(XDE_EBADARG, std::string(who) + ": rows < 0");
  if (D < 1) return fail(XDE_EBADARG, std::string(who) + ": D < 1");
  if (rows > (int64_t(1) << 59) / D) return fail(XDE_EBADARG, std::string(who) + ": rows * D is too large");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, std::string(who) + ": bad dtype");
  if (uses_k && (k < 0 || k > int64_t(0xffffffffLL))) return fail(XDE_EBADARG, std::string(who) + ": k out of range (0 <= k < 2^32)");
  return XDE_OK;
}

// lanes per row: the smallest power of two that covers the blocks a row can touch, at most a wave
int lanes_per_row(int64_t D, int W) {
  const int64_t nb = D % W == 0 ? D / W : (D + 2 * W - 2) / W;  // (a row that starts at the last element of a block: ceil((W - 1 + D) / W))
  int P = 1;
  while (P < 64 && P < nb) P <<= 1;
  return P;
}

dim3 grid_for(int64_t rows, int P) {
  const int64_t per_wave = 64 / P;
  const int64_t waves = (rows + per_wave - 1) / per_wave;
  int64_t blocks = (waves + kWaves - 1) / kWaves;
  if (blocks > grid_cap()) blocks = grid_cap();
  if (blocks < 1) blocks = 1;
  return dim3(static_cast<unsigned>(blocks));
}

// the kernel compiled for (dtype, alignment path, mode)
template <typename T> void launch_step(bool vec, bool step, dim3 gr, hipStream_t st, ProfScope& prof, const KlArgs& a) {
  const dim3 b(kBlock);
  if (vec && step) XDE_LAUNCH((xde_sde_kl_step_kernel<T, true, true>), gr, b, st, prof, a);
  else if (vec) XDE_LAUNCH((xde_sde_kl_step_kernel<T, true, false>), gr, b, st, prof, a);
  else if (step) XDE_LAUNCH((xde_sde_kl_step_kernel<T, false, true>), gr, b, st, prof, a);
  else XDE_LAUNCH((xde_sde_kl_step_kernel<T, false, false>), gr, b, st, prof, a);
}

template <typename T> void launch_backward(bool vec, bool gy, dim3 gr, hipStream_t st, ProfScope& prof, const KlArgs& a) {
  const dim3 b(kBlock);
  if (vec && gy) XDE_LAUNCH((xde_sde_kl_backward_kernel<T, true, true>), gr, b, st, prof, a);
  else if (vec) XDE_LAUNCH((xde_sde_kl_backward_kernel<T, true, false>), gr, b, st, prof, a);
  else if (gy) XDE_LAUNCH((xde_sde_kl_backward_kernel<T, false, true>), gr, b, st, prof, a);
  else XDE_LAUNCH((xde_sde_kl_backward_kernel<T, false, false>), gr, b, st, prof, a);
}

}  // namespace

extern "C" {

// (profiled under the fixed-step fuse id, as xde_sde_em_step: the kernel-id list of xde_hip.h is part of the frozen ABI)
int xde_sde_kl_step(void* y1, double* acc1, const void* y0, const void* f, const void* g, const void* h, const double* acc0,
                    int64_t rows, int64_t D, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_kl_step";
  if (!acc1 || !f || !g || !h) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  if ((y1 == nullptr) != (y0 == nullptr))
    return fail(XDE_EBADARG, std::string(who) + ": y1 and y0 are given together (the step) or null together (accumulate only)");
  const bool step = y1 != nullptr;
  if (int rc = check_shape(who, rows, D, k, step, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const int W = int(16 / esz);
  const void* state[5] = {y1, y0, f, g, h};
  bool vec = D % W == 0;
  for (const void* p : state) {
    if (!p) continue;
    if (!aligned_to(p, esz)) return fail(XDE_EBADARG, std::string(who) + ": operand not aligned to its element type");
    vec = vec && aligned16(p);
  }
  if (!aligned_to(acc1, 8) || !aligned_to(acc0, 8)) return fail(XDE_EBADARG, std::string(who) + ": accumulator not aligned to a double");
  const size_t nbytes = size_t(rows) * size_t(D) * esz, abytes = size_t(rows) * 8;
  const Operand ops[7] = {{y1, nbytes, true}, {acc1, abytes, true}, {y0, nbytes, false}, {f, nbytes, false}, {g, nbytes, false},
                          {h, nbytes, false}, {acc0, abytes, false}};
  const int same[2][2] = {{0, 2}, {1, 6}};
  if (any_overlap(ops, 7, same, 2))
    return fail(XDE_EBADARG, std::string(who) + ": operands overlap (y1 may be y0 and acc1 may be acc0; no other overlap)");
  if (rows == 0) return XDE_OK;
  KlArgs a;
  memset(&a, 0, sizeof(a));
  a.out[0] = y1;
  a.in[0] = y0;
  a.in[1] = f;
  a.in[2] = g;
  a.in[3] = h;
  a.acc1 = acc1;
  a.acc0 = acc0;
  a.rows = rows;
  a.D = D;
  a.dt = dt;
  a.s = s;
  a.key0 = uint32_t(seed);
  a.key1 = uint32_t(seed >> 32);
  a.k = uint32_t(k);
  a.P = lanes_per_row(D, W);
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE_FUSE, double(step ? 5 : 3) * double(nbytes) + double(acc0 ? 2 : 1) * double(abytes));
  const dim3 gr = grid_for(rows, a.P);
  dtype == XDE_F32 ? launch_step<float>(vec, step, gr, st, prof, a) : launch_step<double>(vec, step, gr, st, prof, a);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_sde_kl_backward(void* gf, void* gg, void* gh, const void* gy1, const double* gacc, const void* f, const void* g, const void* h,
                        int64_t rows, int64_t D, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_kl_backward";
  if (!gacc || !f || !g || !h) return fail(XDE_EBADARG, std::string(who) + ": null pointer (gacc, f, g, h)");
  const bool gy = gy1 != nullptr;
  if (int rc = check_shape(who, rows, D, k, gy, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const int W = int(16 / esz);
  const void* state[7] = {gf, gg, gh, gy1, f, g, h};
  bool vec = D % W == 0;
  for (const void* p : state) {
    if (!p) continue;
    if (!aligned_to(p, esz)) return fail(XDE_EBADARG, std::string(who) + ": operand not aligned to its element type");
    vec = vec && aligned16(p);
  }
  if (!aligned_to(gacc, 8)) return fail(XDE_EBADARG, std::string(who) + ": gacc not aligned to a double");
  const size_t nbytes = size_t(rows) * size_t(D) * esz, abytes = size_t(rows) * 8;
  const Operand ops[8] = {{gf, nbytes, true}, {gg, nbytes, true}, {gh, nbytes, true}, {gy1, nbytes, false}, {gacc, abytes, false},
                          {f, nbytes, false}, {g, nbytes, false}, {h, nbytes, false}};
  if (any_overlap(ops, 8, nullptr, 0)) return fail(XDE_EBADARG, std::string(who) + ": an output overlaps another operand");
  const int written = (gf ? 1 : 0) + (gg ? 1 : 0) + (gh ? 1 : 0);
  if (rows == 0 || !written) return XDE_OK;
  KlArgs a;
  memset(&a, 0, sizeof(a));
  a.out[0] = gf;
  a.out[1] = gg;
  a.out[2] = gh;
  a.in[0] = gy1;
  a.in[1] = f;
  a.in[2] = g;
  a.in[3] = h;
  a.acc0 = gacc;
  a.rows = rows;
  a.D = D;
  a.dt = dt;
  a.s = s;
  a.key0 = uint32_t(seed);
  a.key1 = uint32_t(seed >> 32);
  a.k = uint32_t(k);
  a.P = lanes_per_row(D, W);
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double((gy ? 4 : 3) + written) * double(nbytes) + double(abytes));
  const dim3 gr = grid_for(rows, a.P);
  dtype == XDE_F32 ? launch_backward<float>(vec, gy, gr, st, prof, a) : launch_backward<double>(vec, gy, gr, st, prof, a);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"
