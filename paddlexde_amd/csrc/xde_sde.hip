// libxde_hip.so — Ito Euler-Maruyama and Milstein steps with in-kernel Brownian increments (C ABI: include/xde_hip_sde.h; host:
// paddlexde_amd/solver/base_fixed_solver.py).
//
// One lane serves one Philox4x32-10 call: 4 fp32 or 2 fp64 elements, i.e. exactly one 16-byte vector of every operand.  The
// EM forward reads y0, f, g once and writes y1 once (4 n elt bytes), the Milstein forward reads gb as well (5 n); the noise lives in
// registers only, and the backward regenerates it from the same counter instead of reading it back.  The Milstein support point is the
// EM kernels with the generator compiled out (NOISE = false: s in the place of s * Z).  A lane whose block runs past n (the tail), or any launch whose pointers are not
// all 16-byte aligned, takes the scalar path with the same bits.  Grid-stride loop over at most grid_cap() workgroups of kBlock.
// Built with -ffp-contract=off like the rest of the library; the math functions are the precise ones (no fast-math, no __sinf).

#include "xde_common.hpp"
#include "xde_hip_sde.h"

using namespace xde;

namespace {

constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;  // Philox4x32 round multipliers
constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;  // Weyl key increments

struct Words {
  uint32_t w[4];
};

// Philox4x32-10 at counter (j_lo, j_hi, k, 0) under key (key0, key1)
__device__ __forceinline__ Words philox(uint64_t j, uint32_t k, uint32_t key0, uint32_t key1) {
  uint32_t c0 = uint32_t(j), c1 = uint32_t(j >> 32), c2 = k, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      key0 += kW0;
      key1 += kW1;
    }
    const uint32_t hi0 = __umulhi(kM0, c0), lo0 = kM0 * c0;
    const uint32_t hi1 = __umulhi(kM1, c2), lo1 = kM1 * c2;
    c0 = hi1 ^ c1 ^ key0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ key1;
    c3 = lo0;
  }
  return Words{{c0, c1, c2, c3}};
}

template <typename T> struct Block;  // normals per Philox call = elements per 16-byte vector
template <> struct Block<float> { static constexpr int W = 4; };
template <> struct Block<double> { static constexpr int W = 2; };

__device__ __forceinline__ void box_muller(float u1, float u2, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * u2, &sn, &cs);  // cos / sin of 2 pi u2 without rounding 2 pi
  z0 = r * cs;
  z1 = r * sn;
}

__device__ __forceinline__ void box_muller(double u1, double u2, double& z0, double& z1) {
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
}

// the Z of elements W j .. W j + W - 1 at step k (include/xde_hip_sde.h spells the mapping out)
__device__ __forceinline__ void normals(uint64_t j, uint32_t k, uint32_t key0, uint32_t key1, float (&z)[4]) {
  const Words x = philox(j, k, key0, key1);
  float u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = float((x.w[i] >> 8) + 1u) * 0x1p-24f;
  box_muller(u[0], u[1], z[0], z[1]);
  box_muller(u[2], u[3], z[2], z[3]);
}

__device__ __forceinline__ void normals(uint64_t j, uint32_t k, uint32_t key0, uint32_t key1, double (&z)[2]) {
  const Words x = philox(j, k, key0, key1);
  const uint64_t a = ((uint64_t(x.w[1]) << 32) | x.w[0]) >> 11;
  const uint64_t b = ((uint64_t(x.w[3]) << 32) | x.w[2]) >> 11;
  box_muller(double(a + 1u) * 0x1p-53, double(b + 1u) * 0x1p-53, z[0], z[1]);
}

struct SdeArgs {
  void* out0;       // y1 | gf | out
  void* out1;       // gg
  void* out2;       // ggb
  const void* in0;  // y0 | gy1
  const void* in1;  // f
  const void* in2;  // g
  const void* in3;  // gb
  int64_t n;        // elements (bits mode: words)
  int64_t nblk;     // Philox calls = lanes of work
  double dt, s, c;
  uint32_t key0, key1, k;
};

// NOISE = false is the Milstein support point yb = (y0 + f * dt) + g * s: no generator, the same loads and stores
template <typename T, bool VEC, bool NOISE = true>
__global__ __launch_bounds__(kBlock) void xde_sde_em_step_kernel(SdeArgs a) {
  constexpr int W = Block<T>::W;
  using P = Pack<T, true>;
  static_assert(P::W == W, "one Philox call per 16-byte vector");
  const T dt = T(a.dt), s = T(a.s);
  T* y1 = static_cast<T*>(a.out0);
  const T* y0 = static_cast<const T*>(a.in0);
  const T* f = static_cast<const T*>(a.in1);
  const T* g = static_cast<const T*>(a.in2);
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < a.nblk; j += stride) {
    const int64_t e0 = j * W;
    if (VEC && e0 + W <= a.n) {
      const P Y = P::load(y0, j), F = P::load(f, j), G = P::load(g, j);  // (issued before the generator runs)
      T z[W];
      if (NOISE) normals(uint64_t(j), a.k, a.key0, a.key1, z);
      P o;
#pragma unroll
      for (int v = 0; v < W; ++v) o.v[v] = (Y.v[v] + F.v[v] * dt) + G.v[v] * (NOISE ? s * z[v] : s);
      o.store(y1, j);
    } else {
      T z[W];
      if (NOISE) normals(uint64_t(j), a.k, a.key0, a.key1, z);
#pragma unroll
      for (int v = 0; v < W; ++v) {
        const int64_t e = e0 + v;
        if (e < a.n) y1[e] = (y0[e] + f[e] * dt) + g[e] * (NOISE ? s * z[v] : s);
      }
    }
  }
}

template <typename T, bool VEC, bool GF, bool GG, bool NOISE = true>
__global__ __launch_bounds__(kBlock) void xde_sde_em_backward_kernel(SdeArgs a) {
  constexpr int W = Block<T>::W;
  using P = Pack<T, true>;
  const T dt = T(a.dt), s = T(a.s);
  T* gf = static_cast<T*>(a.out0);
  T* gg = static_cast<T*>(a.out1);
  const T* gy = static_cast<const T*>(a.in0);
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < a.nblk; j += stride) {
    const int64_t e0 = j * W;
    if (VEC && e0 + W <= a.n) {
      const P Y = P::load(gy, j);
      if (GF) {
        P o;
#pragma unroll
        for (int v = 0; v < W; ++v) o.v[v] = Y.v[v] * dt;
        o.store(gf, j);
      }
      if (GG) {
        T z[W];
        if (NOISE) normals(uint64_t(j), a.k, a.key0, a.key1, z);
        P o;
#pragma unroll
        for (int v = 0; v < W; ++v) o.v[v] = Y.v[v] * (NOISE ? s * z[v] : s);
        o.store(gg, j);
      }
    } else {
      T z[W];
      if (GG && NOISE) normals(uint64_t(j), a.k, a.key0, a.key1, z);
#pragma unroll
      for (int v = 0; v < W; ++v) {
        const int64_t e = e0 + v;
        if (e < a.n) {
          if (GF) gf[e] = gy[e] * dt;
          if (GG) gg[e] = gy[e] * (NOISE ? s * z[v] : s);
        }
      }
    }
  }
}

// w = s * Z, q = c * (w * w - |dt|), y1 = ((y0 + f * dt) + g * w) + (gb - g) * q
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void xde_sde_milstein_step_kernel(SdeArgs a) {
  constexpr int W = Block<T>::W;
  using P = Pack<T, true>;
  const T dt = T(a.dt), s = T(a.s), c = T(a.c), ad = abs_(dt);
  T* y1 = static_cast<T*>(a.out0);
  const T* y0 = static_cast<const T*>(a.in0);
  const T* f = static_cast<const T*>(a.in1);
  const T* g = static_cast<const T*>(a.in2);
  const T* gb = static_cast<const T*>(a.in3);
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < a.nblk; j += stride) {
    const int64_t e0 = j * W;
    if (VEC && e0 + W <= a.n) {
      const P Y = P::load(y0, j), F = P::load(f, j), G = P::load(g, j), GB = P::load(gb, j);  // (issued before the generator runs)
      T z[W];
      normals(uint64_t(j), a.k, a.key0, a.key1, z);
      P o;
#pragma unroll
      for (int v = 0; v < W; ++v) {
        const T w = s * z[v], q = c * (w * w - ad);
        o.v[v] = ((Y.v[v] + F.v[v] * dt) + G.v[v] * w) + (GB.v[v] - G.v[v]) * q;
      }
      o.store(y1, j);
    } else {
      T z[W];
      normals(uint64_t(j), a.k, a.key0, a.key1, z);
#pragma unroll
      for (int v = 0; v < W; ++v) {
        const int64_t e = e0 + v;
        if (e < a.n) {
          const T w = s * z[v], q = c * (w * w - ad);
          y1[e] = ((y0[e] + f[e] * dt) + g[e] * w) + (gb[e] - g[e]) * q;
        }
      }
    }
  }
}

// gf = gy1 * dt, gg = gy1 * (w - q), ggb = gy1 * q
template <typename T, bool VEC, bool GF, bool GG, bool GGB>
__global__ __launch_bounds__(kBlock) void xde_sde_milstein_backward_kernel(SdeArgs a) {
  constexpr int W = Block<T>::W;
  using P = Pack<T, true>;
  const T dt = T(a.dt), s = T(a.s), c = T(a.c), ad = abs_(dt);
  T* gf = static_cast<T*>(a.out0);
  T* gg = static_cast<T*>(a.out1);
  T* ggb = static_cast<T*>(a.out2);
  const T* gy = static_cast<const T*>(a.in0);
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < a.nblk; j += stride) {
    const int64_t e0 = j * W;
    if (VEC && e0 + W <= a.n) {
      const P Y = P::load(gy, j);
      if (GF) {
        P o;
#pragma unroll
        for (int v = 0; v < W; ++v) o.v[v] = Y.v[v] * dt;
        o.store(gf, j);
      }
      if (GG || GGB) {
        T z[W];
        normals(uint64_t(j), a.k, a.key0, a.key1, z);
        P og, ob;
#pragma unroll
        for (int v = 0; v < W; ++v) {
          const T w = s * z[v], q = c * (w * w - ad);
          og.v[v] = Y.v[v] * (w - q);
          ob.v[v] = Y.v[v] * q;
        }
        if (GG) og.store(gg, j);
        if (GGB) ob.store(ggb, j);
      }
    } else {
      T z[W];
      if (GG || GGB) normals(uint64_t(j), a.k, a.key0, a.key1, z);
#pragma unroll
      for (int v = 0; v < W; ++v) {
        const int64_t e = e0 + v;
        if (e < a.n) {
          const T y = gy[e];
          if (GF) gf[e] = y * dt;
          if (GG || GGB) {
            const T w = s * z[v], q = c * (w * w - ad);
            if (GG) gg[e] = y * (w - q);
            if (GGB) ggb[e] = y * q;
          }
        }
      }
    }
  }
}

template <typename T, bool BITS>
__global__ __launch_bounds__(kBlock) void xde_sde_noise_kernel(SdeArgs a) {
  constexpr int W = BITS ? 4 : Block<T>::W;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < a.nblk; j += stride) {
    const int64_t e0 = j * W;
    if (BITS) {
      const Words x = philox(uint64_t(j), a.k, a.key0, a.key1);
      uint32_t* o = static_cast<uint32_t*>(a.out0);
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (e0 + v < a.n) o[e0 + v] = x.w[v];
    } else {
      T z[Block<T>::W];
      normals(uint64_t(j), a.k, a.key0, a.key1, z);
      T* o = static_cast<T*>(a.out0);
#pragma unroll
      for (int v = 0; v < Block<T>::W; ++v)
        if (e0 + v < a.n) o[e0 + v] = z[v];
    }
  }
}

bool aligned_to(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

dim3 grid_for(int64_t nblk) {
  int64_t blocks = (nblk + kBlock - 1) / kBlock;
  if (blocks > grid_cap()) blocks = grid_cap();
  if (blocks < 1) blocks = 1;
  return dim3(static_cast<unsigned>(blocks));
}

int check_common(const char* who, int64_t n, int64_t k, int dtype) {
  if (n < 0) return fail(XDE_EBADARG, std::string(who) + ": n < 0");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, std::string(who) + ": bad dtype");
  if (k < 0 || k > int64_t(0xffffffffLL)) return fail(XDE_EBADARG, std::string(who) + ": k out of range (0 <= k < 2^32)");
  return XDE_OK;
}

SdeArgs make_args(int64_t n, int W, double dt, double s, uint64_t seed, int64_t k) {
  SdeArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.nblk = (n + W - 1) / W;
  a.dt = dt;
  a.s = s;
  a.key0 = uint32_t(seed);
  a.key1 = uint32_t(seed >> 32);
  a.k = uint32_t(k);
  return a;
}

}  // namespace

extern "C" {

int xde_sde_em_step(void* y1, const void* y0, const void* f, const void* g, int64_t n, double dt, double s, uint64_t seed,
                    int64_t k, int dtype, void* stream) {
  if (!y1 || !y0 || !f || !g) return fail(XDE_EBADARG, "xde_sde_em_step: null pointer");
  if (int rc = check_common("xde_sde_em_step", n, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const void* ptrs[4] = {y1, y0, f, g};
  bool vec = true;
  for (const void* p : ptrs) {
    if (!aligned_to(p, esz)) return fail(XDE_EBADARG, "xde_sde_em_step: operand not aligned to its element type");
    vec = vec && aligned16(p);
  }
  if (n == 0) return XDE_OK;
  SdeArgs a = make_args(n, dtype == XDE_F32 ? 4 : 2, dt, s, seed, k);
  a.out0 = y1;
  a.in0 = y0;
  a.in1 = f;
  a.in2 = g;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // (profiled under the fixed-step fuse id: the kernel-id list of xde_hip.h is part of the frozen ABI — an EM step is the SDE's fuse)
  ProfScope prof(XDE_KID_COMBINE_FUSE, 4.0 * double(n) * double(esz));
  const dim3 gr = grid_for(a.nblk), b(kBlock);
  if (dtype == XDE_F32) {
    if (vec) XDE_LAUNCH((xde_sde_em_step_kernel<float, true>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_em_step_kernel<float, false>), gr, b, st, prof, a);
  } else {
    if (vec) XDE_LAUNCH((xde_sde_em_step_kernel<double, true>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_em_step_kernel<double, false>), gr, b, st, prof, a);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"

namespace {

template <typename T, bool VEC>
void launch_backward(const SdeArgs& a, bool gf, bool gg, dim3 gr, dim3 b, hipStream_t st, ProfScope& prof) {
  if (gf && gg) XDE_LAUNCH((xde_sde_em_backward_kernel<T, VEC, true, true>), gr, b, st, prof, a);
  else if (gf) XDE_LAUNCH((xde_sde_em_backward_kernel<T, VEC, true, false>), gr, b, st, prof, a);
  else XDE_LAUNCH((xde_sde_em_backward_kernel<T, VEC, false, true>), gr, b, st, prof, a);
}

}  // namespace

extern "C" {

int xde_sde_em_backward(void* gf, void* gg, const void* gy1, int64_t n, double dt, double s, uint64_t seed, int64_t k, int dtype,
                        void* stream) {
  if (!gy1) return fail(XDE_EBADARG, "xde_sde_em_backward: null pointer (gy1)");
  if (int rc = check_common("xde_sde_em_backward", n, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const void* ptrs[3] = {gy1, gf, gg};
  bool vec = true;
  for (const void* p : ptrs) {
    if (!p) continue;
    if (!aligned_to(p, esz)) return fail(XDE_EBADARG, "xde_sde_em_backward: operand not aligned to its element type");
    vec = vec && aligned16(p);
  }
  if (n == 0 || (!gf && !gg)) return XDE_OK;
  SdeArgs a = make_args(n, dtype == XDE_F32 ? 4 : 2, dt, s, seed, k);
  a.out0 = gf;
  a.out1 = gg;
  a.in0 = gy1;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double(1 + (gf ? 1 : 0) + (gg ? 1 : 0)) * double(n) * double(esz));
  const dim3 gr = grid_for(a.nblk), b(kBlock);
  if (dtype == XDE_F32) vec ? launch_backward<float, true>(a, gf, gg, gr, b, st, prof) : launch_backward<float, false>(a, gf, gg, gr, b, st, prof);
  else vec ? launch_backward<double, true>(a, gf, gg, gr, b, st, prof) : launch_backward<double, false>(a, gf, gg, gr, b, st, prof);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_sde_noise(void* out, int64_t n, uint64_t seed, int64_t k, int mode, int dtype, void* stream) {
  if (!out) return fail(XDE_EBADARG, "xde_sde_noise: null pointer");
  if (mode != XDE_NOISE_NORMAL && mode != XDE_NOISE_BITS) return fail(XDE_EBADARG, "xde_sde_noise: bad mode");
  if (int rc = check_common("xde_sde_noise", n, k, dtype)) return rc;
  const bool bits = mode == XDE_NOISE_BITS;
  const size_t esz = bits ? 4 : (dtype == XDE_F32 ? 4 : 8);
  if (!aligned_to(out, esz)) return fail(XDE_EBADARG, "xde_sde_noise: output not aligned to its element type");
  if (n == 0) return XDE_OK;
  SdeArgs a = make_args(n, bits ? 4 : (dtype == XDE_F32 ? 4 : 2), 0.0, 0.0, seed, k);
  a.out0 = out;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double(n) * double(esz));
  const dim3 gr = grid_for(a.nblk), b(kBlock);
  if (bits) XDE_LAUNCH((xde_sde_noise_kernel<float, true>), gr, b, st, prof, a);
  else if (dtype == XDE_F32) XDE_LAUNCH((xde_sde_noise_kernel<float, false>), gr, b, st, prof, a);
  else XDE_LAUNCH((xde_sde_noise_kernel<double, false>), gr, b, st, prof, a);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Milstein (derivative-free, Ito, diagonal noise): support point, step, and their backwards
// ------------------------------------------------------------------------------------------
namespace {

// element alignment of every non-null operand; *vec = all of them 16-byte aligned
int check_operands(const char* who, const void* const* ptrs, int count, size_t esz, bool* vec) {
  *vec = true;
  for (int i = 0; i < count; ++i) {
    if (!ptrs[i]) continue;
    if (!aligned_to(ptrs[i], esz)) return fail(XDE_EBADARG, std::string(who) + ": operand not aligned to its element type");
    *vec = *vec && aligned16(ptrs[i]);
  }
  return XDE_OK;
}

template <typename T, bool VEC>
void launch_support_backward(const SdeArgs& a, bool gf, bool gg, dim3 gr, dim3 b, hipStream_t st, ProfScope& prof) {
  if (gf && gg) XDE_LAUNCH((xde_sde_em_backward_kernel<T, VEC, true, true, false>), gr, b, st, prof, a);
  else if (gf) XDE_LAUNCH((xde_sde_em_backward_kernel<T, VEC, true, false, false>), gr, b, st, prof, a);
  else XDE_LAUNCH((xde_sde_em_backward_kernel<T, VEC, false, true, false>), gr, b, st, prof, a);
}

template <typename T, bool VEC>
void launch_milstein_backward(const SdeArgs& a, int mask, dim3 gr, dim3 b, hipStream_t st, ProfScope& prof) {
  switch (mask) {  // bit 0: gf, bit 1: gg, bit 2: ggb
    case 1: XDE_LAUNCH((xde_sde_milstein_backward_kernel<T, VEC, true, false, false>), gr, b, st, prof, a); break;
    case 2: XDE_LAUNCH((xde_sde_milstein_backward_kernel<T, VEC, false, true, false>), gr, b, st, prof, a); break;
    case 3: XDE_LAUNCH((xde_sde_milstein_backward_kernel<T, VEC, true, true, false>), gr, b, st, prof, a); break;
    case 4: XDE_LAUNCH((xde_sde_milstein_backward_kernel<T, VEC, false, false, true>), gr, b, st, prof, a); break;
    case 5: XDE_LAUNCH((xde_sde_milstein_backward_kernel<T, VEC, true, false, true>), gr, b, st, prof, a); break;
    case 6: XDE_LAUNCH((xde_sde_milstein_backward_kernel<T, VEC, false, true, true>), gr, b, st, prof, a); break;
    default: XDE_LAUNCH((xde_sde_milstein_backward_kernel<T, VEC, true, true, true>), gr, b, st, prof, a); break;
  }
}

}  // namespace

extern "C" {

int xde_sde_milstein_support(void* yb, const void* y0, const void* f, const void* g, int64_t n, double dt, double s, int dtype,
                             void* stream) {
  if (!yb || !y0 || !f || !g) return fail(XDE_EBADARG, "xde_sde_milstein_support: null pointer");
  if (int rc = check_common("xde_sde_milstein_support", n, 0, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const void* ptrs[4] = {yb, y0, f, g};
  bool vec;
  if (int rc = check_operands("xde_sde_milstein_support", ptrs, 4, esz, &vec)) return rc;
  if (n == 0) return XDE_OK;
  SdeArgs a = make_args(n, dtype == XDE_F32 ? 4 : 2, dt, s, 0, 0);
  a.out0 = yb;
  a.in0 = y0;
  a.in1 = f;
  a.in2 = g;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, 4.0 * double(n) * double(esz));  // (a stage input: the stage combines' id)
  const dim3 gr = grid_for(a.nblk), b(kBlock);
  if (dtype == XDE_F32) {
    if (vec) XDE_LAUNCH((xde_sde_em_step_kernel<float, true, false>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_em_step_kernel<float, false, false>), gr, b, st, prof, a);
  } else {
    if (vec) XDE_LAUNCH((xde_sde_em_step_kernel<double, true, false>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_em_step_kernel<double, false, false>), gr, b, st, prof, a);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_sde_milstein_support_backward(void* gf, void* gg, const void* gyb, int64_t n, double dt, double s, int dtype, void* stream) {
  if (!gyb) return fail(XDE_EBADARG, "xde_sde_milstein_support_backward: null pointer (gyb)");
  if (int rc = check_common("xde_sde_milstein_support_backward", n, 0, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const void* ptrs[3] = {gyb, gf, gg};
  bool vec;
  if (int rc = check_operands("xde_sde_milstein_support_backward", ptrs, 3, esz, &vec)) return rc;
  if (n == 0 || (!gf && !gg)) return XDE_OK;
  SdeArgs a = make_args(n, dtype == XDE_F32 ? 4 : 2, dt, s, 0, 0);
  a.out0 = gf;
  a.out1 = gg;
  a.in0 = gyb;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double(1 + (gf ? 1 : 0) + (gg ? 1 : 0)) * double(n) * double(esz));
  const dim3 gr = grid_for(a.nblk), b(kBlock);
  if (dtype == XDE_F32) vec ? launch_support_backward<float, true>(a, gf, gg, gr, b, st, prof) : launch_support_backward<float, false>(a, gf, gg, gr, b, st, prof);
  else vec ? launch_support_backward<double, true>(a, gf, gg, gr, b, st, prof) : launch_support_backward<double, false>(a, gf, gg, gr, b, st, prof);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_sde_milstein_step(void* y1, const void* y0, const void* f, const void* g, const void* gb, int64_t n, double dt, double s,
                          double c, uint64_t seed, int64_t k, int dtype, void* stream) {
  if (!y1 || !y0 || !f || !g || !gb) return fail(XDE_EBADARG, "xde_sde_milstein_step: null pointer");
  if (int rc = check_common("xde_sde_milstein_step", n, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const void* ptrs[5] = {y1, y0, f, g, gb};
  bool vec;
  if (int rc = check_operands("xde_sde_milstein_step", ptrs, 5, esz, &vec)) return rc;
  if (n == 0) return XDE_OK;
  SdeArgs a = make_args(n, dtype == XDE_F32 ? 4 : 2, dt, s, seed, k);
  a.c = c;
  a.out0 = y1;
  a.in0 = y0;
  a.in1 = f;
  a.in2 = g;
  a.in3 = gb;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE_FUSE, 5.0 * double(n) * double(esz));  // (the SDE's fuse, as the EM step)
  const dim3 gr = grid_for(a.nblk), b(kBlock);
  if (dtype == XDE_F32) {
    if (vec) XDE_LAUNCH((xde_sde_milstein_step_kernel<float, true>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_milstein_step_kernel<float, false>), gr, b, st, prof, a);
  } else {
    if (vec) XDE_LAUNCH((xde_sde_milstein_step_kernel<double, true>), gr, b, st, prof, a);
    else XDE_LAUNCH((xde_sde_milstein_step_kernel<double, false>), gr, b, st, prof, a);
  }
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_sde_milstein_backward(void* gf, void* gg, void* ggb, const void* gy1, int64_t n, double dt, double s, double c, uint64_t seed,
                              int64_t k, int dtype, void* stream) {
  if (!gy1) return fail(XDE_EBADARG, "xde_sde_milstein_backward: null pointer (gy1)");
  if (int rc = check_common("xde_sde_milstein_backward", n, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  const void* ptrs[4] = {gy1, gf, gg, ggb};
  bool vec;
  if (int rc = check_operands("xde_sde_milstein_backward", ptrs, 4, esz, &vec)) return rc;
  const int mask = (gf ? 1 : 0) | (gg ? 2 : 0) | (ggb ? 4 : 0);
  if (n == 0 || !mask) return XDE_OK;
  SdeArgs a = make_args(n, dtype == XDE_F32 ? 4 : 2, dt, s, seed, k);
  a.c = c;
  a.out0 = gf;
  a.out1 = gg;
  a.out2 = ggb;
  a.in0 = gy1;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(XDE_KID_COMBINE, double(1 + (gf ? 1 : 0) + (gg ? 1 : 0) + (ggb ? 1 : 0)) * double(n) * double(esz));
  const dim3 gr = grid_for(a.nblk), b(kBlock);
  if (dtype == XDE_F32) vec ? launch_milstein_backward<float, true>(a, mask, gr, b, st, prof) : launch_milstein_backward<float, false>(a, mask, gr, b, st, prof);
  else vec ? launch_milstein_backward<double, true>(a, mask, gr, b, st, prof) : launch_milstein_backward<double, false>(a, mask, gr, b, st, prof);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // extern "C"
