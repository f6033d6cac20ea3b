// libxde_hip.so — Ito Euler-Maruyama and Milstein steps with in-kernel Brownian increments (C ABI: include/xde_hip_sde.h; host:
// paddlexde_amd/solver/base_fixed_solver.py).
//
// One lane serves one Philox4x32-10 call: 4 fp32 or 2 fp64 elements, i.e. exactly one 16-byte vector of every operand.  The
// EM forward reads y0, f, g once and writes y1 once (4 n elt bytes), the Milstein forward reads gb as well (5 n); the noise lives in
// registers only, and the backward regenerates it from the same counter instead of reading it back.
//
// The file is three layers.  Each formula is written once, as a per-element functor (EmStep, EmBackward, MilsteinStep,
// MilsteinBackward); the Milstein support point is the EM functors with NOISE = false (s in the place of s * Z, the generator compiled
// out).  One kernel, xde_sde_step_kernel, owns the lane loop for all of them: a lane whose block runs past n (the tail), or any launch
// whose pointers are not all 16-byte aligned, takes the scalar path with the same bits; grid-stride over at most grid_cap() workgroups
// of kBlock.  One host launcher, sde_launch, owns the argument checks, the profiling scope and the dtype x alignment x output-mask
// dispatch; the entry points only name their operands.  xde_sde_noise, the generator alone, keeps a kernel and a host body of its own:
// it is what the tests read Z back with, an independent statement of which counter serves which element.
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
  void* out[3];       // y1 | gf, gg, ggb | the noise kernel's output
  const void* in[4];  // y0, f, g, gb | gy1
  int64_t n;          // elements (bits mode: words)
  int64_t nblk;       // Philox calls = lanes of work
  double dt, s, c;
  uint32_t key0, key1, k;
};

// the step's scalars in the state dtype; ad = |dt|
template <typename T> struct Coef {
  T dt, s, c, ad;
};

// The formulas, one element each: (inputs x, the element's Z, the scalars) -> outputs o, in the written op order.  NI inputs, NO
// outputs, and ZMASK = the outputs that depend on Z (bit i: output i).  NOISE = false puts s in the place of s * Z.
struct EmStep {  // y1 = (y0 + f * dt) + g * (s * Z)        x = y0, f, g
  static constexpr int NI = 3, NO = 1, ZMASK = 1;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    o[0] = (x[0] + x[1] * k.dt) + x[2] * (NOISE ? k.s * z : k.s);
  }
};

struct EmBackward {  // gf = gy1 * dt, gg = gy1 * (s * Z)     x = gy1
  static constexpr int NI = 1, NO = 2, ZMASK = 2;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    o[0] = x[0] * k.dt;
    o[1] = x[0] * (NOISE ? k.s * z : k.s);
  }
};

struct MilsteinStep {  // w = s * Z, q = c * (w * w - |dt|), y1 = ((y0 + f * dt) + g * w) + (gb - g) * q        x = y0, f, g, gb
  static constexpr int NI = 4, NO = 1, ZMASK = 1;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    static_assert(NOISE, "Milstein has no noise-free form");
    const T w = k.s * z, q = k.c * (w * w - k.ad);
    o[0] = ((x[0] + x[1] * k.dt) + x[2] * w) + (x[3] - x[2]) * q;
  }
};

struct MilsteinBackward {  // gf = gy1 * dt, gg = gy1 * (w - q), ggb = gy1 * q     x = gy1
  static constexpr int NI = 1, NO = 3, ZMASK = 6;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    static_assert(NOISE, "Milstein has no noise-free form");
    const T w = k.s * z, q = k.c * (w * w - k.ad);
    o[0] = x[0] * k.dt;
    o[1] = x[0] * (w - q);
    o[2] = x[0] * q;
  }
};

// one lane's vector of the outputs in M: formula on the loaded packs, 16-byte stores
template <typename T, bool NOISE, class Op, int M>
__device__ __forceinline__ void store_packs(const Pack<T, true> (&X)[Op::NI], const T (&z)[Block<T>::W], const Coef<T>& k,
                                            T* const (&out)[Op::NO], int64_t j) {
  if (!M) return;
  Pack<T, true> O[Op::NO];
#pragma unroll
  for (int v = 0; v < Block<T>::W; ++v) {
    T x[Op::NI], o[Op::NO];
#pragma unroll
    for (int i = 0; i < Op::NI; ++i) x[i] = X[i].v[v];
    Op::template apply<NOISE>(x, z[v], k, o);
#pragma unroll
    for (int i = 0; i < Op::NO; ++i) O[i].v[v] = o[i];
  }
#pragma unroll
  for (int i = 0; i < Op::NO; ++i)
    if (M >> i & 1) O[i].store(out[i], j);
}

// The lane loop of every step kernel.  MASK = the outputs to write (bit i: a.out[i]); the others may be null and are never touched: their
// stores, and the generator when no written output depends on Z, are compiled out.  A lane loads all its operands before the generator
// runs (vector path) and before it stores anything, so an output may alias an input; the outputs that do not depend on Z are stored
// ahead of the generator.
template <typename T, bool VEC, bool NOISE, class Op, int MASK>
__global__ __launch_bounds__(kBlock) void xde_sde_step_kernel(SdeArgs a) {
  constexpr int W = Block<T>::W, NI = Op::NI, NO = Op::NO;
  constexpr bool Z = NOISE && (MASK & Op::ZMASK) != 0;
  constexpr int EARLY = Z ? (MASK & ~Op::ZMASK) : 0;
  using P = Pack<T, true>;
  static_assert(P::W == W, "one Philox call per 16-byte vector");
  const int64_t n = a.n, nblk = a.nblk;  // (the scalars are read at entry, in one fetch with dt and s; the pointers where the loop uses them)
  const T dt = T(a.dt);
  const Coef<T> k{dt, T(a.s), T(a.c), abs_(dt)};
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < nblk; j += stride) {
    const int64_t e0 = j * W;
    T z[W] = {};
    const T* in[NI];
    T* out[NO];
#pragma unroll
    for (int i = 0; i < NI; ++i) in[i] = static_cast<const T*>(a.in[i]);
#pragma unroll
    for (int i = 0; i < NO; ++i) out[i] = static_cast<T*>(a.out[i]);
    if (VEC && e0 + W <= n) {
      P X[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) X[i] = P::load(in[i], j);
      store_packs<T, NOISE, Op, EARLY>(X, z, k, out, j);
      if (Z) normals(uint64_t(j), a.k, a.key0, a.key1, z);
      store_packs<T, NOISE, Op, MASK & ~EARLY>(X, z, k, out, j);
    } else {
      if (Z) normals(uint64_t(j), a.k, a.key0, a.key1, z);
#pragma unroll
      for (int v = 0; v < W; ++v) {
        const int64_t e = e0 + v;
        if (e < n) {
          T x[NI], o[NO];
#pragma unroll
          for (int i = 0; i < NI; ++i) x[i] = in[i][e];
          Op::template apply<NOISE>(x, z[v], k, o);
#pragma unroll
          for (int i = 0; i < NO; ++i)
            if (MASK >> i & 1) out[i][e] = o[i];
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
      uint32_t* o = static_cast<uint32_t*>(a.out[0]);
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (e0 + v < a.n) o[e0 + v] = x.w[v];
    } else {
      T z[Block<T>::W];
      normals(uint64_t(j), a.k, a.key0, a.key1, z);
      T* o = static_cast<T*>(a.out[0]);
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

SdeArgs make_args(int64_t n, int W, double dt, double s, double c, uint64_t seed, int64_t k) {
  SdeArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.nblk = (n + W - 1) / W;
  a.dt = dt;
  a.s = s;
  a.c = c;
  a.key0 = uint32_t(seed);
  a.key1 = uint32_t(seed >> 32);
  a.k = uint32_t(k);
  return a;
}

// runtime output mask -> the kernel compiled for it (masks 1 .. 2^NO - 1)
template <typename T, bool VEC, bool NOISE, class Op, int MASK = 1>
void launch_masked(int mask, const SdeArgs& a, dim3 gr, hipStream_t st, ProfScope& prof) {
  if (mask == MASK) XDE_LAUNCH((xde_sde_step_kernel<T, VEC, NOISE, Op, MASK>), gr, dim3(kBlock), st, prof, a);
  else if constexpr (MASK + 1 < (1 << Op::NO)) launch_masked<T, VEC, NOISE, Op, MASK + 1>(mask, a, gr, st, prof);
}

// The host side of every step entry point: checks in the order null pointers, n / dtype / k, alignment; then nothing to do; then one
// launch.  A backward (`backward`, with `cotangent` the name of its single input in the error text) may leave outputs null: they are
// skipped; a forward requires every pointer.  Profiled under `kid` with the bytes the launch moves: every input once, every written
// output once.
template <class Op, bool NOISE = true>
int sde_launch(const char* who, int kid, bool backward, const char* cotangent, void* const (&outs)[Op::NO],
               const void* const (&ins)[Op::NI], int64_t n, double dt, double s, double c, uint64_t seed, int64_t k, int dtype, void* stream) {
  const void* ptrs[Op::NO + Op::NI];
  int mask = 0, written = 0;
  bool null = false;
  for (int i = 0; i < Op::NO; ++i) {
    ptrs[i] = outs[i];
    if (outs[i]) {
      mask |= 1 << i;
      ++written;
    } else if (!backward) {
      null = true;
    }
  }
  for (int i = 0; i < Op::NI; ++i) {
    ptrs[Op::NO + i] = ins[i];
    if (!ins[i]) null = true;
  }
  if (null) return fail(XDE_EBADARG, std::string(who) + ": null pointer" + (backward ? " (" + std::string(cotangent) + ")" : ""));
  if (int rc = check_common(who, n, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  bool vec;
  if (int rc = check_operands(who, ptrs, Op::NO + Op::NI, esz, &vec)) return rc;
  if (n == 0 || !mask) return XDE_OK;
  SdeArgs a = make_args(n, dtype == XDE_F32 ? 4 : 2, dt, s, c, seed, k);
  for (int i = 0; i < Op::NO; ++i) a.out[i] = outs[i];
  for (int i = 0; i < Op::NI; ++i) a.in[i] = ins[i];
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope prof(kid, double(Op::NI + written) * double(n) * double(esz));
  const dim3 gr = grid_for(a.nblk);
  if (dtype == XDE_F32) vec ? launch_masked<float, true, NOISE, Op>(mask, a, gr, st, prof) : launch_masked<float, false, NOISE, Op>(mask, a, gr, st, prof);
  else vec ? launch_masked<double, true, NOISE, Op>(mask, a, gr, st, prof) : launch_masked<double, false, NOISE, Op>(mask, a, gr, st, prof);
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

}  // namespace

extern "C" {

// (profiled under the fixed-step fuse id: the kernel-id list of xde_hip.h is part of the frozen ABI — an EM step is the SDE's fuse)
int xde_sde_em_step(void* y1, const void* y0, const void* f, const void* g, int64_t n, double dt, double s, uint64_t seed,
                    int64_t k, int dtype, void* stream) {
  return sde_launch<EmStep>("xde_sde_em_step", XDE_KID_COMBINE_FUSE, false, nullptr, {y1}, {y0, f, g}, n, dt, s, 0.0, seed, k, dtype, stream);
}

int xde_sde_em_backward(void* gf, void* gg, const void* gy1, int64_t n, double dt, double s, uint64_t seed, int64_t k, int dtype,
                        void* stream) {
  return sde_launch<EmBackward>("xde_sde_em_backward", XDE_KID_COMBINE, true, "gy1", {gf, gg}, {gy1}, n, dt, s, 0.0, seed, k, dtype, stream);
}

// Milstein (derivative-free, Ito, diagonal noise): support point, step, and their backwards.
// (the support point is a stage input: the stage combines' id)
int xde_sde_milstein_support(void* yb, const void* y0, const void* f, const void* g, int64_t n, double dt, double s, int dtype,
                             void* stream) {
  return sde_launch<EmStep, false>("xde_sde_milstein_support", XDE_KID_COMBINE, false, nullptr, {yb}, {y0, f, g}, n, dt, s, 0.0, 0, 0, dtype,
                                   stream);
}

int xde_sde_milstein_support_backward(void* gf, void* gg, const void* gyb, int64_t n, double dt, double s, int dtype, void* stream) {
  return sde_launch<EmBackward, false>("xde_sde_milstein_support_backward", XDE_KID_COMBINE, true, "gyb", {gf, gg}, {gyb}, n, dt, s, 0.0, 0, 0,
                                       dtype, stream);
}

// (the SDE's fuse, as the EM step)
int xde_sde_milstein_step(void* y1, const void* y0, const void* f, const void* g, const void* gb, int64_t n, double dt, double s,
                          double c, uint64_t seed, int64_t k, int dtype, void* stream) {
  return sde_launch<MilsteinStep>("xde_sde_milstein_step", XDE_KID_COMBINE_FUSE, false, nullptr, {y1}, {y0, f, g, gb}, n, dt, s, c, seed, k,
                                  dtype, stream);
}

int xde_sde_milstein_backward(void* gf, void* gg, void* ggb, const void* gy1, int64_t n, double dt, double s, double c, uint64_t seed,
                              int64_t k, int dtype, void* stream) {
  return sde_launch<MilsteinBackward>("xde_sde_milstein_backward", XDE_KID_COMBINE, true, "gy1", {gf, gg, ggb}, {gy1}, n, dt, s, c, seed, k,
                                      dtype, stream);
}

int xde_sde_noise(void* out, int64_t n, uint64_t seed, int64_t k, int mode, int dtype, void* stream) {
  if (!out) return fail(XDE_EBADARG, "xde_sde_noise: null pointer");
  if (mode != XDE_NOISE_NORMAL && mode != XDE_NOISE_BITS) return fail(XDE_EBADARG, "xde_sde_noise: bad mode");
  if (int rc = check_common("xde_sde_noise", n, k, dtype)) return rc;
  const bool bits = mode == XDE_NOISE_BITS;
  const size_t esz = bits ? 4 : (dtype == XDE_F32 ? 4 : 8);
  if (!aligned_to(out, esz)) return fail(XDE_EBADARG, "xde_sde_noise: output not aligned to its element type");
  if (n == 0) return XDE_OK;
  SdeArgs a = make_args(n, bits ? 4 : (dtype == XDE_F32 ? 4 : 2), 0.0, 0.0, 0.0, seed, k);
  a.out[0] = out;
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
