// libxde_hip.so — Ito Euler-Maruyama, Milstein and SRK (strong order 1.5) steps and Stratonovich reversible Heun steps with in-kernel Brownian increments (C ABI:
// include/xde_hip_sde.h; host: paddlexde_amd/solver/base_fixed_solver.py).
//
// One lane serves one Philox4x32-10 call per draw: 4 fp32 or 2 fp64 elements, i.e. exactly one 16-byte vector of every operand.  The
// EM forward reads y0, f, g once and writes y1 once (4 n elt bytes), the Milstein forward reads gb as well (5 n); the noise lives in
// registers only, and the backward regenerates it from the same counter instead of reading it back.  The SRK kernels draw twice per
// lane: Z from the counter's last word 0 (the draw of EM and Milstein) and V from last word 1.
//
// The file is three layers.  Each formula is written once, as a per-element functor (EmStep, EmBackward, MilsteinStep,
// MilsteinBackward, SrkStage1, SrkStage2, SrkStep and their backwards, RheunPredict, RheunCorrect, RheunAdjointStage, RheunAdjointStep); the Milstein support point is the EM functors with
// NOISE = false (s in the place of s * Z, the generator compiled out).  One kernel, xde_sde_step_kernel, owns the lane loop for all of them: a lane whose block runs past n (the tail), or any launch
// whose pointers are not all 16-byte aligned, takes the scalar path with the same bits; grid-stride over at most grid_cap() workgroups
// of kBlock.  One host launcher, sde_launch, owns the argument checks, the profiling scope and the dtype x alignment x output-mask
// dispatch; the entry points only name their operands.  xde_sde_noise, the generator alone, keeps a kernel and a host body of its own:
// it is what the tests read Z back with, an independent statement of which counter serves which element.
// Built with -ffp-contract=off like the rest of the library; the math functions are the precise ones (no fast-math, no __sinf).

#include "xde_common.hpp"
#include "xde_hip_sde.h"
#include "xde_sde_device.hpp"

using namespace xde;

namespace {

// (the generator — philox, Block, box_muller, normals — lives in xde_sde_device.hpp: xde_kl.hip draws the same Z)

struct SdeArgs {
  void* out[6];       // y1 | gf, gg, ggb | Y2, G2, G3 | G4 | ga1, ga2, gb1 .. gb4 | the noise kernel's output
  const void* in[7];  // y0, f, g, gb | gy1 | y0, a1, a2, b1 .. b4
  int64_t n;          // elements (bits mode: words)
  int64_t nblk;       // Philox calls = lanes of work
  double dt, s, c, c3;
  uint32_t key0, key1, k;
  uint32_t draw;  // the noise kernel's counter word 3 (the step kernels draw 0, and 1 as well where the formula takes V)
};

// the step's scalars in the state dtype; ad = |dt|
template <typename T> struct Coef {
  T dt, s, c, ad, c3;
};

// what the formulas below share unless they say otherwise: one draw (Z), and every output skippable on its own
struct OneDraw {
  static constexpr int DRAWS = 1;
  static constexpr bool ok(int) { return true; }
};

// The formulas, one element each: (inputs x, the element's Z, the scalars) -> outputs o, in the written op order.  NI inputs, NO
// outputs, and ZMASK = the outputs that depend on Z (bit i: output i).  NOISE = false puts s in the place of s * Z.
struct EmStep : OneDraw {  // y1 = (y0 + f * dt) + g * (s * Z)        x = y0, f, g
  static constexpr int NI = 3, NO = 1, ZMASK = 1;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    o[0] = (x[0] + x[1] * k.dt) + x[2] * (NOISE ? k.s * z : k.s);
  }
};

struct EmBackward : OneDraw {  // gf = gy1 * dt, gg = gy1 * (s * Z)     x = gy1
  static constexpr int NI = 1, NO = 2, ZMASK = 2;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    o[0] = x[0] * k.dt;
    o[1] = x[0] * (NOISE ? k.s * z : k.s);
  }
};

struct MilsteinStep : OneDraw {  // w = s * Z, q = c * (w * w - |dt|), y1 = ((y0 + f * dt) + g * w) + (gb - g) * q        x = y0, f, g, gb
  static constexpr int NI = 4, NO = 1, ZMASK = 1;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    static_assert(NOISE, "Milstein has no noise-free form");
    const T w = k.s * z, q = k.c * (w * w - k.ad);
    o[0] = ((x[0] + x[1] * k.dt) + x[2] * w) + (x[3] - x[2]) * q;
  }
};

struct MilsteinBackward : OneDraw {  // gf = gy1 * dt, gg = gy1 * (w - q), ggb = gy1 * q     x = gy1
  static constexpr int NI = 1, NO = 3, ZMASK = 6;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    static_assert(NOISE, "Milstein has no noise-free form");
    const T w = k.s * z, q = k.c * (w * w - k.ad);
    o[0] = x[0] * k.dt;
    o[1] = x[0] * (w - q);
    o[2] = x[0] * q;
  }
};

// SRK (Roessler's SRI1W1): the constants are literals rounded to the state dtype, the random quantities are written once
template <typename T> struct SrkK {
  static constexpr T r3 = T(0.57735026918962576451L);  // 1 / sqrt(3)
  static constexpr T third = T(0.33333333333333333333L), two3 = T(0.66666666666666666667L);
  static constexpr T four3 = T(1.3333333333333333333L), five3 = T(1.6666666666666666667L);
};

// w = s * Z, p = 0.5 * (w + (s * V) * r3)
template <typename T> __device__ __forceinline__ void srk_wp(T z, T v, const Coef<T>& k, T& w, T& p) {
  w = k.s * z;
  p = T(0.5) * (w + (k.s * v) * SrkK<T>::r3);
}

// the step's weights: q = c * (w * w - a), u = c3 * ((w * w - 3 * a) * w),
// e1 = ((-w - q) + 2 * p) - 2 * u, e2 = 4/3 * ((w + q) - p) + 5/3 * u, e3 = 2/3 * ((w - p) - u) - 1/3 * q, e4 = u
template <typename T> __device__ __forceinline__ void srk_weights(T z, T v, const Coef<T>& k, T (&e)[4]) {
  using K = SrkK<T>;
  T w, p;
  srk_wp(z, v, k, w, p);
  const T ww = w * w;
  const T q = k.c * (ww - k.ad), u = k.c3 * ((ww - T(3) * k.ad) * w);
  e[0] = ((-w - q) + T(2) * p) - T(2) * u;
  e[1] = K::four3 * ((w + q) - p) + K::five3 * u;
  e[2] = K::two3 * ((w - p) - u) - K::third * q;
  e[3] = u;
}

struct SrkStage1 {  // Y2 = (y + a1 * (0.75 * dt)) + b1 * (1.5 * p), G2 = (y + a1 * (0.25 * dt)) + b1 * (0.5 * s), G3 = (y + a1 * dt) - b1 * s
  static constexpr int NI = 3, NO = 3, ZMASK = 1, DRAWS = 2;  // x = y, a1, b1
  static constexpr bool ok(int m) { return m == 7; }
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, T v, const Coef<T>& k, T (&o)[NO]) {
    static_assert(NOISE, "SRK stage 1 has no noise-free form");
    T w, p;
    srk_wp(z, v, k, w, p);
    o[0] = (x[0] + x[1] * (T(0.75) * k.dt)) + x[2] * (T(1.5) * p);
    o[1] = (x[0] + x[1] * (T(0.25) * k.dt)) + x[2] * (T(0.5) * k.s);
    o[2] = (x[0] + x[1] * k.dt) - x[2] * k.s;
  }
};

struct SrkStage1Backward {  // gy = (gY2 + gG2) + gG3, ga1 = (gY2 * (0.75 * dt) + gG2 * (0.25 * dt)) + gG3 * dt,
                            // gb1 = (gY2 * (1.5 * p) + gG2 * (0.5 * s)) - gG3 * s                              x = gY2, gG2, gG3
  static constexpr int NI = 3, NO = 3, ZMASK = 4, DRAWS = 2;
  static constexpr bool ok(int) { return true; }  // gy | ga1 | gb1: a group each
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, T v, const Coef<T>& k, T (&o)[NO]) {
    static_assert(NOISE, "SRK stage 1 has no noise-free form");
    T w, p;
    srk_wp(z, v, k, w, p);
    o[0] = (x[0] + x[1]) + x[2];
    o[1] = (x[0] * (T(0.75) * k.dt) + x[1] * (T(0.25) * k.dt)) + x[2] * k.dt;
    o[2] = (x[0] * (T(1.5) * p) + x[1] * (T(0.5) * k.s)) - x[2] * k.s;
  }
};

struct SrkStage2 : OneDraw {  // G4 = (y + a1 * (0.25 * dt)) + ((b1 * -5 + b2 * 3) + b3 * 0.5) * s        x = y, a1, b1, b2, b3
  static constexpr int NI = 5, NO = 1, ZMASK = 0;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T, const Coef<T>& k, T (&o)[NO]) {
    static_assert(!NOISE, "SRK stage 2 takes no noise");
    o[0] = (x[0] + x[1] * (T(0.25) * k.dt)) + ((x[2] * T(-5) + x[3] * T(3)) + x[4] * T(0.5)) * k.s;
  }
};

struct SrkStage2Backward {  // ga1 = gG4 * (0.25 * dt), gb1 = gG4 * (-5 * s), gb2 = gG4 * (3 * s), gb3 = gG4 * (0.5 * s)        x = gG4
  static constexpr int NI = 1, NO = 4, ZMASK = 0, DRAWS = 1;
  static constexpr bool ok(int m) { return m == 1 || m == 14 || m == 15; }  // the drift group (ga1) | the diffusion group (gb1 .. gb3)
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T, const Coef<T>& k, T (&o)[NO]) {
    static_assert(!NOISE, "SRK stage 2 takes no noise");
    o[0] = x[0] * (T(0.25) * k.dt);
    o[1] = x[0] * (T(-5) * k.s);
    o[2] = x[0] * (T(3) * k.s);
    o[3] = x[0] * (T(0.5) * k.s);
  }
};

struct SrkStep {  // y1 = ((((y + (1/3 * a1 + 2/3 * a2) * dt) + b1 * e1) + b2 * e2) + b3 * e3) + b4 * e4        x = y, a1, a2, b1 .. b4
  static constexpr int NI = 7, NO = 1, ZMASK = 1, DRAWS = 2;
  static constexpr bool ok(int) { return true; }
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, T v, const Coef<T>& k, T (&o)[NO]) {
    static_assert(NOISE, "the SRK step has no noise-free form");
    using K = SrkK<T>;
    T e[4];
    srk_weights(z, v, k, e);
    o[0] = ((((x[0] + (K::third * x[1] + K::two3 * x[2]) * k.dt) + x[3] * e[0]) + x[4] * e[1]) + x[5] * e[2]) + x[6] * e[3];
  }
};

struct SrkStepBackward {  // ga1 = gy1 * (1/3 * dt), ga2 = gy1 * (2/3 * dt), gb_i = gy1 * e_i        x = gy1
  static constexpr int NI = 1, NO = 6, ZMASK = 60, DRAWS = 2;
  static constexpr bool ok(int m) { return m == 3 || m == 60 || m == 63; }  // the drift group (ga1, ga2) | the diffusion group (gb1 .. gb4)
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, T v, const Coef<T>& k, T (&o)[NO]) {
    static_assert(NOISE, "the SRK step has no noise-free form");
    using K = SrkK<T>;
    T e[4];
    srk_weights(z, v, k, e);
    o[0] = x[0] * (K::third * k.dt);
    o[1] = x[0] * (K::two3 * k.dt);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[2 + i] = x[0] * e[i];
  }
};

// REVERSIBLE HEUN (Stratonovich, diagonal noise; include/xde_hip_sde.h).  The entry points hand dt and s over already multiplied by
// the direction (+1 / -1: exact), and take the NOISE = false form (s in the place of s * Z, the generator compiled out) where s == 0.
struct RheunPredict : OneDraw {  // yh1 = (((y0 + y0) - yh0) + f0 * dt) + g0 * w        x = y0, yh0, f0, g0
  static constexpr int NI = 4, NO = 1, ZMASK = 1;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    const T w = NOISE ? k.s * z : k.s;
    o[0] = (((x[0] + x[0]) - x[1]) + x[2] * k.dt) + x[3] * w;
  }
};

struct RheunCorrect : OneDraw {  // y1 = (y0 + (f0 + f1) * (0.5 * dt)) + (g0 + g1) * (0.5 * w)        x = y0, f0, f1, g0, g1
  static constexpr int NI = 5, NO = 1, ZMASK = 1;
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    const T w = NOISE ? k.s * z : k.s;
    o[0] = (x[0] + (x[1] + x[2]) * (T(0.5) * k.dt)) + (x[3] + x[4]) * (T(0.5) * w);
  }
};

// the cotangent sweep's two launches; FIRST = the first backward step, whose af1, ag1 (stage) or ayh1 (step) are zero and not read
template <bool FIRST> struct RheunAdjointStage {  // bf = af1 + ay1 * (0.5 * dt), bg = ag1 + ay1 * (0.5 * w)        x = ay1, af1, ag1
  static constexpr int NI = FIRST ? 1 : 3, NO = 2, ZMASK = 2, DRAWS = 1;
  static constexpr bool ok(int m) { return m == 3; }
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    const T w = NOISE ? k.s * z : k.s;
    const T hf = x[0] * (T(0.5) * k.dt), hg = x[0] * (T(0.5) * w);
    if constexpr (FIRST) {
      o[0] = hf;
      o[1] = hg;
    } else {
      o[0] = x[1] + hf;
      o[1] = x[2] + hg;
    }
  }
};

template <bool FIRST> struct RheunAdjointStep {  // A = ayh1 + v, ay0 = ay1 + (A + A), ayh0 = -A, af0 = ay1 * (0.5 * dt) + A * dt,
                                                 // ag0 = ay1 * (0.5 * w) + A * w        x = ay1, v, ayh1
  static constexpr int NI = FIRST ? 2 : 3, NO = 4, ZMASK = 8, DRAWS = 1;
  static constexpr bool ok(int m) { return m == 15; }
  template <bool NOISE, typename T> __device__ static void apply(const T (&x)[NI], T z, const Coef<T>& k, T (&o)[NO]) {
    const T w = NOISE ? k.s * z : k.s;
    T A = x[1];
    if constexpr (!FIRST) A = x[2] + x[1];
    o[0] = x[0] + (A + A);
    o[1] = -A;
    o[2] = x[0] * (T(0.5) * k.dt) + A * k.dt;
    o[3] = x[0] * (T(0.5) * w) + A * w;
  }
};

// one element of a formula: with both draws where it takes V
template <bool NOISE, class Op, typename T>
__device__ __forceinline__ void apply_op(const T (&x)[Op::NI], T z, T v, const Coef<T>& k, T (&o)[Op::NO]) {
  if constexpr (Op::DRAWS == 2) Op::template apply<NOISE>(x, z, v, k, o);
  else Op::template apply<NOISE>(x, z, k, o);
}

// one lane's vector of the outputs in M: formula on the loaded packs, 16-byte stores
template <typename T, bool NOISE, class Op, int M>
__device__ __forceinline__ void store_packs(const Pack<T, true> (&X)[Op::NI], const T (&z)[Block<T>::W], const T (&zv)[Block<T>::W],
                                            const Coef<T>& k, T* const (&out)[Op::NO], int64_t j) {
  if (!M) return;
  Pack<T, true> O[Op::NO];
#pragma unroll
  for (int v = 0; v < Block<T>::W; ++v) {
    T x[Op::NI], o[Op::NO];
#pragma unroll
    for (int i = 0; i < Op::NI; ++i) x[i] = X[i].v[v];
    apply_op<NOISE, Op>(x, z[v], zv[v], k, o);
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
  const Coef<T> k{dt, T(a.s), T(a.c), abs_(dt), T(a.c3)};
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < nblk; j += stride) {
    const int64_t e0 = j * W;
    T z[W] = {}, zv[W] = {};
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
      store_packs<T, NOISE, Op, EARLY>(X, z, zv, k, out, j);
      if (Z) normals(uint64_t(j), a.k, a.key0, a.key1, 0u, z);
      if (Z && Op::DRAWS == 2) normals(uint64_t(j), a.k, a.key0, a.key1, 1u, zv);
      store_packs<T, NOISE, Op, MASK & ~EARLY>(X, z, zv, k, out, j);
    } else {
      if (Z) normals(uint64_t(j), a.k, a.key0, a.key1, 0u, z);
      if (Z && Op::DRAWS == 2) normals(uint64_t(j), a.k, a.key0, a.key1, 1u, zv);
#pragma unroll
      for (int v = 0; v < W; ++v) {
        const int64_t e = e0 + v;
        if (e < n) {
          T x[NI], o[NO];
#pragma unroll
          for (int i = 0; i < NI; ++i) x[i] = in[i][e];
          apply_op<NOISE, Op>(x, z[v], zv[v], k, o);
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
      const Words x = philox(uint64_t(j), a.k, a.key0, a.key1, a.draw);
      uint32_t* o = static_cast<uint32_t*>(a.out[0]);
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (e0 + v < a.n) o[e0 + v] = x.w[v];
    } else {
      T z[Block<T>::W];
      normals(uint64_t(j), a.k, a.key0, a.key1, a.draw, z);
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

SdeArgs make_args(int64_t n, int W, double dt, double s, double c, double c3, uint64_t seed, int64_t k) {
  SdeArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.nblk = (n + W - 1) / W;
  a.dt = dt;
  a.s = s;
  a.c = c;
  a.c3 = c3;
  a.key0 = uint32_t(seed);
  a.key1 = uint32_t(seed >> 32);
  a.k = uint32_t(k);
  return a;
}

// runtime output mask -> the kernel compiled for it (the masks 1 .. 2^NO - 1 that Op::ok admits: every one, or whole groups only)
template <typename T, bool VEC, bool NOISE, class Op, int MASK = 1>
void launch_masked(int mask, const SdeArgs& a, dim3 gr, hipStream_t st, ProfScope& prof) {
  if constexpr (Op::ok(MASK)) {
    if (mask == MASK) {
      XDE_LAUNCH((xde_sde_step_kernel<T, VEC, NOISE, Op, MASK>), gr, dim3(kBlock), st, prof, a);
      return;
    }
  }
  if constexpr (MASK + 1 < (1 << Op::NO)) launch_masked<T, VEC, NOISE, Op, MASK + 1>(mask, a, gr, st, prof);
}

// The host side of every step entry point: checks in the order null pointers, n / dtype / k, alignment; then nothing to do; then one
// launch.  A backward (`backward`, with `cotangent` the name of its input(s) in the error text) may leave outputs null: they are
// skipped — one by one, or where the formula groups them (Op::ok) a whole group at a time, and a group given in part is refused with
// the null pointers; a forward requires every pointer.  Profiled under `kid` with the bytes the launch moves: every input once, every
// written output once.
template <class Op, bool NOISE = true>
int sde_launch(const char* who, int kid, bool backward, const char* cotangent, void* const (&outs)[Op::NO],
               const void* const (&ins)[Op::NI], int64_t n, double dt, double s, double c, double c3, uint64_t seed, int64_t k, int dtype,
               void* stream) {
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
  if (mask && !Op::ok(mask)) return fail(XDE_EBADARG, std::string(who) + ": the outputs of a group are given or skipped together");
  if (int rc = check_common(who, n, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8;
  bool vec;
  if (int rc = check_operands(who, ptrs, Op::NO + Op::NI, esz, &vec)) return rc;
  if (n == 0 || !mask) return XDE_OK;
  SdeArgs a = make_args(n, dtype == XDE_F32 ? 4 : 2, dt, s, c, c3, seed, k);
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

// The host side of the reversible Heun entry points: the direction first (+1 / -1; it multiplies dt and s, exactly), then sde_launch —
// the form without the generator where s == 0 (w = s there: a zero-length step adds exact zeros).
template <class Op>
int rheun_launch(const char* who, int kid, void* const (&outs)[Op::NO], const void* const (&ins)[Op::NI], int64_t n, double dt, double s,
                 int direction, uint64_t seed, int64_t k, int dtype, void* stream) {
  if (direction != 1 && direction != -1) return fail(XDE_EBADARG, std::string(who) + ": direction must be +1 or -1");
  const double d = direction;
  if (s != 0.0) return sde_launch<Op>(who, kid, false, nullptr, outs, ins, n, d * dt, d * s, 0.0, 0.0, seed, k, dtype, stream);
  return sde_launch<Op, false>(who, kid, false, nullptr, outs, ins, n, d * dt, d * s, 0.0, 0.0, seed, k, dtype, stream);
}

}  // namespace

extern "C" {

// (profiled under the fixed-step fuse id: the kernel-id list of xde_hip.h is part of the frozen ABI — an EM step is the SDE's fuse)
int xde_sde_em_step(void* y1, const void* y0, const void* f, const void* g, int64_t n, double dt, double s, uint64_t seed,
                    int64_t k, int dtype, void* stream) {
  return sde_launch<EmStep>("xde_sde_em_step", XDE_KID_COMBINE_FUSE, false, nullptr, {y1}, {y0, f, g}, n, dt, s, 0.0, 0.0, seed, k, dtype, stream);
}

int xde_sde_em_backward(void* gf, void* gg, const void* gy1, int64_t n, double dt, double s, uint64_t seed, int64_t k, int dtype,
                        void* stream) {
  return sde_launch<EmBackward>("xde_sde_em_backward", XDE_KID_COMBINE, true, "gy1", {gf, gg}, {gy1}, n, dt, s, 0.0, 0.0, seed, k, dtype, stream);
}

// Milstein (derivative-free, Ito, diagonal noise): support point, step, and their backwards.
// (the support point is a stage input: the stage combines' id)
int xde_sde_milstein_support(void* yb, const void* y0, const void* f, const void* g, int64_t n, double dt, double s, int dtype,
                             void* stream) {
  return sde_launch<EmStep, false>("xde_sde_milstein_support", XDE_KID_COMBINE, false, nullptr, {yb}, {y0, f, g}, n, dt, s, 0.0, 0.0, 0, 0, dtype,
                                   stream);
}

int xde_sde_milstein_support_backward(void* gf, void* gg, const void* gyb, int64_t n, double dt, double s, int dtype, void* stream) {
  return sde_launch<EmBackward, false>("xde_sde_milstein_support_backward", XDE_KID_COMBINE, true, "gyb", {gf, gg}, {gyb}, n, dt, s, 0.0, 0.0, 0, 0,
                                       dtype, stream);
}

// (the SDE's fuse, as the EM step)
int xde_sde_milstein_step(void* y1, const void* y0, const void* f, const void* g, const void* gb, int64_t n, double dt, double s,
                          double c, uint64_t seed, int64_t k, int dtype, void* stream) {
  return sde_launch<MilsteinStep>("xde_sde_milstein_step", XDE_KID_COMBINE_FUSE, false, nullptr, {y1}, {y0, f, g, gb}, n, dt, s, c, 0.0, seed, k,
                                  dtype, stream);
}

int xde_sde_milstein_backward(void* gf, void* gg, void* ggb, const void* gy1, int64_t n, double dt, double s, double c, uint64_t seed,
                              int64_t k, int dtype, void* stream) {
  return sde_launch<MilsteinBackward>("xde_sde_milstein_backward", XDE_KID_COMBINE, true, "gy1", {gf, gg, ggb}, {gy1}, n, dt, s, c, 0.0, seed, k,
                                      dtype, stream);
}

// SRK (Roessler's SRI1W1, Ito, diagonal noise): three forward launches and their backwards.
// (stage inputs: the stage combines' id)
int xde_sde_srk_stage1(void* Y2, void* G2, void* G3, const void* y0, const void* a1, const void* b1, int64_t n, double dt, double s,
                       uint64_t seed, int64_t k, int dtype, void* stream) {
  return sde_launch<SrkStage1>("xde_sde_srk_stage1", XDE_KID_COMBINE, false, nullptr, {Y2, G2, G3}, {y0, a1, b1}, n, dt, s, 0.0, 0.0, seed, k,
                               dtype, stream);
}

int xde_sde_srk_stage2(void* G4, const void* y0, const void* a1, const void* b1, const void* b2, const void* b3, int64_t n, double dt,
                       double s, int dtype, void* stream) {
  return sde_launch<SrkStage2, false>("xde_sde_srk_stage2", XDE_KID_COMBINE, false, nullptr, {G4}, {y0, a1, b1, b2, b3}, n, dt, s, 0.0, 0.0, 0,
                                      0, dtype, stream);
}

// (the SDE's fuse, as the EM step)
int xde_sde_srk_step(void* y1, const void* y0, const void* a1, const void* a2, const void* b1, const void* b2, const void* b3,
                     const void* b4, int64_t n, double dt, double s, double c, double c3, uint64_t seed, int64_t k, int dtype,
                     void* stream) {
  return sde_launch<SrkStep>("xde_sde_srk_step", XDE_KID_COMBINE_FUSE, false, nullptr, {y1}, {y0, a1, a2, b1, b2, b3, b4}, n, dt, s, c, c3,
                             seed, k, dtype, stream);
}

int xde_sde_srk_stage1_backward(void* gy, void* ga1, void* gb1, const void* gY2, const void* gG2, const void* gG3, int64_t n, double dt,
                                double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  return sde_launch<SrkStage1Backward>("xde_sde_srk_stage1_backward", XDE_KID_COMBINE, true, "gY2, gG2, gG3", {gy, ga1, gb1},
                                       {gY2, gG2, gG3}, n, dt, s, 0.0, 0.0, seed, k, dtype, stream);
}

int xde_sde_srk_stage2_backward(void* ga1, void* gb1, void* gb2, void* gb3, const void* gG4, int64_t n, double dt, double s, int dtype,
                                void* stream) {
  return sde_launch<SrkStage2Backward, false>("xde_sde_srk_stage2_backward", XDE_KID_COMBINE, true, "gG4", {ga1, gb1, gb2, gb3}, {gG4}, n,
                                              dt, s, 0.0, 0.0, 0, 0, dtype, stream);
}

int xde_sde_srk_step_backward(void* ga1, void* ga2, void* gb1, void* gb2, void* gb3, void* gb4, const void* gy1, int64_t n, double dt,
                              double s, double c, double c3, uint64_t seed, int64_t k, int dtype, void* stream) {
  return sde_launch<SrkStepBackward>("xde_sde_srk_step_backward", XDE_KID_COMBINE, true, "gy1", {ga1, ga2, gb1, gb2, gb3, gb4}, {gy1}, n,
                                     dt, s, c, c3, seed, k, dtype, stream);
}

// REVERSIBLE HEUN (Stratonovich, diagonal noise): predict, correct, and the cotangent sweep's stage and step.  dt and s go to the
// kernel times the direction; a step with s == 0 takes no noise (rheun_launch: the generator is compiled out of that form).
// (the prediction is a stage input: the stage combines' id)
int xde_sde_rheun_predict(void* yh1, const void* y0, const void* yh0, const void* f0, const void* g0, int64_t n, double dt, double s,
                          int direction, uint64_t seed, int64_t k, int dtype, void* stream) {
  return rheun_launch<RheunPredict>("xde_sde_rheun_predict", XDE_KID_COMBINE, {yh1}, {y0, yh0, f0, g0}, n, dt, s, direction, seed, k, dtype, stream);
}

// (the SDE's fuse, as the EM step)
int xde_sde_rheun_correct(void* y1, const void* y0, const void* f0, const void* f1, const void* g0, const void* g1, int64_t n, double dt,
                          double s, int direction, uint64_t seed, int64_t k, int dtype, void* stream) {
  return rheun_launch<RheunCorrect>("xde_sde_rheun_correct", XDE_KID_COMBINE_FUSE, {y1}, {y0, f0, f1, g0, g1}, n, dt, s, direction, seed, k, dtype,
                                    stream);
}

// (af1 and ag1 null together: the first backward step, which does not read them; one of them null is refused with the null pointers)
int xde_sde_rheun_adjoint_stage(void* bf, void* bg, const void* af1, const void* ag1, const void* ay1, int64_t n, double dt, double s,
                                uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_rheun_adjoint_stage";
  if (!af1 && !ag1) return rheun_launch<RheunAdjointStage<true>>(who, XDE_KID_COMBINE, {bf, bg}, {ay1}, n, dt, s, 1, seed, k, dtype, stream);
  return rheun_launch<RheunAdjointStage<false>>(who, XDE_KID_COMBINE, {bf, bg}, {ay1, af1, ag1}, n, dt, s, 1, seed, k, dtype, stream);
}

// (ayh1 null: the first backward step)
int xde_sde_rheun_adjoint_step(void* ay0, void* ayh0, void* af0, void* ag0, const void* ay1, const void* ayh1, const void* v, int64_t n,
                               double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_rheun_adjoint_step";
  if (!ayh1) return rheun_launch<RheunAdjointStep<true>>(who, XDE_KID_COMBINE, {ay0, ayh0, af0, ag0}, {ay1, v}, n, dt, s, 1, seed, k, dtype, stream);
  return rheun_launch<RheunAdjointStep<false>>(who, XDE_KID_COMBINE, {ay0, ayh0, af0, ag0}, {ay1, v, ayh1}, n, dt, s, 1, seed, k, dtype, stream);
}

}  // extern "C"

namespace {

// the generator alone, at counter word 3 = draw
int noise_launch(const char* who, void* out, int64_t n, uint64_t seed, int64_t k, int draw, int mode, int dtype, void* stream) {
  if (!out) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  if (mode != XDE_NOISE_NORMAL && mode != XDE_NOISE_BITS) return fail(XDE_EBADARG, std::string(who) + ": bad mode");
  if (draw != 0 && draw != 1) return fail(XDE_EBADARG, std::string(who) + ": bad draw (0: Z, 1: V)");
  if (int rc = check_common(who, n, k, dtype)) return rc;
  const bool bits = mode == XDE_NOISE_BITS;
  const size_t esz = bits ? 4 : (dtype == XDE_F32 ? 4 : 8);
  if (!aligned_to(out, esz)) return fail(XDE_EBADARG, std::string(who) + ": output not aligned to its element type");
  if (n == 0) return XDE_OK;
  SdeArgs a = make_args(n, bits ? 4 : (dtype == XDE_F32 ? 4 : 2), 0.0, 0.0, 0.0, 0.0, seed, k);
  a.draw = uint32_t(draw);
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

}  // namespace

extern "C" {

int xde_sde_noise(void* out, int64_t n, uint64_t seed, int64_t k, int mode, int dtype, void* stream) {
  return noise_launch("xde_sde_noise", out, n, seed, k, 0, mode, dtype, stream);
}

int xde_sde_noise_draw(void* out, int64_t n, uint64_t seed, int64_t k, int draw, int mode, int dtype, void* stream) {
  return noise_launch("xde_sde_noise_draw", out, n, seed, k, draw, mode, dtype, stream);
}

}  // extern "C"
