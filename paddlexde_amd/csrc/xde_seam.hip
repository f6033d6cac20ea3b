// libxde_hip.so — the seam between two attempted steps of an FSAL pair as ONE resident launch.  C ABI: include/xde_hip_seam.h.
//
// Phase 1 is xde_errnorm_pre_kernel's pass (same grid, same elements per lane in the same order, same records in the same slots), with the
// y1 and k_last vectors kept in registers.  A grid barrier follows (the ticketed arrival of block_reduce_store, released by its last
// arriver through generation words; bounded poll).  In phase 2 every workgroup reduces the records in the controller's fixed order and
// runs the controller (xde_control_device.hpp: shared with xde_rk_control); workgroup 0 alone publishes; every lane then writes the next
// attempt's first stage input from the registers it carried (accepted) or from the attempt's own (y0, f0) (rejected: the rare path).

#include "xde_common.hpp"
#include "xde_reduce.hpp"
#include "xde_errnorm_device.hpp"
#include "xde_control_device.hpp"
#include "xde_hip_seam.h"

using namespace xde;

namespace {

constexpr int kSeamCap = XDE_SEAM_CAP;
constexpr int kSeamBatch = 4;         // iterations whose loads are requested together (4 arrays x 4 x 16 bytes in flight per lane)
constexpr int kSeamBlocksPerCU = 2;   // the error-norm pass's own geometry: 512 workgroups of 256 lanes on 256 CUs
static_assert(kSeamCap % kSeamBatch == 0, "whole batches");

// Device-resident barrier state, one per control block: a generation word per first-level arrival shard (a 128-byte line each) and the
// tag of the first launch whose barrier expired.  Tags are ctrl->seq + 1 of the launch: strictly increasing, never 0.
struct alignas(128) SeamLine {
  unsigned long long gen;
  unsigned long long pad[15];
};
struct SeamState {
  SeamLine line[kTicketShards];
  SeamLine expired;
};

struct SeamCtrl {
  xde_ctrl_t* ctrl;
  xde_ctrl_params_t p;
  const double* t_span;
  const double* step_t;
  void* t_stage_out;
  xde_ctrl_t* mirror;
  int flags;
};

struct SeamArgs {
  ErrArgs e;           // the error-norm pass's own argument block (e_pre form: k[0] = k_last)
  const void* f0[2];   // the attempt's f0 candidates (rejected: out = y0 + f0 * (a21 dt'))
  void* out;           // may alias e.e_pre: a lane writes only elements it has read
  double a21;
  SeamState* st;
  long long spin_limit;
};

template <typename T, int NORM, bool NT>
__global__ __launch_bounds__(kBlock, kSeamBlocksPerCU) void xde_seam_kernel(SeamArgs s, SeamCtrl tl) {
  __shared__ double seg_val[XDE_MAX_SEG];
  __shared__ double seg_nf[XDE_MAX_SEG];
  __shared__ xde_ctrl_t zs;
  __shared__ TimePrefetch pfs;
  __shared__ xde_ctrl_t sink;                  // where the workgroups that do not publish "write" their block ...
  __shared__ double t_sink[XDE_MAX_STAGE];     // ... and their stage times
  __shared__ int s_expired;
  using P = Pack<T, true>;
  constexpr int W = P::W;
  const ErrArgs& a = s.e;
  const bool pub = blockIdx.x == 0;
  // the control block is fetched into LDS while phase 1 runs; nobody writes it before the barrier
  control_prologue(tl.ctrl, tl.p, tl.t_span, tl.step_t, pub ? tl.mirror : nullptr, tl.flags, &zs, &pfs);

  // ---- phase 1: errnorm_pre_body's pass, one segment, lb = blockIdx.x, nb = gridDim.x ----
  const T* epre = static_cast<const T*>(a.e_pre);
  const T* __restrict__ kl = static_cast<const T*>(a.k[0]);
  const T* __restrict__ y1 = static_cast<const T*>(a.y1);
  const int64_t start = a.map.seg_start[0];
  const int64_t len = a.map.seg_len[0];
  const int64_t nvec = len / W;
  const int64_t vbase = start / W;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  const int64_t b0 = int64_t(blockIdx.x) * kBlock;
  const int64_t i0 = b0 + threadIdx.x;
  const double dtd = __builtin_nontemporal_load(&a.ctrl->dt);
  const int32_t accw = __builtin_nontemporal_load(&a.ctrl->accept);
  unsigned long long prior = 0;
  if (threadIdx.x == 0) prior = __hip_atomic_load(&s.st->expired.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const T rtol = T(a.rtol), atol = T(a.atol);
  const int sel = (a.use_sel && accw) ? 1 : 0;
  const T* __restrict__ y0 = static_cast<const T*>(a.y0[sel]);
  const T c = T(dtd) * T(a.coef[0]);  // `dt * tableau.c_error`
  T acc = T(0);
  int nfw = 0;  // per-wave count (errnorm_pre_body)
  P cy[kSeamCap], ck[kSeamCap];  // the carried vectors: slot j holds vector i0 + j * stride
  auto one = [&](bool on, T e, T y0e, T y1e) {
    T tol = atol + rtol * fmax_(abs_(y0e), abs_(y1e));
    T ar = abs_(e / tol);
    if (on) {
      if (NORM == XDE_NORM_RMS) {
        acc = acc + ar * ar;
      } else {
        acc = (ar != ar || acc != acc) ? (ar != ar ? ar : acc) : (ar > acc ? ar : acc);
      }
    }
    nfw += __popcll(__ballot(on && nonfinite_class(y0e)));
  };
#pragma unroll
  for (int jb = 0; jb < kSeamCap; jb += kSeamBatch) {
    if (b0 + int64_t(jb) * stride < nvec) {  // (workgroup-uniform: some lane of this workgroup has a vector in this batch)
      P ep[kSeamBatch], yv[kSeamBatch];
      // a lane past the end loads the last vector again (in bounds) and does not count it: no load sits behind a divergent branch
#pragma unroll
      for (int u = 0; u < kSeamBatch; ++u) {
        const int64_t i = i0 + int64_t(jb + u) * stride;
        const int64_t ic = vbase + (i < nvec ? i : nvec - 1);
        cy[jb + u] = P::load(y1, ic);
        ep[u] = NT ? P::load_nt(epre, ic) : P::load(epre, ic);
        ck[jb + u] = P::load(kl, ic);
        yv[u] = NT ? P::load_nt(y0, ic) : P::load(y0, ic);
      }
#pragma unroll
      for (int u = 0; u < kSeamBatch; ++u) {
        const bool on = i0 + int64_t(jb + u) * stride < nvec;
#pragma unroll
        for (int w = 0; w < W; ++w) one(on, ep[u].v[w] + ck[jb + u].v[w] * c, yv[u].v[w], cy[jb + u].v[w]);
      }
    }
  }
  // the scalar tail of the segment (len % W elements), by the first workgroup
  const int64_t tj = start + nvec * W + threadIdx.x;
  const bool ton = blockIdx.x == 0 && tj < start + len;
  T ty1 = T(1), tk = T(0);
  if (blockIdx.x == 0) {
    T e = T(0), y0e = T(0);
    if (ton) {
      tk = kl[tj];
      e = epre[tj] + tk * c;
      y0e = y0[tj];
      ty1 = y1[tj];
    }
    if (ton) {
      T tol = atol + rtol * fmax_(abs_(y0e), abs_(ty1));
      T ar = abs_(e / tol);
      if (NORM == XDE_NORM_RMS) acc = acc + ar * ar;
      else acc = (ar != ar || acc != acc) ? (ar != ar ? ar : acc) : (ar > acc ? ar : acc);
    }
    nfw += __popcll(__ballot(ton && nonfinite_class(y0e)));
  }
  const double acc_d = NORM == XDE_NORM_RMS ? 0.0 + double(acc) : double(acc);  // (no 64-iteration flush below kSeamCap iterations)
  const double nf_d = (threadIdx.x & 63) == 0 ? double(nfw) : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.slot->nblocks = gridDim.x;
    a.slot->n_seg = 1;
    a.slot->norm_kind = NORM;
  }
  // the record goes out write-through and drained, then this workgroup's ticket is taken (xde_reduce.hpp)
  const bool last = block_reduce_store<NORM, true>(acc_d, nf_d, a.slot, 0);

  // ---- grid barrier ----
  const unsigned long long tag = (unsigned long long)(zs.seq + 1);  // (zs: visible since the reduction's barriers)
  if (last) {
    // every workgroup has arrived, so every record is in memory: re-arm the arrival counter, then open the barrier
    if (threadIdx.x < kTicketShards)
      __hip_atomic_store(&a.slot->shard[threadIdx.x].count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0) __hip_atomic_store(&a.slot->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x < kTicketShards)
      __hip_atomic_store(&s.st->line[threadIdx.x].gen, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 0) {
    int expired = prior != 0 ? 1 : 0;
    if (!last) {
      const unsigned nsh = gridDim.x < unsigned(kTicketShards) ? gridDim.x : unsigned(kTicketShards);
      const unsigned long long* word = &s.st->line[blockIdx.x % nsh].gen;
      long long spins = 0;
      while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != tag) {
        if (++spins > s.spin_limit) {
          expired = 1;
          unsigned long long none = 0;
          __hip_atomic_compare_exchange_strong(&s.st->expired.gen, &none, tag, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        __builtin_amdgcn_s_sleep(8);
      }
    }
    s_expired = expired;
  }
  if (threadIdx.x < XDE_MAX_SEG) {
    seg_val[threadIdx.x] = 0.0;
    seg_nf[threadIdx.x] = 0.0;
  }
  __syncthreads();

  // ---- phase 2: the controller, in every workgroup ----
  reduce_partials<true>(a.slot, seg_val, seg_nf, int(gridDim.x), 1, NORM);  // (write-through records: sc1 loads)
  if (threadIdx.x == 0 && s_expired) seg_nf[0] += 1.0;  // an expired barrier stops the solve (XDE_STATUS_NONFINITE); the host names it
  __syncthreads();
  control_tail(pub ? tl.ctrl : &sink, tl.p, seg_val, seg_nf, tl.t_span, tl.step_t, pub ? tl.t_stage_out : static_cast<void*>(t_sink),
               pub ? tl.mirror : nullptr, tl.flags, &zs, &pfs);
  const int acc_new = zs.accept;
  const T c1 = T(s.a21) * T(zs.dt);  // xde_stage_combine: `T(beta) * dt`, with the step just planned
  T* out = static_cast<T*>(s.out);
  if (acc_new) {
#pragma unroll
    for (int j = 0; j < kSeamCap; ++j) {
      const int64_t i = i0 + int64_t(j) * stride;
      if (i < nvec) {
        P o;
#pragma unroll
        for (int w = 0; w < W; ++w) o.v[w] = cy[j].v[w] + ck[j].v[w] * c1;
        o.store(out, vbase + i);
      }
    }
    if (ton) out[tj] = ty1 + tk * c1;
  } else {
    const T* __restrict__ fb = static_cast<const T*>(s.f0[sel]);
    for (int64_t i = i0; i < nvec; i += stride) {
      P y = P::load(y0, vbase + i);
      P f = P::load(fb, vbase + i);
      P o;
#pragma unroll
      for (int w = 0; w < W; ++w) o.v[w] = y.v[w] + f.v[w] * c1;
      o.store(out, vbase + i);
    }
    if (ton) out[tj] = y0[tj] + fb[tj] * c1;
  }
}

// workgroups of one variant the current device holds at once: the occupancy query (at most kSeamBlocksPerCU) x CUs, asked once
template <typename T, int NORM, bool NT>
int seam_resident() {
  static int cache[64];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    return 0;
  }
  std::lock_guard<std::mutex> lk(mu);
  if (cache[dev] == 0) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xde_seam_kernel<T, NORM, NT>, kBlock, 0) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    if (per_cu > kSeamBlocksPerCU) per_cu = kSeamBlocksPerCU;
    cache[dev] = per_cu * cus > 0 ? per_cu * cus : -1;
  }
  return cache[dev] > 0 ? cache[dev] : 0;
}

int seam_resident_of(int dtype, int norm_kind, bool nt) {
#define SEAM_RES(T, NORM) (nt ? seam_resident<T, NORM, true>() : seam_resident<T, NORM, false>())
  if (dtype == XDE_F32) return norm_kind == XDE_NORM_RMS ? SEAM_RES(float, XDE_NORM_RMS) : SEAM_RES(float, XDE_NORM_LINF);
  return norm_kind == XDE_NORM_RMS ? SEAM_RES(double, XDE_NORM_RMS) : SEAM_RES(double, XDE_NORM_LINF);
#undef SEAM_RES
}

// blocks and vectors per lane of the pass over one n-element segment (xde_error_norm_partial's grid for it)
int seam_geometry(int64_t n, int dtype, int* blocks_out, int* per_lane_out) {
  xde_segments_t segs;
  memset(&segs, 0, sizeof(segs));
  segs.struct_size = sizeof(segs);
  segs.n_seg = 1;
  segs.seg_len[0] = n;
  const int width = dtype == XDE_F32 ? 4 : 2;
  SegMap m;
  int blocks = 0;
  if (int rc = build_segmap(&segs, width, true, &m, &blocks)) return rc;
  const int64_t nvec = n / width;
  const int64_t lanes = int64_t(blocks) * kBlock;
  *blocks_out = blocks;
  *per_lane_out = int((nvec + lanes - 1) / lanes);
  return XDE_OK;
}

}  // namespace

extern "C" {

int64_t xde_seam_state_bytes(void) { return int64_t(sizeof(SeamState)); }

int xde_seam_plan(int64_t n, int dtype, xde_seam_plan_t* plan_out) {
  if (!plan_out) return fail(XDE_EBADARG, "xde_seam_plan: null pointer");
  if (dtype != XDE_F32 && dtype != XDE_F64) return fail(XDE_EBADARG, "xde_seam_plan: bad dtype");
  if (n < 1) return fail(XDE_EBADARG, "xde_seam_plan: n must be positive");
  memset(plan_out, 0, sizeof(*plan_out));
  int blocks = 0, per_lane = 0;
  if (int rc = seam_geometry(n, dtype, &blocks, &per_lane)) return rc;
  plan_out->blocks = blocks;
  plan_out->per_lane = per_lane;
  // (the variants differ in a cache-policy bit and the norm's merge: the most demanding answer is the smallest)
  int resident = seam_resident_of(dtype, XDE_NORM_RMS, false);
  const int others[3] = {seam_resident_of(dtype, XDE_NORM_RMS, true), seam_resident_of(dtype, XDE_NORM_LINF, false),
                         seam_resident_of(dtype, XDE_NORM_LINF, true)};
  for (int r : others) resident = r < resident ? r : resident;
  plan_out->resident = resident;
  plan_out->fits = (blocks <= resident && per_lane <= kSeamCap) ? 1 : 0;
  return XDE_OK;
}

int xde_seam_attempt(const void* k_last, double c_last, const void* e_pre, const void* y0, const void* y0_alt, const void* f0,
                     const void* f0_alt, const void* y1, void* out, double a21, int64_t n, int dtype, void* ws, void* state,
                     xde_ctrl_t* ctrl, const xde_ctrl_params_t* params, const double* t_span_dev, const double* step_t_dev,
                     void* t_stage_out, xde_ctrl_t* host_mirror, int64_t spin_limit, void* stream) {
  if (!k_last || !e_pre || !y0 || !f0 || !y1 || !out || !ws || !state || !ctrl || !t_span_dev || !t_stage_out)
    return fail(XDE_EBADARG, "xde_seam_attempt: null pointer");
  int rc = check_params(params, "xde_seam_attempt");
  if (rc != XDE_OK) return rc;
  if (params->n_seg != 1) return fail(XDE_EBADARG, "xde_seam_attempt: one segment only");
  if (params->n_step_t > 0 && !step_t_dev) return fail(XDE_EBADARG, "xde_seam_attempt: n_step_t > 0 without step_t_dev");
  if (dtype != params->state_dtype) return fail(XDE_EBADARG, "xde_seam_attempt: dtype does not match params->state_dtype");
  if ((y0_alt == nullptr) != (f0_alt == nullptr)) return fail(XDE_EBADARG, "xde_seam_attempt: y0_alt/f0_alt must come together");
  if (n < 1) return fail(XDE_EBADARG, "xde_seam_attempt: n must be positive");
  if (spin_limit <= 0) return fail(XDE_EBADARG, "xde_seam_attempt: spin_limit must be positive (the wait is bounded)");
  xde_segments_t segs;
  memset(&segs, 0, sizeof(segs));
  segs.struct_size = sizeof(segs);
  segs.n_seg = 1;
  segs.seg_len[0] = n;
  SeamArgs s;
  memset(&s, 0, sizeof(s));
  bool vec = false;
  int nblocks = 0;
  double bytes = 0;
  const void* kk[1] = {k_last};
  rc = setup_err_args("xde_seam_attempt", kk, nullptr, &c_last, 1, y0, y0_alt, y1, params->rtol, params->atol, 0.0, ctrl, &segs,
                      params->norm_kind, dtype, ws, e_pre, &s.e, &vec, &nblocks, &bytes);
  if (rc != XDE_OK) return rc;
  vec = vec && aligned16(out) && aligned16(f0) && (!f0_alt || aligned16(f0_alt));
  if (!vec) return fail(XDE_EBADARG, "xde_seam_attempt: operands must be 16-byte aligned");
  const int width = dtype == XDE_F32 ? 4 : 2;
  const int64_t lanes = int64_t(nblocks) * kBlock;
  const int64_t per_lane = (n / width + lanes - 1) / lanes;
  const int resident = seam_resident_of(dtype, params->norm_kind, s.e.nt != 0);
  if (nblocks > resident || per_lane > kSeamCap)
    return fail(XDE_EBADARG, "xde_seam_attempt: the state does not fit the resident launch (" + std::to_string(nblocks) + " workgroups, " +
                                 std::to_string(resident) + " resident; " + std::to_string(per_lane) + " vectors per lane, " +
                                 std::to_string(kSeamCap) + " carried): take the separate launches");
  s.f0[0] = f0;
  s.f0[1] = f0_alt ? f0_alt : f0;
  s.out = out;
  s.a21 = a21;
  s.st = static_cast<SeamState*>(state);
  s.spin_limit = spin_limit;
  SeamCtrl tl;
  tl.ctrl = ctrl;
  tl.p = *params;
  tl.t_span = t_span_dev;
  tl.step_t = step_t_dev;
  tl.t_stage_out = t_stage_out;
  tl.mirror = host_mirror;
  tl.flags = ctrl_flags();
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the pass's four arrays in, the stage input out
  ProfScope prof(XDE_KID_ERRNORM, 5.0 * double(n) * (dtype == XDE_F32 ? 4.0 : 8.0));
  dim3 g(nblocks), b(kBlock);
#define LAUNCH_SEAM(T, NORM)                                                   \
  do {                                                                         \
    if (s.e.nt)                                                                \
      XDE_LAUNCH((xde_seam_kernel<T, NORM, true>), g, b, st, prof, s, tl);     \
    else                                                                       \
      XDE_LAUNCH((xde_seam_kernel<T, NORM, false>), g, b, st, prof, s, tl);    \
  } while (0)
  if (dtype == XDE_F32) {
    if (params->norm_kind == XDE_NORM_RMS) LAUNCH_SEAM(float, XDE_NORM_RMS);
    else LAUNCH_SEAM(float, XDE_NORM_LINF);
  } else {
    if (params->norm_kind == XDE_NORM_RMS) LAUNCH_SEAM(double, XDE_NORM_RMS);
    else LAUNCH_SEAM(double, XDE_NORM_LINF);
  }
#undef LAUNCH_SEAM
  HIP_TRY(hipGetLastError());
  return XDE_OK;
}

int xde_seam_expired(const void* state, int64_t* tag_out, void* stream) {
  if (!state || !tag_out) return fail(XDE_EBADARG, "xde_seam_expired: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(tag_out, &static_cast<const SeamState*>(state)->expired.gen, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return XDE_OK;
}

}  // extern "C"
