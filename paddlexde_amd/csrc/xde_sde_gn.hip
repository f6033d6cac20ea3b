// libxde_hip.so — the Ito Euler-Maruyama step with general (and scalar) noise, and its cotangents (C ABI: include/xde_hip_gn.h; host:
// paddlexde_amd/solver/base_fixed_solver.py, sdeint's option noise_type).  The kernels, their design and the launch helpers are in
// xde_sde_gn_device.hpp; this file instantiates the step kernel in its Euler mode and the plain backward kernel.

#include "xde_sde_gn_device.hpp"

using namespace xde;
using namespace xde::gn;

extern "C" {

// (profiled under the fixed-step fuse id, as xde_sde_em_step: the kernel-id list of xde_hip.h is part of the frozen ABI)
int xde_sde_gn_step(void* y1, const void* y0, const void* f, const void* g, int64_t rows, int64_t D, int64_t M, double dt, double s,
                    uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_gn_step";
  if (!y1 || !y0 || !f || !g) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  if (int rc = gn_check_shape(who, rows, D, M, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8, nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if (int rc = gn_check_operands(who, {y1}, nullptr, {y0, f}, g, true, nbytes, gbytes, esz, "operands overlap (y1 may be y0; no other overlap)"))
    return rc;
  GnArgs a;
  gn_fill(a, rows, D, M, dt, s, seed, k);
  a.out[0] = y1;
  a.in[0] = y0;
  a.in[1] = f;
  a.in[2] = g;
  ProfScope prof(XDE_KID_COMBINE_FUSE, double(4 + M) * double(nbytes));
  return gn_launch_step<kGnStep>(a, dtype, static_cast<hipStream_t>(stream), prof);
}

int xde_sde_gn_backward(void* gf, void* gg, const void* gy1, int64_t rows, int64_t D, int64_t M, double dt, double s, uint64_t seed,
                        int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_gn_backward";
  if (!gy1) return fail(XDE_EBADARG, std::string(who) + ": null pointer (gy1)");
  if (int rc = gn_check_shape(who, rows, D, M, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8, nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if (int rc = gn_check_operands(who, {gf}, gg, {gy1}, nullptr, false, nbytes, gbytes, esz, "an output overlaps another operand")) return rc;
  if (!gf && !gg) return XDE_OK;
  GnArgs a;
  gn_fill(a, rows, D, M, dt, s, seed, k);
  a.out[0] = gf;
  a.out[1] = gg;
  a.in[0] = gy1;
  ProfScope prof(XDE_KID_COMBINE, double(1 + (gf ? 1 : 0)) * double(nbytes) + (gg ? double(gbytes) : 0.0));
  return gn_launch_backward<false>(a, dtype, static_cast<hipStream_t>(stream), prof);
}

}  // extern "C"
