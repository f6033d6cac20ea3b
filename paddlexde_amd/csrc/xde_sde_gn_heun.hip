// libxde_hip.so — the Stratonovich Heun step with general (and scalar) noise: predictor, corrector and the one cotangent launch of both
// (C ABI: include/xde_hip_gn.h; host: FixedSolver._heun_step, solver=Heun).  The kernels are those of xde_sde_gn_device.hpp in their
// predict / correct modes and with the backward kernel's extra operands; nothing of the tiling is restated here.

#include "xde_sde_gn_device.hpp"

using namespace xde;
using namespace xde::gn;

extern "C" {

int xde_sde_gn_heun_predict(void* yp, void* a0, const void* y0, const void* f0, const void* g0, int64_t rows, int64_t D, int64_t M,
                            double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_gn_heun_predict";
  if (!yp || !a0 || !y0 || !f0 || !g0) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  if (int rc = gn_check_shape(who, rows, D, M, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8, nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if (int rc = gn_check_operands(who, {yp, a0}, nullptr, {y0, f0}, g0, false, nbytes, gbytes, esz, "operands overlap (no output may overlap another operand)"))
    return rc;
  GnArgs a;
  gn_fill(a, rows, D, M, dt, s, seed, k);
  a.out[0] = yp;
  a.out[1] = a0;
  a.in[0] = y0;
  a.in[1] = f0;
  a.in[2] = g0;
  ProfScope prof(XDE_KID_COMBINE_FUSE, double(5 + M) * double(nbytes));
  return gn_launch_step<kGnPredict>(a, dtype, static_cast<hipStream_t>(stream), prof);
}

int xde_sde_gn_heun_correct(void* y1, const void* y0, const void* f0, const void* f1, const void* a0, const void* g1, int64_t rows,
                            int64_t D, int64_t M, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_gn_heun_correct";
  if (!y1 || !y0 || !f0 || !f1 || !a0 || !g1) return fail(XDE_EBADARG, std::string(who) + ": null pointer");
  if (int rc = gn_check_shape(who, rows, D, M, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8, nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if (int rc = gn_check_operands(who, {y1}, nullptr, {y0, f0, f1, a0}, g1, true, nbytes, gbytes, esz, "operands overlap (y1 may be y0; no other overlap)"))
    return rc;
  GnArgs a;
  gn_fill(a, rows, D, M, dt, s, seed, k);
  a.out[0] = y1;
  a.in[0] = y0;
  a.in[1] = f0;
  a.in[2] = g1;
  a.in[3] = f1;
  a.in[4] = a0;
  ProfScope prof(XDE_KID_COMBINE_FUSE, double(5 + M) * double(nbytes));
  return gn_launch_step<kGnCorrect>(a, dtype, static_cast<hipStream_t>(stream), prof);
}

int xde_sde_gn_heun_backward(void* gf, void* ga, void* gg, const void* gy, const void* gc, int64_t rows, int64_t D, int64_t M, double cf,
                             double ca, double s, uint64_t seed, int64_t k, int dtype, void* stream) {
  const char* who = "xde_sde_gn_heun_backward";
  if (!gy && !gc) return fail(XDE_EBADARG, std::string(who) + ": null pointer (gy and gc: one of them must be given)");
  if (!gy && (gf || ga)) return fail(XDE_EBADARG, std::string(who) + ": gf and ga are multiples of gy: with gy null they must be null");
  if (int rc = gn_check_shape(who, rows, D, M, k, dtype)) return rc;
  const size_t esz = dtype == XDE_F32 ? 4 : 8, nbytes = size_t(rows) * size_t(D) * esz, gbytes = nbytes * size_t(M);
  if (int rc = gn_check_operands(who, {gf, ga}, gg, {gy, gc}, nullptr, false, nbytes, gbytes, esz, "an output overlaps another operand")) return rc;
  if (!gf && !ga && !gg) return XDE_OK;
  GnArgs a;
  gn_fill(a, rows, D, M, cf, s, seed, k);
  a.ca = ca;
  a.out[0] = gf;
  a.out[1] = gg;
  a.out[2] = ga;
  a.in[0] = gy;
  a.in[1] = gc;
  ProfScope prof(XDE_KID_COMBINE, double((gy ? 1 : 0) + (gc && gg ? 1 : 0) + (gf ? 1 : 0) + (ga ? 1 : 0)) * double(nbytes) + (gg ? double(gbytes) : 0.0));
  return gn_launch_backward<true>(a, dtype, static_cast<hipStream_t>(stream), prof);
}

}  // extern "C"
