/*
 * xde_hip_cdehead.h — entry points of libxde_hip.so for a neural CDE whose field ends in a linear layer: the last layer, its
 * activation and the contraction with the control's derivative as ONE launch, so that F[B, H, C] is never written
 * (host side: paddlexde_amd/xde/base_cde.py, CDELinearHead / CdeHeadFn).
 *
 *   pre[b, n] = sum_k a[b, k] * W[n, k] + bias[n]             n = h C + c
 *   out[b, h] = sum_c act(pre[b, h C + c]) * dX[b, c]         act: identity or tanh
 *
 * and on the way back, with y = act(pre) computed again on chip,
 *
 *   s[b, n] = gout[b, h] * dX[b, c] * act'(pre[b, n])          (tanh: 1 - y y;  identity: 1)
 *
 * a[B, K] is the output of the user's trunk; W[H C, K] and bias[H C] (or null) are a linear layer's weight and bias in their own
 * layout; s[B, H C] is the cotangent of pre, from which the host forms ga = s W, gW = s^T a and gbias = sum_b s with its BLAS.
 *
 * Same conventions as xde_hip.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*, XDE_F32 /
 * XDE_F64, XDE_HISTORY_*).  The control (series[B, Tn, C], knots[Tn], the time t_dev / t_host / time_dtype, the method) and dX are
 * those of the contraction of xde_hip_cde.h, bit for bit: the same device functions build dX on chip.  `coef` non-null means the natural
 * control of xde_hip_spline.h: `series` is then its Y, `coef` its M, and `method` is not read.  Arguments are validated on the host before
 * anything is enqueued: a refused call writes nothing.  All arrays are contiguous.
 *
 * SERVED: dtype XDE_F32 and 1 <= K <= XDE_CDEHEAD_MAX_K.  XDE_F64 and a longer K are refused; the plan query below says so beforehand
 * (`served`), and the host then takes the unfused route.
 *
 * THE TILE WALK.  The products run on the matrix cores (v_mfma_f32_32x32x2_f32): 32 rows n of W on the instruction's M axis, 32 batch
 * rows b on its N axis.  A work item is 32 consecutive batch rows and a slice of whole rows h; its four waves take chunks of 32
 * consecutive n.  With KH = 4 ceil(K / 8), lane half 0 of a wave holds k in [0, min(KH, K)) of its batch row and lane half 1 holds
 * k in [KH, K), in registers, for the whole walk over n.
 *
 * ARITHMETIC, AND WHAT CAN BE SAID OF ITS ORDER.
 *   - acc = +0; for j = 0, 1, ..., min(KH, K) - 1 in ascending order, one instruction:
 *         acc <- acc + ( a[b, j] W[n, j]  +  a[b, KH + j] W[n, KH + j] )          (the second product is +0 * +0 where KH + j >= K)
 *     How the hardware rounds and orders the two products and the accumulator inside one instruction is not documented by the ISA, so
 *     this is the first kernel of the library whose result a host program cannot restate bit for bit.  It is held to an error bound
 *     (the standard gamma_{K + 2} one), to determinism and to row independence instead.
 *   - pre = acc + bias[n] (one rounding; no bias: pre = acc);  y = tanhf(pre) or pre;  p = y * dX[b, c]   (one rounding each, -ffp-contract=off)
 *   - out[b, h] = (...((+0 + p_0) + p_1) + ...) + p_{C-1}: sequential, in ascending c, whatever chunk boundaries cut the run.
 *   - backward: s = (gout[b, h] * dX[b, c]) * (1 - y * y)  for tanh,  s = gout[b, h] * dX[b, c]  for the identity.
 * No atomics.  A row b of the result depends on row b of the operands only: not on B, on its position in the tile, on the grid or on
 * the plan.  Two launches on the same operands give the same bits.
 */
#ifndef XDE_HIP_CDEHEAD_H
#define XDE_HIP_CDEHEAD_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XDE_CDEHEAD_ACT_IDENTITY 0
#define XDE_CDEHEAD_ACT_TANH 1
#define XDE_CDEHEAD_MAX_K 256 /* K / 2 registers per lane hold the batch tile of a */
#define XDE_CDEHEAD_MAX_HC 2147483392 /* 2^31 - 256: the kernel walks n = h C + c in int, 128 at a time */

/* out[b, h] as above.  One launch; W is read once per 32 batch rows (from L2), a once, F never exists.
 * Refused (XDE_EBADARG): a null out / a / W / series / knots, B, H, C or K < 1, H C > XDE_CDEHEAD_MAX_HC, Tn < 2, a dtype or time_dtype that
 * is not XDE_F32 / XDE_F64, XDE_HISTORY_BEZIER or an unknown method (coef null), an act that is not XDE_CDEHEAD_ACT_*, a shape the plan
 * does not serve (XDE_F64, K > XDE_CDEHEAD_MAX_K), a pointer not aligned to its element type. */
int xde_cdehead_forward(void* out, const void* a, const void* W, const void* bias, const void* series, const void* coef, const void* knots,
                        const void* t_dev, double t_host, int time_dtype, int64_t B, int H, int C, int K, int Tn, int method, int act,
                        int dtype, void* stream);

/* s[b, n] as above, every element written.  One launch.  Same checks (null s / gout / a / W / series / knots). */
int xde_cdehead_backward(void* s, const void* gout, const void* a, const void* W, const void* bias, const void* series, const void* coef,
                         const void* knots, const void* t_dev, double t_host, int time_dtype, int64_t B, int H, int C, int K, int Tn,
                         int method, int act, int dtype, void* stream);

/* THE LAUNCH PLAN of both entry points, by the function the launches themselves use.  The bits of a result never depend on it. */
typedef struct xde_cdehead_plan {
  int32_t served;    /* 0: XDE_F64, K > XDE_CDEHEAD_MAX_K or an unknown act — the entry points refuse the call */
  int32_t tile_b;    /* batch rows of a work item (the instruction's N axis) */
  int32_t tile_n;    /* rows of W per wave and chunk (the instruction's M axis) */
  int32_t pass_n;    /* rows of W one workgroup covers between two barriers: tile_n times its waves */
  int32_t kh;        /* KH: the k at which lane half 1 starts */
  int32_t kq;        /* 16-byte vectors of k a lane walks: KH / 4 */
  int32_t kq_regs;   /* vectors of k the kernel instantiation holds per lane: the least of 1, 2, 4, ..., 32 that is >= kq */
  int32_t S, Hc;     /* slices of H per batch tile, rows h per slice (the last slice may be shorter) */
  int32_t lds_dx;    /* the dX tile [32, C] is kept in LDS (else C is beyond it and dX is evaluated per use) */
  int32_t lds_bytes; /* LDS of the forward workgroup: product tiles, carries, the dX tile */
  int32_t k_cap;     /* XDE_CDEHEAD_MAX_K */
  int64_t items;     /* work items: ceil(B / tile_b) * S */
  int64_t blocks;    /* workgroups launched: min(items, the grid cap) */
} xde_cdehead_plan_t;

/* Enqueues nothing and needs no device.  Refused (XDE_EBADARG): a null plan, B, H, C or K < 1, a dtype that is not XDE_F32 / XDE_F64.
 * An unserved shape is NOT refused here: it is reported, served = 0.  (16-byte vector access of a, W and s is decided per launch from
 * K % 4, H C % 4 and the pointers; it changes no bit and is not part of the plan.) */
int xde_cdehead_plan(int64_t B, int H, int C, int K, int dtype, int act, xde_cdehead_plan_t* plan);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_CDEHEAD_H */
