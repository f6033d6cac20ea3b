/*
 * xde_hip_mlp.h — entry points of libxde_hip.so for a neural ODE's vector field that is a small multi-layer perceptron: every linear
 * layer and every activation between them as ONE launch, so that no hidden activation is ever written to device memory (host side:
 * paddlexde_amd/xde/mlp_field.py, MLPField).
 *
 *   h_0[r, k]   = x[r, k]                                                       k < widths[0]
 *   pre_l[r, n] = sum_k h_l[r, k] * W_l[n, k] + bias_l[n]                        n < widths[l + 1],  l = 0 .. n_layers - 1
 *   pre_0[r, n] = pre_0[r, n] + t_r * W_0[n, widths[0]]                          (time != 0 only: the time column, a rank-one add)
 *   h_{l+1}     = act(pre_l)                                                    act: identity or tanh; l < n_layers - 1
 *   out[r, n]   = pre_{n_layers - 1}[r, n]                                      (no activation after the last layer)
 *
 * x[rows, widths[0]] and out[rows, widths[n_layers]] are contiguous arrays of float.  W[l] is a linear layer's weight in its own
 * layout, [widths[l + 1], widths[l]] row-major — [widths[1], widths[0] + 1] for l = 0 with time != 0, whose last column multiplies
 * the time — and bias[l] its bias [widths[l + 1]], or null: no bias in that layer (a null `bias` array: none in any).  t_r is
 * t_rows[r], an array of `rows` floats, or with a null t_rows the scalar t converted to float; with time == 0 neither is read.
 *
 * Same conventions as xde_hip.h: status codes, device pointers borrowed from the caller (W, bias and widths themselves are HOST arrays
 * of n_layers, n_layers and n_layers + 1 entries, read before the call returns), `stream` = hipStream_t as void*, XDE_F32 / XDE_F64.
 * Arguments are validated on the host before anything is enqueued: a refused call writes nothing.
 *
 * SERVED: dtype XDE_F32, 1 <= n_layers <= XDE_MLP_MAX_LAYERS, every width in [1, XDE_MLP_MAX_WIDTH], act one of XDE_MLP_ACT_*.
 * Anything else is refused by the launch; the plan query below says so beforehand (`served`), and the host then takes the plain
 * composition.  Not built: a backward, float64, wider layers.
 *
 * THE TILE WALK.  A work item is a tile of 32 state rows (two such tiles where the plan pairs them).  Its activations live in two
 * buffers of LDS, laid out [k][row], that the layers fill in turn: layer l reads one and writes the other, with one workgroup barrier
 * per layer boundary; x is read from device memory once per item and only the last layer writes to it.  The products run on the
 * matrix cores (v_mfma_f32_32x32x2_f32): 32 neurons n of W_l on the instruction's M axis, the tile's 32 state rows on its N axis.  The
 * four waves of a workgroup take chunks of 32 consecutive n; a wave reads its rows of W_l with 16-byte loads (from L2) where the row
 * stride is a multiple of 4 and the pointer allows, else by element, and each value it loads meets both tiles of a pair before the
 * next is taken.  With K = widths[l] and KH = 4 ceil(K / 8), lane half 0 of a wave walks k in [0, min(KH, K)) and lane half 1 walks
 * k in [KH, K).  Workgroups loop over the items where there are more items than workgroups.
 *
 * ARITHMETIC, AND WHAT CAN BE SAID OF ITS ORDER.
 *   - acc = +0; for j = 0, 1, ..., min(KH, K) - 1 in ascending order, one instruction:
 *         acc <- acc + ( h[r, j] W[n, j]  +  h[r, KH + j] W[n, KH + j] )          (the second product is +0 * +0 where KH + j >= K)
 *     How the hardware rounds and orders the two products and the accumulator inside one instruction is not documented by the ISA:
 *     a host program cannot restate this sum bit for bit.  It is held to an error bound against float64, to determinism and to row
 *     independence instead; where every product and partial sum is an integer below 2^24 it is exact in any order.
 *   - pre = acc + bias[n]            one rounding; no bias: pre = acc
 *   - pre = pre + t_r * W_0[n, K]    layer 0 with time: one rounding for the product, one for the add
 *   - h = tanhf(pre) or pre          (the last layer: out = pre)
 * A neuron chunk past widths[l + 1], a k past K and a state row past `rows` contribute +0 * +0, are never read and never written.
 * Built with -ffp-contract=off: every op outside the matrix instruction is rounded on its own.  No atomics: each out[r, n] is written
 * once, by one lane.  out must not overlap an operand.  A row r of the result depends on row r of x, on t_r and on the weights only: not
 * on rows, on its tile, on its place in the tile, on the grid or on the plan; 16-byte or element access changes no bit.  Two launches
 * on the same operands give the same bits.
 */
#ifndef XDE_HIP_MLP_H
#define XDE_HIP_MLP_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XDE_MLP_ACT_IDENTITY 0
#define XDE_MLP_ACT_TANH 1
#define XDE_MLP_MAX_LAYERS 4   /* linear layers of one launch */
#define XDE_MLP_MAX_WIDTH 256  /* of the input, of every hidden layer and of the output: two [256][32] float buffers are 64 KiB of LDS */
#define XDE_MLP_PAIR_WIDTH 128 /* input and hidden widths up to which two tiles of 32 rows share the buffers and every read of W */

/* out as above.  One launch on `stream`.
 * Refused (XDE_EBADARG): a null out / x / W / widths or a null W[l], n_layers, rows or a width < 1, a dtype that is not XDE_F32 /
 * XDE_F64, an act that is not XDE_MLP_ACT_*, a shape the plan does not serve (XDE_F64, n_layers > XDE_MLP_MAX_LAYERS, a width >
 * XDE_MLP_MAX_WIDTH), a device pointer not aligned to its element type. */
int xde_mlp_field(void* out, const void* x, const void* t_rows, double t, const void* const* W, const void* const* bias,
                  const int32_t* widths, int n_layers, int64_t rows, int act, int time, int dtype, void* stream);

/* THE LAUNCH PLAN, by the function the launch itself uses.  The bits of a result never depend on it. */
typedef struct xde_mlp_plan {
  int32_t served;    /* 0: XDE_F64, too many layers, a width beyond the cap or an unknown act — the launch refuses the call */
  int32_t tiles;     /* tiles of 32 state rows of a work item: 2 where the input and hidden widths are <= XDE_MLP_PAIR_WIDTH and the
                        single tiles alone would outnumber the workgroups the chip holds, else 1 */
  int32_t tile_r;    /* state rows of a work item: 32 * tiles */
  int32_t tile_n;    /* neurons per wave and chunk (the instruction's M axis) */
  int32_t pass_n;    /* neurons the four waves of a workgroup cover side by side: tile_n times its waves */
  int32_t max_width; /* the widest of the input and the hidden layers: what the LDS buffers hold */
  int32_t x_vec;     /* widths[0] % 4 == 0: x is read with 16-byte loads where its pointer allows too (no bit depends on it) */
  int32_t out_vec;   /* widths[n_layers] % 4 == 0: out is written with 16-byte stores where its pointer allows too */
  int32_t lds_bytes; /* LDS of the workgroup: the two activation buffers */
  int32_t width_cap; /* XDE_MLP_MAX_WIDTH */
  int64_t items;     /* work items: ceil(rows / tile_r) */
  int64_t blocks;    /* workgroups launched: min(items, the grid cap); each loops over items blocks apart */
} xde_mlp_plan_t;

/* Enqueues nothing and needs no device.  Refused (XDE_EBADARG): a null plan or widths, rows or n_layers < 1, a width < 1 among those
 * read (the first min(n_layers, XDE_MLP_MAX_LAYERS) + 1), a dtype that is not XDE_F32 / XDE_F64.  An unserved shape is NOT refused
 * here: it is reported, served = 0. */
int xde_mlp_plan(int64_t rows, const int32_t* widths, int n_layers, int dtype, int act, int time, xde_mlp_plan_t* plan);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_MLP_H */
