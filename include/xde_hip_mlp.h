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
 * composition.  Not built: float64, wider or deeper fields, a fused tape for back-propagation through a solve's steps (the vector-
 * Jacobian product the adjoint method needs IS built: xde_mlp_field_vjp, below).
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

/*
 * THE VECTOR-JACOBIAN PRODUCT: the field recomputed and the cotangent a[rows, widths[n_layers]] carried back through every layer, in
 * two launches; the hidden activations and their cotangents exist only in LDS.  With L = n_layers, pre_l and h_l as above:
 *
 *   f            = pre_{L-1}                                                    the bits of xde_mlp_field's out
 *   dpre_{L-1}   = a
 *   dh_l[r, k]   = sum_n dpre_l[r, n] * W_l[n, k]                                k < widths[l]: the time column is not part of it
 *   dpre_{l-1}   = dh_l * (1 - h_l * h_l)   (tanh)      |      dh_l   (identity)
 *   gx           = dh_0
 *   gW_l[n, k]   = sum_r dpre_l[r, n] * h_l[r, k]         gb_l[n] = sum_r dpre_l[r, n]
 *   gW_0[n, widths[0]] = sum_r dpre_0[r, n] * t_r                                (time != 0: the time column)
 *   gt           = sum_n ( sum_r dpre_0[r, n] ) * W_0[n, widths[0]]              (time != 0)
 *
 * THE TILE WALK.  A work item is a tile of 32 state rows; a workgroup of four waves loops over items `blocks` apart.  LDS holds one
 * buffer per layer boundary, h_0 .. h_{L-1}, and one for a, all at once: sum(widths[0 .. L]) * 32 floats, [k][row] at a pitch of 32
 * floats with the row index XOR-swizzled by k % 32 (both the reads along rows and the reads along k then meet 32 distinct banks; a
 * padded pitch would push 128-128-128-128 past the bound).  A shape whose widths sum past XDE_MLP_VJP_LDS_BYTES / 128 = 512 is not
 * served.  dpre_{l-1} is written IN PLACE over h_l, each element by the one lane that read it; gW_l and gb_l are taken before that.
 * All three products run on the matrix cores (v_mfma_f32_32x32x2_f32).
 *
 * ARITHMETIC, AND WHAT CAN BE SAID OF ITS ORDER.
 *   - f: the forward's instructions, operand for operand (above).
 *   - dh_l[r, k]: with N = widths[l + 1] and NH = 4 ceil(N / 8): acc = +0; for j = 0 .. min(NH, N) - 1 ascending, one instruction:
 *         acc <- acc + ( dpre[r, j] W[j, k]  +  dpre[r, NH + j] W[NH + j, k] )     (the second product is +0 * +0 where NH + j >= N)
 *   - dpre_{l-1} = dh * (1 - h * h): three roundings (tanh); dh itself (identity).
 *   - one item's share of gW_l[n, k], with r counted from the tile's first row: acc = +0; for j = 0 .. 15 ascending, one instruction:
 *         acc <- acc + ( dpre[j, n] h[j, k]  +  dpre[16 + j, n] h[16 + j, k] )
 *   - one item's share of gb_l[n]: the 32 values dpre[r, n] summed pairwise: v_r <- v_r + v_{r+1} for even r, then v_r <- v_r + v_{r+2}
 *     for r % 4 == 0, ... five levels, the share is v_0; of the time column: the same tree over dpre[r, n] * t_r (one rounding each).
 *   - over items: workgroup b adds the shares of its items b, b + blocks, ... in that order into slab b of the workspace (the first is
 *     stored, not added); the second launch adds the slabs in ascending b, starting from slab 0's value.
 *   - gt = ((S_0 W_0[0, K]) + S_1 W_0[1, K]) + ..., ascending n, S_n the fully reduced row sum of dpre_0[., n], K = widths[0].
 *   As above, what one matrix instruction does with its two products and the accumulator is not documented: none of these sums can
 *   be restated bit for bit by a host program.  They are held to an error bound against float64, to determinism and (f, gx) to row
 *   independence; on small integers they are exact in any order.
 * A row past `rows` enters as x = +0 and a = +0: every product it contributes is a zero.  A k past widths[l] and an n past
 * widths[l + 1] contribute +0 * +0.  None of them is read from or written to memory.  Built with -ffp-contract=off.  No atomics.  f,
 * gx, gW[l], gb[l], gt and the workspace must not overlap one another or an operand.  Row r of f and of gx depends on row r of x and a,
 * on t_r and on the weights only.  gW, gb and gt depend on the operands and on `blocks` of the plan (the order of the sum over
 * items), on nothing else.  Two calls on the same operands give the same bits.
 */
#define XDE_MLP_VJP_LDS_BYTES 65536 /* LDS of a workgroup of the vjp: the widths of a served shape sum to at most 512 */
#define XDE_MLP_VJP_MAX_BLOCKS 256  /* the grid cap of the vjp's first launch: one workgroup per compute unit; it bounds the workspace */

/* f[rows, widths[n_layers]], gx[rows, widths[0]], gW[l] in W[l]'s shape, gb[l][widths[l + 1]] and the scalar gt as above.  gW and gb
 * are HOST arrays of n_layers device pointers like W and bias; a null gb, or a null gb[l], leaves that gradient out (the bias may be
 * null or not).  gt may be null with time == 0, when it is not written.  `workspace` is device memory of at least the plan's
 * workspace_bytes that the call may overwrite; it need not be cleared.  max_blocks: 0 for the plan's grid cap, or a positive limit on
 * the workgroups of the first launch (a smaller grid puts more items through each slab: tests and profiles use it).  Two launches on
 * `stream`.
 * Refused (XDE_EBADARG): a null f / gx / gW / x / a / W / widths / workspace, a null W[l] or gW[l], a null gt with time != 0, rows,
 * n_layers or a width < 1, a dtype that is not XDE_F32 / XDE_F64, max_blocks < 0, an act that is not XDE_MLP_ACT_*, a shape the plan
 * does not serve (XDE_F64, n_layers > XDE_MLP_MAX_LAYERS, a width > XDE_MLP_MAX_WIDTH, widths that sum beyond the LDS bound), a
 * workspace_bytes below the plan's, a device pointer not aligned to its element type. */
int xde_mlp_field_vjp(void* f, void* gx, void* const* gW, void* const* gb, void* gt, const void* x, const void* a, const void* t_rows,
                      double t, const void* const* W, const void* const* bias, const int32_t* widths, int n_layers, int64_t rows, int act,
                      int time, int dtype, void* workspace, int64_t workspace_bytes, int max_blocks, void* stream);

/* THE VJP'S PLAN, by the function the launch itself uses.  f and gx never depend on it; gW, gb and gt depend on `blocks` alone. */
typedef struct xde_mlp_vjp_plan {
  int32_t served;          /* 0: XDE_F64, too many layers, a width beyond the cap, widths that sum beyond the LDS bound or an unknown act */
  int32_t tile_r;          /* state rows of a work item: 32 */
  int32_t pitch;           /* floats between two k of an LDS buffer: 32 (swizzled, not padded) */
  int32_t sum_widths;      /* widths[0] + ... + widths[n_layers]: what the LDS buffers hold per state row */
  int32_t lds_bytes;       /* sum_widths * pitch * 4: what the shape needs */
  int32_t lds_cap;         /* XDE_MLP_VJP_LDS_BYTES: what a workgroup takes */
  int32_t grid_cap;        /* XDE_MLP_VJP_MAX_BLOCKS */
  int32_t gx_vec;          /* widths[0] % 4 == 0: x is read and gx written with 16-byte accesses where the pointers allow too */
  int64_t params;          /* P, floats of a slab: per layer gW_l and one row sum per neuron */
  int64_t workspace_bytes; /* blocks * params * 4 */
  int64_t items;           /* work items: ceil(rows / tile_r) */
  int64_t blocks;          /* workgroups of the first launch: min(items, grid_cap, max_blocks where that is > 0) */
} xde_mlp_vjp_plan_t;

/* Enqueues nothing and needs no device.  Refused (XDE_EBADARG): what xde_mlp_plan refuses, and max_blocks < 0.  An unserved shape is
 * NOT refused here: it is reported, served = 0. */
int xde_mlp_vjp_plan(int64_t rows, const int32_t* widths, int n_layers, int dtype, int act, int time, int max_blocks,
                     xde_mlp_vjp_plan_t* plan);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_MLP_H */
