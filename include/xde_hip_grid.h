/*
 * xde_hip_grid.h — entry point of libxde_hip.so for the fixed-step solvers' sub-stepping
 * (options step_size / grid_constructor; host side: paddlexde_amd/solver/base_fixed_solver.py).
 *
 * A fixed-step solve that walks a grid of its own produces each output time by interpolating inside the grid step that brackets
 * it (reference: interpolation/functional/interp_fn.py:4-20).  One launch writes the G output rows of one step from ONE read of the
 * step's operands.
 *
 * Same conventions as xde_hip.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*,
 * XDE_F32 / XDE_F64).  Arguments are validated on the host before anything is enqueued.
 */
#ifndef XDE_HIP_GRID_H
#define XDE_HIP_GRID_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XDE_INTERP_MAX_ROWS 8 /* rows of one xde_interp_rows launch */

#define XDE_INTERP_LINEAR 0 /* operands y_a, y_b */
#define XDE_INTERP_CUBIC 1  /* operands y_a, y_b, f_a, f_b */

#define XDE_ROW_INTERP 0 /* the interpolant at the row's weights */
#define XDE_ROW_COPY_A 1 /* an exact copy of y_a (the output time is the step's start) */
#define XDE_ROW_COPY_B 2 /* an exact copy of y_b (the output time is the step's end) */

/*
 * The operands are contiguous arrays of n = outer * chunk elements.  Element e = o * chunk + c of row r is written to
 * rows[r][o * row_stride + c] (a solution [..., T*L, D]: chunk = L*D, row_stride = T*L*D, rows[r] = the row's first element).
 * w: G x 4 weights, row-major, converted to the state dtype; per kind of row r (kinds[r]):
 *     XDE_ROW_INTERP, mode LINEAR:  y_a + w[4r] * (y_b - y_a)
 *     XDE_ROW_INTERP, mode CUBIC:   ((w[4r] * y_a + w[4r+1] * f_a) + w[4r+2] * y_b) + w[4r+3] * f_b
 *     XDE_ROW_COPY_A / _COPY_B:     y_a / y_b, bit for bit
 * f_a / f_b are read in mode CUBIC only.  1 <= G <= XDE_INTERP_MAX_ROWS; rows may not overlap the operands.
 */
int xde_interp_rows(void* const* rows, const int* kinds, const double* w, int G, const void* y_a, const void* y_b, const void* f_a,
                    const void* f_b, int mode, int64_t outer, int64_t chunk, int64_t row_stride, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_GRID_H */
