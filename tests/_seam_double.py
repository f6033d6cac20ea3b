"""TEST DOUBLE of the resident seam launch's entry points (include/xde_hip_seam.h) on the numpy double of the kernel backend: the error
norm of the attempt (e_pre form), the controller, and the next attempt's first stage input, composed from the double's own statements of
the three launches the seam replaces.  HipBackend keeps the methods private (its public methods are the contract tests/test_cabi.py
freezes against tests/_cpu_double.py), so they live here.

``expire_at``: the seam launch with that index (0-based, counted over the double's life) behaves as a workgroup whose grid barrier
expired — one is added to the non-finite count its controller sees and the launch's tag is recorded — which is all the kernel does."""
import numpy as np

from paddlexde_amd import _hip

from ._cpu_double import NumpyDoubleBackend

SEAM_CAP = 16  # XDE_SEAM_CAP
NORM_GRID = 512  # the norm launches' default grid cap (csrc/xde_common.hpp)


def seam_geometry(n, width):
    """(blocks, per_lane) of include/xde_hip_seam.h for an n-element segment of `width` elements per 16 bytes."""
    per_block = 256 * width
    blocks = max(1, min(-(-n // per_block), NORM_GRID))
    lanes = blocks * 256
    return blocks, -(-(n // width) // lanes)


class SeamDoubleBackend(NumpyDoubleBackend):
    name = "numpy-double+seam(test)"
    RESIDENT = 512  # two workgroups on each of 256 CUs

    def __init__(self):
        super().__init__()
        self.seam_launches = 0
        self.expire_at = None
        self._expired_tag = 0

    def _seam_plan(self, n, dtype):
        blocks, per_lane = seam_geometry(int(n), 4 if dtype.itemsize == 4 else 2)
        return {"blocks": blocks, "per_lane": per_lane, "resident": self.RESIDENT,
                "fits": int(blocks <= self.RESIDENT and per_lane <= SEAM_CAP)}

    def _seam_attempt(self, k_last, c_last, e_pre, y0, f0, y1, out, a21, ws, ctrl, params, t_span_dev, step_t_dev, t_stage, *,
                      y0_alt=None, f0_alt=None):
        assert params.n_seg == 1 and (y0_alt is None) == (f0_alt is None)
        n = len(self.launches)
        sel = 1 if (y0_alt is not None and self._c(ctrl).accept) else 0  # the candidates this attempt ran on
        yb, fb = (y0_alt, f0_alt) if sel else (y0, f0)
        self.error_norm_partial([k_last], [c_last], y0, y1, params.rtol, params.atol, _hip.make_segments([(0, y0.numel())]), params.norm_kind,
                                ws, ctrl=ctrl, y0_alt=y0_alt, e_pre=e_pre)
        prior = self._expired_tag != 0
        if self.expire_at == self.seam_launches or prior:
            vals, nfs, kind, n_seg = self._slots[0]
            self._slots[0] = (vals, [nfs[0] + 1.0], kind, n_seg)
            if not prior:
                self._expired_tag = int(self._c(ctrl).seq) + 1
        self.rk_control(ctrl, params, ws, None, t_span_dev, step_t_dev, t_stage)
        # (y0', f0') = (y1, k_last) if the controller has just accepted, else the attempt's own; dt' = the step it planned
        self.stage_combine(out, yb, [fb], [a21], _hip.COMBINE_RK, ctrl=ctrl, y0_alt=y1, k0_alt=k_last)
        del self.launches[n:]
        self.launches.append("seam")
        self.seam_launches += 1

    def _seam_expired(self, ctrl):
        return self._expired_tag
