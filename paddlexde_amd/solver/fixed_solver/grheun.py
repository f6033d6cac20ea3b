"""GeneralReversibleHeun: the reversible Heun scheme under general and scalar noise (FixedSolver._rheun_step's matrix-noise branch) —
what ``sdeint_adjoint`` differentiates in constant memory when the diffusion is a ``[D, M]`` matrix per row."""
from .rheun import ReversibleHeun


class GeneralReversibleHeun(ReversibleHeun):
    """ReversibleHeun that also steps ``options={"noise_type": "general" | "scalar"}``: ``yh1 = 2 y0 - yh0 + fh0 dt + gh0 dW`` and
    ``y1 = y0 + (fh0 + fh1) dt/2 + (gh0 dW + gh1 dW)/2`` with ``gh dW`` the sequential sum over the M columns (include/xde_hip_gn.h).
    STRATONOVICH, one drift and one diffusion evaluation per step, strong order 1/2 in general.  The step carries ``a = gh dW`` besides
    ``(yh, fh, gh)``, so each diffusion matrix is streamed once per product; where nothing is differentiated one launch does step k's
    corrector and step k + 1's predictor in a single pass over ``gh1``.  Under diagonal noise it is its parent: the same launches,
    the same bits.  ``logqp``, ``pipeline="graph"``, ``interp="cubic"`` and an ODE are refused as for the parent."""

    steps_matrix_noise = True
