"""Stochastic-equation problem wrapper (reference: paddlexde/xde/base_sde.py:11-61).

``dy = f(t, y) dt + g(t, y) dW`` with diagonal noise: ``W`` has the state's shape and ``g(t, y)`` returns a tensor of ``y``'s shape
and dtype that multiplies the Brownian increment element by element.  ``move`` evaluates both coefficients and ``fuse`` is the Ito
Euler-Maruyama update ``(y0 + f*dt) + g*dW``, the step the reference meant (its ``move`` computes ``f(t0, y0)`` and
``g(t0, y0) * I_k`` with ``I_k = bm(t0, t1)``; its ``fuse`` is marked TODO).  The fixed-step solvers never call ``fuse``: they map a
``BaseSDE`` onto xde_sde_em_step (Euler), xde_sde_milstein_step (Milstein) or xde_sde_srk_step (SRK), which form ``dW = sqrt(|dt|) * Z`` from a counter-based generator inside the kernel (no Brownian
object: the noise of element e at grid step k is a function of (seed, k, e) — include/xde_hip_sde.h).

``noise_type="general"``: ``g(t, y)`` returns ``y.shape + (M,)`` and every row of the state (its last axis) is driven by an
M-dimensional Brownian motion through its ``[D, M]`` matrix; ``"scalar"`` is ``M == 1``.  Euler maps such a problem onto
xde_sde_gn_step (include/xde_hip_gn.h), whose normals are those of the flat ``[rows, M]`` array.
"""
import numpy as np
import torch

from .base_xde import BaseXDE

_SEED_LIMIT = 1 << 64


def draw_seed():
    """A 64-bit seed from torch's default CPU generator (``torch.manual_seed`` makes it repeatable)."""
    lo, hi = (int(x) for x in torch.randint(0, 1 << 32, (2,), dtype=torch.int64))
    return (hi << 32) | lo


def check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise TypeError("the SDE seed must be an integer, 0 <= seed < 2**64, got {!r}".format(seed))
    seed = int(seed)
    if not 0 <= seed < _SEED_LIMIT:
        raise ValueError("the SDE seed must satisfy 0 <= seed < 2**64, got {}".format(seed))
    return seed


NOISE_TYPES = ("diagonal", "general", "scalar")


def check_noise_type(noise_type):
    if noise_type not in NOISE_TYPES:
        raise ValueError("noise_type must be 'diagonal', 'general' or 'scalar', got {!r}".format(noise_type))
    return noise_type


class BaseSDE(BaseXDE):
    def __init__(self, f, g, y0, t_span, reverse=False, seed=None, prior=None, noise_type="diagonal"):
        super().__init__(name="SDE", var_nums=2, y0=y0, t_span=t_span)
        if isinstance(y0, (tuple, list)):
            raise NotImplementedError("BaseSDE takes a tensor y0, not a tuple: stack the members into one state tensor")
        self.__dict__["f"] = f  # (plain attributes: see BaseXDE.__init__)
        self.__dict__["g"] = g
        self.__dict__["h"] = prior  # the prior drift of a latent SDE (sdeint's options logqp / prior_drift), or None
        self.__dict__["seed"] = draw_seed() if seed is None else check_seed(seed)
        # "diagonal": g(t, y) has y's shape and W has the state's shape; "general": g(t, y) is y.shape + (M,) and every row of the state
        # (its last axis) is driven by an M-dimensional Brownian motion through its [D, M] matrix; "scalar": general noise with M = 1
        self.__dict__["noise_type"] = check_noise_type(noise_type)
        self.__dict__["noise_dim"] = 1 if noise_type == "scalar" else None  # M: fixed by the first evaluation of a general diffusion
        # `reverse` is accepted and has no effect, as in the reference (base_sde.py:40-41: `t_span.clip(0)`, result discarded)
        self.init_y0(y0)

    def init_y0(self, y0):
        self.__dict__["y0"] = y0

    def handle(self, h, ts):
        pass

    def diffusion(self, t, y):
        """``g(t, y)``, checked: a tensor of y's shape and dtype (diagonal noise).  Milstein's support evaluation and SRK's stage evaluations call it too."""
        g = self.g(t, y)
        if self.noise_type != "diagonal":
            return self._matrix_diffusion(g, y)
        if not torch.is_tensor(g) or g.shape != y.shape or g.dtype != y.dtype:
            got = "{} {}".format(tuple(g.shape), g.dtype) if torch.is_tensor(g) else type(g).__name__
            raise ValueError("the diffusion g(t, y) must return a tensor of y's shape {} and dtype {} (diagonal noise), got {}".format(
                tuple(y.shape), y.dtype, got))
        return g

    def _matrix_diffusion(self, g, y):
        """The check of a general or scalar diffusion: a tensor of shape ``y.shape + (M,)`` and y's dtype, ``M >= 1`` the same at every
        evaluation (scalar: 1)."""
        M = self.noise_dim
        ok = torch.is_tensor(g) and g.dtype == y.dtype and g.dim() == y.dim() + 1 and g.shape[:-1] == y.shape and g.shape[-1] >= 1
        if ok and M is None:
            self.__dict__["noise_dim"] = M = int(g.shape[-1])
        if not ok or g.shape[-1] != M:
            got = "{} {}".format(tuple(g.shape), g.dtype) if torch.is_tensor(g) else type(g).__name__
            want = "(M,) with M >= 1" if M is None else "({},)".format(M)
            raise ValueError("the diffusion g(t, y) must return a tensor of y's shape {} + {} and dtype {} ({} noise), got {}".format(
                tuple(y.shape), want, y.dtype, self.noise_type, got))
        return g

    def prior(self, t, y):
        """``h(t, y)``, the prior drift of a latent SDE, checked as ``diffusion`` checks ``g``: a tensor of y's shape and dtype."""
        if self.h is None:
            raise ValueError("this BaseSDE has no prior drift: pass prior= (sdeint: options={'logqp': True, 'prior_drift': h})")
        h = self.h(t, y)
        if not torch.is_tensor(h) or h.shape != y.shape or h.dtype != y.dtype:
            got = "{} {}".format(tuple(h.shape), h.dtype) if torch.is_tensor(h) else type(h).__name__
            raise ValueError("the prior drift h(t, y) must return a tensor of y's shape {} and dtype {}, got {}".format(
                tuple(y.shape), y.dtype, got))
        return h

    def move(self, t0, dt, y0):
        """base_sde.py:43-58 — the drift and the diffusion at (t0, y0); the solver draws the increment."""
        return self.f(t0, y0), self.diffusion(t0, y0)

    def fuse(self, dy, dt, y0):
        """Euler-Maruyama: ``dy = (f, g, dW)`` -> ``(y0 + f*dt) + g*dW`` (the kernel's op order, with ``dW = s*Z``)."""
        f, g, dw = dy
        if self.noise_type != "diagonal":
            # general / scalar: g is [.., D, M] and dw [.., M]; the sum over m sequential, as xde_sde_gn_step takes it
            a = g[..., 0] * dw[..., 0:1]
            for m in range(1, g.shape[-1]):
                a = a + g[..., m] * dw[..., m : m + 1]
            return (y0 + f * dt) + a
        return (y0 + f * dt) + g * dw

    def call_func(self, t, y0):
        return self.f(t, y0)
