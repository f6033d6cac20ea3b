#!/usr/bin/env python3
"""SDE-GAN demo on paddlexde_amd: a neural SDE with GENERAL noise as the generator and a neural CDE on its sample paths as the
discriminator (Kidger, Foster, Li, Oberhauser, Lyons, "Neural SDEs as Infinite-Dimensional GANs", ICML 2021), at toy size.

Data: ``batch`` Ornstein-Uhlenbeck series at ``T`` times, generated from a seed.  Generator: a seeded latent ``v`` gives the initial
hidden state ``x0 = init(v)``; the hidden state (D dimensions) follows ``dx = f(t, x) dt + g(t, x) dW`` with an M-dimensional Brownian
motion and a ``[D, M]`` diffusion matrix,

    xs = sdeint(f, g, x0, t, solver=Euler, options={"noise_type": "general", "step_size": dt})

— one fused launch per step that streams ``g`` once — and a linear read-out gives the series.  Discriminator: the generated (or real)
series with time as a channel is the control of a neural CDE, ``CubicHermiteSpline(series, differentiable=True)``, so the score's
gradient flows back through ``cdeint`` and the control into the generator's drift and diffusion.  Trained as a Wasserstein GAN with
weight clipping, one discriminator step and one generator step per iteration.

    python examples/sde_gan_demo.py --iters 200
    python examples/sde_gan_demo.py --iters 200 --solver heun

``--solver heun`` reads the generator's equation in the Stratonovich sense, as the paper does, with the trapezoidal ``solver=Heun``:
two launches per step that stream ``g`` twice.  The default is Ito Euler-Maruyama.

    python examples/sde_gan_demo.py --iters 200 --solver grheun --adjoint

``--solver grheun`` is the paper's own scheme, reversible Heun on the ``[D, M]`` diffusion (``solver=GeneralReversibleHeun``:
Stratonovich, one evaluation per step), and ``--adjoint`` trains the generator through ``sdeint_adjoint``, whose backward recomputes
the path instead of keeping it: memory that does not grow with the number of steps.

    python examples/sde_gan_demo.py --iters 200 --fused-head

``--fused-head`` declares the generator's diffusion as an ``SDELinearHead``: under Euler its last layer, the ``tanh``, the product with
the Brownian increment and the update are one launch per step, and the ``[B, D, M]`` matrix is neither written nor kept for the
backward.  Heun and reversible Heun evaluate the same module as the plain composition.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlexde_amd.functional import cdeint, sdeint, sdeint_adjoint  # noqa: E402
from paddlexde_amd.interpolation import CubicHermiteSpline  # noqa: E402
from paddlexde_amd.solver import RK4, Euler, GeneralReversibleHeun, Heun  # noqa: E402
from paddlexde_amd.xde import SDELinearHead  # noqa: E402


def make_data(device, batch=64, T=17, t1=2.0, theta=1.0, mu=0.0, sigma=0.5, seed=0):
    """``batch`` Ornstein-Uhlenbeck series ``[batch, T]`` at ``T`` times, from the exact transition law, drawn from ``seed``."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.linspace(0.0, t1, T)
    x = torch.empty(batch, T)
    x[:, 0] = mu + 0.5 * torch.randn(batch, generator=gen)
    for i in range(1, T):
        a = math.exp(-theta * float(t[i] - t[i - 1]))
        sd = sigma * math.sqrt((1.0 - a * a) / (2.0 * theta))
        x[:, i] = mu + (x[:, i - 1] - mu) * a + sd * torch.randn(batch, generator=gen)
    return t.to(device), x.to(device)


class Generator(nn.Module):
    """latent [B, V] -> series [B, T]: hidden state D, Brownian motion M, diffusion ``[B, 1, D, M]``."""

    def __init__(self, latent=4, hidden=16, noise=3, width=32, solver=Euler, adjoint=False, fused_head=False):
        super().__init__()
        self.latent, self.hidden, self.noise, self.solver, self.adjoint = latent, hidden, noise, solver, adjoint
        self.init = nn.Linear(latent, hidden)
        self.f_net = nn.Sequential(nn.Linear(hidden, width), nn.Softplus(), nn.Linear(width, hidden), nn.Tanh())
        self.g_net = nn.Sequential(nn.Linear(hidden, width), nn.Softplus(), nn.Linear(width, hidden * noise), nn.Tanh())
        # the same network with its last layer declared (and shared: g_net[2] IS the head's linear layer), for the one-launch step
        self.g_head = None
        if fused_head:
            self.g_head = SDELinearHead(lambda t, x: self.g_net[1](self.g_net[0](x)), width, hidden, noise)
            self.g_head.head = self.g_net[2]
        self.readout = nn.Linear(hidden, 1)

    def f(self, t, x):
        return self.f_net(x)

    def g(self, t, x):
        return self.g_net(x).reshape(x.shape + (self.noise,))

    def forward(self, v, t, step_size, seed=None):
        x0 = self.init(v).unsqueeze(1)  # [B, 1, D]
        options = {"norm": None, "noise_type": "general", "interp": "linear"}
        if step_size:
            options["step_size"] = step_size
        if seed is not None:
            options["seed"] = seed
        g = self.g if self.g_head is None else self.g_head
        if self.adjoint and torch.is_grad_enabled():
            params = tuple(self.f_net.parameters()) + tuple(self.g_net.parameters())
            xs = sdeint_adjoint(self.f, self.g, x0, t, solver=self.solver, options=options, adjoint_params=params)
        else:
            xs = sdeint(self.f, g, x0, t, solver=self.solver, options=options)  # [B, T, D]
        return self.readout(xs).squeeze(-1)  # [B, T]


class Discriminator(nn.Module):
    """series [B, T] -> score [B]: a neural CDE driven by the cubic Hermite spline through ``(time, value)``."""

    CHANNELS = 2

    def __init__(self, hidden=8, width=32):
        super().__init__()
        self.initial = nn.Linear(self.CHANNELS, hidden)
        self.net = nn.Sequential(nn.Linear(hidden, width), nn.Tanh(), nn.Linear(width, hidden * self.CHANNELS), nn.Tanh())
        self.readout = nn.Linear(hidden, 1)

    def field(self, t, z):
        return self.net(z).reshape(z.shape + (self.CHANNELS,))

    def forward(self, t, x):
        series = torch.stack([t[None, :].expand_as(x), x], dim=-1)  # [B, T, 2]
        X = CubicHermiteSpline(series, differentiable=True)  # (stays on the series' autograd graph: the generator is behind it)
        knots = X.grid_points
        z0 = self.initial(series[:, 0, :])
        zT = cdeint(self.field, X, z0, knots, RK4).reshape(knots.numel(), *z0.shape)[-1]
        return self.readout(zT)[:, 0]

    def clip(self, bound=1.0):
        with torch.no_grad():
            for p in self.parameters():
                p.clamp_(-bound, bound)


def train(iters=200, log_every=20, seed=0, device="cuda:0", batch=64, step_size=0.0625, solver=Euler, adjoint=False, fused_head=False):
    """Alternate one discriminator and one generator step for ``iters`` iterations; returns one ``{"iters", "d_loss", "g_loss",
    "diffusion_grad"}`` per iteration, ``diffusion_grad`` the largest magnitude of the gradient the generator step left on the first
    weight of the generator's diffusion network."""
    torch.manual_seed(seed)
    t, real = make_data(device, batch=batch, seed=seed)
    gen, dis = Generator(solver=solver, adjoint=adjoint, fused_head=fused_head).to(device), Discriminator().to(device)
    g_opt = torch.optim.Adam(gen.parameters(), lr=2e-3, betas=(0.5, 0.9))
    d_opt = torch.optim.Adam(dis.parameters(), lr=4e-3, betas=(0.5, 0.9))
    latents = torch.Generator().manual_seed(seed + 1)
    history = []
    for it in range(1, iters + 1):
        v = torch.randn(batch, gen.latent, generator=latents).to(device)
        # the discriminator's step: the generated paths are data here
        with torch.no_grad():
            fake = gen(v, t, step_size)
        d_loss = dis(t, fake).mean() - dis(t, real).mean()
        d_opt.zero_grad()
        d_loss.backward()
        d_opt.step()
        dis.clip()
        # the generator's step: through the discriminator's CDE and its control, into the SDE's steps
        g_loss = -dis(t, gen(v, t, step_size)).mean()
        g_opt.zero_grad()
        g_loss.backward()
        grad = gen.g_net[0].weight.grad
        g_opt.step()
        history.append({"iters": it, "d_loss": d_loss.item(), "g_loss": g_loss.item(),
                        "diffusion_grad": 0.0 if grad is None else float(grad.abs().max())})
        if log_every and it % log_every == 0:
            print("Iter {iters:04d} | d_loss {d_loss:.4f} | g_loss {g_loss:.4f} | max |grad g_net| {diffusion_grad:.3e}".format(**history[-1]),
                  flush=True)
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-size", type=float, default=0.0625, help="the generator's grid step under the observation times (0: step on the times)")
    ap.add_argument("--solver", choices=("euler", "heun", "grheun"), default="euler",
                    help="the generator's scheme: Ito Euler-Maruyama, Stratonovich Heun, or Stratonovich reversible Heun")
    ap.add_argument("--adjoint", action="store_true", help="with --solver grheun: train through sdeint_adjoint (constant memory)")
    ap.add_argument("--fused-head", action="store_true", help="the generator's diffusion as an SDELinearHead: one launch per Euler step")
    a = ap.parse_args()
    hist = train(a.iters, step_size=a.step_size, solver={"euler": Euler, "heun": Heun, "grheun": GeneralReversibleHeun}[a.solver], adjoint=a.adjoint,
                 fused_head=a.fused_head)
    print(json.dumps(hist[-1]))
