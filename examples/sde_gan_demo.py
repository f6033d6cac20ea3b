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
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlexde_amd.functional import cdeint, sdeint  # noqa: E402
from paddlexde_amd.interpolation import CubicHermiteSpline  # noqa: E402
from paddlexde_amd.solver import RK4, Euler  # noqa: E402


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

    def __init__(self, latent=4, hidden=16, noise=3, width=32):
        super().__init__()
        self.latent, self.hidden, self.noise = latent, hidden, noise
        self.init = nn.Linear(latent, hidden)
        self.f_net = nn.Sequential(nn.Linear(hidden, width), nn.Softplus(), nn.Linear(width, hidden), nn.Tanh())
        self.g_net = nn.Sequential(nn.Linear(hidden, width), nn.Softplus(), nn.Linear(width, hidden * noise), nn.Tanh())
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
        xs = sdeint(self.f, self.g, x0, t, solver=Euler, options=options)  # [B, T, D]
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


def train(iters=200, log_every=20, seed=0, device="cuda:0", batch=64, step_size=0.0625):
    """Alternate one discriminator and one generator step for ``iters`` iterations; returns one ``{"iters", "d_loss", "g_loss",
    "diffusion_grad"}`` per iteration, ``diffusion_grad`` the largest magnitude of the gradient the generator step left on the first
    weight of the generator's diffusion network."""
    torch.manual_seed(seed)
    t, real = make_data(device, batch=batch, seed=seed)
    gen, dis = Generator().to(device), Discriminator().to(device)
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
    a = ap.parse_args()
    hist = train(a.iters, step_size=a.step_size)
    print(json.dumps(hist[-1]))
