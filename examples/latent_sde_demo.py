#!/usr/bin/env python3
"""Latent SDE demo on paddlexde_amd: a variational fit of noisy Ornstein-Uhlenbeck series (Li, Wong, Chen, Duvenaud, "Scalable Gradients
for Stochastic Differential Equations", AISTATS 2020, section 5).

Data: ``batch`` series of ``dx = theta (mu - x) dt + sigma dW`` observed with noise at ``T`` times, generated from a seed.  Model: an
encoder (a GRU read backwards over the series) gives the mean and scale of ``q(z0)``; the latent path follows the posterior SDE
``dz = f(t, z, ctx) dt + g(z) dW``, the prior is ``dz = h(t, z) dt + g(z) dW`` with the SAME diagonal diffusion ``g`` (bounded away from
zero), and a linear decoder reads ``x`` off ``z``.  The loss is the reconstruction term plus the KL divergence between the two path
measures, which ``sdeint(..., options={"logqp": True, "prior_drift": h})`` accumulates inside its step launch, plus the KL of ``z0``:

    zs, logqp = sdeint(f, g, z0, t, solver=Euler, options={"logqp": True, "prior_drift": h, "step_size": dt})
    loss = recon(zs) + logqp.sum(-1).mean() + kl(z0)

    python examples/latent_sde_demo.py --iters 200 [--solver euler | milstein] [--step-size 0.05]
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlexde_amd.functional import sdeint  # noqa: E402
from paddlexde_amd.solver import Euler, Milstein  # noqa: E402

SOLVERS = {"euler": Euler, "milstein": Milstein}


def make_data(device, batch=64, T=21, t1=2.0, theta=1.5, mu=0.5, sigma=0.4, obs_noise=0.05, seed=0):
    """``batch`` noisy Ornstein-Uhlenbeck series at ``T`` times: the exact transition law, drawn from ``seed``."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.linspace(0.0, t1, T)
    x = torch.empty(batch, T)
    x[:, 0] = mu + torch.randn(batch, generator=gen)
    for i in range(1, T):
        a = math.exp(-theta * float(t[i] - t[i - 1]))
        sd = sigma * math.sqrt((1.0 - a * a) / (2.0 * theta))
        x[:, i] = mu + (x[:, i - 1] - mu) * a + sd * torch.randn(batch, generator=gen)
    x = x + obs_noise * torch.randn(batch, T, generator=gen)
    return t.to(device), x.to(device)


class LatentSDE(nn.Module):
    def __init__(self, latent=4, ctx=8, hidden=32):
        super().__init__()
        self.latent = latent
        self.encoder = nn.GRU(1, hidden, batch_first=True)
        self.q_z0 = nn.Linear(hidden, 2 * latent)
        self.ctx = nn.Linear(hidden, ctx)
        self.f_net = nn.Sequential(nn.Linear(latent + ctx, hidden), nn.Softplus(), nn.Linear(hidden, latent))  # posterior drift
        self.h_net = nn.Sequential(nn.Linear(latent, hidden), nn.Softplus(), nn.Linear(hidden, latent))  # prior drift
        self.g_net = nn.Sequential(nn.Linear(latent, hidden), nn.Softplus(), nn.Linear(hidden, latent))  # the shared diagonal diffusion
        self.decoder = nn.Linear(latent, 1)
        self.pz0_mean = nn.Parameter(torch.zeros(latent))
        self.pz0_logstd = nn.Parameter(torch.zeros(latent))
        self._c = None

    def f(self, t, z):  # [B, 1, latent]
        return self.f_net(torch.cat([z, self._c], dim=-1))

    def h(self, t, z):
        return self.h_net(z)

    def g(self, t, z):
        return 0.1 + torch.sigmoid(self.g_net(z))  # non-zero: the KL term divides by it

    def forward(self, t, x, solver, step_size, obs_std=0.05):
        """``(loss, recon, kl)`` of one batch of series ``x`` [B, T] at times ``t``."""
        out, _ = self.encoder(torch.flip(x, dims=(1,)).unsqueeze(-1))
        last = out[:, -1]  # the GRU's state after reading the series back to its start
        self._c = self.ctx(last).unsqueeze(1)
        mean, logstd = self.q_z0(last).chunk(2, dim=-1)
        z0 = (mean + torch.randn_like(mean) * logstd.exp()).unsqueeze(1)  # [B, 1, latent]
        options = {"norm": None, "logqp": True, "prior_drift": self.h, "interp": "linear"}
        if step_size:
            options["step_size"] = step_size
        zs, logqp = sdeint(self.f, self.g, z0, t, solver=solver, options=options)  # [B, T, latent], [B, 1, T-1]
        xs = self.decoder(zs).squeeze(-1)  # [B, T]
        recon = (0.5 * ((xs - x) / obs_std) ** 2 + math.log(obs_std) + 0.5 * math.log(2 * math.pi)).sum(-1).mean()
        # KL(q(z0) || p(z0)) of two diagonal normals
        var_ratio = (2 * (logstd - self.pz0_logstd)).exp()
        kl_z0 = (0.5 * (var_ratio + ((mean - self.pz0_mean) / self.pz0_logstd.exp()) ** 2 - 1.0) - (logstd - self.pz0_logstd)).sum(-1).mean()
        kl = logqp.sum(-1).mean() + kl_z0
        return recon + kl, recon, kl


def train(iters=200, solver=Euler, step_size=0.05, seed=0, device="cuda:0", log_every=20, batch=64):
    """Fit the model for ``iters`` steps of Adam; returns one ``{"iters", "loss", "recon", "kl"}`` per step."""
    torch.manual_seed(seed)
    t, x = make_data(device, batch=batch, seed=seed)
    model = LatentSDE().to(device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    history = []
    for it in range(1, iters + 1):
        loss, recon, kl = model(t, x, solver, step_size)
        opt.zero_grad()
        loss.backward()
        opt.step()
        history.append({"iters": it, "loss": loss.item(), "recon": recon.item(), "kl": kl.item()})
        if log_every and it % log_every == 0:
            print("Iter {iters:04d} | loss {loss:.4f} | recon {recon:.4f} | kl {kl:.4f}".format(**history[-1]), flush=True)
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--solver", choices=sorted(SOLVERS), default="euler")
    ap.add_argument("--step-size", type=float, default=0.05, help="the solver's grid step under the observation times (0: step on the times)")
    a = ap.parse_args()
    hist = train(a.iters, SOLVERS[a.solver], a.step_size)
    print(json.dumps(hist[-1]))
