#!/usr/bin/env python3
"""Latent-ODE style demo of per-sample output times: ``odeint(..., options={"t_eval": tq})``.

Data: spirals ``y' = (y^3) A`` from random starting points, every series observed at ITS OWN random times on [0, 4] — between 60 % and
100 % of ``Q`` observations per series, the rest of its row padded with NaN (NaturalCubicSpline's convention for a missing observation).
The "true" observations come from the same entry point: one joint Dopri5 solve whose dense output is read at every row's own times.

Model: an encoder takes a series' first observation to a latent state, a small MLP is the latent dynamics, a linear decoder reads the
observations off the latent path at the series' own times.  One ``odeint`` call per iteration: one step sequence for the batch, every
row written at its own times only, gradients through the accepted steps.  The union-of-times route would write ``rows * Q`` full
states for the same loss.

    python examples/latent_ode_demo.py --max-steps 200
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlexde_amd import Dopri5, odeint  # noqa: E402

T_END = 4.0


class LatentFunc(nn.Module):
    def __init__(self, latent=8, hidden=32):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(latent, hidden), nn.Tanh(), nn.Linear(hidden, latent))

    def forward(self, t, z):
        return self.net(z)


class Model(nn.Module):
    def __init__(self, latent=8):
        super().__init__()
        self.enc = nn.Sequential(nn.Linear(2, 32), nn.Tanh(), nn.Linear(32, latent))
        self.func = LatentFunc(latent)
        self.dec = nn.Linear(latent, 2)

    def forward(self, x0, tq, t_span):
        z = odeint(self.func, self.enc(x0), t_span, Dopri5, rtol=1e-4, atol=1e-6, options={"t_eval": tq})  # [Q, rows, latent]
        return self.dec(z)


def make_data(rows, Q, gen, device):
    """``(x0 [rows, 2], tq [rows, Q] with trailing NaN, obs [Q, rows, 2] with 0 where tq is NaN)``; column 0 is the start time."""
    A = torch.tensor([[-0.1, 2.0], [-2.0, -0.1]], device=device)
    angle = 6.2832 * torch.rand(rows, generator=gen)
    radius = 1.0 + torch.rand(rows, generator=gen)
    x0 = torch.stack([radius * torch.cos(angle), radius * torch.sin(angle)], dim=1).to(device)
    tq = torch.sort(T_END * torch.rand(rows, Q, generator=gen), dim=1).values
    tq[:, 0] = 0.0
    seen = torch.randint(int(0.6 * Q), Q + 1, (rows,), generator=gen)
    tq[torch.arange(Q)[None, :] >= seen[:, None]] = float("nan")
    tq = tq.to(device)
    with torch.no_grad():
        obs = odeint(lambda t, y: (y**3) @ A, x0, torch.tensor([0.0, T_END], device=device), Dopri5, rtol=1e-6, atol=1e-8,
                     options={"t_eval": tq})
    return x0, tq, obs


def train(max_steps=200, rows=64, Q=12, seed=0, device="cuda:0", log_every=20):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    x0, tq, obs = make_data(rows, Q, gen, device)
    t_span = torch.tensor([0.0, T_END], device=device)
    seen = ~torch.isnan(tq).t()[:, :, None]  # [Q, rows, 1]
    model = Model().to(device)
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    losses = []
    t0 = time.perf_counter()
    for step in range(1, max_steps + 1):
        pred = model(x0, tq, t_span)
        loss = (((pred - obs) ** 2) * seen).sum() / (2 * seen.sum())  # (the prediction at a padded entry is dec(0): masked out)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if log_every and step % log_every == 0:
            print("Iter {:04d} | masked MSE {:.6f} | {:.1f} it/s".format(step, losses[-1], step / (time.perf_counter() - t0)), flush=True)
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--queries", type=int, default=12)
    a = ap.parse_args()
    ls = train(a.max_steps, a.rows, a.queries)
    print("first-5 mean loss {:.4f} -> last-5 mean loss {:.4f}".format(sum(ls[:5]) / 5, sum(ls[-5:]) / 5))
