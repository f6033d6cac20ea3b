#!/usr/bin/env python3
"""Spiral neural-SDE demo on paddlexde_amd — counterpart of the reference's example/sde_demo.py.

Data: one sample path of ``dy = 2 y A dt + y dW`` (A = [[-0.1, 2], [-2, -0.1]], diagonal noise, the reference's Lambda_f / Lambda_g)
from y0 = [2, 0] over t in [0, 25], integrated by ``sdeint(..., solver=Euler)`` (Ito Euler-Maruyama).  ``--solver milstein`` trains
through the strong order 1.0 Milstein steps instead, ``--solver srk`` through the strong order 1.5 SRK steps and ``--solver rheun``
through the reversible Heun steps, which read the model as a Stratonovich equation (the data path stays Euler's).  ``--adjoint``
(with ``--solver rheun``) trains through ``sdeint_adjoint``: the same gradients up to rounding, from a backward sweep that recomputes
the path instead of keeping every step's operands.  Model (example/sde_demo.py:
SDEFunc / SDEDiffusion): an MLP drift on y^3 and an MLP diffusion on y^2, both trained by back-propagating through ``sdeint`` on
windows of ``batch_time`` points of the path (loss: mean |pred - data|).  Every call draws its own Brownian path from torch's
generator, so ``torch.manual_seed`` makes a run repeatable.

    python examples/sde_demo.py --max-steps 200 [--solver milstein | srk | rheun [--adjoint]]
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlexde_amd.functional import sdeint, sdeint_adjoint  # noqa: E402
from paddlexde_amd.solver import SRK, Euler, Milstein, ReversibleHeun  # noqa: E402

TRUE_A = [[-0.1, 2.0], [-2.0, -0.1]]


def _mlp():
    net = nn.Sequential(nn.Linear(2, 50), nn.Tanh(), nn.Linear(50, 2))
    for m in net:
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, mean=0.0, std=0.1)
            nn.init.zeros_(m.bias)
    return net


class SDEFunc(nn.Module):
    """The drift."""

    def __init__(self):
        super().__init__()
        self.net = _mlp()

    def forward(self, t, y):
        return self.net(y**3)


class SDEDiffusion(nn.Module):
    """The diffusion (diagonal: the state's shape)."""

    def __init__(self):
        super().__init__()
        self.net = _mlp()

    def forward(self, t, y):
        return self.net(y**2)


def make_data(device, data_size=1000, seed=0):
    A = torch.tensor(TRUE_A, device=device)
    t = torch.linspace(0.0, 25.0, data_size, device=device)
    with torch.no_grad():
        true_y = sdeint(lambda t_, y: torch.mm(2 * y, A), lambda t_, y: y, torch.tensor([[2.0, 0.0]], device=device), t, solver=Euler,
                        options={"norm": None, "seed": seed})  # [data_size, 2]
    return t, true_y


def get_batch(true_y, t, batch_size, batch_time, gen):
    s = torch.randperm(len(true_y) - batch_time, generator=gen)[:batch_size].to(true_y.device)
    batch_y0 = true_y[s][:, None, :]  # [B, 1, 2]
    batch_y = torch.stack([true_y[s + i] for i in range(batch_time)], dim=1)  # [B, T, 2]
    return batch_y0, t[:batch_time], batch_y


def train(max_steps=200, batch_size=20, batch_time=10, seed=42, device="cuda:0", log_every=50, solver=Euler, adjoint=False):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    t, true_y = make_data(device)
    func, diffusion = SDEFunc().to(device), SDEDiffusion().to(device)
    opt = torch.optim.RMSprop(list(func.parameters()) + list(diffusion.parameters()), lr=1e-3)
    losses = []
    t0 = time.perf_counter()
    for step in range(1, max_steps + 1):
        y0, bt, by = get_batch(true_y, t, batch_size, batch_time, gen)
        pred = (sdeint_adjoint if adjoint else sdeint)(func, diffusion, y0, bt, solver=solver)  # [B, T, 2]
        loss = torch.mean(torch.abs(pred - by))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if log_every and step % log_every == 0:
            print("Iter {:04d} | Total Loss {:.6f} | {:.1f} it/s".format(step, losses[-1], step / (time.perf_counter() - t0)), flush=True)
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--batch-size", type=int, default=20)
    ap.add_argument("--batch-time", type=int, default=10)
    ap.add_argument("--solver", choices=["euler", "milstein", "srk", "rheun"], default="euler")
    ap.add_argument("--adjoint", action="store_true", help="train through sdeint_adjoint (needs --solver rheun)")
    a = ap.parse_args()
    ls = train(a.max_steps, a.batch_size, a.batch_time, solver={"euler": Euler, "milstein": Milstein, "srk": SRK, "rheun": ReversibleHeun}[a.solver],
               adjoint=a.adjoint)
    print("first-10 mean loss {:.4f} -> last-10 mean loss {:.4f}".format(sum(ls[:10]) / 10, sum(ls[-10:]) / 10))
