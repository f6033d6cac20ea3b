#!/usr/bin/env python3
"""A delayed-feedback system with a LEARNED delay on paddlexde_amd: ``y'(t) = f(y(t), y(t - tau))``, trained through
``ddeint_steps(RK4)``.

Unlike examples/dde_demo.py, whose delayed states are gathered once from the history and stay fixed during the solve, the delay here
reaches into the solution being computed: the window moves with ``t``, over a roll-out longer than the history.

Data: ``y' = -1.5 tanh(y(t - 1)) - 0.2 y`` from a batch of initial functions ``a cos(2 t) + c`` on ``[-1.5, 0]``, solved with the same
call at the true delay.  Model: a small MLP on ``(y, y(t - tau))`` and the delay ``tau`` itself, started at 0.6; the loss is the mean
absolute error of the path on ``[0, 2]``.  The delay's gradient comes out of the Hermite tape (``d y(t - tau) / d tau = -H'(t - tau)``,
one launch per stage) and is summed by xde_lag_grad.

    python examples/dde_steps_demo.py --iters 200
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlexde_amd import RK4  # noqa: E402
from paddlexde_amd.functional import ddeint_steps  # noqa: E402

STEP = 0.125  # the grid step: a delay must stay at least this long
MAX_DELAY = 1.5  # the history's length


class Field(nn.Module):
    def __init__(self, D=2, hidden=16):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(2 * D, hidden), nn.Tanh(), nn.Linear(hidden, D))

    def forward(self, t, y, y_lags):
        """y [B, 1, D], y_lags [B, 1, D] (the state one delay ago) -> [B, 1, D]"""
        return self.net(torch.cat([y, y_lags], dim=-1))


def make_data(device, batch=16, D=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    a, c = torch.rand(batch, 1, D, generator=g) + 0.5, torch.randn(batch, 1, D, generator=g) * 0.5
    his_span = torch.linspace(-MAX_DELAY, 0.0, 13)
    s = his_span.view(1, -1, 1)
    his, his_d = a * torch.cos(2 * s) + c, -2 * a * torch.sin(2 * s)
    t_span = torch.linspace(0.0, 2.0, 17)
    his, his_d = his.to(device), his_d.to(device)
    with torch.no_grad():
        truth = ddeint_steps(lambda t, y, yl: -1.5 * torch.tanh(yl) - 0.2 * y, his, his_span, t_span, torch.tensor([1.0]), solver=RK4,
                             his_derivative=his_d)
    return his, his_d, his_span, t_span, truth


def train(iters=200, lr=2e-2, seed=0, device="cuda:0", log_every=20):
    torch.manual_seed(seed)
    his, his_d, his_span, t_span, truth = make_data(device, seed=seed)
    field = Field().to(device)
    delay = torch.tensor([0.6], device=device, requires_grad=True)
    opt = torch.optim.Adam(list(field.parameters()) + [delay], lr=lr)
    hist, t0 = [], time.perf_counter()
    for it in range(1, iters + 1):
        pred = ddeint_steps(field, his, his_span, t_span, delay, solver=RK4, his_derivative=his_d)
        loss = (pred - truth).abs().mean()
        opt.zero_grad()
        loss.backward()
        hist.append({"iters": it, "loss": loss.item(), "delay": delay.item(), "delay_grad": delay.grad.item()})
        opt.step()
        with torch.no_grad():
            delay.clamp_(STEP, MAX_DELAY)
        if log_every and it % log_every == 0:
            print("Iter {:04d} | loss {:.5f} | delay {:.4f} | {:.1f} it/s".format(it, hist[-1]["loss"], hist[-1]["delay"],
                                                                                 it / (time.perf_counter() - t0)), flush=True)
    return hist


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    h = train(args.iters, device=args.device)
    print("loss {:.5f} -> {:.5f}; delay 0.6 -> {:.4f} (true 1.0)".format(h[0]["loss"], h[-1]["loss"], h[-1]["delay"]))
