#!/usr/bin/env python3
"""Neural-CDE demo on paddlexde_amd: tell clockwise spirals from anticlockwise ones.

Data (generated from a seed, nothing downloaded): ``n`` spirals of ``length`` points ``(time, x, y)`` with a random phase and a little
noise, half of them turning each way.  Model: the control ``X`` is the cubic Hermite spline through each series (time is a channel, the
knots are the unit grid); ``z0 = initial(X.evaluate(t0))``, ``dz = f_theta(z) dX`` with an MLP field returning ``[B, H, C]``, and a
linear read-out of ``z`` at the last time gives the logit (loss: binary cross-entropy).  Trained through ``cdeint`` with RK4 on the
knots (gradients through the steps), or with ``--adjoint`` through ``cdeint_adjoint`` with Dopri5 (the continuous adjoint).

``--control natural`` drives the model with ``NaturalCubicSpline`` instead: the C2 natural cubic spline through the observed points, on
the series' own times.  With it ``--irregular`` samples the spirals at times drawn from the seed (not ``linspace``) and ``--missing P``
sets a share ``P`` of the x / y entries to NaN ("not observed"), also from the seed.

``--encoder`` puts a small trainable map in front of the spline — a per-channel affine on x and y (time, the knots' channel, passes
through; unobserved entries stay unobserved) — and trains it through the control: the spline is rebuilt from the encoded series each
iteration with ``differentiable=True``, and ``cdeint`` / ``cdeint_adjoint`` carry the loss gradient back to the series.

``--logsig DEPTH --window L`` is the log-ODE method for long series: a spiral of ``8 * length + 1`` points is cut into windows of ``L``
steps, each replaced by its depth-``DEPTH`` logsignature (``logsig_path``: increments and, at depth 2, Levy areas), and the CDE is solved
with one RK4 step per window on the piecewise linear path through them; the field then has ``logsignature_channels(3, DEPTH)`` columns.

    python examples/cde_demo.py --max-steps 60 [--adjoint] [--control natural [--irregular] [--missing 0.3]] [--encoder]
    python examples/cde_demo.py --max-steps 60 --logsig 2 --window 8
"""
import argparse
import math
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlexde_amd.functional import cdeint, cdeint_adjoint  # noqa: E402
from paddlexde_amd.interpolation import (CubicHermiteSpline, LinearInterpolation, NaturalCubicSpline, logsig_path,  # noqa: E402
                                         logsignature_channels)
from paddlexde_amd.solver import RK4, Dopri5  # noqa: E402

CHANNELS = 3  # (time, x, y)


def make_data(n=128, length=32, seed=0, device="cuda:0", irregular=False, missing=0.0):
    """series [n, length, 3] and labels [n] (1: clockwise).  ``irregular``: the sample times are drawn from the seed (the ends stay 0
    and 4 pi); ``missing``: that share of the x / y entries after the first row is NaN, drawn from the seed."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.linspace(0.0, 4.0 * math.pi, length)
    extra = torch.Generator().manual_seed(seed + 1)  # (its own stream: the draws below are the same with and without the options)
    if irregular:
        # each interior time moves up to 0.4 of a grid step either way: spacings between 0.2 and 1.8 steps
        jitter = 0.8 * (torch.rand(length - 2, generator=extra) - 0.5)
        t = t + (4.0 * math.pi / (length - 1)) * torch.cat([torch.zeros(1), jitter, torch.zeros(1)])
    phase = 2.0 * math.pi * torch.rand(n, 1, generator=gen)
    labels = (torch.arange(n) % 2).float()
    sign = (1.0 - 2.0 * labels)[:, None]  # anticlockwise: +1, clockwise: -1
    r = 1.0 / (1.0 + 0.2 * t)[None, :]
    x = r * torch.cos(phase + sign * t[None, :]) + 0.01 * torch.randn(n, length, generator=gen)
    y = r * torch.sin(phase + sign * t[None, :]) + 0.01 * torch.randn(n, length, generator=gen)
    if missing > 0.0:
        gone = torch.rand(n, length, 2, generator=extra) < missing
        gone[:, 0, :] = False  # (every column keeps an observed value)
        x = x.masked_fill(gone[..., 0], float("nan"))
        y = y.masked_fill(gone[..., 1], float("nan"))
    series = torch.stack([t[None, :].expand(n, -1), x, y], dim=-1)
    return series.to(device), labels.to(device)


class CDEFunc(nn.Module):
    """f_theta: z [B, H] -> [B, H, C] (``channels``: the control's, K of a logsignature path)."""

    def __init__(self, hidden, channels=CHANNELS):
        super().__init__()
        self.channels = channels
        self.net = nn.Sequential(nn.Linear(hidden, 32), nn.Tanh(), nn.Linear(32, hidden * channels), nn.Tanh())

    def forward(self, t, z):
        return self.net(z).reshape(z.shape + (self.channels,))


class ChannelAffine(nn.Module):
    """series [B, T, C] -> the same with x and y scaled and shifted per channel (starts as the identity).  Time passes through; a NaN
    entry stays NaN and takes no part in the gradient."""

    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(CHANNELS - 1))
        self.shift = nn.Parameter(torch.zeros(CHANNELS - 1))

    def forward(self, series):
        seen = ~torch.isnan(series)
        filled = torch.nan_to_num(series, nan=0.0)
        mapped = torch.cat([filled[..., :1], filled[..., 1:] * self.scale + self.shift], dim=-1)
        return torch.where(seen, mapped, series)


class NeuralCDE(nn.Module):
    def __init__(self, hidden=8, encoder=False, channels=CHANNELS):
        super().__init__()
        self.initial = nn.Linear(CHANNELS, hidden)
        self.func = CDEFunc(hidden, channels)
        self.readout = nn.Linear(hidden, 1)
        if encoder:
            self.encoder = ChannelAffine()

    def forward(self, X, adjoint=False, first=None):
        """``first``: the control's value at the first knot where ``X.evaluate`` is not differentiable (a differentiable cubic
        Hermite control: it is the series' first row)."""
        knots = X.grid_points
        z0 = self.initial(X.evaluate(knots[:1])[:, 0, :] if first is None else first)  # [B, H]
        if adjoint:
            zT = cdeint_adjoint(self.func, X, z0, knots[[0, -1]], solver=Dopri5, rtol=1e-3, atol=1e-5)[-1]
        else:
            zT = cdeint(self.func, X, z0, knots, RK4).reshape(knots.numel(), *z0.shape)[-1]  # (fixed solvers stack time on axis -2)
        return self.readout(zT)[:, 0]


def train(max_steps=60, n=128, length=32, hidden=8, seed=0, device="cuda:0", adjoint=False, log_every=10, control="cubic", irregular=False,
          missing=0.0, encoder=False, logsig=0, window=8):
    if logsig:
        if adjoint or encoder or irregular or missing > 0.0 or control != "cubic":
            raise ValueError("--logsig runs on its own: RK4 on the piecewise linear path through the windows' logsignatures")
        return train_logsig(max_steps, n, 8 * length + 1, hidden, seed, device, log_every, logsig, window)
    if control not in ("cubic", "natural"):
        raise ValueError("control must be 'cubic' or 'natural', got {!r}".format(control))
    if control == "cubic" and (irregular or missing > 0.0):
        raise ValueError("irregular times and missing values need control='natural': CubicHermiteSpline keeps the reference's "
                         "uniform-grid conventions and has no notion of an unobserved entry")
    torch.manual_seed(seed)
    series, labels = make_data(n, length, seed, device, irregular, missing)
    make = (lambda x, **kw: CubicHermiteSpline(x, **kw)) if control == "cubic" else (
        lambda x, **kw: NaturalCubicSpline(x, series[0, :, 0], **kw))  # (channel 0 is the time)
    X = None if encoder else make(series)
    model = (NeuralCDE(hidden, encoder=True) if encoder else NeuralCDE(hidden)).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    t0 = time.perf_counter()
    for step in range(1, max_steps + 1):
        if encoder:
            # the control comes from something that is trained: rebuilt each iteration, attached to the encoder's graph
            encoded = model.encoder(series)
            logits = model(make(encoded, differentiable=True), adjoint, first=encoded[:, 0, :] if control == "cubic" else None)
        else:
            logits = model(X, adjoint)
        loss = nn.functional.binary_cross_entropy_with_logits(logits, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if log_every and step % log_every == 0:
            acc = ((logits > 0).float() == labels).float().mean().item()
            print("Iter {:04d} | Loss {:.6f} | Accuracy {:.3f} | {:.1f} it/s".format(step, losses[-1], acc, step / (time.perf_counter() - t0)),
                  flush=True)
    return losses


def train_logsig(max_steps, n, length, hidden, seed, device, log_every, depth, window):
    """The log-ODE method: the control is the piecewise linear path through the cumulated logsignatures of the windows (built once: the
    series is data), the field has one column per logsignature channel, and RK4 takes one step per window."""
    torch.manual_seed(seed)
    series, labels = make_data(n, length, seed, device)
    X = LinearInterpolation(logsig_path(series, depth, window))
    model = NeuralCDE(hidden, channels=logsignature_channels(CHANNELS, depth)).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    t0 = time.perf_counter()
    for step in range(1, max_steps + 1):
        logits = model(X, first=series[:, 0, :])
        loss = nn.functional.binary_cross_entropy_with_logits(logits, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if log_every and step % log_every == 0:
            acc = ((logits > 0).float() == labels).float().mean().item()
            print("Iter {:04d} | Loss {:.6f} | Accuracy {:.3f} | {:.1f} it/s | {} points -> {} windows".format(
                step, losses[-1], acc, step / (time.perf_counter() - t0), length, X.grid_points.numel() - 1), flush=True)
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-steps", type=int, default=60)
    ap.add_argument("--adjoint", action="store_true", help="train through cdeint_adjoint (Dopri5) instead of cdeint (RK4)")
    ap.add_argument("--control", choices=("cubic", "natural"), default="cubic", help="the control path through the series")
    ap.add_argument("--irregular", action="store_true", help="sample times drawn from the seed (needs --control natural)")
    ap.add_argument("--missing", type=float, default=0.0, metavar="P", help="share of x / y entries set to NaN (needs --control natural)")
    ap.add_argument("--encoder", action="store_true", help="train a per-channel affine in front of the spline through differentiable=True")
    ap.add_argument("--logsig", type=int, default=0, metavar="DEPTH", help="the log-ODE method: windows of logsignatures of this depth (1 or 2)")
    ap.add_argument("--window", type=int, default=8, metavar="L", help="steps per logsignature window (with --logsig)")
    a = ap.parse_args()
    ls = train(a.max_steps, adjoint=a.adjoint, control=a.control, irregular=a.irregular, missing=a.missing, encoder=a.encoder,
               logsig=a.logsig, window=a.window)
    print("first loss {:.4f} -> last loss {:.4f}".format(ls[0], ls[-1]))
