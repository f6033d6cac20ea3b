"""A neural ODE's vector field as a small multi-layer perceptron whose every evaluation without a tape is ONE launch.

``MLPField(in_features, hidden, out_features)`` owns ordinary ``nn.Linear`` layers (``self.layers``) and computes

    L_n(act(L_{n-1}(... act(L_1(x)) ...))),        x = y, or y with t appended as one more input column (``time=True``)

Called with grad mode on and anything that requires grad, on a tensor that is not float32 on a ROCm device, with ``fuse = False`` or
on a shape the kernel does not serve, it is exactly that composition of ``F.linear`` and ``torch.tanh``.  Everywhere else — the forward
solve of ``odeint_adjoint``, ``options={"per_sample": True}``, ``options={"t_eval": ...}``, inference under ``torch.no_grad()`` — the
whole network is one launch on the current stream (xde_mlp_field, include/xde_hip_mlp.h): the hidden activations stay in LDS, and any
solver, pipeline or captured graph that calls ``func(t, y)`` gets it without knowing.

``field.vjp(t, y, cotangent)`` is the adjoint method's half: the field recomputed and the cotangent carried back to the state, the time
and every parameter in two launches (xde_mlp_field_vjp), where the taped composition and ``torch.autograd.grad`` take 25 to 30.  Nothing
uses it unasked: pass it as ``odeint_adjoint(field, y0, t, adjoint_options={"vjp": field.vjp})`` or ``AdjointProblem(vjp=field.vjp)``.
It serves what ``forward`` serves as long as the widths sum to at most ``_hip.XDE_MLP_VJP_LDS_BYTES // 128``.

Not built: a fused tape (a grad-enabled ``forward``, and the adjoint's augmented dynamics without the hook, take the plain route),
float64, more than ``_hip.XDE_MLP_MAX_LAYERS`` layers or a width beyond ``_hip.XDE_MLP_MAX_WIDTH`` (both take the plain route),
capture of the hook by ``graph_func``, and fusing a solver's stage combine into the first layer.
"""
import torch
import torch.nn.functional as F

from .. import _hip


class MLPField(torch.nn.Module):
    """``hidden`` is an int or a sequence of 1 to ``XDE_MLP_MAX_LAYERS - 1`` ints; ``out_features`` defaults to ``in_features``;
    ``activation`` is "tanh" or None (the identity).  ``forward(t, y)`` takes ``y [..., in_features]`` and returns
    ``[..., out_features]``; ``t`` is a number, a 0-d tensor or, under a per-sample solver, a tensor that broadcasts to ``y[..., :1]``,
    and is read only with ``time=True``.  ``fuse = False`` on an instance keeps it on the plain route."""

    fuse = True
    vjp_max_blocks = 0  # 0: the plan's grid cap; a positive limit on ``vjp``'s workgroups (tests and profiles reach the item loop with it)

    def __init__(self, in_features, hidden, out_features=None, activation="tanh", time=False, bias=True):
        super().__init__()
        if activation not in ("tanh", None):
            raise ValueError("MLPField: activation must be 'tanh' or None (the identity), got {!r}".format(activation))
        hidden = [hidden] if isinstance(hidden, int) else list(hidden)
        if not 1 <= len(hidden) <= _hip.XDE_MLP_MAX_LAYERS - 1:
            raise ValueError("MLPField: hidden must be an int or 1 to {} ints, got {!r}".format(_hip.XDE_MLP_MAX_LAYERS - 1, hidden))
        widths = [int(in_features)] + [int(h) for h in hidden] + [int(in_features if out_features is None else out_features)]
        if min(widths) < 1:
            raise ValueError("MLPField: in_features, hidden and out_features must be >= 1, got {}".format(widths))
        self.in_features, self.out_features, self.widths = widths[0], widths[-1], tuple(widths)
        self.activation, self.time = activation, bool(time)
        fan_in = [widths[0] + int(self.time)] + widths[1:-1]
        self.layers = torch.nn.ModuleList(torch.nn.Linear(k, n, bias=bias) for k, n in zip(fan_in, widths[1:]))
        self._served = {}  # rows -> the plan's answer
        self._vjp_plans, self._vjp_work = {}, {}  # rows -> the vjp's plan; (rows, device) -> its workspace

    def _input(self, t, y):
        if not self.time:
            return y
        col = torch.as_tensor(t, dtype=y.dtype, device=y.device)
        return torch.cat([y, torch.broadcast_to(col, y[..., :1].shape)], dim=-1)

    def _plain(self, t, y):
        h = self._input(t, y)
        for i, layer in enumerate(self.layers):
            if i:
                h = torch.tanh(h) if self.activation == "tanh" else h
            h = F.linear(h, layer.weight, layer.bias)
        return h

    def _fusable(self, t, y):
        if not self.fuse or not y.is_cuda or y.dtype != torch.float32 or y.dim() < 1 or y.shape[-1] != self.in_features or y.numel() == 0:
            return False
        params = [p for layer in self.layers for p in (layer.weight, layer.bias) if p is not None]
        if any(p.device != y.device or p.dtype != y.dtype for p in params):
            return False
        if torch.is_grad_enabled() and (y.requires_grad or any(p.requires_grad for p in params) or
                                        (self.time and torch.is_tensor(t) and t.requires_grad)):
            return False
        rows = y.numel() // self.in_features
        served = self._served.get(rows)
        if served is None:
            served = self._served[rows] = bool(
                _hip.get_backend()._mlp_plan(rows, self.widths, y.dtype, self.activation, self.time)["served"])
        return served

    def forward(self, t, y):
        if not self._fusable(t, y):
            return self._plain(t, y)
        y = y.contiguous()
        t_rows, t_num = None, 0.0
        if self.time:
            if torch.is_tensor(t) and (t.is_cuda or t.numel() != 1):  # (a device scalar is not read back: that would stall the stream)
                t_rows = torch.broadcast_to(t.to(device=y.device, dtype=y.dtype), y[..., :1].shape).reshape(-1).contiguous()
            else:
                t_num = float(t)
        out = torch.empty(y.shape[:-1] + (self.out_features,), dtype=y.dtype, device=y.device)
        weights = [layer.weight.detach().contiguous() for layer in self.layers]
        biases = [None if layer.bias is None else layer.bias.detach().contiguous() for layer in self.layers]
        _hip.get_backend()._mlp_field(out, y, t_rows, t_num, weights, biases, self.activation, self.time)
        return out

    def _vjp_plan(self, y):
        """The plan of the fused vector-Jacobian product at ``y``, or None where the plain route is taken."""
        if not self.fuse or not y.is_cuda or y.dtype != torch.float32 or y.dim() < 1 or y.shape[-1] != self.in_features or y.numel() == 0:
            return None
        if any(p.device != y.device or p.dtype != y.dtype for p in self.parameters()):
            return None
        rows = y.numel() // self.in_features
        plan = self._vjp_plans.get(rows)
        if plan is None:
            plan = self._vjp_plans[rows] = _hip.get_backend()._mlp_vjp_plan(rows, self.widths, y.dtype, self.activation, self.time)
        return plan if plan["served"] else None

    def vjp(self, t, y, cotangent):
        """``(f, vjp_t, vjp_y, *vjp_params)`` with ``f = self(t, y)`` and ``vjp_* = cotangent^T df/d*``: the convention of
        ``adjoint_options={"vjp": field.vjp}`` (``odeint_adjoint``) and ``AdjointProblem(vjp=field.vjp)``.  The parameter entries come
        in ``self.parameters()`` order, weight then bias per layer; ``vjp_t`` is None without ``time`` and a 0-d tensor with it.  On a
        served float32 ROCm state it is two launches (xde_mlp_field_vjp, include/xde_hip_mlp.h) and ``f`` has ``forward``'s fused
        bits; everywhere else it is the taped plain composition and ``torch.autograd.grad``."""
        plan = self._vjp_plan(y)
        if plan is None or cotangent.device != y.device:
            with torch.enable_grad():
                t_var = torch.as_tensor(t, dtype=y.dtype, device=y.device).detach().requires_grad_(self.time)
                y_var, params = y.detach().requires_grad_(True), list(self.parameters())
                f = self._plain(t_var, y_var)
                grads = torch.autograd.grad(f, ([t_var] if self.time else []) + [y_var] + params, cotangent.to(f.dtype), allow_unused=True)
            grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, ([t_var] if self.time else []) + [y_var] + params)]
            vjp_t = grads.pop(0).sum() if self.time else None
            return (f.detach(), vjp_t, *grads)
        y, a = y.detach().contiguous(), cotangent.detach().to(y.dtype).contiguous()
        t_rows, t_num = None, 0.0
        if self.time:
            if torch.is_tensor(t) and (t.is_cuda or t.numel() != 1):  # (a device scalar is not read back: that would stall the stream)
                t_rows = torch.broadcast_to(t.detach().to(device=y.device, dtype=y.dtype), y[..., :1].shape).reshape(-1).contiguous()
            else:
                t_num = float(t)
        key = (y.numel() // self.in_features, y.device)
        work = self._vjp_work.get(key)
        if work is None:  # (overwritten by every call, never cleared: the kernel's first item of a workgroup stores)
            work = self._vjp_work[key] = torch.empty(max(plan["workspace_bytes"] // 4, 1), dtype=y.dtype, device=y.device)
        f = torch.empty(y.shape[:-1] + (self.out_features,), dtype=y.dtype, device=y.device)
        gx, gt = torch.empty_like(y), (torch.empty((), dtype=y.dtype, device=y.device) if self.time else None)
        weights = [layer.weight.detach().contiguous() for layer in self.layers]
        biases = [None if layer.bias is None else layer.bias.detach().contiguous() for layer in self.layers]
        gW, gb = [torch.empty_like(w) for w in weights], [None if b is None else torch.empty_like(b) for b in biases]
        _hip.get_backend()._mlp_field_vjp(f, gx, gW, gb, gt, y, a, t_rows, t_num, weights, biases, self.activation, self.time, work,
                                          self.vjp_max_blocks)
        return (f, gt, gx, *[g for pair in zip(gW, gb) for g in pair if g is not None])
