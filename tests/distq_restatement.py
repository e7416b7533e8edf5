"""Float64 restatement of the C51 and QR-DQN paths (reference c51.py:66-67, 120-158; qrdqn.py:19-20, 94-129;
algorithm_base.py:796, 1213-1215) -- the yardstick of the distributional tests.  Written from the description of what the
reference computes, step by step; pinned to the reference by tests/test_host_distq.py against tests/golden/distq.npz.

  `dist_values`        expected value per action (softmax over atoms, then the sum with the support) or mean quantile,
                       and the first argmax under compute_q_value's whole-tensor mask offset
  `c51_head`           the projected target distribution, the cross entropy and d loss / d raw
  `qr_head`            the quantile Huber loss, the priorities and d loss / d raw
  `DistqRestatement`   a fully-connected net on one flat vector, Adam, the lagged copy with the `_iter` rule; C51 reads
                       the successor rows AFTER that copy (its `_target_dist` runs inside `_update_with_batch`), QR-DQN
                       before it (its `_target_q` runs inside `_preprocess_batch`)
The support and the quantile midpoints are the reference's float32 values (torch.linspace in float32) carried in float64.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from dqn_restatement import DqnRestatement


def support_of(v_min: float, v_max: float, n: int) -> np.ndarray:
    return torch.linspace(v_min, v_max, n).double().numpy()


def tau_hat_of(n: int) -> np.ndarray:
    tau = torch.linspace(0, 1, n + 1)
    return ((tau[:-1] + tau[1:]) / 2).double().numpy()


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype)


def _np(x):
    return x.detach().to(torch.float64).numpy()


def dist_values(raw, A: int, N: int, support=None, mask=None, dtype=torch.float64):
    """raw [R, A * N] -> dict(q [R, A], act [R] under `mask`, probs [R, A, N] or None)."""
    x = _t(raw, dtype).reshape(-1, A, N)
    if support is not None:
        probs = torch.softmax(x, dim=-1)
        q = (probs * _t(support, dtype)).sum(2)
    else:
        probs, q = None, x.mean(2)
    sel = q
    if mask is not None:
        sel = q + (1 - _t(np.asarray(mask, bool), dtype)) * (q.min() - q.max() - 1.0)
    return dict(q=_np(q), act=sel.argmax(dim=1).numpy(), probs=None if probs is None else _np(probs))


def _returns(x, mc, gpow, vmask, dtype):
    """target_q * value_mask * gamma^m + mc, per atom."""
    vm = _t(np.asarray(vmask, bool), dtype).reshape(-1, 1)
    return x * vm * _t(gpow, dtype).reshape(-1, 1) + _t(mc, dtype).reshape(-1, 1)


def c51_head(raw, raw_next_on, raw_next_tg, mask_next, act, mc, gpow, vmask, weight, support, v_min, v_max, A: int, N: int,
             dtype=torch.float64) -> dict:
    """raw_next_tg None: no target network.  -> returns [B, N], prio [B], loss, d_out [B, A * N], a_star [B], q_taken [B]."""
    z = _t(support, dtype)
    B = np.asarray(raw).shape[0]
    rows = torch.arange(B)
    a_star = torch.as_tensor(dist_values(raw_next_on, A, N, support, mask_next, dtype)["act"])
    nxt = _t(raw_next_on if raw_next_tg is None else raw_next_tg, dtype).reshape(B, A, N)
    next_dist = torch.softmax(nxt, dim=-1)[rows, a_star]
    returns = _returns(z.reshape(1, N).repeat(B, 1), mc, gpow, vmask, dtype)
    tz = returns.clamp(v_min, v_max)
    dz = (v_max - v_min) / (N - 1)
    # m[b][j] = sum_k clamp(1 - |tz[b][k] - z[j]| / dz, 0, 1) next_dist[b][k]
    m = ((1 - (tz.unsqueeze(1) - z.view(1, N, 1)).abs() / dz).clamp(0, 1) * next_dist.unsqueeze(1)).sum(-1)
    x = _t(raw, dtype).clone().requires_grad_(True)
    a = torch.as_tensor(np.asarray(act, np.int64))
    p = torch.softmax(x.reshape(B, A, N), dim=-1)[rows, a]
    ce = -(m * torch.log(p + 1e-8)).sum(1)
    loss = (ce * (1.0 if weight is None else _t(weight, dtype))).mean()
    loss.backward()
    return dict(returns=_np(returns), prio=_np(ce), loss=float(loss.item()), d_out=_np(x.grad), a_star=a_star.numpy(),
                q_taken=_np((p * z).sum(1)))


def qr_head(raw, raw_next_on, raw_next_tg, mask_next, act, mc, gpow, vmask, weight, tau_hat, A: int, N: int,
            dtype=torch.float64) -> dict:
    B = np.asarray(raw).shape[0]
    rows = torch.arange(B)
    a_star = torch.as_tensor(dist_values(raw_next_on, A, N, None, mask_next, dtype)["act"])
    nxt = _t(raw_next_on if raw_next_tg is None else raw_next_tg, dtype).reshape(B, A, N)[rows, a_star]
    returns = _returns(nxt, mc, gpow, vmask, dtype)
    x = _t(raw, dtype).clone().requires_grad_(True)
    a = torch.as_tensor(np.asarray(act, np.int64))
    curr = x.reshape(B, A, N)[rows, a]
    u = returns.unsqueeze(1) - curr.unsqueeze(2)                      # u[b][i][j] = target_j - curr_i
    au = u.abs()
    h = torch.where(au < 1.0, 0.5 * u * u, au - 0.5)
    k = (_t(tau_hat, dtype).view(1, N, 1) - (u.detach() <= 0).to(dtype)).abs()
    per_row = (h * k).sum(-1).mean(1)
    loss = (per_row * (1.0 if weight is None else _t(weight, dtype))).mean()
    loss.backward()
    return dict(returns=_np(returns), prio=_np(h.abs().sum(-1).mean(1)), loss=float(loss.item()), d_out=_np(x.grad),
                a_star=a_star.numpy(), q_taken=_np(curr.mean(1)), u=_np(u))


class DistqRestatement(DqnRestatement):
    """kind "c51" (support, v_min, v_max) or "qr" (tau_hat) around the net dims[0] -> ... -> A * N."""

    def __init__(self, flat, dims, kind: str, A: int, N: int, lr: float = 1e-3, target_update_freq: int = 0, v_min=-10.0,
                 v_max=10.0, dtype=torch.float64) -> None:
        super().__init__(flat, dims, lr=lr, target_update_freq=target_update_freq, dtype=dtype)
        assert kind in ("c51", "qr") and self.dims[-1] == A * N
        self.kind, self.A, self.N, self.v_min, self.v_max = kind, A, N, float(v_min), float(v_max)
        self.support, self.tau_hat = support_of(v_min, v_max, N), tau_hat_of(N)

    def _next(self, obs_next):
        with torch.no_grad():
            on = self.net(self.params, obs_next).numpy()
            tg = self.net(self.target, obs_next).numpy() if self.freq > 0 else None
        return on, tg

    def update(self, obs, act, obs_next, mask_next, mc, gpow, vmask, weight=None) -> dict:
        """`obs_next`: the rows the algorithm reads its a* and next distribution from -- the one-step successors for C51,
        the rows at idx_n for QR-DQN (the caller picks them)."""
        if self.kind == "qr":
            on, tg = self._next(obs_next)
        if self.freq > 0 and self._iter % self.freq == 0:
            for p, t in zip(self.params, self.target):
                t.data.copy_(p.data)
        self._iter += 1
        if self.kind == "c51":
            on, tg = self._next(obs_next)
        raw = self.net(self.params, obs)
        args = (raw.detach().numpy(), on, tg, mask_next, act, mc, gpow, vmask, weight)
        if self.kind == "c51":
            h = c51_head(*args, self.support, self.v_min, self.v_max, self.A, self.N, self.dtype)
        else:
            h = qr_head(*args, self.tau_hat, self.A, self.N, self.dtype)
        self.opt.zero_grad()
        raw.backward(torch.as_tensor(h["d_out"]).to(self.dtype))
        h["grads"] = self.flat_of([p.grad for p in self.params])
        self.opt.step()
        return h

    def min_kink_gap(self, xs) -> float:
        """The smallest |ReLU pre-activation| and greedy top-2 gap of the value per action over the rows `xs`."""
        gap = np.inf
        with torch.no_grad():
            for ps in [self.params] + ([self.target] if self.target is not None else []):
                x = torch.as_tensor(np.asarray(xs)).to(self.dtype)
                L = len(self.dims) - 1
                for i in range(L):
                    x = F.linear(x, ps[2 * i], ps[2 * i + 1])
                    if i < L - 1:
                        gap = min(gap, float(x.abs().min()))
                        x = F.relu(x)
                q = dist_values(x.numpy(), self.A, self.N, self.support if self.kind == "c51" else None)["q"]
                top = np.sort(q, axis=1)
                gap = min(gap, float(np.abs(top[:, -1] - top[:, -2]).min()))
        return gap
