"""Float64 restatement of the IQN path (reference iqn.py:72-100, 156-183; qrdqn.py:19-20, 94-106; utils/net/discrete.py:145-161,
208-216; algorithm_base.py:796, 1213-1215) -- the yardstick of the IQN tests.  Written from the description of what the
reference computes, step by step; pinned to the reference by tests/test_host_iqn.py against tests/golden/iqn.npz.

  `embed`             cos(tau * pi i), the linear layer, the ReLU and the product with the features; with `grads`, the
                      gradients of sum(e * d_e) with respect to f, We and be
  `iqn_values`        the mean over the fractions and the first argmax under compute_q_value's whole-tensor mask offset
  `iqn_head`          the quantile Huber loss over per-row fractions, the priorities and d loss / d out
  `IqnRestatement`    preprocess MLP (ending in its ReLU when `feature_act`), embedding, `last` MLP on one flat vector in
                      `parameters()` order; Adam; the lagged copy with the `_iter` rule; the successor forwards BEFORE that copy
Fractions are always given: every forward of an update takes the next array of `taus`, in the reference's order.
Layout here: out [B, S, A] (sample-major); the reference's logits are its transpose [B, A, S].
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def _t(x, dtype=torch.float64):
    return torch.as_tensor(np.asarray(x)).to(dtype)


def _np(x):
    return x.detach().to(torch.float64).numpy()


def _embed(f, taus, We, be, feature_act: bool):
    """torch: f [R, H], taus [R, S] -> (e [R, S, H], the embedding's pre-activation [R, S, H])."""
    C = We.shape[1]
    i_pi = np.pi * torch.arange(1, C + 1, dtype=taus.dtype).view(1, 1, C)
    pre = F.linear(torch.cos(taus.unsqueeze(2) * i_pi), We, be)
    g = F.relu(f) if feature_act else f
    return g.unsqueeze(1) * F.relu(pre), pre


def embed(f, taus, We, be, feature_act: bool = False, d_e=None, dtype=torch.float64) -> dict:
    """-> dict(e [R * S, H], pre [R * S, H]) and, given d_e [R * S, H], d_f, dWe, dbe."""
    f, We, be = (_t(x, dtype).clone().requires_grad_(True) for x in (f, We, be))
    e, pre = _embed(f, _t(taus, dtype), We, be, feature_act)
    H = We.shape[0]
    out = dict(e=_np(e).reshape(-1, H), pre=_np(pre).reshape(-1, H))
    if d_e is not None:
        e.backward(_t(d_e, dtype).reshape(e.shape))
        out.update(d_f=_np(f.grad), dWe=_np(We.grad), dbe=_np(be.grad))
    return out


def iqn_values(out, mask=None, dtype=torch.float64) -> dict:
    """out [R, S, A] -> dict(q [R, A], act [R] under `mask`)."""
    q = _t(out, dtype).transpose(1, 2).mean(2)
    sel = q
    if mask is not None:
        sel = q + (1 - _t(np.asarray(mask, bool), dtype)) * (q.min() - q.max() - 1.0)
    return dict(q=_np(q), act=sel.argmax(dim=1).numpy())


def iqn_head(out, out_next_on, out_next_tg, mask_next, taus, act, mc, gpow, vmask, weight, dtype=torch.float64) -> dict:
    """out [B, N, A]; out_next_on [B, N_on, A] chooses a*; out_next_tg [B, N', A] or None (then the online forward is the next
    distribution).  -> returns [B, N'], prio [B], loss, d_out [B, N, A], a_star [B], q_taken [B], u [B, N, N']."""
    B = np.asarray(out).shape[0]
    rows = torch.arange(B)
    a_star = torch.as_tensor(iqn_values(out_next_on, mask_next, dtype)["act"])
    nxt = _t(out_next_on if out_next_tg is None else out_next_tg, dtype)[rows, :, a_star]            # [B, N']
    vm = _t(np.asarray(vmask, bool), dtype).reshape(-1, 1)
    returns = nxt * vm * _t(gpow, dtype).reshape(-1, 1) + _t(mc, dtype).reshape(-1, 1)
    x = _t(out, dtype).clone().requires_grad_(True)
    curr = x[rows, :, torch.as_tensor(np.asarray(act, np.int64))]                                   # [B, N]
    u = returns.unsqueeze(1) - curr.unsqueeze(2)                                                     # u[b][i][j]
    au = u.abs()
    h = torch.where(au < 1.0, 0.5 * u * u, au - 0.5)
    k = (_t(taus, dtype).unsqueeze(2) - (u.detach() <= 0).to(dtype)).abs()
    per_row = (h * k).sum(-1).mean(1)
    loss = (per_row * (1.0 if weight is None else _t(weight, dtype))).mean()
    loss.backward()
    return dict(returns=_np(returns), prio=_np(h.abs().sum(-1).mean(1)), loss=float(loss.item()), d_out=_np(x.grad),
                a_star=a_star.numpy(), q_taken=_np(curr.mean(1)), u=_np(u))


class IqnRestatement:
    """pre_dims[0] -> ... -> H (ReLU between layers, and after the last when `feature_act`), the cosine embedding with C
    cosines, H -> hidden -> A."""

    def __init__(self, flat, pre_dims, last_dims, C: int, feature_act: bool = True, lr: float = 1e-3,
                 target_update_freq: int = 0, dtype=torch.float64) -> None:
        self.pre_dims, self.last_dims, self.C = [int(d) for d in pre_dims], [int(d) for d in last_dims], int(C)
        assert self.pre_dims[-1] == self.last_dims[0]
        self.feature_act, self.dtype, self.lr, self.freq = bool(feature_act), dtype, lr, int(target_update_freq)
        self.params = self._split(flat, True)
        self.target = self._split(flat, False) if self.freq > 0 else None
        self.opt = torch.optim.Adam(self.params, lr=lr)
        self._iter = 0

    def shapes(self):
        out = []
        for dims in (self.pre_dims, self.last_dims):
            for i in range(len(dims) - 1):
                out += [(dims[i + 1], dims[i]), (dims[i + 1],)]
        H = self.pre_dims[-1]
        return out + [(H, self.C), (H,)]

    def _split(self, flat, grad: bool):
        flat = torch.as_tensor(np.asarray(flat, np.float64)).to(self.dtype)
        out, o = [], 0
        for shp in self.shapes():
            n = int(np.prod(shp))
            out.append(flat[o:o + n].reshape(shp).clone().requires_grad_(grad))
            o += n
        assert o == flat.numel()
        return out

    def net(self, ps, x, taus, kinks: list | None = None):
        """-> out [B, S, A]; `kinks` collects every pre-activation that a ReLU reads."""
        x = _t(x, self.dtype)
        n_pre, n_last = len(self.pre_dims) - 1, len(self.last_dims) - 1
        for i in range(n_pre):
            x = F.linear(x, ps[2 * i], ps[2 * i + 1])
            if i < n_pre - 1 or self.feature_act:
                if kinks is not None:
                    kinks.append(x)
                if i < n_pre - 1:
                    x = F.relu(x)
        e, pre = _embed(x, _t(taus, self.dtype), ps[-2], ps[-1], self.feature_act)
        if kinks is not None:
            kinks.append(pre)
        x = e
        for i in range(n_last):
            x = F.linear(x, ps[2 * (n_pre + i)], ps[2 * (n_pre + i) + 1])
            if i < n_last - 1:
                if kinks is not None:
                    kinks.append(x)
                x = F.relu(x)
        return x

    @staticmethod
    def flat_of(ts) -> np.ndarray:
        return torch.cat([t.detach().reshape(-1).to(torch.float64) for t in ts]).numpy()

    def weights(self) -> np.ndarray:
        return self.flat_of(self.params)

    def targets(self) -> np.ndarray:
        return self.flat_of(self.target)

    def update(self, obs, act, obs_next, mask_next, mc, gpow, vmask, taus, weight=None) -> dict:
        """`taus`: the fractions of this update's forwards in the reference's order -- online on the successor rows, lagged
        on the successor rows (with a target network), online on the sampled rows.  The successor forwards come first, then
        the `_iter` rule's copy, then the loss, its gradient and one Adam step."""
        taus = list(taus)
        kinks: list = []
        with torch.no_grad():
            on = self.net(self.params, obs_next, taus.pop(0), kinks).numpy()
            tg = self.net(self.target, obs_next, taus.pop(0), kinks).numpy() if self.freq > 0 else None
        if self.freq > 0 and self._iter % self.freq == 0:
            for p, t in zip(self.params, self.target):
                t.data.copy_(p.data)
        self._iter += 1
        tau = taus.pop(0)
        assert not taus
        out = self.net(self.params, obs, tau, kinks)
        h = iqn_head(out.detach().numpy(), on, tg, mask_next, tau, act, mc, gpow, vmask, weight, self.dtype)
        self.opt.zero_grad()
        out.backward(torch.as_tensor(h["d_out"]).to(self.dtype))
        h["grads"] = self.flat_of([p.grad for p in self.params])
        self.opt.step()
        q = iqn_values(on)["q"]
        top = np.sort(q, axis=1)
        # the distance to the nearest point of non-smoothness: of the ReLUs (pre-activations at 0), and of the head (top-2 gaps
        # of q, u at 0, |u| at 1)
        h["relu_gap"] = min(float(k.detach().abs().min()) for k in kinks)
        h["head_gap"] = min(float((top[:, -1] - top[:, -2]).min()), float(np.abs(h["u"]).min()),
                            float(np.abs(np.abs(h["u"]) - 1.0).min()))
        return h

    def adam_cond(self) -> np.ndarray:
        """lr / (sqrt(v^) + eps) per parameter: how far one Adam step moves a parameter per unit of gradient error."""
        out = []
        for p in self.params:
            st = self.opt.state[p]
            v_hat = st["exp_avg_sq"].detach().to(torch.float64) / (1.0 - 0.999 ** float(st["step"]))
            out.append((self.lr / (torch.sqrt(v_hat) + 1e-8)).reshape(-1))
        return torch.cat(out).numpy()
