"""Float64 restatement of the Discrete SAC path (reference discrete_sac.py:147-196, sac.py:203-209, algorithm_base.py:796,
1213-1215, torch.distributions.Categorical, torch.optim.Adam) -- the yardstick of the Discrete SAC tests.  Written from the
description of what the reference computes, step by step, in numpy with closed-form gradients; pinned to the reference by
tests/test_host_dsac.py against tests/golden/dsac.npz.

  `categorical`       ln = logits - logsumexp, p = exp(ln), H = -sum clamp(ln, finfo.min) p   (Categorical.entropy)
  `target`            sum_a p min(q1, q2) + alpha H, then the n-step line
  `critic_head`       both squared-error losses, their gradients, (td1 + td2) / 2
  `actor_loss`, `actor_head`   -(alpha H + sum_a p min(q1, q2)).mean() and its closed-form gradient
  `alpha_step`        AutoAlpha.update: the loss, the gradient, one Adam step on log_alpha
  `DsacRestatement`   actor, two critics, two lagged critics on flat vectors, three Adams, the reference's order of steps
"""
from __future__ import annotations

import numpy as np
import torch

from dqn_restatement import DqnRestatement


def categorical(logits, dtype=np.float64):
    x = np.asarray(logits, dtype)
    mx = x.max(-1, keepdims=True)
    ln = x - (mx + np.log(np.exp(x - mx).sum(-1, keepdims=True)))
    p = np.exp(ln)
    H = -(np.maximum(ln, np.finfo(dtype).min) * p).sum(-1)
    return p, ln, H


def target(logits_next, q1, q2, alpha, mc, gpow, vmask, dtype=np.float64) -> np.ndarray:
    """`dtype`: the precision every step runs in (float64: the yardstick; float32: what the reference's own run costs)."""
    p, _, H = categorical(logits_next, dtype)
    tq = (p * np.minimum(np.asarray(q1, dtype), np.asarray(q2, dtype))).sum(-1) + dtype(alpha) * H
    return tq * np.asarray(vmask, bool).astype(dtype) * np.asarray(gpow, dtype) + np.asarray(mc, dtype)


def critic_head(q1, q2, act, returns, weight=None, dtype=np.float64) -> dict:
    q1, q2, ret = (np.asarray(v, dtype) for v in (q1, q2, returns))
    B = q1.shape[0]
    rows, a = np.arange(B), np.asarray(act, np.int64)
    w = np.ones(B, dtype) if weight is None else np.asarray(weight, dtype)
    out = {}
    for k, q in ((1, q1), (2, q2)):
        td = q[rows, a] - ret
        d = np.zeros_like(q)
        d[rows, a] = dtype(2.0) * td * w / dtype(B)
        out.update({f"td{k}": td, f"loss{k}": float((td * td * w).mean()), f"dq{k}": d})
    out["prio"] = (out["td1"] + out["td2"]) / dtype(2.0)
    return out


def actor_loss(logits, q1, q2, alpha) -> float:
    p, _, H = categorical(logits)
    q = np.minimum(np.asarray(q1, np.float64), np.asarray(q2, np.float64))
    return float(-(float(alpha) * H + (p * q).sum(-1)).mean())


def actor_head(logits, q1, q2, alpha, dtype=np.float64) -> dict:
    """d loss / d logits[b][j] = p[j] (alpha (ln[j] + H) - (q[j] - V)) / B,  V = sum_a p[a] q[a]:
    dV/dx[j] = p[j] (q[j] - V) and dH/dx[j] = -p[j] (ln[j] + H) from dp[a]/dx[j] = p[a] (1[a = j] - p[j])."""
    p, ln, H = categorical(logits, dtype)
    q = np.minimum(np.asarray(q1, dtype), np.asarray(q2, dtype))
    V = (p * q).sum(-1)
    B = p.shape[0]
    d = p * (dtype(alpha) * (ln + H[:, None]) - (q - V[:, None])) / dtype(B)
    return dict(entropy=H, d_logits=d, loss=float(-(dtype(alpha) * H + V).mean()), mean_entropy=float(H.mean()),
                gap=float(np.abs(np.asarray(q1, dtype) - np.asarray(q2, dtype)).min()))


def alpha_state(log_alpha: float) -> dict:
    return dict(log_alpha=float(log_alpha), m=0.0, v=0.0, t=0)


def alpha_step(st: dict, mean_entropy: float, target_entropy: float, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8) -> float:
    """-> alpha_loss; `st` moves by one torch Adam step (amsgrad off, no weight decay)."""
    deficit = float(target_entropy) - float(mean_entropy)
    loss = -(st["log_alpha"] * deficit)
    g = -deficit
    st["t"] += 1
    st["m"] = betas[0] * st["m"] + (1.0 - betas[0]) * g
    st["v"] = betas[1] * st["v"] + (1.0 - betas[1]) * g * g
    step_size = lr / (1.0 - betas[0] ** st["t"])
    denom = np.sqrt(st["v"]) / np.sqrt(1.0 - betas[1] ** st["t"]) + eps
    st["log_alpha"] -= step_size * st["m"] / denom
    return loss


class DsacRestatement:
    """Nets dims[0] -> ... -> dims[-1] (ReLU) on flat vectors in `parameters()` order.  alpha: a float, or a dict from
    `alpha_state` with `target_entropy` / `alpha_lr` for the auto-tuned kind."""

    def __init__(self, actor, critic1, critic2, dims, alpha, tau: float, lr: float = 1e-3, target_entropy: float | None = None,
                 alpha_lr: float = 1e-3) -> None:
        self.nets = {k: DqnRestatement(f, dims, lr=lr, target_update_freq=1) for k, f in
                     (("actor", actor), ("critic", critic1), ("critic2", critic2))}
        self.alpha, self.tau, self.target_entropy, self.alpha_lr = alpha, float(tau), target_entropy, alpha_lr
        self.kink = np.inf

    @property
    def alpha_value(self) -> float:
        return float(np.exp(self.alpha["log_alpha"])) if isinstance(self.alpha, dict) else float(self.alpha)

    def weights(self, name: str) -> np.ndarray:
        if name.endswith("_old"):
            return self.nets[name[:-4]].targets()
        return self.nets[name].weights()

    def _fwd(self, name: str, x, old: bool = False, grad: bool = False):
        """The net on rows x; the smallest |ReLU pre-activation| met goes into `self.kink`."""
        R = self.nets[name]
        ps = R.target if old else R.params
        h = torch.as_tensor(np.asarray(x)).to(torch.float64)
        L = len(R.dims) - 1
        with torch.set_grad_enabled(grad):
            for i in range(L):
                h = torch.nn.functional.linear(h, ps[2 * i], ps[2 * i + 1])
                if i < L - 1:
                    self.kink = min(self.kink, float(h.detach().abs().min()))
                    h = torch.relu(h)
        return h

    def returns(self, obs_next, mc, gpow, vmask) -> np.ndarray:
        ln = self._fwd("actor", obs_next).numpy()
        q1, q2 = self._fwd("critic", obs_next, old=True).numpy(), self._fwd("critic2", obs_next, old=True).numpy()
        self.kink = min(self.kink, float(np.abs(q1 - q2).min()))
        return target(ln, q1, q2, self.alpha_value, mc, gpow, vmask)

    def _step(self, name: str, out: torch.Tensor, d_out: np.ndarray) -> np.ndarray:
        R = self.nets[name]
        R.opt.zero_grad()
        out.backward(torch.as_tensor(d_out))
        g = R.flat_of([p.grad for p in R.params])
        R.opt.step()
        return g

    def update(self, obs, act, obs_next, mc, gpow, vmask, weight=None) -> dict:
        ret = self.returns(obs_next, mc, gpow, vmask)
        q1, q2 = self._fwd("critic", obs, grad=True), self._fwd("critic2", obs, grad=True)
        ch = critic_head(q1.detach().numpy(), q2.detach().numpy(), act, ret, weight)
        grads = dict(critic=self._step("critic", q1, ch["dq1"]), critic2=self._step("critic2", q2, ch["dq2"]))
        logits = self._fwd("actor", obs, grad=True)
        q1a, q2a = self._fwd("critic", obs).numpy(), self._fwd("critic2", obs).numpy()   # after the critics' steps
        alpha_used = self.alpha_value
        ah = actor_head(logits.detach().numpy(), q1a, q2a, alpha_used)
        self.kink = min(self.kink, ah["gap"])
        grads["actor"] = self._step("actor", logits, ah["d_logits"])
        alpha_loss = None
        if isinstance(self.alpha, dict):
            alpha_loss = alpha_step(self.alpha, ah["mean_entropy"], self.target_entropy, lr=self.alpha_lr)
        for name in ("critic", "critic2"):
            R = self.nets[name]
            with torch.no_grad():
                for p, t in zip(R.params, R.target):
                    t.data.copy_(self.tau * p.data + (1.0 - self.tau) * t.data)
        return dict(returns=ret, prio=ch["prio"], critic1_loss=ch["loss1"], critic2_loss=ch["loss2"], actor_loss=ah["loss"],
                    mean_entropy=ah["mean_entropy"], alpha=self.alpha_value, alpha_loss=alpha_loss, grads=grads,
                    alpha_used=alpha_used)

    def adam_cond(self, name: str) -> np.ndarray:
        return self.nets[name].adam_cond()
