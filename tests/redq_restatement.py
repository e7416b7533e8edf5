"""Float64 restatement of REDQ (reference redq.py:254-304, ddpg.py:287-339, utils/net/common.py:522-554, sac.py:176-209,
algorithm_base.py:796, 1213-1215, torch.optim.Adam) -- the yardstick of the REDQ tests.  Written from the description of what
the reference computes, step by step, in numpy with closed-form gradients of everything between a network product and an
optimiser step (the networks themselves run in torch float64); pinned to the reference by tests/test_host_redq.py against
tests/golden/redq.npz.  The Gaussian-tanh action and the actor's head are cac_restatement's (`sac_action`, `sac_actor_head`
with one critic: the ensemble's mean and its input gradient).

  `subset_mask`      bit e set for every member of the subset
  `target`           min or mean over the subset of the lagged ensemble, minus alpha logp, then the n-step line
  `critic_head`      the ensemble's squared loss, its gradient, the signed ensemble mean of td
  `mean_q`           the ensemble mean
  `ens_forward`      the grouped MLP on a flat vector (per layer weight [E, in, out], then bias_weights [E, 1, out]), numpy
  `RedqRestatement`  the nets on flat vectors, their Adams, the reference's order of steps
"""
from __future__ import annotations

import numpy as np
import torch

from cac_restatement import _Net, flat_of, sac_action, sac_actor_head
from dsac_restatement import alpha_state, alpha_step  # noqa: F401


def subset_mask(indices, E: int) -> int:
    idx = [int(i) for i in np.asarray(indices).reshape(-1)]
    assert idx and len(set(idx)) == len(idx) and 0 <= min(idx) and max(idx) < E <= 64
    return sum(1 << i for i in idx)


def target(q, indices, mode, logp, alpha, mc, gpow, vmask, dtype=np.float64) -> np.ndarray:
    qs = np.asarray(q, dtype).reshape(len(q), -1)[np.sort(np.asarray(indices).reshape(-1))]
    tq = qs.min(0) if mode == "min" else qs.mean(0)
    if logp is not None:
        tq = tq - dtype(alpha) * np.asarray(logp, dtype).reshape(-1)
    return tq * np.asarray(vmask, bool).astype(dtype) * np.asarray(gpow, dtype) + np.asarray(mc, dtype)


def critic_head(q, returns, weight=None, dtype=np.float64) -> dict:
    q = np.asarray(q, dtype).reshape(len(q), -1)
    E, B = q.shape
    w = np.ones(B, dtype) if weight is None else np.asarray(weight, dtype).reshape(-1)
    td = q - np.asarray(returns, dtype).reshape(1, -1)
    return dict(td=td, loss=float((td * td * w).mean()), dq=dtype(2.0) * td * w / dtype(E * B), prio=td.mean(0))


def mean_q(q, dtype=np.float64) -> np.ndarray:
    return np.asarray(q, dtype).reshape(len(q), -1).mean(0)


def ens_layers(flat, dims, E: int):
    """[(W [E, in, out], b [E, 1, out])] views of a flat vector in the ensemble layout."""
    flat, out, o = np.asarray(flat), [], 0
    for i in range(len(dims) - 1):
        k, m = int(dims[i]), int(dims[i + 1])
        W = flat[o:o + E * k * m].reshape(E, k, m)
        o += E * k * m
        out.append((W, flat[o:o + E * m].reshape(E, 1, m)))
        o += E * m
    assert o == flat.size, (o, flat.size)
    return out


def ens_forward(flat, dims, E: int, x, act="relu", dtype=np.float64):
    """-> the activations per layer, [E, B, dims[l]]; the last one is the output."""
    h = np.broadcast_to(np.asarray(x, dtype), (E,) + np.asarray(x).shape)
    acts, L = [], len(dims) - 1
    for i, (W, b) in enumerate(ens_layers(np.asarray(flat, dtype), dims, E)):
        h = np.einsum("ebk,ekm->ebm", h, W) + b
        if i < L - 1:
            h = np.maximum(h, 0) if act == "relu" else (np.tanh(h) if act == "tanh" else h)
        acts.append(h)
    return acts


class _EnsNet:
    """E nets dims[0] -> ... -> dims[-1] (ReLU) on one flat vector in the ensemble layout, torch float64."""

    def __init__(self, flat, dims, E, lr, owner) -> None:
        self.dims, self.E, self.owner = [int(d) for d in dims], int(E), owner
        self.params = [torch.as_tensor(np.array(t, np.float64)).requires_grad_(True)
                       for Wb in ens_layers(np.asarray(flat, np.float64), self.dims, self.E) for t in Wb]
        self.opt = torch.optim.Adam(self.params, lr=lr)

    def twin(self):
        return [p.detach().clone() for p in self.params]

    def fwd(self, ps, x):
        h = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, np.float64))
        L = len(self.dims) - 1
        for i in range(L):
            h = torch.matmul(h, ps[2 * i]) + ps[2 * i + 1]
            if i < L - 1:
                self.owner.kink = min(self.owner.kink, float(h.detach().abs().min()))
                h = torch.relu(h)
        return h   # [E, B, 1]

    def step(self, out: torch.Tensor, d_out) -> np.ndarray:
        self.opt.zero_grad()
        out.backward(torch.as_tensor(np.asarray(d_out, np.float64)).reshape(out.shape))
        g = flat_of([p.grad for p in self.params])
        self.opt.step()
        return g


class RedqRestatement:
    """`init`: dict of flat vectors actor (last layer [mu_raw | sigma_raw]) and critic (the ensemble layout).  alpha: a float,
    or a dict from `alpha_state` with `target_entropy` / `alpha_lr`."""

    def __init__(self, init, actor_dims, critic_dims, E, subset_size, mode, tau, lr=1e-3, actor_delay=20, max_action=1.0,
                 unbounded=False, alpha=0.2, target_entropy=None, alpha_lr=1e-3) -> None:
        self.E, self.M_sub, self.mode, self.tau = int(E), int(subset_size), mode, float(tau)
        self.M, self.unbounded, self.actor_delay = float(max_action), bool(unbounded), int(actor_delay)
        self.alpha, self.target_entropy, self.alpha_lr = alpha, target_entropy, alpha_lr
        self.kink = np.inf
        self.D = actor_dims[0]
        self.Ad = critic_dims[0] - self.D
        self.actor = _Net(init["actor"], actor_dims, lr, self)
        self.critic = _EnsNet(init["critic"], critic_dims, E, lr, self)
        self.critic_old = self.critic.twin()
        self.step_count, self._last = 0, 0.0

    @property
    def alpha_value(self) -> float:
        return float(np.exp(self.alpha["log_alpha"])) if isinstance(self.alpha, dict) else float(self.alpha)

    def weights(self, name: str) -> np.ndarray:
        return flat_of({"actor": self.actor.params, "critic": self.critic.params, "critic_old": self.critic_old}[name])

    def _x(self, obs, act):
        return torch.cat([torch.as_tensor(np.asarray(obs, np.float64)), torch.as_tensor(np.asarray(act, np.float64))], 1)

    def returns(self, obs_next, mc, gpow, vmask, z, subset) -> np.ndarray:
        with torch.no_grad():
            raw = self.actor.fwd(self.actor.params, obs_next).numpy()
            s = sac_action(raw[:, :self.Ad], raw[:, self.Ad:], z, self.M, self.unbounded)
            q = self.critic.fwd(self.critic_old, self._x(obs_next, s["a"])).numpy()[:, :, 0]
        return target(q, subset, self.mode, s["logp"], self.alpha_value, mc, gpow, vmask)

    def update(self, obs, act, obs_next, mc, gpow, vmask, subset, weight=None, z_target=None, z_actor=None) -> dict:
        ret = self.returns(obs_next, mc, gpow, vmask, z_target, subset)
        q = self.critic.fwd(self.critic.params, self._x(obs, act))
        ch = critic_head(q.detach().numpy()[:, :, 0], ret, weight)
        grads = dict(critic=self.critic.step(q, ch["dq"]))
        self.step_count += 1
        out = dict(returns=ret, prio=ch["prio"], critic_loss=ch["loss"], alpha_loss=None, grads=grads)
        if self.step_count % self.actor_delay == 0:
            raw = self.actor.fwd(self.actor.params, torch.as_tensor(np.asarray(obs, np.float64)))
            r = raw.detach().numpy()
            m_raw, s_raw = r[:, :self.Ad], r[:, self.Ad:]
            a = torch.as_tensor(sac_action(m_raw, s_raw, z_actor, self.M, self.unbounded)["a"]).clone().requires_grad_(True)
            qa = self.critic.fwd(self.critic.params, torch.cat([torch.as_tensor(np.asarray(obs, np.float64)), a], 1))
            q_mean = qa.mean(0).reshape(-1)
            (g_mean,) = torch.autograd.grad(q_mean.sum(), a)
            ah = sac_actor_head(m_raw, s_raw, z_actor, q_mean.detach().numpy(), None, g_mean.numpy(), None, self.alpha_value,
                                self.M, self.unbounded)
            grads["actor"] = self.actor.step(raw, np.concatenate([ah["d_mu"], ah["d_sigma"]], 1))
            if isinstance(self.alpha, dict):
                out["alpha_loss"] = alpha_step(self.alpha, ah["mean_entropy"], self.target_entropy, lr=self.alpha_lr)
            self._last = ah["loss"]
            out.update(q_mean=q_mean.detach().numpy(), g_mean=g_mean.numpy())
        for p, t in zip(self.critic.params, self.critic_old):
            t.copy_(self.tau * p.detach() + (1.0 - self.tau) * t)
        out.update(actor_loss=self._last, alpha=self.alpha_value)
        return out
