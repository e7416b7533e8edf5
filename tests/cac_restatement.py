"""Float64 restatement of the continuous-action actor-critics DDPG, TD3 and SAC (reference ddpg.py:267-339, 397-410,
td3.py:94-102, 190-226, sac.py:25-39, 108-131, 298-336, utils/net/continuous.py:86-88, 238-247, algorithm_base.py:796, 1213-1215,
torch.distributions.Normal, torch.optim.Adam) -- the yardstick of the continuous actor-critic tests.  Written from the
description of what the reference computes, step by step, in numpy with closed-form gradients of everything between a network
product and an optimiser step (the networks themselves run in torch float64); pinned to the reference by
tests/test_host_cac.py against tests/golden/cac.npz.

  `det_action`       max_action tanh(raw) (+ clamp(policy_noise z, +-noise_clip)), and 1 - tanh^2
  `sac_action`       mu, sigma, x = mu + sigma z, a = tanh(x), logp with the tanh correction
  `target`           min of the lagged critics (- alpha logp), then the n-step line
  `critic_head`      the squared-error losses, their gradients, td or (td1 + td2) / 2
  `det_actor_head`   -mean Q and its gradient w.r.t. the actor's raw output
  `sac_actor_head`   mean(alpha logp - min(q1a, q2a)) and its closed-form gradient w.r.t. mu_raw and sigma_raw
  `CacRestatement`   the nets on flat vectors, their Adams, the reference's order of steps for "ddpg" / "td3" / "sac"
"""
from __future__ import annotations

import numpy as np
import torch

from dsac_restatement import alpha_state, alpha_step  # noqa: F401  (AutoAlpha.update is the same for both SACs)

SIGMA_MIN, SIGMA_MAX = -20.0, 2.0
EPS32 = float(np.finfo(np.float32).eps)
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def det_action(raw, max_action=1.0, z=None, policy_noise=0.0, noise_clip=0.0, dtype=np.float64):
    th = np.tanh(np.asarray(raw, dtype))
    a = dtype(max_action) * th
    if z is not None:
        nz = np.asarray(z, dtype) * dtype(policy_noise)
        if noise_clip > 0.0:
            nz = np.clip(nz, -dtype(noise_clip), dtype(noise_clip))
        a = a + nz
    return a, 1.0 - th * th


def sac_action(mu_raw, sigma_raw, z=None, max_action=1.0, unbounded=False, dtype=np.float64) -> dict:
    m, s = np.asarray(mu_raw, dtype), np.asarray(sigma_raw, dtype)
    s = np.broadcast_to(s, m.shape)
    z = np.zeros_like(m) if z is None else np.asarray(z, dtype)
    th = np.tanh(m)
    mu = m if unbounded else dtype(max_action) * th
    c = np.clip(s, dtype(SIGMA_MIN), dtype(SIGMA_MAX))
    sigma = np.exp(c)
    x = mu + sigma * z
    a = np.tanh(x)
    logp = (-(z * z) / 2 - c - dtype(LOG_SQRT_2PI)).sum(-1) - np.log(1 - a * a + dtype(EPS32)).sum(-1)
    return dict(a=a, logp=logp, sigma=sigma, x=x, z=z, passm=((s >= SIGMA_MIN) & (s <= SIGMA_MAX)).astype(dtype),
                omt2=np.ones_like(m) if unbounded else 1.0 - th * th)


def target(q1, q2, logp, alpha, mc, gpow, vmask, dtype=np.float64) -> np.ndarray:
    tq = np.asarray(q1, dtype).reshape(-1)
    if q2 is not None:
        tq = np.minimum(tq, np.asarray(q2, dtype).reshape(-1))
    if logp is not None:
        tq = tq - dtype(alpha) * np.asarray(logp, dtype).reshape(-1)
    return tq * np.asarray(vmask, bool).astype(dtype) * np.asarray(gpow, dtype) + np.asarray(mc, dtype)


def critic_head(q1, q2, returns, weight=None, dtype=np.float64) -> dict:
    ret = np.asarray(returns, dtype).reshape(-1)
    B = ret.shape[0]
    w = np.ones(B, dtype) if weight is None else np.asarray(weight, dtype).reshape(-1)
    out = {}
    for k, q in ((1, q1), (2, q2)):
        if q is None:
            continue
        td = np.asarray(q, dtype).reshape(-1) - ret
        out.update({f"td{k}": td, f"loss{k}": float((td * td * w).mean()), f"dq{k}": dtype(2.0) * td * w / dtype(B)})
    out["prio"] = out["td1"] if q2 is None else (out["td1"] + out["td2"]) / dtype(2.0)
    return out


def det_actor_head(dq_da, omt2, q_pi, max_action=1.0, dtype=np.float64) -> dict:
    g = np.asarray(dq_da, dtype)
    B = g.shape[0]
    return dict(d_raw=-(g * dtype(max_action) * np.asarray(omt2, dtype)) / dtype(B), loss=float(-np.asarray(q_pi, dtype).mean()))


def sac_actor_head(mu_raw, sigma_raw, z, q1a, q2a, g1, g2, alpha, max_action=1.0, unbounded=False, dtype=np.float64) -> dict:
    """With t = 1 - a^2 and G = d min(q1a, q2a) / d a (the smaller critic's input gradient, half of each at a tie):
    gx = alpha 2 a t / (t + eps) - t G;  d loss / d mu_raw = gx M (1 - tanh^2 mu_raw) / B (unbounded: gx / B);
    d loss / d sigma_raw = pass (gx sigma z - alpha) / B."""
    s = sac_action(mu_raw, sigma_raw, z, max_action, unbounded, dtype)
    a, B = s["a"], s["a"].shape[0]
    q1a = np.asarray(q1a, dtype).reshape(-1)
    if q2a is None:
        qmin, G, gap = q1a, np.asarray(g1, dtype), np.inf
    else:
        q2a = np.asarray(q2a, dtype).reshape(-1)
        w1 = np.where(q1a < q2a, 1.0, np.where(q2a < q1a, 0.0, 0.5)).astype(dtype)[:, None]
        qmin, G = np.minimum(q1a, q2a), w1 * np.asarray(g1, dtype) + (1 - w1) * np.asarray(g2, dtype)
        gap = float(np.abs(q1a - q2a).min())
    t = 1 - a * a
    gx = dtype(alpha) * 2 * a * t / (t + dtype(EPS32)) - t * G
    M = dtype(1.0 if unbounded else max_action)
    return dict(d_mu=gx * M * s["omt2"] / dtype(B), d_sigma=s["passm"] * (gx * s["sigma"] * s["z"] - dtype(alpha)) / dtype(B),
                logp=s["logp"], a=a, loss=float((dtype(alpha) * s["logp"] - qmin).mean()), mean_entropy=float((-s["logp"]).mean()),
                gap=gap)


class _Net:
    """dims[0] -> ... -> dims[-1] (ReLU) on a flat vector in `parameters()` order, torch float64."""

    def __init__(self, flat, dims, lr, owner, n_extra=0) -> None:
        """n_extra: entries behind the layers on the flat vector (SAC's state-independent sigma_param), under the same Adam."""
        self.dims, self.owner = [int(d) for d in dims], owner
        flat = np.asarray(flat, np.float64)
        self.params = self._split(flat[:flat.size - n_extra], True)
        self.extra = [torch.as_tensor(flat[flat.size - n_extra:]).clone().requires_grad_(True)] if n_extra else []
        self.opt = torch.optim.Adam(self.params + self.extra, lr=lr)

    def _split(self, flat, grad):
        flat = torch.as_tensor(np.asarray(flat, np.float64))
        out, o = [], 0
        for i in range(len(self.dims) - 1):
            for shp in ((self.dims[i + 1], self.dims[i]), (self.dims[i + 1],)):
                n = int(np.prod(shp))
                out.append(flat[o:o + n].reshape(shp).clone().requires_grad_(grad))
                o += n
        assert o == flat.numel(), (o, flat.numel(), self.dims)
        return out

    def twin(self):
        return [p.detach().clone() for p in self.params]

    def fwd(self, ps, x):
        h = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, np.float64))
        L = len(self.dims) - 1
        for i in range(L):
            h = torch.nn.functional.linear(h, ps[2 * i], ps[2 * i + 1])
            if i < L - 1:
                self.owner.kink = min(self.owner.kink, float(h.detach().abs().min()))
                h = torch.relu(h)
        return h

    def step(self, out: torch.Tensor, d_out, extra_grad=None) -> np.ndarray:
        self.opt.zero_grad()
        out.backward(torch.as_tensor(np.asarray(d_out, np.float64)).reshape(out.shape))
        for p, gr in zip(self.extra, [extra_grad] if self.extra else []):
            p.grad = torch.as_tensor(np.asarray(gr, np.float64)).reshape(p.shape)
        g = flat_of([p.grad for p in self.params + self.extra])
        self.opt.step()
        return g


def flat_of(ts) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1).to(torch.float64) for t in ts]).numpy()


class CacRestatement:
    """kind "ddpg" | "td3" | "sac".  `init`: dict of flat vectors actor, critic[, critic2]; SAC's actor ends in the layer
    [mu_raw | sigma_raw] (conditioned sigma), or in mu_raw with the state-independent sigma_param as the vector's last act_dim
    entries (actor_dims[-1] == act_dim).  alpha: a float, or a dict from `alpha_state` with `target_entropy` / `alpha_lr`."""

    def __init__(self, kind, init, actor_dims, critic_dims, tau, lr=1e-3, max_action=1.0, unbounded=False, policy_noise=0.2,
                 noise_clip=0.5, update_actor_freq=2, alpha=0.2, target_entropy=None, alpha_lr=1e-3) -> None:
        self.kind, self.tau, self.M, self.unbounded = kind, float(tau), float(max_action), bool(unbounded)
        self.policy_noise, self.noise_clip, self.freq = policy_noise, noise_clip, int(update_actor_freq)
        self.alpha, self.target_entropy, self.alpha_lr = alpha, target_entropy, alpha_lr
        self.kink = np.inf
        self.D = actor_dims[0]
        self.Ad = critic_dims[0] - self.D
        self.cond = kind != "sac" or actor_dims[-1] == 2 * self.Ad
        self.nets = {"actor": _Net(init["actor"], actor_dims, lr, self, 0 if self.cond else self.Ad), "critic": _Net(init["critic"], critic_dims, lr, self)}
        self.old = {"critic": self.nets["critic"].twin()}
        if kind != "ddpg":
            self.nets["critic2"] = _Net(init.get("critic2", init["critic"]), critic_dims, lr, self)
            self.old["critic2"] = self.nets["critic2"].twin()
        if kind != "sac":
            self.old["actor"] = self.nets["actor"].twin()
        self._cnt, self._last = 0, 0.0

    @property
    def alpha_value(self) -> float:
        return float(np.exp(self.alpha["log_alpha"])) if isinstance(self.alpha, dict) else float(self.alpha)

    def weights(self, name: str) -> np.ndarray:
        if name.endswith("_old"):
            return flat_of(self.old[name[:-4]])
        return flat_of(self.nets[name].params + self.nets[name].extra)

    def _mu_sigma(self, raw):
        """(mu_raw, sigma_raw) of the SAC actor's output: its two halves, or the output beside sigma_param."""
        if self.cond:
            return raw[:, :self.Ad], raw[:, self.Ad:]
        return raw, self.nets["actor"].extra[0].detach().numpy()

    def _q(self, name, obs, act, old=False, grad=False):
        net = self.nets[name]
        x = torch.cat([torch.as_tensor(np.asarray(obs, np.float64)), torch.as_tensor(np.asarray(act, np.float64))], 1)
        with torch.set_grad_enabled(grad):
            return net.fwd(self.old[name] if old else net.params, x)

    def _q_and_dqda(self, name, obs, act):
        """The critic on [obs | act] -> (q [B], d q / d act [B, Ad])."""
        a = torch.as_tensor(np.asarray(act, np.float64)).clone().requires_grad_(True)
        x = torch.cat([torch.as_tensor(np.asarray(obs, np.float64)), a], 1)
        q = self.nets[name].fwd(self.nets[name].params, x)
        (g,) = torch.autograd.grad(q.sum(), a)
        return q.detach().numpy().reshape(-1), g.numpy()

    def _actor(self, obs, old=False, grad=False):
        net = self.nets["actor"]
        with torch.set_grad_enabled(grad):
            return net.fwd(self.old["actor"] if old else net.params, obs)

    def returns(self, obs_next, mc, gpow, vmask, z=None) -> np.ndarray:
        Ad = self.Ad
        if self.kind == "sac":
            raw = self._actor(obs_next).numpy()
            s = sac_action(*self._mu_sigma(raw), z, self.M, self.unbounded)
            a, logp = s["a"], s["logp"]
        else:
            raw = self._actor(obs_next, old=True).numpy()
            a, _ = det_action(raw, self.M, z if self.kind == "td3" else None, self.policy_noise, self.noise_clip)
            logp = None
        q1 = self._q("critic", obs_next, a, old=True).numpy()
        q2 = self._q("critic2", obs_next, a, old=True).numpy() if self.kind != "ddpg" else None
        if q2 is not None and "critic2" in self.nets:
            self.kink = min(self.kink, float(np.abs(q1 - q2).min()) if not np.array_equal(q1, q2) else np.inf)
        return target(q1, q2, logp, self.alpha_value, mc, gpow, vmask)

    def _polyak(self, names) -> None:
        for n in names:
            for p, t in zip(self.nets[n].params, self.old[n]):
                t.copy_(self.tau * p.detach() + (1.0 - self.tau) * t)

    def update(self, obs, act, obs_next, mc, gpow, vmask, weight=None, z_target=None, z_actor=None) -> dict:
        ret = self.returns(obs_next, mc, gpow, vmask, z_target)
        twin = self.kind != "ddpg"
        q1 = self._q("critic", obs, act, grad=True)
        q2 = self._q("critic2", obs, act, grad=True) if twin else None
        ch = critic_head(q1.detach().numpy(), None if q2 is None else q2.detach().numpy(), ret, weight)
        grads = dict(critic=self.nets["critic"].step(q1, ch["dq1"]))
        if twin:
            grads["critic2"] = self.nets["critic2"].step(q2, ch["dq2"])
        out = dict(returns=ret, prio=ch["prio"], critic1_loss=ch["loss1"], critic2_loss=ch.get("loss2"), alpha_loss=None,
                   grads=grads)
        Ad = self.Ad
        if self.kind == "sac":
            raw = self._actor(obs, grad=True)
            r = raw.detach().numpy()
            m_raw, s_raw = self._mu_sigma(r)
            a = sac_action(m_raw, s_raw, z_actor, self.M, self.unbounded)["a"]
            q1a, g1 = self._q_and_dqda("critic", obs, a)
            q2a, g2 = self._q_and_dqda("critic2", obs, a)
            alpha_used = self.alpha_value
            ah = sac_actor_head(m_raw, s_raw, z_actor, q1a, q2a, g1, g2, alpha_used, self.M, self.unbounded)
            if not np.array_equal(q1a, q2a):
                self.kink = min(self.kink, ah["gap"])
            if self.cond:
                grads["actor"] = self.nets["actor"].step(raw, np.concatenate([ah["d_mu"], ah["d_sigma"]], 1))
            else:   # sigma_param is one row for the whole batch: its gradient is the sum over the rows
                grads["actor"] = self.nets["actor"].step(raw, ah["d_mu"], ah["d_sigma"].sum(0))
            if isinstance(self.alpha, dict):
                out["alpha_loss"] = alpha_step(self.alpha, ah["mean_entropy"], self.target_entropy, lr=self.alpha_lr)
            self._polyak(["critic", "critic2"])
            out.update(actor_loss=ah["loss"], alpha=self.alpha_value, alpha_used=alpha_used, mean_entropy=ah["mean_entropy"])
        else:
            if self.kind == "ddpg" or self._cnt % self.freq == 0:
                raw = self._actor(obs, grad=True)
                a, omt2 = det_action(raw.detach().numpy(), self.M)
                q_pi, g = self._q_and_dqda("critic", obs, a)
                ah = det_actor_head(g, omt2, q_pi, self.M)
                grads["actor"] = self.nets["actor"].step(raw, ah["d_raw"])
                self._last = ah["loss"]
                self._polyak(["critic", "actor"] + (["critic2"] if twin else []))
            self._cnt += 1
            out["actor_loss"] = self._last
        return out
