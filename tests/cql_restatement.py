"""Float64 restatement of the offline continuous learners CQL / Cal-QL and TD3+BC (reference imitation/cql.py:203-400,
imitation/td3_bc.py:102-127, algorithm_base.py:651-717, 1079-1134, torch.optim.Adam) and of every kernel of csrc/cql.hip --
the yardstick of the CQL tests.  Written from the description of what the reference computes, step by step, in numpy with
closed-form gradients of everything between a network product and an optimiser step (the networks themselves run in torch
float64, as in tests/cac_restatement.py, whose action and target pieces are used as they are); pinned to the reference by
tests/test_host_cql.py against tests/golden/cql.npz.

  `uniform`            the Philox site of tsm_cql_uniform: lo + u01(word) (hi - lo) at one counter, sub = element / 4
  `rows`               the stacked critic rows [B + 3 B R, D + Ad] (NaN where tsm_sac_action writes) and the actor's rows
  `head`, `finalize`   both critics' CQL loss, its gradient w.r.t. every Q, the statistics, the multiplier's gradient and step
  `td3bc_actor_head`   -lmbda mean Q + mse(a, a_data) and its gradient w.r.t. the actor's raw output
  `calibration_returns`   discounted return-to-go per buffer row, cut at episode ends and at unfinished tails
  `CqlRestatement`, `Td3bcRestatement`   the nets on flat vectors, their Adams, the reference's order of steps
"""
from __future__ import annotations

import numpy as np
import torch

from cac_restatement import (CacRestatement, _Net, critic_head, det_action, flat_of, sac_action, sac_actor_head,  # noqa: F401
                             target)
from dsac_restatement import alpha_state, alpha_step  # noqa: F401
from philox_restatement import M64, philox4, u01
from sampling_restatement import counters, own

UNIFORM_KEY = 0x43514C554E49464F   # csrc/cql.hip kUniformKey


def uniform(n: int, lo, hi, seed: int, offset: int = 0, offset_dev=None, dtype=np.float32):
    """Element j: word j % 4 of block (the ONE counter offset + *offset_dev, sub j / 4) under the key seed ^ UNIFORM_KEY;
    u01 (hi - lo) + lo, each step rounded to `dtype`.  -> (values [n], the words owned)."""
    key = (int(seed) ^ UNIFORM_KEY) & M64
    ctr = counters(offset, offset_dev, np.zeros(1, np.int64))
    w = philox4(key, ctr[0], np.arange((int(n) + 3) // 4))
    lo, hi = dtype(lo), dtype(hi)
    v = (u01(w, dtype).reshape(-1)[:int(n)] * dtype(hi - lo) + lo).astype(dtype)
    used = set()
    for j in range(int(n)):
        used |= own(key, ctr, j // 4, (j % 4,))
    return v, used


def rows(obs, obs_next, act, rand_act, R: int):
    obs, obs_next, act, rand_act = (np.asarray(v, np.float64) for v in (obs, obs_next, act, rand_act))
    B, Ad = act.shape
    rep, rep_next = np.repeat(obs, R, 0), np.repeat(obs_next, R, 0)
    hole = np.full((B * R, Ad), np.nan)
    X = np.concatenate([np.concatenate([obs, act], 1), np.concatenate([rep, rand_act], 1), np.concatenate([rep, hole], 1),
                        np.concatenate([rep, hole], 1)], 0)
    return X, np.concatenate([rep, rep_next], 0)


def _lse3(v, T):
    """T logsumexp(v / T) over the last axis with the maximum subtracted, and the softmax."""
    m = v.max(-1, keepdims=True)
    e = np.exp((v - m) / T)
    s = e.sum(-1, keepdims=True)
    return (m + T * np.log(s))[..., 0], e / s


def head(q1, q2, tgt, logp_cur, logp_next, R: int, Ad: int, calib=None, temperature=1.0, cql_weight=1.0, alpha_min=0.0,
         alpha_max=1e6, log_alpha=None, dtype=np.float64) -> dict:
    """Per critic k: mse_k, qmean_k, lse_k (mean over the B R groups), cql_k = w lse_k - w qmean_k and dq_k, the gradient of
    mse_k + cql_alpha cql_k (cql_alpha = clamp(exp(log_alpha)), or 1 without the multiplier).  `gap`: the smallest distance of
    a conservative value from its calibration return."""
    tgt = np.asarray(tgt, dtype).reshape(-1)
    B = tgt.shape[0]
    BR = B * R
    T, w = dtype(temperature), dtype(cql_weight)
    ca = dtype(1.0) if log_alpha is None else np.clip(np.exp(dtype(log_alpha)), dtype(alpha_min), dtype(alpha_max))
    logc = dtype(np.log(0.5 ** Ad))
    lp = np.stack([np.full(BR, logc), np.asarray(logp_cur, dtype).reshape(-1), np.asarray(logp_next, dtype).reshape(-1)], 1)
    out = dict(cql_alpha=float(ca), gap=np.inf)
    for k, q in ((1, q1), (2, q2)):
        q = np.asarray(q, dtype).reshape(-1)
        v = q[B:].reshape(3, BR).T - lp          # [BR, 3]: random, current, next
        passm = np.ones_like(v)
        if calib is not None:
            c = np.repeat(np.asarray(calib, dtype).reshape(-1), R)[:, None]
            out["gap"] = min(out["gap"], float(np.abs(v - c).min()))
            passm = np.where(v > c, 1.0, np.where(v == c, 0.5, 0.0)).astype(dtype)
            v = np.maximum(v, c)
        lse, sm = _lse3(v, T)
        td = q[:B] - tgt
        dq = np.empty_like(q)
        dq[:B] = 2 * td / dtype(B) - ca * w / dtype(B)
        dq[B:] = (ca * w * sm * passm / dtype(BR)).T.reshape(-1)
        out.update({f"dq{k}": dq, f"mse{k}": float((td * td).mean()), f"qmean{k}": float(q[:B].mean()), f"lse{k}": float(lse.mean()),
                    f"cql{k}": float(w * lse.mean() - w * q[:B].mean())})
    return out


def finalize(h: dict, lagrange_threshold=10.0, alpha_min=0.0, alpha_max=1e6, log_alpha=None, state: dict | None = None,
             lr=1e-4, betas=(0.9, 0.999), eps=1e-8) -> dict:
    """-> critic1_loss, critic2_loss, cql_alpha, cql_alpha_loss, d_log_alpha (None without the multiplier); `state` (a dict
    from `alpha_state`, whose log_alpha is the multiplier's) moves by one torch Adam step."""
    if log_alpha is None:
        return dict(critic1_loss=h["mse1"] + h["cql1"], critic2_loss=h["mse2"] + h["cql2"], cql_alpha=None, cql_alpha_loss=None,
                    d_log_alpha=None)
    ea = float(np.exp(log_alpha))
    ca = min(max(ea, alpha_min), alpha_max)
    excess = (h["cql1"] - lagrange_threshold) + (h["cql2"] - lagrange_threshold)
    g = -0.5 * excess * ea if alpha_min <= ea <= alpha_max else 0.0
    out = dict(critic1_loss=h["mse1"] + ca * (h["cql1"] - lagrange_threshold),
               critic2_loss=h["mse2"] + ca * (h["cql2"] - lagrange_threshold), cql_alpha=ca, cql_alpha_loss=-0.5 * ca * excess,
               d_log_alpha=g)
    if state is not None:
        st = state
        st["t"] += 1
        st["m"] = betas[0] * st["m"] + (1.0 - betas[0]) * g
        st["v"] = betas[1] * st["v"] + (1.0 - betas[1]) * g * g
        st["log_alpha"] -= lr / (1.0 - betas[0] ** st["t"]) * st["m"] / (np.sqrt(st["v"]) / np.sqrt(1.0 - betas[1] ** st["t"]) + eps)
    return out


def td3bc_actor_head(dq_da, omt2, q_pi, a, a_data, alpha, max_action=1.0, dtype=np.float64) -> dict:
    g, q, a, ad = np.asarray(dq_da, dtype), np.asarray(q_pi, dtype).reshape(-1), np.asarray(a, dtype), np.asarray(a_data, dtype)
    B, Ad = g.shape
    lmbda = dtype(alpha) / np.abs(q).mean()
    diff = a - ad
    d_raw = (-lmbda / dtype(B) * g + 2 * diff / dtype(B * Ad)) * dtype(max_action) * np.asarray(omt2, dtype)
    return dict(d_raw=d_raw, loss=float(-lmbda * q.mean() + (diff * diff).mean()), lmbda=float(lmbda))


def calibration_returns(rew, done, order_per_sub, gamma: float) -> np.ndarray:
    """compute_episodic_return(gamma, gae_lambda = 1) with no value estimate: per sub-buffer over its rows in time order
    (`order_per_sub`: the flat indices, oldest first), ret = rew + gamma ret_next, cut after a done row and at the tail."""
    rew, done = np.asarray(rew, np.float64), np.asarray(done, bool)
    out = np.zeros_like(rew)
    for order in order_per_sub:
        acc = 0.0
        for j, i in enumerate(reversed(list(order))):
            acc = rew[i] + (0.0 if (done[i] or j == 0) else gamma * acc)
            out[i] = acc
    return out


def clip_grad(params, max_norm: float) -> None:
    """torch.nn.utils.clip_grad_norm_ on the .grad of `params`."""
    total = float(torch.sqrt(sum((p.grad.detach() ** 2).sum() for p in params)))
    coef = min(max_norm / (total + 1e-6), 1.0)
    for p in params:
        p.grad.mul_(coef)


class CqlRestatement:
    """`init`: flat vectors actor ([mu_raw | sigma_raw] last layer), critic[, critic2].  alpha: a float, or a dict from
    `alpha_state` with `target_entropy` / `alpha_lr`."""

    def __init__(self, init, actor_dims, critic_dims, tau, gamma, lr=1e-3, max_action=1.0, alpha=0.2, target_entropy=None,
                 alpha_lr=1e-3, cql_alpha_lr=1e-4, cql_weight=1.0, temperature=1.0, with_lagrange=True, lagrange_threshold=10.0,
                 num_repeat_actions=10, alpha_min=0.0, alpha_max=1e6, max_grad_norm=1.0, calibrated=True) -> None:
        self.kink, self.calib_gap = np.inf, np.inf
        self.tau, self.gamma, self.M = float(tau), float(gamma), float(max_action)
        self.alpha, self.target_entropy, self.alpha_lr = alpha, target_entropy, alpha_lr
        self.cql_alpha_lr, self.w, self.T, self.lagrange, self.thr = cql_alpha_lr, cql_weight, temperature, with_lagrange, lagrange_threshold
        self.R, self.alpha_min, self.alpha_max, self.max_grad_norm, self.calibrated = num_repeat_actions, alpha_min, alpha_max, max_grad_norm, calibrated
        self.D = actor_dims[0]
        self.Ad = critic_dims[0] - self.D
        self.nets = {"actor": _Net(init["actor"], actor_dims, lr, self), "critic": _Net(init["critic"], critic_dims, lr, self),
                     "critic2": _Net(init.get("critic2", init["critic"]), critic_dims, lr, self)}
        self.old = {n: self.nets[n].twin() for n in ("critic", "critic2")}
        self.cql = alpha_state(0.0)

    weights = CacRestatement.weights
    alpha_value = CacRestatement.alpha_value
    _q_and_dqda = CacRestatement._q_and_dqda

    def _fwd(self, name, x, old=False, grad=False):
        net = self.nets[name]
        with torch.set_grad_enabled(grad):
            return net.fwd(self.old[name] if old else net.params, x)

    def _sample(self, obs, z):
        raw = self._fwd("actor", obs).numpy()
        s = sac_action(raw[:, :self.Ad], raw[:, self.Ad:], z, self.M, False)
        return s["a"], s["logp"]

    def _critic_step(self, name, q, dq) -> np.ndarray:
        net = self.nets[name]
        net.opt.zero_grad()
        q.backward(torch.as_tensor(dq).reshape(q.shape))
        g = flat_of([p.grad for p in net.params])   # before the clip: what the backward gives
        clip_grad(net.params, self.max_grad_norm)
        net.opt.step()
        return g

    def update(self, obs, act, rew, done, obs_next, calib, z_actor, z_target, z_cur, z_next, u) -> dict:
        obs, act, obs_next = (np.asarray(v, np.float64) for v in (obs, act, obs_next))
        B, R, Ad = obs.shape[0], self.R, self.Ad
        # 1. the actor's step against the critics as they are
        raw = self._fwd("actor", obs, grad=True)
        r = raw.detach().numpy()
        a = sac_action(r[:, :Ad], r[:, Ad:], z_actor, self.M, False)["a"]
        q1a, g1 = self._q_and_dqda("critic", obs, a)
        q2a, g2 = self._q_and_dqda("critic2", obs, a)
        ah = sac_actor_head(r[:, :Ad], r[:, Ad:], z_actor, q1a, q2a, g1, g2, self.alpha_value, self.M, False)
        if not np.array_equal(q1a, q2a):
            self.kink = min(self.kink, ah["gap"])
        grads = dict(actor=self.nets["actor"].step(raw, np.concatenate([ah["d_mu"], ah["d_sigma"]], 1)))
        # 2. the entropy coefficient
        alpha_loss = None
        if isinstance(self.alpha, dict):
            alpha_loss = alpha_step(self.alpha, ah["mean_entropy"], self.target_entropy, lr=self.alpha_lr)
        # 3. the one-step target with the moved actor and the new alpha
        a_n, logp_n = self._sample(obs_next, z_target)
        x_n = np.concatenate([obs_next, a_n], 1)
        tq1, tq2 = self._fwd("critic", x_n, old=True).numpy().reshape(-1), self._fwd("critic2", x_n, old=True).numpy().reshape(-1)
        if not np.array_equal(tq1, tq2):
            self.kink = min(self.kink, float(np.abs(tq1 - tq2).min()))
        # logical_not(done) * gamma is a float32 tensor in any run (cql.py:290): gamma enters the product rounded to float32
        tgt = target(tq1, tq2, logp_n, self.alpha_value, rew, np.full(B, np.float64(np.float32(self.gamma))), ~np.asarray(done, bool))
        # 4. the conservative term on the stacked rows
        X, A = rows(obs, obs_next, act, u, R)
        a_pi, logp_pi = self._sample(A, np.concatenate([z_cur, z_next], 0))
        X[B + B * R:, self.D:] = a_pi
        q1, q2 = self._fwd("critic", X, grad=True), self._fwd("critic2", X, grad=True)
        la = self.cql["log_alpha"] if self.lagrange else None
        h = head(q1.detach().numpy(), q2.detach().numpy(), tgt, logp_pi[:B * R], logp_pi[B * R:], R, Ad,
                 calib if self.calibrated else None, self.T, self.w, self.alpha_min, self.alpha_max, la)
        self.calib_gap = min(self.calib_gap, h["gap"])
        # 5. the multiplier's step (the gradients in h hold the cql_alpha of before it)
        fin = finalize(h, self.thr, self.alpha_min, self.alpha_max, la, self.cql if self.lagrange else None, lr=self.cql_alpha_lr)
        # 6. the critics' clipped steps, 7. the Polyak move
        grads["critic"] = self._critic_step("critic", q1, h["dq1"])
        grads["critic2"] = self._critic_step("critic2", q2, h["dq2"])
        for n in ("critic", "critic2"):
            for p, t in zip(self.nets[n].params, self.old[n]):
                t.copy_(self.tau * p.detach() + (1.0 - self.tau) * t)
        return dict(actor_loss=ah["loss"], alpha=self.alpha_value, alpha_loss=alpha_loss, target=tgt, grads=grads,
                    cql_log_alpha=self.cql["log_alpha"], **fin)


class Td3bcRestatement(CacRestatement):
    """TD3 with TD3+BC's actor loss (td3_bc.py:113-119)."""

    def __init__(self, *args, bc_alpha=2.5, **kwargs) -> None:
        super().__init__("td3", *args, **kwargs)
        self.bc_alpha = bc_alpha

    def update(self, obs, act, obs_next, mc, gpow, vmask, weight=None, z_target=None, z_actor=None) -> dict:
        ret = self.returns(obs_next, mc, gpow, vmask, z_target)
        q1, q2 = self._q("critic", obs, act, grad=True), self._q("critic2", obs, act, grad=True)
        ch = critic_head(q1.detach().numpy(), q2.detach().numpy(), ret, weight)
        grads = dict(critic=self.nets["critic"].step(q1, ch["dq1"]), critic2=self.nets["critic2"].step(q2, ch["dq2"]))
        if self._cnt % self.freq == 0:
            raw = self._actor(obs, grad=True)
            a, omt2 = det_action(raw.detach().numpy(), self.M)
            q_pi, g = self._q_and_dqda("critic", obs, a)
            ah = td3bc_actor_head(g, omt2, q_pi, a, act, self.bc_alpha, self.M)
            grads["actor"] = self.nets["actor"].step(raw, ah["d_raw"])
            self._last = ah["loss"]
            self._polyak(["critic", "actor", "critic2"])
        self._cnt += 1
        return dict(returns=ret, prio=ch["prio"], critic1_loss=ch["loss1"], critic2_loss=ch["loss2"], alpha_loss=None,
                    actor_loss=self._last, grads=grads)
