"""The Gaussian policy of csrc/gauss.hip restated in float64 torch: `torch.distributions` for the density, autograd for every
gradient, nothing of the library.  continuous.py:238-247 (mu, sigma), reinforce.py:183-192 (Independent(Normal, 1)),
algorithm_base.py:255-288 (map_action), ppo.py:182-211 and a2c.py:260-270 (the policy terms)."""
from __future__ import annotations

import numpy as np
import torch
from torch.distributions import Independent, Normal

import sampling_restatement as sr

GAUSS_KEY = 0x4741555353504F4C   # csrc/gauss.hip kGaussKey


def dist(mu_raw, sigma_raw, cond: bool, unbounded: bool, max_action: float):
    """mu_raw [B, Ad]; sigma_raw [B, Ad] (conditioned: clamped to [-20, 2]) or [Ad] (sigma_param: not clamped)."""
    mu = mu_raw if unbounded else max_action * torch.tanh(mu_raw)
    log_sigma = torch.clamp(sigma_raw, min=-20.0, max=2.0) if cond else sigma_raw.view(1, -1) + torch.zeros_like(mu)
    return Independent(Normal(mu, log_sigma.exp()), 1)


def normals(B: int, Ad: int, seed: int, offset: int, offset_dev, dtype=np.float64) -> np.ndarray:
    """The launch's draw [B, Ad]: cac_normal's pairing over the elements b Ad + k, under this site's key."""
    return sr.cac_normal(B * Ad, seed ^ sr.NORMAL_KEY ^ GAUSS_KEY, offset, offset_dev, dtype)[0].reshape(B, Ad)


def map_action(act, bound, low, high):
    act = np.asarray(act, np.float64)
    act = np.clip(act, -1.0, 1.0) if bound == "clip" else np.tanh(act) if bound == "tanh" else act
    return act if low is None else low + (high - low) * (act + 1.0) / 2.0


def policy_terms(d, act, logp_old, adv, eps_clip=0.2, dual_clip=None, loss_kind=0):
    """-> (obj [M], entropy [M], ratio [M]) of ppo.py:187-196 (kind 0) / a2c.py:263 (kind 1); adv already normalised."""
    logp = d.log_prob(act)
    ratio = (logp - logp_old).exp()
    if loss_kind == 1:
        return logp * adv, d.entropy(), ratio
    clip1 = torch.min(ratio * adv, ratio.clamp(1.0 - eps_clip, 1.0 + eps_clip) * adv)
    if dual_clip:
        clip1 = torch.where(adv < 0, torch.max(clip1, dual_clip * adv), clip1)
    return clip1, d.entropy(), ratio


def head(mu_raw, sigma_raw, act, logp_old, adv, cond, unbounded, max_action, adv_norm, ent_coef=0.01, **kw) -> dict:
    """One minibatch, float64 numpy in: loss = -mean(obj) - ent_coef mean(entropy) and its autograd gradients."""
    t = lambda x: torch.as_tensor(np.asarray(x, np.float64))  # noqa: E731
    m, s = t(mu_raw).requires_grad_(), t(sigma_raw).requires_grad_()
    a = t(adv)
    if adv_norm:
        a = (a - a.mean()) / (a.std() + 1e-8)
    obj, ent, ratio = policy_terms(dist(m, s, cond, unbounded, max_action), t(act), t(logp_old), a, **kw)
    clip_loss, ent_loss = -obj.mean(), ent.mean()
    (clip_loss - ent_coef * ent_loss).backward()
    return dict(d_mu=m.grad.numpy(), d_sigma=s.grad.numpy(), clip_loss=float(clip_loss.detach()), ent_loss=float(ent_loss.detach()),
                ratio=ratio.detach().numpy(), adv=a.numpy())


def mlp(f):
    """A float64 torch copy of a FlatMLP's layers."""
    layers = []
    for i in range(f.n_layers):
        lin = torch.nn.Linear(f.dims[i], f.dims[i + 1]).double()
        with torch.no_grad():
            lin.weight.copy_(f.weight(i).cpu().double())
            lin.bias.copy_(f.bias(i).cpu().double())
        layers += [lin] + ([torch.nn.Tanh() if f.act == "tanh" else torch.nn.ReLU()] if i + 1 < f.n_layers else [])
    return torch.nn.Sequential(*layers)


def update(net, store, gae, bounds, perms, N, glob, lr, max_grad_norm, eps_clip=0.2, vf_coef=0.5, ent_coef=0.01):
    """One PPO update (value clip and advantage normalisation on) on float64 copies of `net`: store = dict of the time-major
    [T, B, N, ...] arrays, gae(v_s, v_next) -> (ret, adv) [T, L]; perms: per repeat the permuted units (lanes, or joint rows with
    a centralized critic), bounds their minibatch split.  -> (actor, sigma_param | None, critic, per-step [loss, clip, vf, ent])."""
    actor, critic = mlp(net.actor), mlp(net.critic)
    a_net = net.actor
    cond = a_net.conditioned_sigma
    sigma = None if cond else torch.nn.Parameter(a_net.sigma_param.cpu().double().clone())
    params = list(actor.parameters()) + ([] if cond else [sigma]) + list(critic.parameters())
    opt = torch.optim.Adam(params, lr=lr)
    t = lambda x: torch.as_tensor(np.asarray(x)).double()  # noqa: E731
    obs, obs_next, act = t(store["obs"]), t(store["obs_next"]), t(store["act"])
    T, B, _, D = obs.shape
    Ad = act.shape[-1]

    def policy(x):
        raw = actor(x)
        return dist(raw[..., :Ad], raw[..., Ad:] if cond else sigma, cond, a_net.unbounded, a_net.max_action)

    def values(o):
        return critic(o.reshape(T * B, N * D)).reshape(T * B, 1).expand(T * B, N) if glob else critic(o.reshape(T * B, N, D)).squeeze(-1)

    with torch.no_grad():
        v_s, v_n = values(obs), values(obs_next)
        logp_old = policy(obs.reshape(-1, D)).log_prob(act.reshape(-1, Ad)).float().double()   # (the update reads it as f32)
    ret, adv = gae(v_s.numpy().astype(np.float32).reshape(T, B * N), v_n.numpy().astype(np.float32).reshape(T, B * N))
    ret, adv, v_old = t(ret.astype(np.float32)).reshape(-1), t(adv.astype(np.float32)).reshape(-1), v_s.reshape(-1).float().double()
    losses = []
    for perm in perms:
        for s, e in bounds:
            units = torch.as_tensor(perm[s:e])
            lanes = (units.view(-1, 1) * N + torch.arange(N).view(1, -1)).reshape(-1) if glob else units
            a = adv[lanes]
            a = (a - a.mean()) / (a.std() + 1e-8)
            obj, ent, _ = policy_terms(policy(obs.reshape(-1, D)[lanes]), act.reshape(-1, Ad)[lanes], logp_old[lanes], a, eps_clip)
            value = values(obs).reshape(-1)[lanes]
            v_clip = v_old[lanes] + (value - v_old[lanes]).clamp(-eps_clip, eps_clip)
            vf = torch.max((ret[lanes] - value) ** 2, (ret[lanes] - v_clip) ** 2).mean()
            clip_loss, ent_loss = -obj.mean(), ent.mean()
            loss = clip_loss + vf_coef * vf - ent_coef * ent_loss
            opt.zero_grad()
            loss.backward()
            if max_grad_norm:
                torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
            opt.step()
            losses.append([float(x.detach()) for x in (loss, clip_loss, vf, ent_loss)])
    return actor, sigma, critic, np.asarray(losses)
