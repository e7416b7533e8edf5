"""DDPG, TD3 and SAC: the off-policy actor-critics for `Box` actions on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelfree/ddpg.py (`ContinuousPolicyWithExplorationNoise` :45-111,
`ContinuousDeterministicPolicy` :114-190, `DDPG` :342-410), td3.py (`TD3` :105-226) and sac.py (`SACPolicy` :54-131, `SAC`
:212-336) on actor_critic.py's learner core, twin-critic base and entropy coefficient; `ContinuousActionRows` adds what only a
`Box` action asks for.  The actors and critics are `FlatMLP`s (utils/net.py: `ContinuousActorDeterministic`,
`ContinuousActorProbabilistic`, `ContinuousCritic`; csrc/dense.hip); the critics read rows [obs | act] built by
`tsm_maddpg_joint_rows` with one agent; the n-step walk is `tsm_nstep_return`; what lies between a network product and an
optimiser step is one launch each in csrc/cac.hip.  There is no autograd fallback.

Kept quirks: Q44 -- DDPG's and TD3's actor loss reads the critic AFTER its step of the same call; Q45 --
TD3 steps the actor, moves the lagged nets and reports a fresh actor_loss only on calls 0, f, 2f, ...; otherwise `_last` is
reported again; Q46 -- TD3's smoothed target action is not clamped to the action bounds; Q47 -- SAC's target samples from the
ONLINE actor (there is no actor_old); Q48 -- `critic2=None` is a copy of `critic` that stays identical to it, and at q1 = q2 the
minimum's gradient is half of each (torch.min's backward); Q49 -- the log-prob correction is log(1 - a^2 + finfo(float32).eps);
Q50 -- SAC's alpha is stepped from the entropy of before the actor's step, and the actor loss used the alpha of before that.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Any, Literal

import numpy as np
import torch
from torch import nn

from .. import ops
from ..data.batch import Batch
from ..data.stats import TrainingStats
from ..utils.learner import act_result, result_slot, sample_counter, slab_workspace
from ..utils.net import (ContinuousActorDeterministic, ContinuousActorProbabilistic, ContinuousCritic, FlatMLP, lagged_copy)
from ..utils.tensor import to_tensor
from .actor_critic import ActorCriticOffPolicyAlgorithm, ActorDualCriticsOffPolicyAlgorithm, Alpha, EntropyCoefficient
from .dqn import _obs_rows
from .optim import AdamOptimizerFactory


@dataclass(kw_only=True)
class DDPGTrainingStats(TrainingStats):
    actor_loss: float
    critic_loss: float


@dataclass(kw_only=True)
class TD3TrainingStats(TrainingStats):
    actor_loss: float
    critic1_loss: float
    critic2_loss: float


@dataclass(kw_only=True)
class SACTrainingStats(TrainingStats):
    actor_loss: float
    critic1_loss: float
    critic2_loss: float
    alpha: float | None = None
    alpha_loss: float | None = None


class GaussianNoise:
    """exploration/random.py `GaussianNoise`: `noise(size)` -> numpy normal(mu, sigma) draws from numpy's global RNG."""

    def __init__(self, mu: float = 0.0, sigma: float = 1.0) -> None:
        assert sigma >= 0, "Noise std should not be negative."
        self._mu, self._sigma = mu, sigma

    def __call__(self, size) -> np.ndarray:
        return np.random.normal(self._mu, self._sigma, size)

    def reset(self) -> None:
        pass


# ---- the policies (ddpg.py:45-190, sac.py:54-131) -----------------------------------------------------------------------
class _ContinuousPolicy(nn.Module):
    """ddpg.py:45-111 and `Policy.map_action` (algorithm_base.py) for a `Box`."""

    _actor_cls: type = FlatMLP

    def __init__(self, actor, exploration_noise, action_space, observation_space, action_scaling: bool, action_bound_method,
                 seed: int) -> None:
        super().__init__()
        if not isinstance(actor, self._actor_cls):
            raise TypeError(f"{type(self).__name__} needs a {self._actor_cls.__name__} actor: the update runs in HIP, there is "
                            f"no autograd fallback (got {type(actor).__name__})")
        if not all(hasattr(action_space, k) for k in ("low", "high", "shape")):
            raise ValueError(f"{type(self).__name__} only supports a Box action space, got {type(action_space).__name__}")
        if len(action_space.shape) != 1 or int(action_space.shape[0]) != actor.act_dim:
            raise ValueError(f"{type(self).__name__}: the actor gives {actor.act_dim} action components, the Box has shape "
                             f"{tuple(action_space.shape)}")
        if action_bound_method not in ("clip", None):
            raise ValueError(f"action_bound_method must be 'clip' or None, got {action_bound_method!r}")
        if exploration_noise == "default":
            exploration_noise = GaussianNoise(sigma=0.1)
        self.actor = actor
        self.exploration_noise = exploration_noise
        self.action_space, self.observation_space = action_space, observation_space
        self.action_scaling, self.action_bound_method = bool(action_scaling), action_bound_method
        self.act_dim = actor.act_dim
        self.seed = int(seed)
        self._sample_ctr = 0
        self.is_within_training_step = False
        dev, Ad = actor.flat.device, actor.act_dim
        self._low = torch.as_tensor(np.broadcast_to(np.asarray(action_space.low, np.float32), (Ad,)).copy(), device=dev)
        self._high = torch.as_tensor(np.broadcast_to(np.asarray(action_space.high, np.float32), (Ad,)).copy(), device=dev)
        self._unit = (-torch.ones(Ad, device=dev), torch.ones(Ad, device=dev))
        # map_action's scaling moves nothing for a Box of [-1, 1]: decided here, on the host bounds
        self._rescale = bool(action_scaling) and not (np.all(np.asarray(action_space.low) == -1.0) and
                                                      np.all(np.asarray(action_space.high) == 1.0))
        self._half_span = (self._high - self._low) / 2.0
        self._sigma_dev = torch.zeros(1, dtype=torch.float32, device=dev)

    @property
    def device(self) -> torch.device:
        return self.actor.flat.device

    def set_exploration_noise(self, noise) -> None:
        self.exploration_noise = noise

    def add_exploration_noise(self, act, batch):
        """ddpg.py:101-111, on the host."""
        if self.exploration_noise is None:
            return act
        if isinstance(act, np.ndarray):
            return act + self.exploration_noise(act.shape)
        warnings.warn("Cannot add exploration noise to non-numpy_array action.")
        return act

    def map_action(self, act):
        """Policy.map_action: clip to [-1, 1] ("clip"), then scale to [low, high] (action_scaling); numpy in, numpy out."""
        act = np.asarray(act)
        if self.action_bound_method == "clip":
            act = np.clip(act, -1.0, 1.0)
        if self.action_scaling:
            low, high = np.asarray(self.action_space.low), np.asarray(self.action_space.high)
            act = low + (high - low) * (act + 1.0) / 2.0
        return act

    def _obs(self, batch: Batch) -> torch.Tensor:
        obs, mask = _obs_rows(batch.obs)
        if mask is not None:
            raise NotImplementedError(f"{type(self).__name__}: action masks have no meaning for a Box action")
        return to_tensor(obs, self.device, torch.float32).reshape(-1, self.actor.dims[0])

    def _emit(self, act: torch.Tensor, sigma: float, out: dict | None, offset_dev, row_offset: int, **extra) -> dict:
        """The acting epilogue through `tsm_maddpg_act` with one agent: sigma times a normal draw, the clip of `map_action`;
        its scaling to the Box, where the Box is not [-1, 1], is low + (a + 1) (high - low) / 2 in place on the result."""
        self._sigma_dev.fill_(float(sigma))
        lo, hi = self._unit if self.action_bound_method == "clip" else (None, None)
        n = act.numel()
        a = ops.maddpg_act([act], self._sigma_dev, self.seed, offset=sample_counter(self, n, row_offset, offset_dev),
                           offset_dev=offset_dev, low=lo, high=hi, out=None if out is None else out["act"])
        if self._rescale:
            a.view(-1, self.act_dim).add_(1.0).mul_(self._half_span).add_(self._low)
        return act_result(out, a, **extra)


class ContinuousDeterministicPolicy(_ContinuousPolicy):
    """ddpg.py:114-190 with a `ContinuousActorDeterministic`.  `seed` keys the Philox draws (`act_device`'s exploration noise,
    TD3's target smoothing)."""

    _actor_cls = ContinuousActorDeterministic

    def __init__(self, *, actor: ContinuousActorDeterministic, exploration_noise: Any | Literal["default"] | None = None,
                 action_space: Any, observation_space: Any = None, action_scaling: bool = True,
                 action_bound_method: Literal["clip"] | None = "clip", seed: int = 0) -> None:
        if action_scaling and isinstance(actor, ContinuousActorDeterministic) and not np.isclose(actor.max_action, 1.0):
            warnings.warn("action_scaling and action_bound_method are only intended to deal with unbounded model action space, "
                          f"but find actor model bound action space with max_action={actor.max_action}.")
        super().__init__(actor, exploration_noise, action_space, observation_space, action_scaling, action_bound_method, seed)

    def forward(self, batch: Batch, state: Any = None, model: ContinuousActorDeterministic | None = None, **kwargs: Any) -> Batch:
        """-> Batch(act = max_action * tanh(model(obs)) as numpy f32 [B, Ad], state)."""
        model = self.actor if model is None else model
        raw = FlatMLP.forward(model, self._obs(batch), save=False)
        return Batch(act=ops.cac_det_action(raw, model.max_action).cpu().numpy(), state=state)

    def act_device(self, obs: torch.Tensor, out: dict | None = None, offset_dev: torch.Tensor | None = None,
                   row_offset: int = 0) -> dict:
        """obs [..., D] in HBM -> act f32 [rows, Ad]: the actor, its tanh, then `_emit` with the exploration sigma within a
        training step (a `GaussianNoise`-like object's `_sigma`; its mean is not served here)."""
        raw = FlatMLP.forward(self.actor, obs.reshape(-1, self.actor.dims[0]), save=False)
        act = ops.cac_det_action(raw, self.actor.max_action)
        noise = self.exploration_noise if self.is_within_training_step else None
        return self._emit(act, 0.0 if noise is None else float(noise._sigma), out, offset_dev, row_offset)


class SACPolicy(_ContinuousPolicy):
    """sac.py:54-131 with a `ContinuousActorProbabilistic`; the normal draws come from `tsm_cac_normal` under `seed`."""

    _actor_cls = ContinuousActorProbabilistic

    def __init__(self, *, actor: ContinuousActorProbabilistic, exploration_noise: Any | Literal["default"] | None = None,
                 deterministic_eval: bool = True, action_scaling: bool = True, action_space: Any,
                 observation_space: Any = None, seed: int = 0) -> None:
        super().__init__(actor, exploration_noise, action_space, observation_space, action_scaling, None, seed)
        self.deterministic_eval = deterministic_eval

    @property
    def _deterministic(self) -> bool:
        return bool(self.deterministic_eval and not self.is_within_training_step)

    def _sample(self, x: torch.Tensor, z: torch.Tensor | None = None):
        """The actor on rows x -> (raw, act [B, Ad], logp [B]); z None: a draw, or the mode when deterministic."""
        raw = FlatMLP.forward(self.actor, x, save=False)
        if z is None and not self._deterministic:
            n = x.shape[0] * self.act_dim
            z = ops.cac_normal(n, self.seed, offset=self._sample_ctr, device=x.device).view(x.shape[0], self.act_dim)
            self._sample_ctr += n
        act, logp = ops.sac_action(raw, z, self.actor.max_action, self.actor.unbounded, sigma_param=self.actor.sigma_param)
        return raw, act, logp

    def forward(self, batch: Batch, state: Any = None, **kwargs: Any) -> Batch:
        """-> Batch(logits = the actor's raw output in HBM ([mu_raw | sigma_raw], or mu_raw beside the actor's sigma_param), act numpy f32 [B, Ad], log_prob [B, 1] in HBM,
        state).  The reference's `dist` field is not carried."""
        raw, act, logp = self._sample(self._obs(batch))
        return Batch(logits=raw, act=act.cpu().numpy(), state=state, log_prob=logp.unsqueeze(-1))

    def act_device(self, obs: torch.Tensor, out: dict | None = None, offset_dev: torch.Tensor | None = None,
                   row_offset: int = 0) -> dict:
        _, act, logp = self._sample(obs.reshape(-1, self.actor.dims[0]))
        return self._emit(act, 0.0, out, offset_dev, row_offset)


# ---- the learners (ddpg.py:196-410, td3.py, sac.py:212-336) -------------------------------------------------------------
class ContinuousActionRows:
    """What a `Box` action adds to actor_critic.py's learner core, in front of it in a learner's bases: the critic
    [obs | act] -> 1 and its checks, the rows [obs | act], the normal draws, the deterministic and the SAC-style actor step, the
    twin target, and the policy's Philox counter in the checkpoint."""

    _policy_cls: type = _ContinuousPolicy
    noise_source = None   # (rows, act_dim) -> f32 [rows, act_dim] in HBM: stands in for the Philox draws (tests)

    def _check_bounds(self, policy, n_step: int) -> None:
        ops.cac_check(policy.act_dim, n_step)

    def _check_critic(self, name: str, net) -> None:
        actor = self.policy.actor
        D, Ad, dev = actor.dims[0], self.policy.act_dim, actor.flat.device
        if not isinstance(net, FlatMLP):
            raise TypeError(f"{type(self).__name__}: {name} must be a ContinuousCritic / FlatMLP [obs | act] -> 1 "
                            f"(got {type(net).__name__})")
        if net.dims[0] != D + Ad or net.dims[-1] != 1 or net.flat.device != dev:
            raise ValueError(f"{type(self).__name__}: {name} maps {net.dims[0]} -> {net.dims[-1]} on {net.flat.device}; it must "
                             f"map {D} + {Ad} -> 1 on {dev}")

    def _normal(self, B: int) -> torch.Tensor:
        """Standard normals f32 [B, act_dim]: `noise_source`'s, or `tsm_cac_normal` at the policy's Philox counter."""
        Ad = self.policy.act_dim
        if self.noise_source is not None:
            return to_tensor(self.noise_source(B, Ad), self.device, torch.float32).reshape(B, Ad).contiguous()
        z = ops.cac_normal(B * Ad, self.policy.seed, offset=self.policy._sample_ctr, device=self.device).view(B, Ad)
        self.policy._sample_ctr += B * Ad
        return z

    def _work(self, B: int, **slabs: int) -> dict:
        D, Ad, dev = self.policy.actor.dims[0], self.policy.act_dim, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        return slab_workspace(self._ws, B, dev, more=lambda: dict(
            x=torch.empty(B, D + Ad, **f32), x_next=torch.empty(B, D + Ad, **f32), x_pi=torch.empty(B, D + Ad, **f32),
            ones=torch.ones(B, 1, **f32)), **slabs)

    def _batch_rows(self, batch: Batch):
        """-> (obs [B, D], act [B, Ad]) of the batch as f32 in HBM."""
        obs = self.policy._obs(batch)
        act = to_tensor(batch.act, self.device, torch.float32).reshape(obs.shape[0], self.policy.act_dim).contiguous()
        return obs, act

    def _successors(self, batch: Batch, buffer, indices, agent):
        """The n-step walk -> (obs_next[idx_n] [B, D], the workspace, the rows [obs_next | .]: the observation columns are
        copied in, the action columns are the caller's action kernel's to fill)."""
        _, idx_n, col = self._nstep_rows(batch, buffer, indices, agent)
        nxt, mask_next = self._successor_rows(buffer, idx_n, col)
        if mask_next is not None:
            raise NotImplementedError(f"{type(self).__name__}: action masks have no meaning for a Box action")
        w = self._work(nxt.shape[0], **self._slab_widths())
        w["x_next"][:, :nxt.shape[1]].copy_(nxt)
        return nxt, w, w["x_next"]

    def _begin_update(self, batch: Batch):
        dev = self.device
        weight = self._pop_weight(batch)
        obs, act = self._batch_rows(batch)
        B = obs.shape[0]
        w = self._work(B, **self._slab_widths())
        x = ops.maddpg_joint_rows([obs], [act], out=w["x"])
        returns = to_tensor(batch.returns, dev, torch.float32).reshape(-1)
        return obs, act, B, w, x, returns, None if weight is None else to_tensor(weight, dev, torch.float32).reshape(-1)

    def _det_actor_step(self, w: dict, obs, act, B: int):
        """actor_loss = -critic(obs, actor(obs)).mean() against the critic as it is now, the actor's Adam step.
        -> the head's partials."""
        actor, D, Ad = self.policy.actor, obs.shape[1], self.policy.act_dim
        raw = FlatMLP.forward(actor, obs, save=True)
        x_pi = ops.maddpg_joint_rows([obs], [act], out=w["x_pi"])
        _, omt2 = ops.cac_det_action(raw, actor.max_action, out=x_pi, col0=D, want_backward=True)
        q_pi = FlatMLP.forward(self.critic, x_pi, save=True)
        dq_da = self.critic.input_grad(w["ones"], D, Ad)
        ah = self._det_actor_head(dq_da, omt2, q_pi, x_pi[:, D:], act)
        actor.backward(ah["d_raw"], w["n_split"], slabs=w["slabs_a"])
        self.policy_optim.step(w["slabs_a"])
        return ah["partial"]

    def _det_actor_head(self, dq_da, omt2, q_pi, act_pi, act) -> dict:
        """The deterministic actor's loss head -> dict(d_raw, partial): -mean Q (ddpg.py:406, td3.py:216); a subclass with
        another actor loss (TD3+BC) reads the policy's action `act_pi` and the batch's `act` as well."""
        return ops.cac_det_actor_head(dq_da, omt2, q_pi, self.policy.actor.max_action)

    def _sac_actor_step(self, w: dict, obs, act, B: int, critics, alpha_dev) -> dict:
        """The Gaussian-tanh actor's step (sac.py:315-322, redq.py:284-291): a sample of the actor in the action columns of
        x_pi, `critics(x_pi)` -> (q1a, q2a, g1, g2) the critic values there and their gradients to the action (q2a, g2 None:
        one value), `tsm_sac_actor_head`, the actor's backward and Adam step.  -> the head's dict."""
        actor, D = self.policy.actor, obs.shape[1]
        raw = FlatMLP.forward(actor, obs, save=True)
        z = self._normal(B)
        x_pi = ops.maddpg_joint_rows([obs], [act], out=w["x_pi"])
        ops.sac_action(raw, z, actor.max_action, actor.unbounded, sigma_param=actor.sigma_param, out=x_pi, col0=D)
        q1a, q2a, g1, g2 = critics(x_pi)
        ah = ops.sac_actor_head(raw, z, q1a, q2a, g1, g2, alpha_dev, actor.max_action, actor.unbounded,
                                sigma_param=actor.sigma_param)
        P = actor.flat.numel()   # the layers' gradient slabs, and behind them sigma_param's: the head's rows summed
        actor.backward(ah["d_raw"], w["n_split"], slabs=w["slabs_a"], slab_stride=P)
        if ah["d_sigma"] is not None:
            ops.cac_col_sum(ah["d_sigma"], w["slabs_a"][:, actor.n_mlp_params:])
        self.policy_optim.step(w["slabs_a"])
        return ah

    def _twin_target(self, batch: Batch, x_next, logp=None, alpha_dev=None):
        """The minimum of the two lagged critics on the rows x_next (minus alpha logp: SAC's) as the n-step target."""
        q1 = FlatMLP.forward(self.critic_old, x_next, save=False)
        q2 = FlatMLP.forward(self.critic2_old, x_next, save=False)
        return ops.cac_target(q1, q2, batch.mc, batch.gpow, batch.vmask, logp_next=logp, alpha_dev=alpha_dev)

    # ---- checkpoints: the policy's Philox counter beside the core's entries --------------------------------------------
    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = super().state_dict()
        sd["sample_ctr"] = self.policy._sample_ctr
        return sd

    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        super().load_state_dict(sd)
        self.policy._sample_ctr = int(sd.get("sample_ctr", 0))


class DDPG(ContinuousActionRows, ActorCriticOffPolicyAlgorithm):
    """ddpg.py:342-410."""

    _policy_cls = ContinuousDeterministicPolicy

    def __init__(self, *, policy: ContinuousDeterministicPolicy, policy_optim: AdamOptimizerFactory, critic: ContinuousCritic,
                 critic_optim: AdamOptimizerFactory, tau: float = 0.005, gamma: float = 0.99,
                 n_step_return_horizon: int = 1) -> None:
        super().__init__(policy=policy, policy_optim=policy_optim, critic=critic, critic_optim=critic_optim, tau=tau,
                         gamma=gamma, n_step_return_horizon=n_step_return_horizon)
        self.actor_old = lagged_copy(policy.actor)

    def _lagged(self):
        return super()._lagged() + [(self.actor_old, self.policy.actor)]

    def _nets(self):
        return super()._nets() + [("actor_old.module.", self.actor_old)]

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The n-step walk, the lagged actor and the lagged critic on obs_next[idx_n], the target (ddpg.py:287-339, 397-399)."""
        nxt, w, x_next = self._successors(batch, buffer, indices, agent)
        raw = FlatMLP.forward(self.actor_old, nxt, save=False)
        ops.cac_det_action(raw, self.actor_old.max_action, out=x_next, col0=nxt.shape[1])
        q = FlatMLP.forward(self.critic_old, x_next, save=False)
        batch.returns = ops.cac_target(q, None, batch.mc, batch.gpow, batch.vmask)
        return batch

    def _update_with_batch(self, batch: Batch) -> DDPGTrainingStats:
        """The critic's step, the actor's step against the stepped critic (quirk Q44), the Polyak moves; both losses land in
        one pinned slot, read after the one synchronisation."""
        obs, act, B, w, x, returns, weight = self._begin_update(batch)
        ch = self._critic_step(w, x, lambda q1, q2: ops.cac_critic_head(q1, q2, returns, weight), twin=False)
        batch.weight = ch["prio"]  # prio-buffer
        ap = self._det_actor_step(w, obs, act, B)
        slot = result_slot(w, 2, 2)
        h = slot["h"]
        ops.qmix_finalize(ch["partial"], B, h[0])
        ops.qmix_finalize(ap, B, h[1])
        self._polyak()
        slot["event"].record()
        slot["event"].synchronize()
        return DDPGTrainingStats(actor_loss=float(h[1, 0]), critic_loss=float(h[0, 0]))


class TD3(ContinuousActionRows, ActorDualCriticsOffPolicyAlgorithm):
    """td3.py:105-226."""

    _policy_cls = ContinuousDeterministicPolicy

    def __init__(self, *, policy: ContinuousDeterministicPolicy, policy_optim: AdamOptimizerFactory, critic: ContinuousCritic,
                 critic_optim: AdamOptimizerFactory, critic2: ContinuousCritic | None = None,
                 critic2_optim: AdamOptimizerFactory | None = None, tau: float = 0.005, gamma: float = 0.99,
                 policy_noise: float = 0.2, update_actor_freq: int = 2, noise_clip: float = 0.5,
                 n_step_return_horizon: int = 1) -> None:
        super().__init__(policy=policy, policy_optim=policy_optim, critic=critic, critic_optim=critic_optim, critic2=critic2,
                         critic2_optim=critic2_optim, tau=tau, gamma=gamma, n_step_return_horizon=n_step_return_horizon)
        self.actor_old = lagged_copy(policy.actor)
        self.policy_noise, self.update_actor_freq, self.noise_clip = policy_noise, update_actor_freq, noise_clip
        self._cnt = 0
        self._last = 0

    def _lagged(self):
        return super()._lagged() + [(self.actor_old, self.policy.actor)]

    def _nets(self):
        return super()._nets() + [("actor_old.module.", self.actor_old)]

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The n-step walk, the lagged actor with the smoothing noise (not clamped to the bounds, quirk Q46), the minimum of
        the lagged critics (td3.py:190-202, 94-102)."""
        nxt, w, x_next = self._successors(batch, buffer, indices, agent)
        raw = FlatMLP.forward(self.actor_old, nxt, save=False)
        ops.cac_det_action(raw, self.actor_old.max_action, z=self._normal(nxt.shape[0]), policy_noise=self.policy_noise,
                           noise_clip=self.noise_clip, out=x_next, col0=nxt.shape[1])
        batch.returns = self._twin_target(batch, x_next)
        return batch

    def _update_with_batch(self, batch: Batch) -> TD3TrainingStats:
        """Both critics' steps; on calls 0, f, 2f, ... the actor's step against the stepped critic and the Polyak moves
        (quirk Q45)."""
        obs, act, B, w, x, returns, weight = self._begin_update(batch)
        ch = self._critic_step(w, x, lambda q1, q2: ops.cac_critic_head(q1, q2, returns, weight), twin=True)
        batch.weight = ch["prio"]  # prio-buffer
        slot = result_slot(w, 2, 2)
        h = slot["h"]
        ops.qmix_finalize(ch["partial"], B, h[0])
        stepped = self._cnt % self.update_actor_freq == 0
        if stepped:
            ops.qmix_finalize(self._det_actor_step(w, obs, act, B), B, h[1])
            self._polyak()
        self._cnt += 1
        slot["event"].record()
        slot["event"].synchronize()
        if stepped:
            self._last = float(h[1, 0])
        return TD3TrainingStats(actor_loss=self._last, critic1_loss=float(h[0, 0]), critic2_loss=float(h[0, 1]))

    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = super().state_dict()
        sd.update(_cnt=self._cnt, _last=self._last)
        return sd

    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        super().load_state_dict(sd)
        self._cnt, self._last = int(sd["_cnt"]), sd["_last"]


class SAC(EntropyCoefficient, ContinuousActionRows, ActorDualCriticsOffPolicyAlgorithm):
    """sac.py:212-336."""

    _policy_cls = SACPolicy

    def __init__(self, *, policy: SACPolicy, policy_optim: AdamOptimizerFactory, critic: ContinuousCritic,
                 critic_optim: AdamOptimizerFactory, critic2: ContinuousCritic | None = None,
                 critic2_optim: AdamOptimizerFactory | None = None, tau: float = 0.005, gamma: float = 0.99,
                 alpha: float | Alpha = 0.2, n_step_return_horizon: int = 1, deterministic_eval: bool = True) -> None:
        super().__init__(policy=policy, policy_optim=policy_optim, critic=critic, critic_optim=critic_optim, critic2=critic2,
                         critic2_optim=critic2_optim, tau=tau, gamma=gamma, n_step_return_horizon=n_step_return_horizon)
        self.deterministic_eval = deterministic_eval
        self._init_alpha(alpha)

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The n-step walk, a sample of the ONLINE actor on obs_next[idx_n] (quirk Q47), the soft target (sac.py:298-302)."""
        nxt, w, x_next = self._successors(batch, buffer, indices, agent)
        actor = self.policy.actor
        raw = FlatMLP.forward(actor, nxt, save=False)
        _, logp = ops.sac_action(raw, self._normal(nxt.shape[0]), actor.max_action, actor.unbounded,
                                 sigma_param=actor.sigma_param, out=x_next, col0=nxt.shape[1])
        batch.returns = self._twin_target(batch, x_next, logp, self.alpha.device_scalar(self.device))
        return batch

    def _update_with_batch(self, batch: Batch) -> SACTrainingStats:
        """Both critics' steps, the actor's step against the stepped critics, the alpha step from the entropy of before the
        actor moved (quirk Q50), the Polyak moves; every statistic lands in one pinned slot."""
        obs, act, B, w, x, returns, weight = self._begin_update(batch)
        D, Ad = obs.shape[1], self.policy.act_dim
        alpha_dev = self.alpha.device_scalar(self.device)
        ch = self._critic_step(w, x, lambda q1, q2: ops.cac_critic_head(q1, q2, returns, weight), twin=True)
        batch.weight = ch["prio"]  # prio-buffer

        def critics(x_pi):   # each critic's value at the sampled action, then its gradient to the action columns
            q1a = FlatMLP.forward(self.critic, x_pi, save=True)
            g1 = self.critic.input_grad(w["ones"], D, Ad)
            q2a = FlatMLP.forward(self.critic2, x_pi, save=True)
            return q1a, q2a, g1, self.critic2.input_grad(w["ones"], D, Ad)

        ah = self._sac_actor_step(w, obs, act, B, critics, alpha_dev)   # sac.py:315-322
        slot = result_slot(w, 3, 2)
        h = slot["h"]   # {critic1_loss, critic2_loss}, {actor_loss, mean entropy}, {alpha_loss, alpha}
        ops.qmix_finalize(ch["partial"], B, h[0])
        ops.qmix_finalize(ah["partial"], B, h[1])
        self._alpha_step(ah["partial"], B, h[2])   # alpha.update(entropy) (:325-326), from before the actor's step
        self._polyak()
        slot["event"].record()
        slot["event"].synchronize()
        return SACTrainingStats(actor_loss=float(h[1, 0]), critic1_loss=float(h[0, 0]), critic2_loss=float(h[0, 1]),
                                **self._alpha_stats(h[2]))
