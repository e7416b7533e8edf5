"""REDQ (arXiv 2101.05982): the randomized-ensemble off-policy actor-critic for `Box` actions on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelfree/redq.py (`REDQPolicy` :37-131, `REDQ` :134-304) on cac.py's and
actor_critic.py's plumbing: `SACPolicy._sample` for the Gaussian-tanh action, `ContinuousActionRows` for the rows [obs | act], the
n-step walk, workspaces and the SAC-style actor step, `ActorCriticOffPolicyAlgorithm` for the Adams, checkpoints and schedulers,
`EntropyCoefficient` for alpha.  The critic is an `EnsembleCritic` (utils/net.py):
ONE flat vector, one grouped launch per layer and role for all E members (csrc/ensemble.hip); the subset target, the ensemble's
squared loss and the ensemble mean are one launch each in csrc/redq.hip; the actor's head is `tsm_sac_actor_head` fed the
ensemble's mean Q and its input gradient with d_out = 1 / E.  There is no autograd fallback.

Kept quirks: Q51 -- the subset is ONE np.random.choice(E, M, replace=False) on numpy's global RNG per target
computation, shared by the whole batch; Q52 -- the target samples from the ONLINE actor (ddpg.py:304-312, as Q47); Q53 -- the
actor steps when critic_gradient_step % actor_delay == 0 AFTER the increment, so call `actor_delay` is the first one (TD3, Q45,
steps on call 0); before that `actor_loss` reports 0.0, alpha is stepped on actor calls only and `alpha_loss` is None otherwise;
Q54 -- Polyak moves critic_old on every call, there is no actor_old; Q55 -- `REDQPolicy`'s default action_bound_method is "clip"
(`SACPolicy` passes None); Q56 -- batch.weight is the SIGNED ensemble mean of td.  The log-prob epsilon is Q49's.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Literal

import numpy as np
import torch

from .. import ops
from ..data.batch import Batch
from ..utils.learner import result_slot
from ..utils.net import ContinuousActorProbabilistic, EnsembleCritic, FlatMLP
from .actor_critic import ActorCriticOffPolicyAlgorithm, Alpha, EntropyCoefficient
from .cac import ContinuousActionRows, DDPGTrainingStats, SACPolicy, _ContinuousPolicy
from .optim import AdamOptimizerFactory


@dataclass(kw_only=True)
class REDQTrainingStats(DDPGTrainingStats):
    alpha: float | None = None
    alpha_loss: float | None = None


class REDQPolicy(SACPolicy):
    """redq.py:37-131 with a `ContinuousActorProbabilistic`: `SACPolicy`'s sampling and acting, the reference's argument order,
    and "clip" as the default action_bound_method (quirk Q55)."""

    def __init__(self, *, actor: ContinuousActorProbabilistic, exploration_noise: Any | Literal["default"] | None = None,
                 action_space: Any, deterministic_eval: bool = True, action_scaling: bool = True,
                 action_bound_method: Literal["clip"] | None = "clip", observation_space: Any = None, seed: int = 0) -> None:
        _ContinuousPolicy.__init__(self, actor, exploration_noise, action_space, observation_space, action_scaling,
                                   action_bound_method, seed)
        self.deterministic_eval = deterministic_eval


class REDQ(EntropyCoefficient, ContinuousActionRows, ActorCriticOffPolicyAlgorithm):
    """redq.py:134-304.  `subset_source` (None: numpy's global RNG, quirk Q51) stands in for the subset draw as `noise_source`
    stands in for the normal draws: (ensemble_size, subset_size) -> the member indices of this target computation."""

    _policy_cls = REDQPolicy

    def __init__(self, *, policy: REDQPolicy, policy_optim: AdamOptimizerFactory, critic: EnsembleCritic,
                 critic_optim: AdamOptimizerFactory, ensemble_size: int = 10, subset_size: int = 2, tau: float = 0.005,
                 gamma: float = 0.99, alpha: float | Alpha = 0.2, n_step_return_horizon: int = 1, actor_delay: int = 20,
                 deterministic_eval: bool = True, target_mode: Literal["mean", "min"] = "min") -> None:
        if target_mode not in ("min", "mean"):
            raise ValueError(f"Unsupported target_mode: {target_mode}")
        if not 0 < subset_size <= ensemble_size:
            raise ValueError(f"Invalid choice of ensemble size or subset size. Should be 0 < {subset_size=} <= {ensemble_size=}")
        if isinstance(critic, EnsembleCritic) and critic.ensemble_size != ensemble_size:
            raise ValueError(f"REDQ: the critic holds {critic.ensemble_size} members, ensemble_size = {ensemble_size}")
        super().__init__(policy=policy, policy_optim=policy_optim, critic=critic, critic_optim=critic_optim, tau=tau,
                         gamma=gamma, n_step_return_horizon=n_step_return_horizon)
        self.ensemble_size, self.subset_size = int(ensemble_size), int(subset_size)
        self.target_mode = target_mode
        self.critic_gradient_step = 0
        self.actor_delay = actor_delay
        self.deterministic_eval = deterministic_eval
        self._last_actor_loss = 0.0  # only for logging purposes
        self._init_alpha(alpha)
        self.subset_source = None   # (ensemble_size, subset_size) -> member indices: stands in for np.random.choice (tests)

    def _check_critic(self, name: str, net) -> None:
        actor = self.policy.actor
        D, Ad, dev = actor.dims[0], self.policy.act_dim, actor.flat.device
        if not isinstance(net, EnsembleCritic):
            raise TypeError(f"REDQ: {name} must be an EnsembleCritic: the update runs in HIP, there is no autograd fallback "
                            f"(got {type(net).__name__})")
        if net.dims[0] != D + Ad or net.flat.device != dev:
            raise ValueError(f"REDQ: {name} maps {net.dims[0]} -> 1 on {net.flat.device}; it must map {D} + {Ad} -> 1 on {dev}")

    def _work(self, B: int, **slabs: int) -> dict:
        w = super()._work(B, **slabs)
        if "inv_e" not in w:   # d_out of the actor loss's ensemble mean: 1 / E for every member and row
            E = self.ensemble_size
            w["inv_e"] = torch.full((E, B, 1), 1.0 / E, dtype=torch.float32, device=self.device)
        return w

    def _subset(self) -> np.ndarray:
        if self.subset_source is not None:
            return np.asarray(self.subset_source(self.ensemble_size, self.subset_size), np.int64).reshape(-1)
        return np.random.choice(self.ensemble_size, self.subset_size, replace=False)

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The n-step walk, a sample of the ONLINE actor on obs_next[idx_n] (quirk Q52), one subset draw for the whole batch
        (quirk Q51), the subset's min or mean of the lagged ensemble minus alpha logp (redq.py:254-269)."""
        nxt, w, x_next = self._successors(batch, buffer, indices, agent)
        actor = self.policy.actor
        raw = FlatMLP.forward(actor, nxt, save=False)
        _, logp = ops.sac_action(raw, self._normal(nxt.shape[0]), actor.max_action, actor.unbounded,
                                 sigma_param=actor.sigma_param, out=x_next, col0=nxt.shape[1])
        mask = ops.redq_subset_mask(self._subset(), self.ensemble_size)
        q = self.critic_old.forward(x_next, save=False)
        batch.returns = ops.redq_target(q, mask, self.target_mode, batch.mc, batch.gpow, batch.vmask, logp_next=logp,
                                        alpha_dev=self.alpha.device_scalar(self.device))
        return batch

    def _update_with_batch(self, batch: Batch) -> REDQTrainingStats:
        """The ensemble's step; when critic_gradient_step % actor_delay == 0 after the increment (quirk Q53) the actor's step
        against the stepped ensemble's mean and the alpha step; the Polyak move on every call (quirk Q54)."""
        obs, act, B, w, x, returns, weight = self._begin_update(batch)
        D, Ad, E = obs.shape[1], self.policy.act_dim, self.ensemble_size
        q = self.critic.forward(x, save=True)
        ch = ops.redq_critic_head(q, returns, weight)
        self.critic.backward(ch["dq"], w["n_split"], slabs=w["slabs_c1"])
        self.critic_optim.step(w["slabs_c1"])
        batch.weight = ch["prio"]  # prio-buffer
        self.critic_gradient_step += 1
        slot = result_slot(w, 3, 2)
        h = slot["h"]   # {critic_loss, 0}, {actor_loss, mean entropy}, {alpha_loss, alpha}
        ops.qmix_finalize(ch["partial"], E * B, h[0])
        stepped = self.critic_gradient_step % self.actor_delay == 0
        if stepped:   # redq.py:284-295: the ensemble's mean Q and its gradient to the action, d_out = 1 / E for every member
            ah = self._sac_actor_step(w, obs, act, B, lambda x_pi: (
                ops.redq_mean_q(self.critic.forward(x_pi, save=True)), None, self.critic.input_grad(w["inv_e"], D, Ad), None),
                self.alpha.device_scalar(self.device))
            ops.qmix_finalize(ah["partial"], B, h[1])
            self._alpha_step(ah["partial"], B, h[2])   # alpha.update(entropy) (:292-293), from before the actor's step
        self._polyak()
        slot["event"].record()
        slot["event"].synchronize()
        if stepped:
            self._last_actor_loss = float(h[1, 0])
        return REDQTrainingStats(actor_loss=self._last_actor_loss, critic_loss=float(h[0, 0]), **self._alpha_stats(h[2], stepped))

    # ---- checkpoints ---------------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = super().state_dict()
        sd.update(critic_gradient_step=self.critic_gradient_step, _last_actor_loss=self._last_actor_loss)
        if "alpha" in sd:   # the entropy coefficient's entry stays the last one
            sd.move_to_end("alpha")
        return sd

    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        super().load_state_dict(sd)
        self.critic_gradient_step, self._last_actor_loss = int(sd["critic_gradient_step"]), float(sd["_last_actor_loss"])
