"""Discrete SAC (soft actor, twin critics with Polyak-lagged copies, fixed or auto-tuned entropy coefficient) on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelfree/discrete_sac.py (`DiscreteSACPolicy` :31-80, `DiscreteSAC` :83-196).
As in the reference the learner is an `ActorDualCriticsOffPolicyAlgorithm` (actor_critic.py: the nets, their Adams, lagged copies,
schedulers and checkpoints) with an entropy coefficient (`Alpha` / `FixedAlpha` / `AutoAlpha`, importable from here as before).
The actor and both critics are `FlatMLP`s obs -> n actions (csrc/dense.hip); the n-step walk is `tsm_nstep_return`; what lies
between the forwards and the optimisers' steps is one launch each (csrc/dsac.hip): `tsm_dsac_target`, `tsm_dsac_critic_head`,
`tsm_dsac_actor_head`, `tsm_dsac_alpha_step`.  The lagged critics move with `tsm_polyak`.  There is no autograd fallback.

Kept quirks: Q24 -- the critics' td is q - returns, the opposite of DQN's sign, and `batch.weight`
leaves as (td1 + td2) / 2; Q25 -- the actor loss reads both critics AFTER their own steps of the same call; Q26 -- alpha is
stepped from the entropy computed before the actor moved, and the actor loss used the alpha from before that step; Q27 --
the reference samples an action in `policy(batch)` that neither the target nor the update reads: it only advances torch's
RNG, and nothing is drawn here; Q28 -- action masks are not part of the reference's Discrete SAC and are refused here.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import torch
from torch import nn

from .. import ops
from ..data.batch import Batch
from ..data.stats import TrainingStats
from ..utils.learner import act_result, result_slot, sample_counter, slab_workspace
from ..utils.net import FlatMLP, ref_layer_keys
from ..utils.tensor import to_tensor
from .actor_critic import ActorDualCriticsOffPolicyAlgorithm, EntropyCoefficient
from .actor_critic import Alpha, AutoAlpha, FixedAlpha  # noqa: F401  (public names of this module, as before)
from .dqn import _obs_rows
from .optim import AdamOptimizerFactory

_NO_MASK = ("action masks are not part of the reference's Discrete SAC (discrete_sac.py builds Categorical(logits) from the "
            "actor's raw output): {what} carries a mask, which would be ignored")


@dataclass(kw_only=True)
class DiscreteSACTrainingStats(TrainingStats):
    """sac.py `SACTrainingStats` / discrete_sac.py `DiscreteSACTrainingStats`."""
    actor_loss: float
    critic1_loss: float
    critic2_loss: float
    alpha: float | None = None
    alpha_loss: float | None = None


# ---- the policy (discrete_sac.py:31-80) ---------------------------------------------------------------------------------
class DiscreteSACPolicy(nn.Module):
    """discrete_sac.py:31-80 with a `FlatMLP` actor (obs -> ... -> n action logits).  Samples come from the project's Philox
    stream (`tsm_categorical_sample`, keyed by `seed`), not from torch's generator."""

    def __init__(self, *, actor: FlatMLP, deterministic_eval: bool = True, action_space: Any, observation_space: Any = None,
                 seed: int = 0) -> None:
        super().__init__()
        if not isinstance(actor, FlatMLP):
            raise TypeError("DiscreteSACPolicy needs a FlatMLP actor: the update runs in HIP, there is no autograd fallback "
                            f"(got {type(actor).__name__})")
        n = getattr(action_space, "n", None)
        if n is None or int(n) != actor.dims[-1]:
            raise ValueError(f"DiscreteSACPolicy: the actor has {actor.dims[-1]} outputs, the action space "
                             f"{'no size' if n is None else f'{int(n)} actions'}")
        ops.dsac_check(int(n))
        self.actor = actor
        self.deterministic_eval = deterministic_eval
        self.action_space, self.observation_space = action_space, observation_space
        self.n_act = int(n)
        self.seed = int(seed)
        self._sample_ctr = 0
        self.is_within_training_step = False

    @property
    def device(self) -> torch.device:
        return self.actor.flat.device

    @property
    def _deterministic(self) -> bool:
        return bool(self.deterministic_eval and not self.is_within_training_step)

    def forward(self, batch: Batch, state: Any = None, **kwargs: Any) -> Batch:
        """-> Batch(logits [B, A] in HBM, act (numpy i64): the mode when `deterministic_eval` outside a training step, else a
        Philox sample, state).  The reference's `dist` field is not carried."""
        obs, mask = _obs_rows(batch.obs)
        if mask is not None:
            raise NotImplementedError(_NO_MASK.format(what="batch.obs"))
        x = to_tensor(obs, self.device, torch.float32)
        logits = FlatMLP.forward(self.actor, x.reshape(-1, self.actor.dims[0]), save=False)
        act, _ = ops.categorical_sample(logits, self.seed, offset=self._sample_ctr, deterministic=self._deterministic,
                                        want_logp=False)
        self._sample_ctr += logits.shape[0]   # as `act_device`: a row takes its counter whether or not it draws
        return Batch(logits=logits, act=act.to(torch.int64).cpu().numpy(), state=state)

    def add_exploration_noise(self, act, batch):
        """Policy.add_exploration_noise (algorithm_base.py): the exploration is the sampling itself."""
        return act

    def act_device(self, obs: torch.Tensor, out: dict | None = None, offset_dev: torch.Tensor | None = None,
                   row_offset: int = 0, mask: torch.Tensor | None = None) -> dict:
        """obs [..., D] in HBM -> act i32 [rows] (the actor, then tsm_categorical_sample: a draw within a training step or
        without `deterministic_eval`, else the mode), logp of that action, value = 0.  The Philox counter is offset_dev (the
        env's device tick: captured graphs advance it) or the policy's own."""
        if mask is not None:
            raise NotImplementedError(_NO_MASK.format(what="act_device"))
        rows = obs.reshape(-1, self.actor.dims[0])
        logits = FlatMLP.forward(self.actor, rows, save=False)
        act, logp = ops.categorical_sample(logits, self.seed, offset=sample_counter(self, rows.shape[0], row_offset, offset_dev),
                                           deterministic=self._deterministic, offset_dev=offset_dev,
                                           out=None if out is None else (out["act"].view(-1), out["logp"].view(-1)))
        return act_result(out, act, logp, logits=logits)


# ---- the learner (discrete_sac.py:83-196) -------------------------------------------------------------------------------
class DiscreteSAC(EntropyCoefficient, ActorDualCriticsOffPolicyAlgorithm):
    """discrete_sac.py:83-196 on the device buffer.  Every `*_optim` is an `AdamOptimizerFactory` (its hyper-parameters drive
    the HIP Adam over that network's flat vector)."""

    _policy_cls = DiscreteSACPolicy

    def __init__(self, *, policy: DiscreteSACPolicy, policy_optim: AdamOptimizerFactory, critic: FlatMLP,
                 critic_optim: AdamOptimizerFactory, critic2: FlatMLP | None = None,
                 critic2_optim: AdamOptimizerFactory | None = None, tau: float = 0.005, gamma: float = 0.99,
                 alpha: float | Alpha = 0.2, n_step_return_horizon: int = 1) -> None:
        super().__init__(policy=policy, policy_optim=policy_optim, critic=critic, critic_optim=critic_optim, critic2=critic2,
                         critic2_optim=critic2_optim, tau=tau, gamma=gamma, n_step_return_horizon=n_step_return_horizon)
        self._init_alpha(alpha)

    def _check_bounds(self, policy, n_step: int) -> None:
        ops.dsac_check(policy.n_act, n_step)

    def _check_critic(self, name: str, net) -> None:
        actor, n_act = self.policy.actor, self.policy.n_act
        dev = actor.flat.device
        if not isinstance(net, FlatMLP):
            raise TypeError(f"DiscreteSAC: {name} must be a FlatMLP obs -> n_act (got {type(net).__name__})")
        if net.dims[0] != actor.dims[0] or net.dims[-1] != n_act or net.flat.device != dev:
            raise ValueError(f"DiscreteSAC: {name} maps {net.dims[0]} -> {net.dims[-1]} on {net.flat.device}; the actor maps "
                             f"{actor.dims[0]} -> {n_act} on {dev}")

    # every net is a `DiscreteActor` / `DiscreteCritic` around a `Net(hidden_sizes=[...])` (`ref_layer_keys`: "head")
    @staticmethod
    def _ref_views(net) -> list:
        return net.named_layers(ref_layer_keys(net.n_layers, "head"))

    # ---- ActorCriticOffPolicyAlgorithm._preprocess_batch (ddpg.py:287-339) with discrete_sac.py:147-155 -----------------
    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The n-step walk, the online actor and both lagged critics on obs_next[idx_n], the soft target: the batch leaves
        with `returns` (quirk Q27: no action is sampled on the way)."""
        _, idx_n, col = self._nstep_rows(batch, buffer, indices, agent)
        nxt, mask_next = self._successor_rows(buffer, idx_n, col)
        if mask_next is not None:
            raise NotImplementedError(_NO_MASK.format(what="the buffer"))
        logits_next = FlatMLP.forward(self.policy.actor, nxt, save=False)
        q1_next = FlatMLP.forward(self.critic_old, nxt, save=False)
        q2_next = FlatMLP.forward(self.critic2_old, nxt, save=False)
        batch.returns = ops.dsac_target(logits_next, q1_next, q2_next, self.alpha.device_scalar(self.device), batch.mc,
                                        batch.gpow, batch.vmask)
        return batch

    # ---- DiscreteSAC._update_with_batch (discrete_sac.py:157-196) ---------------------------------------------------------
    def _update_with_batch(self, batch: Batch) -> DiscreteSACTrainingStats:
        """Both critics' steps, the actor's step against the updated critics (quirk Q25), the alpha step (Q26), the Polyak
        move of the lagged critics; every statistic lands in one pinned slot, read after the one synchronisation."""
        dev = self.device
        weight = self._pop_weight(batch)
        obs, mask = _obs_rows(batch.obs)
        if mask is not None:
            raise NotImplementedError(_NO_MASK.format(what="batch.obs"))
        actor = self.policy.actor
        x = to_tensor(obs, dev, torch.float32).reshape(-1, actor.dims[0])
        B = x.shape[0]
        act = to_tensor(batch.act, dev, torch.int64).reshape(-1)
        returns = to_tensor(batch.returns, dev, torch.float32).reshape(-1)
        w = slab_workspace(self._ws, B, dev, **self._slab_widths())
        alpha_dev = self.alpha.device_scalar(dev)
        # critics (discrete_sac.py:162-174)
        ch = self._critic_step(w, x, lambda q1, q2: ops.dsac_critic_head(
            q1, q2, act, returns, None if weight is None else to_tensor(weight, dev, torch.float32).reshape(-1)), twin=True)
        batch.weight = ch["prio"]  # prio-buffer
        # actor (:177-184)
        logits = FlatMLP.forward(actor, x, save=True)
        q1a = FlatMLP.forward(self.critic, x, save=False)
        q2a = FlatMLP.forward(self.critic2, x, save=False)
        ah = ops.dsac_actor_head(logits, q1a, q2a, alpha_dev)
        actor.backward(ah["d_logits"], w["n_split"], slabs=w["slabs_a"])
        self.policy_optim.step(w["slabs_a"])
        slot = result_slot(w, 3, 2)
        h = slot["h"]   # {critic1_loss, critic2_loss}, {actor_loss, mean entropy}, {alpha_loss, alpha}
        ops.qmix_finalize(ch["partial"], B, h[0])
        ops.qmix_finalize(ah["partial"], B, h[1])
        self._alpha_step(ah["partial"], B, h[2])   # alpha.update(entropy.detach()) (:186), from before the actor's step
        self._polyak()   # self._update_lagged_network_weights() (:188)
        slot["event"].record()
        slot["event"].synchronize()
        return DiscreteSACTrainingStats(actor_loss=float(h[1, 0]), critic1_loss=float(h[0, 0]), critic2_loss=float(h[0, 1]),
                                        **self._alpha_stats(h[2]))
