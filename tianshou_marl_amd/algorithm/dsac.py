"""Discrete SAC (soft actor, twin critics with Polyak-lagged copies, fixed or auto-tuned entropy coefficient) on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelfree/discrete_sac.py (`DiscreteSACPolicy` :31-80, `DiscreteSAC` :83-196),
of sac.py's `Alpha` / `FixedAlpha` / `AutoAlpha` (:134-209) and of the bases it stands on (td3.py:32-102, ddpg.py:196-339).
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

from abc import ABC, abstractmethod
from collections import OrderedDict
from dataclasses import dataclass
from typing import Any, Union

import torch
from torch import nn

from .. import ops
from ..data.batch import Batch
from ..data.stats import TrainingStats
from ..utils.learner import act_result, result_slot, sample_counter, slab_workspace
from ..utils.net import FlatMLP, lagged_copy, ref_layer_keys
from ..utils.tensor import to_tensor
from .dqn import DeviceOffPolicyRows, _obs_rows
from .optim import AdamOptimizerFactory, flat_adam_of

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


# ---- the entropy coefficient (sac.py:134-209) ---------------------------------------------------------------------------
class Alpha(ABC):
    """sac.py:134-159.  Beside the reference's interface both kinds hand out `device_scalar(device)`: alpha as f32 [1] in HBM,
    which the kernels read, so that a changing alpha needs no host round trip."""

    @staticmethod
    def from_float_or_instance(alpha: Union[float, "Alpha"]) -> "Alpha":
        if isinstance(alpha, float):
            return FixedAlpha(alpha)
        elif isinstance(alpha, Alpha):
            return alpha
        else:
            raise ValueError(f"Expected float or Alpha instance, but got {alpha=}")

    @property
    @abstractmethod
    def value(self) -> float:
        """The current alpha as a host float (a device read for `AutoAlpha`: only when asked)."""

    @abstractmethod
    def update(self, entropy: torch.Tensor) -> float | None:
        """sac.py:151-159: the loss value if alpha is auto-tuned, otherwise None."""

    @abstractmethod
    def device_scalar(self, device) -> torch.Tensor:
        """alpha as f32 [1] on `device`."""


class FixedAlpha(Alpha):
    """sac.py:162-173."""

    def __init__(self, alpha: float):
        self._value = alpha
        self._dev: torch.Tensor | None = None

    @property
    def value(self) -> float:
        return self._value

    def update(self, entropy: torch.Tensor) -> float | None:
        return None

    def device_scalar(self, device) -> torch.Tensor:
        if self._dev is None or self._dev.device != torch.device(device):
            self._dev = torch.full((1,), float(self._value), dtype=torch.float32, device=device)
        return self._dev


class AutoAlpha(nn.Module, Alpha):
    """sac.py:176-209 with `log_alpha`, its Adam moments and step count in HBM; `tsm_dsac_alpha_step` is the update.  The
    scalars are created on the host and follow the learner's networks (`DiscreteSAC` moves them)."""

    def __init__(self, target_entropy: float, log_alpha: float, optim: AdamOptimizerFactory):
        super().__init__()
        if not isinstance(optim, AdamOptimizerFactory):
            raise TypeError(f"AutoAlpha: optim must be an AdamOptimizerFactory (the step is the HIP Adam), got {type(optim).__name__}")
        if optim.lr_scheduler_factory is not None:
            raise ValueError(f"Learning rate schedulers are not supported by {self.__class__.__name__}")
        self._target_entropy = target_entropy
        self._log_alpha = nn.Parameter(torch.tensor(log_alpha, dtype=torch.float32), requires_grad=False)
        self._adam = optim.adam_kwargs()
        for name, t in (("_exp_avg", torch.zeros(1)), ("_exp_avg_sq", torch.zeros(1)), ("_step", torch.zeros(1, dtype=torch.int64)),
                        ("_alpha_dev", torch.tensor([log_alpha], dtype=torch.float32).exp())):
            self.register_buffer(name, t, persistent=False)

    @property
    def value(self) -> float:
        return self._log_alpha.detach().exp().item()

    def device_scalar(self, device) -> torch.Tensor:
        if self._alpha_dev.device != torch.device(device):
            self.to(device)
        return self._alpha_dev

    def step_device(self, entropy_partial: torch.Tensor, B: int, out: torch.Tensor) -> None:
        """One Adam step on log_alpha from `ops.dsac_actor_head`'s f64 partials over B rows; out f32 [2] (HBM or pinned) <-
        {alpha_loss, the new alpha}.  No host read."""
        kw = self._adam
        ops.dsac_alpha_step(entropy_partial, B, self._log_alpha.data, self._exp_avg, self._exp_avg_sq, self._step,
                            self._target_entropy, self._alpha_dev, out, lr=kw["lr"], betas=kw["betas"], eps=kw["adam_eps"],
                            weight_decay=kw["weight_decay"])

    def update(self, entropy: torch.Tensor) -> float:
        """sac.py:203-209 for entropies f32 [B] in HBM (`ops.dsac_actor_head`'s): they are laid out as one f64 partial pair
        per row, which the kernel sums in a fixed order.  Returns alpha_loss: one host read.  The learner does not come
        this way: it hands the actor head's partials to `step_device`."""
        if not entropy.is_cuda:
            raise RuntimeError("AutoAlpha.update needs device (HIP) tensors; there is no CPU path")
        h = entropy.reshape(-1).double()
        out = torch.empty(2, dtype=torch.float32, device=entropy.device)
        self.device_scalar(entropy.device)
        self.step_device(torch.stack([torch.zeros_like(h), h], 1).contiguous(), h.numel(), out)
        return float(out[0])

    def adam_state(self) -> dict:
        """The Adam moments and step count of log_alpha, and alpha as the kernels last left it."""
        return dict(exp_avg=self._exp_avg.detach().cpu().clone(), exp_avg_sq=self._exp_avg_sq.detach().cpu().clone(),
                    step=int(self._step.item()), alpha=self._alpha_dev.detach().cpu().clone())

    @torch.no_grad()
    def load_adam_state(self, sd: dict) -> None:
        self._exp_avg.copy_(sd["exp_avg"])
        self._exp_avg_sq.copy_(sd["exp_avg_sq"])
        self._step.fill_(int(sd["step"]))
        if sd.get("alpha") is not None:
            self._alpha_dev.copy_(sd["alpha"])

    @torch.no_grad()
    def set_log_alpha(self, log_alpha) -> None:
        self._log_alpha.data.copy_(torch.as_tensor(log_alpha, dtype=torch.float32).reshape(()))
        self._alpha_dev.copy_(self._log_alpha.data.exp().reshape(1))


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
class _Schedulers:
    def __init__(self, scheds: list) -> None:
        self.scheds = scheds

    def step(self) -> None:
        for s in self.scheds:
            s.step()


class DiscreteSAC(DeviceOffPolicyRows, nn.Module):
    """discrete_sac.py:83-196 on the device buffer.  Every `*_optim` is an `AdamOptimizerFactory` (its hyper-parameters drive
    the HIP Adam over that network's flat vector)."""

    def __init__(self, *, policy: DiscreteSACPolicy, policy_optim: AdamOptimizerFactory, critic: FlatMLP,
                 critic_optim: AdamOptimizerFactory, critic2: FlatMLP | None = None,
                 critic2_optim: AdamOptimizerFactory | None = None, tau: float = 0.005, gamma: float = 0.99,
                 alpha: float | Alpha = 0.2, n_step_return_horizon: int = 1) -> None:
        super().__init__()
        if not isinstance(policy, DiscreteSACPolicy):
            raise TypeError(f"DiscreteSAC needs a DiscreteSACPolicy, got {type(policy).__name__}")
        assert 0.0 <= tau <= 1.0, f"tau should be in [0, 1] but got: {tau}"
        assert 0.0 <= gamma <= 1.0, f"gamma should be in [0, 1] but got: {gamma}"
        assert n_step_return_horizon > 0, f"n_step_return_horizon should be greater than 0 but got: {n_step_return_horizon}"
        ops.dsac_check(policy.n_act, int(n_step_return_horizon))
        actor = policy.actor
        dev = actor.flat.device
        for name, net in (("critic", critic), ("critic2", critic2)):
            if net is None and name == "critic2":
                continue
            if not isinstance(net, FlatMLP):
                raise TypeError(f"DiscreteSAC: {name} must be a FlatMLP obs -> n_act (got {type(net).__name__})")
            if net.dims[0] != actor.dims[0] or net.dims[-1] != policy.n_act or net.flat.device != dev:
                raise ValueError(f"DiscreteSAC: {name} maps {net.dims[0]} -> {net.dims[-1]} on {net.flat.device}; the actor maps "
                                 f"{actor.dims[0]} -> {policy.n_act} on {dev}")
        self.policy = policy
        self.critic = critic
        # critic2 or deepcopy(critic) (td3.py:90): the same weights in storage of its own, made as the lagged copies are
        self.critic2 = critic2 if critic2 is not None else lagged_copy(critic)
        self.critic_old = lagged_copy(self.critic)
        self.critic2_old = lagged_copy(self.critic2)
        adams = [flat_adam_of(given, net, f"DiscreteSAC: {name}", True, ("factory",)) for name, net, given in (
            ("policy_optim", actor, policy_optim), ("critic_optim", self.critic, critic_optim),
            ("critic2_optim", self.critic2, critic2_optim or critic_optim))]
        (self.policy_optim, self.critic_optim, self.critic2_optim), scheds = zip(*adams)
        scheds = [s for s in scheds if s is not None]
        self.lr_scheduler = _Schedulers(scheds) if scheds else None
        self.tau, self.gamma = tau, gamma
        self.n_step = self.n_step_return_horizon = int(n_step_return_horizon)
        self.alpha = Alpha.from_float_or_instance(alpha)
        self.alpha.device_scalar(dev)
        self._ws: dict = {}

    @property
    def device(self) -> torch.device:
        return self.policy.device

    @property
    def is_within_training_step(self) -> bool:
        return self.policy.is_within_training_step

    @is_within_training_step.setter
    def is_within_training_step(self, v: bool) -> None:
        self.policy.is_within_training_step = bool(v)

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
        actor, alpha = self.policy.actor, self.alpha
        x = to_tensor(obs, dev, torch.float32).reshape(-1, actor.dims[0])
        B = x.shape[0]
        act = to_tensor(batch.act, dev, torch.int64).reshape(-1)
        returns = to_tensor(batch.returns, dev, torch.float32).reshape(-1)
        w = slab_workspace(self._ws, B, dev, slabs_a=actor.flat.numel(), slabs_c1=self.critic.flat.numel(),
                           slabs_c2=self.critic2.flat.numel())
        alpha_dev = alpha.device_scalar(dev)
        # critics (discrete_sac.py:162-174)
        q1 = FlatMLP.forward(self.critic, x, save=True)
        q2 = FlatMLP.forward(self.critic2, x, save=True)
        ch = ops.dsac_critic_head(q1, q2, act, returns, None if weight is None else to_tensor(weight, dev, torch.float32).reshape(-1))
        self.critic.backward(ch["dq1"], w["n_split"], slabs=w["slabs_c1"])
        self.critic_optim.step(w["slabs_c1"])
        self.critic2.backward(ch["dq2"], w["n_split"], slabs=w["slabs_c2"])
        self.critic2_optim.step(w["slabs_c2"])
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
        auto = isinstance(alpha, AutoAlpha)
        ops.qmix_finalize(ah["partial"], B, h[1])
        if auto:   # alpha.update(entropy.detach()) (:186), from the entropy partials of before the actor's step
            alpha.step_device(ah["partial"], B, h[2])
        # self._update_lagged_network_weights() (:188)
        ops.polyak(self.critic_old.flat.data, self.critic.flat.data, self.tau)
        ops.polyak(self.critic2_old.flat.data, self.critic2.flat.data, self.tau)
        slot["event"].record()
        slot["event"].synchronize()
        return DiscreteSACTrainingStats(actor_loss=float(h[1, 0]), critic1_loss=float(h[0, 0]), critic2_loss=float(h[0, 1]),
                                        alpha=float(h[2, 1]) if auto else alpha.value,
                                        alpha_loss=float(h[2, 0]) if auto else None)

    # ---- checkpoints ---------------------------------------------------------------------------------------------
    def _nets(self) -> list[tuple[str, FlatMLP]]:
        return [("policy.actor.", self.policy.actor), ("critic.", self.critic), ("critic_old.module.", self.critic_old),
                ("critic2.", self.critic2), ("critic2_old.module.", self.critic2_old)]

    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = OrderedDict((name.rstrip("."), net.flat.data.detach().clone().cpu()) for name, net in self._nets())
        sd.update(policy_optim=self.policy_optim.state_dict(), critic_optim=self.critic_optim.state_dict(),
                  critic2_optim=self.critic2_optim.state_dict())
        if isinstance(self.alpha, AutoAlpha):
            sd["alpha"] = dict(log_alpha=self.alpha._log_alpha.detach().clone().cpu(), **self.alpha.adam_state())
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        for name, net in self._nets():
            net.flat.data.copy_(sd[name.rstrip(".")])
        self.policy_optim.load_state_dict(sd["policy_optim"])
        self.critic_optim.load_state_dict(sd["critic_optim"])
        self.critic2_optim.load_state_dict(sd["critic2_optim"])
        if isinstance(self.alpha, AutoAlpha):
            self.alpha.set_log_alpha(sd["alpha"]["log_alpha"])
            self.alpha.load_adam_state(sd["alpha"])

    def to_reference_state_dict(self) -> OrderedDict:
        """The module state_dict of the reference's DiscreteSAC: `policy.actor.*`, `critic.*`, `critic_old.module.*`,
        `critic2.*`, `critic2_old.module.*` (lagged_network.py wraps the copies in an EvalModeModuleWrapper), and
        `alpha._log_alpha` when alpha is auto-tuned.  Every net is a `DiscreteActor` / `DiscreteCritic` around a
        `Net(hidden_sizes=[...])` (`ref_layer_keys`: "head")."""
        sd = OrderedDict()
        for prefix, net in self._nets():
            net.export_layers(ref_layer_keys(net.n_layers, "head"), prefix, sd)
        if isinstance(self.alpha, AutoAlpha):
            sd["alpha._log_alpha"] = self.alpha._log_alpha.detach().clone().cpu()
        return sd

    @torch.no_grad()
    def load_reference_state_dict(self, sd) -> None:
        for prefix, net in self._nets():
            net.import_layers(sd, ref_layer_keys(net.n_layers, "head"), prefix)
        if isinstance(self.alpha, AutoAlpha):
            self.alpha.set_log_alpha(sd["alpha._log_alpha"])
