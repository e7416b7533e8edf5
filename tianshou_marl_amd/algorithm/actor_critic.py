"""What the off-policy actor-critics share whatever their action space: the entropy coefficient, the learner core, its twin-critic
form and the schedulers' holder.  cac.py (DDPG, TD3, SAC), redq.py and dsac.py (Discrete SAC) stand on it.

Mirror of /root/reference/tianshou/algorithm/modelfree/ddpg.py (`ActorCriticOffPolicyAlgorithm` :196-339), td3.py
(`ActorDualCriticsOffPolicyAlgorithm` :32-102) and sac.py (`Alpha` / `FixedAlpha` / `AutoAlpha` :134-209).  Every network is a flat
parameter vector (utils/net.py) under a HIP Adam of its own; the lagged copies move with `tsm_polyak`, the alpha step is
`tsm_dsac_alpha_step`.  What depends on the action space -- the critic's shape, the bound checks, the rows a critic reads --
is the subclass's: `ContinuousActionRows` (cac.py) for a `Box`, `DiscreteSAC` itself for discrete actions.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from collections import OrderedDict
from typing import Union

import torch
from torch import nn

from .. import ops
from ..utils.net import FlatMLP, export_views, import_views, lagged_copy
from .dqn import DeviceOffPolicyRows
from .optim import AdamOptimizerFactory, flat_adam_of


class _Schedulers:
    def __init__(self, scheds: list) -> None:
        self.scheds = scheds

    def step(self) -> None:
        for s in self.scheds:
            s.step()


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

    def checkpoint(self) -> dict | None:
        """What a learner's checkpoint keeps of alpha; None: nothing to save (a constant comes back with the constructor)."""
        return None

    def load_checkpoint(self, sd: dict | None) -> None:
        """Takes back what `checkpoint` gave; sd None: the learner's checkpoint holds no entry.  A constant reads nothing."""


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
    scalars are created on the host and move to the learner's device the first time it asks for `device_scalar`."""

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

    def checkpoint(self) -> dict:
        return dict(log_alpha=self._log_alpha.detach().clone().cpu(), **self.adam_state())

    def load_checkpoint(self, sd: dict | None) -> None:
        if sd is None:
            raise KeyError("alpha: the checkpoint holds no entry for an auto-tuned alpha")
        self.set_log_alpha(sd["log_alpha"])
        if "exp_avg" in sd:   # the reference's layout carries log_alpha alone
            self.load_adam_state(sd)


class EntropyCoefficient:
    """The alpha of SAC, REDQ and Discrete SAC, in front of the learner core in their bases: its setup, its step from the
    actor head's partials, its two statistics and its entries in both checkpoint layouts."""

    def _init_alpha(self, alpha: float | Alpha) -> None:
        self.alpha = Alpha.from_float_or_instance(alpha)
        self.alpha.device_scalar(self.device)

    def _alpha_step(self, partial: torch.Tensor, B: int, h_row: torch.Tensor) -> None:
        """alpha.update(entropy) from the actor head's partials over B rows; h_row (pinned f32 [2]) <- {alpha_loss, alpha}."""
        if isinstance(self.alpha, AutoAlpha):
            self.alpha.step_device(partial, B, h_row)

    def _alpha_stats(self, h_row: torch.Tensor, stepped: bool = True) -> dict:
        """`alpha` and `alpha_loss` of the statistics, after the slot's synchronisation; `stepped`: `_alpha_step` ran."""
        if stepped and isinstance(self.alpha, AutoAlpha):
            return dict(alpha=float(h_row[1]), alpha_loss=float(h_row[0]))
        return dict(alpha=self.alpha.value, alpha_loss=None)

    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = super().state_dict()
        entry = self.alpha.checkpoint()
        if entry is not None:
            sd["alpha"] = entry
        return sd

    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        super().load_state_dict(sd)
        self.alpha.load_checkpoint(sd.get("alpha"))

    def to_reference_state_dict(self) -> OrderedDict:
        sd = super().to_reference_state_dict()
        entry = self.alpha.checkpoint()
        if entry is not None:
            sd["alpha._log_alpha"] = entry["log_alpha"]
        return sd

    def load_reference_state_dict(self, sd) -> None:
        super().load_reference_state_dict(sd)
        log_alpha = sd.get("alpha._log_alpha")
        self.alpha.load_checkpoint(None if log_alpha is None else dict(log_alpha=log_alpha))


# ---- the learner core (ddpg.py:196-339, td3.py:32-102) ------------------------------------------------------------------
class ActorCriticOffPolicyAlgorithm(DeviceOffPolicyRows, nn.Module):
    """ddpg.py:196-339 on the device buffer: policy, critic, lagged critic, their Adams, the critic step, the Polyak moves and
    the checkpoints.  Every `*_optim` is an `AdamOptimizerFactory` (its hyper-parameters drive the HIP Adam over that network's
    flat vector).  A subclass says what its action space asks: `_policy_cls`; `_check_bounds(policy, n_step)`, which raises beyond
    the kernels' limits; `_check_critic(name, net)`, which raises unless `net` is a critic of the kind, shape and device it needs."""

    _policy_cls: type = nn.Module

    def __init__(self, *, policy, policy_optim: AdamOptimizerFactory, critic, critic_optim: AdamOptimizerFactory,
                 tau: float = 0.005, gamma: float = 0.99, n_step_return_horizon: int = 1) -> None:
        super().__init__()
        name = type(self).__name__
        if not isinstance(policy, self._policy_cls):
            raise TypeError(f"{name} needs a {self._policy_cls.__name__}, got {type(policy).__name__}")
        assert 0.0 <= tau <= 1.0, f"tau should be in [0, 1] but got: {tau}"
        assert 0.0 <= gamma <= 1.0, f"gamma should be in [0, 1] but got: {gamma}"
        assert n_step_return_horizon > 0, f"n_step_return_horizon should be greater than 0 but got: {n_step_return_horizon}"
        self._check_bounds(policy, int(n_step_return_horizon))
        self.policy = policy
        self._check_critic("critic", critic)
        self.critic = critic
        self.critic_old = lagged_copy(critic)
        self.policy_optim, s_a = flat_adam_of(policy_optim, policy.actor, f"{name}: policy_optim", True, ("factory",))
        self.critic_optim, s_c = flat_adam_of(critic_optim, critic, f"{name}: critic_optim", True, ("factory",))
        self._scheds = [s for s in (s_a, s_c) if s is not None]
        self.tau, self.gamma = tau, gamma
        self.n_step = self.n_step_return_horizon = int(n_step_return_horizon)
        self._ws: dict = {}

    @property
    def lr_scheduler(self):
        return _Schedulers(self._scheds) if self._scheds else None

    @property
    def device(self) -> torch.device:
        return self.policy.device

    @property
    def is_within_training_step(self) -> bool:
        return self.policy.is_within_training_step

    @is_within_training_step.setter
    def is_within_training_step(self, v: bool) -> None:
        self.policy.is_within_training_step = bool(v)

    def _critic_step(self, w: dict, x, head, twin: bool) -> dict:
        """_minimize_critic_squared_loss for the critic (and critic2): forward, `head(q1, q2)` -> {dq1, dq2, ...}, backward,
        Adam step.  -> the head's dict."""
        q1 = FlatMLP.forward(self.critic, x, save=True)
        q2 = FlatMLP.forward(self.critic2, x, save=True) if twin else None
        ch = head(q1, q2)
        self.critic.backward(ch["dq1"], w["n_split"], slabs=w["slabs_c1"])
        self.critic_optim.step(w["slabs_c1"])
        if twin:
            self.critic2.backward(ch["dq2"], w["n_split"], slabs=w["slabs_c2"])
            self.critic2_optim.step(w["slabs_c2"])
        return ch

    def _slab_widths(self) -> dict:
        return dict(slabs_a=self.policy.actor.flat.numel(), slabs_c1=self.critic.flat.numel())

    def _lagged(self) -> list:
        return [(self.critic_old, self.critic)]

    def _polyak(self) -> None:
        for old, net in self._lagged():
            ops.polyak(old.flat.data, net.flat.data, self.tau)

    # ---- checkpoints ---------------------------------------------------------------------------------------------
    def _nets(self) -> list[tuple[str, FlatMLP]]:
        """(reference prefix, net) in the reference's module order."""
        return [("policy.actor.", self.policy.actor), ("critic.", self.critic), ("critic_old.module.", self.critic_old)]

    def _optims(self) -> dict:
        return dict(policy_optim=self.policy_optim, critic_optim=self.critic_optim)

    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = OrderedDict((name.rstrip("."), net.flat.data.detach().clone().cpu()) for name, net in self._nets())
        sd.update({k: o.state_dict() for k, o in self._optims().items()})
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        for name, net in self._nets():
            net.flat.data.copy_(sd[name.rstrip(".")])
        for k, o in self._optims().items():
            o.load_state_dict(sd[k])

    @staticmethod
    def _ref_views(net) -> list:
        """[(key, view)] of a net under the reference's names: the net's own statement, unless a learner knows better."""
        return net.reference_named_views()

    def to_reference_state_dict(self) -> OrderedDict:
        """The module state_dict of the reference's learner: `policy.actor.*`, `critic.*`, `critic_old.module.*`
        (lagged_network.py wraps the copies in an EvalModeModuleWrapper), ..."""
        sd = OrderedDict()
        for prefix, net in self._nets():
            export_views(self._ref_views(net), prefix, sd)
        return sd

    def load_reference_state_dict(self, sd) -> None:
        for prefix, net in self._nets():
            import_views(self._ref_views(net), sd, prefix)


class ActorDualCriticsOffPolicyAlgorithm(ActorCriticOffPolicyAlgorithm):
    """td3.py:32-102: a second critic (None: a copy of the first, quirk Q48) with its lagged copy and Adam."""

    def __init__(self, *, policy, policy_optim: AdamOptimizerFactory, critic, critic_optim: AdamOptimizerFactory, critic2=None,
                 critic2_optim: AdamOptimizerFactory | None = None, tau: float = 0.005, gamma: float = 0.99,
                 n_step_return_horizon: int = 1) -> None:
        super().__init__(policy=policy, policy_optim=policy_optim, critic=critic, critic_optim=critic_optim, tau=tau,
                         gamma=gamma, n_step_return_horizon=n_step_return_horizon)
        if critic2 is not None:
            self._check_critic("critic2", critic2)
        self.critic2 = critic2 if critic2 is not None else lagged_copy(critic)   # critic2 or deepcopy(critic) (td3.py:90)
        self.critic2_old = lagged_copy(self.critic2)
        self.critic2_optim, s = flat_adam_of(critic2_optim or critic_optim, self.critic2, f"{type(self).__name__}: critic2_optim",
                                             True, ("factory",))
        if s is not None:
            self._scheds.append(s)

    def _slab_widths(self) -> dict:
        return dict(super()._slab_widths(), slabs_c2=self.critic2.flat.numel())

    def _optims(self) -> dict:
        return dict(super()._optims(), critic2_optim=self.critic2_optim)

    def _lagged(self) -> list:
        return super()._lagged() + [(self.critic2_old, self.critic2)]

    def _nets(self):
        return super()._nets() + [("critic2.", self.critic2), ("critic2_old.module.", self.critic2_old)]
