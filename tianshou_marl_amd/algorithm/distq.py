"""C51 and QR-DQN (distributional Q-learning heads over DQN's n-step / prioritized-replay / dispatch machinery) on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelfree/c51.py (`C51Policy` :16-67, `C51` :70-160) and qrdqn.py
(`QRDQNPolicy` :18-20, `QRDQN` :26-131).  The Q-network is a `FlatMLP` whose last layer has A * N outputs, read per row as
[A][N]; the softmax that the reference's `Net(num_atoms=N, softmax=True)` applies inside the module belongs to the head
kernels (csrc/distq.hip): `tsm_distq_values` reduces a row to one value per action (and, for C51, its probabilities),
`tsm_c51_head` / `tsm_qrdqn_head` form the target, the loss and its gradient in one launch each.  Acting is
`tsm_dqn_egreedy` on those values.  There is no autograd fallback.

Kept quirks: Q20 -- C51 bootstraps its n-step returns at row idx_n but takes a* and the next
distribution from `batch.obs_next`, the ONE-step successor of the sampled row (c51.py:124), after the lagged copy of the
same call; Q21 -- QR-DQN takes both at idx_n, before that copy (qrdqn.py:95-98); Q22 -- neither has an `is_double` switch:
a* always comes from the online net, the values from the lagged net when there is one; Q23 -- the cross entropy is
-sum m log(p + 1e-8) and its gradient goes through the 1e-8.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any

import torch

from .. import ops
from ..data.batch import Batch
from ..data.stats import TrainingStats
from ..utils.net import FlatMLP
from ..utils.tensor import to_tensor
from .dqn import DQN, DiscreteQLearningPolicy, SimpleLossTrainingStats
from .pg import LossSequenceTrainingStats


class _DistributionalPolicy(DiscreteQLearningPolicy):
    """A `DiscreteQLearningPolicy` whose net emits `n_atoms` numbers per action."""

    def __init__(self, *, model: FlatMLP, action_space: Any, observation_space: Any, n_atoms: int, eps_training: float,
                 eps_inference: float, seed: int) -> None:
        n = getattr(action_space, "n", None)
        if n is not None and isinstance(model, FlatMLP):
            ops.distq_check(int(n), int(n_atoms))
        super().__init__(model=model, action_space=action_space, observation_space=observation_space,
                         eps_training=eps_training, eps_inference=eps_inference, seed=seed, atoms=int(n_atoms))
        self.n_atoms = int(n_atoms)

    @property
    def support_or_none(self):
        return None

    def values(self, raw: torch.Tensor, want_probs: bool = False):
        """raw [R, A * N] in HBM -> the value per action [R, A] before the mask (and the probabilities, C51 only)."""
        return ops.distq_values(raw, self.n_act, self.n_atoms, support=self.support_or_none, want_probs=want_probs)

    def compute_q_value(self, logits: torch.Tensor, mask) -> torch.Tensor:
        """c51.py:66-67 / qrdqn.py:19-20 on the raw network output [R, A * N] (or [R, A, N]), then dqn.py:145-151."""
        raw = to_tensor(logits, self.device, torch.float32).reshape(-1, self.n_act * self.n_atoms)
        return super().compute_q_value(self.values(raw), mask)

    def _logits(self, raw: torch.Tensor):
        """-> (q [R, A], `Batch.logits` [R, A, N])."""
        return self.values(raw), raw.view(-1, self.n_act, self.n_atoms)

    def _forward_values(self, x: torch.Tensor, model):
        """`Batch.logits` is [B, A, N] (C51: the probabilities)."""
        q, logits = self._logits(super()._forward_values(x, model)[0])
        return q, logits, {}

    def _act_values(self, rows: torch.Tensor, ctr: int, offset_dev) -> torch.Tensor:
        return self.values(super()._act_values(rows, ctr, offset_dev))


class C51Policy(_DistributionalPolicy):
    """c51.py:16-67 with a `FlatMLP` Q-network (obs -> ... -> n actions x num_atoms raw outputs)."""

    def __init__(self, *, model: FlatMLP, action_space: Any, observation_space: Any = None, num_atoms: int = 51,
                 v_min: float = -10.0, v_max: float = 10.0, eps_training: float = 0.0, eps_inference: float = 0.0,
                 seed: int = 0) -> None:
        assert num_atoms > 1, f"num_atoms should be greater than 1 but got: {num_atoms}"
        assert v_min < v_max, f"v_max should be larger than v_min, but got {v_min=} and {v_max=}"
        super().__init__(model=model, action_space=action_space, observation_space=observation_space, n_atoms=num_atoms,
                         eps_training=eps_training, eps_inference=eps_inference, seed=seed)
        self.num_atoms, self.v_min, self.v_max = int(num_atoms), v_min, v_max
        # the reference's own values: linspace in float32 on the host, then to HBM
        self.support = torch.linspace(self.v_min, self.v_max, self.num_atoms).to(self.device)

    @property
    def support_or_none(self):
        return self.support

    def _logits(self, raw: torch.Tensor):
        return self.values(raw, want_probs=True)


class QRDQNPolicy(_DistributionalPolicy):
    """qrdqn.py:18-20.  The reference infers the number of quantiles from the net's [B, A, N] output; the flat output of a
    `FlatMLP` needs it said."""

    def __init__(self, *, model: FlatMLP, action_space: Any, observation_space: Any = None, eps_training: float = 0.0,
                 eps_inference: float = 0.0, num_quantiles: int = 200, seed: int = 0) -> None:
        assert num_quantiles > 1, f"num_quantiles should be greater than 1 but got: {num_quantiles}"
        super().__init__(model=model, action_space=action_space, observation_space=observation_space, n_atoms=num_quantiles,
                         eps_training=eps_training, eps_inference=eps_inference, seed=seed)
        self.num_quantiles = int(num_quantiles)


class _DistributionalQLearning(DQN):
    """QLearningOffPolicyAlgorithm (dqn.py:180-285) as `DQN` carries it -- the walk, the lagged copy, `update`, the
    checkpoints -- with the successor rows, the head and the constants of a distributional learner."""

    _policy_cls: type = _DistributionalPolicy
    _next_at_idx_n = True   # where a* and the next distribution are read: idx_n (QR-DQN) or the sampled row itself (C51)

    def __init__(self, *, policy, optim: Any, gamma: float, n_step_return_horizon: int, target_update_freq: int) -> None:
        if not isinstance(policy, self._policy_cls):
            raise TypeError(f"{type(self).__name__} needs a {self._policy_cls.__name__}, got {type(policy).__name__}")
        super().__init__(policy=policy, optim=optim, gamma=gamma, n_step_return_horizon=n_step_return_horizon,
                         target_update_freq=target_update_freq)

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The n-step walk, then the successor rows this learner reads (quirks Q20 / Q21) with the mask the buffer keeps for
        them.  QR-DQN runs its forwards here, before the lagged copy; C51 in `_update_with_batch`, after it."""
        idx, idx_n, col = self._nstep_rows(batch, buffer, indices, agent)
        batch.rows_next, mask_next = self._successor_rows(buffer, idx_n if self._next_at_idx_n else idx, col)
        if mask_next is not None:
            batch.mask_next = mask_next
        if self._next_at_idx_n:
            self._next_forwards(batch)
        return batch

    def _next_forwards(self, batch: Batch) -> None:
        """The online net's values per action on the successor rows (for a*), and the raw output that supplies the next
        distribution: the lagged net's when there is one (quirk Q22)."""
        raw_on = FlatMLP.forward(self.policy.model, batch.rows_next, save=False)
        batch.q_next_online = self.policy.values(raw_on)
        batch.raw_next = FlatMLP.forward(self.model_old, batch.rows_next, save=False) if self.use_target_network else raw_on

    def _after_lagged_copy(self, batch: Batch) -> None:
        if not self._next_at_idx_n:
            self._next_forwards(batch)

    def _constants(self) -> "OrderedDict[str, torch.Tensor]":
        """The reference's non-trainable parameters that lead its state_dict."""
        raise NotImplementedError

    def to_reference_state_dict(self) -> OrderedDict:
        sd = OrderedDict((k, v.detach().clone().cpu()) for k, v in self._constants().items())
        sd.update(super().to_reference_state_dict())
        return sd


class C51(_DistributionalQLearning):
    """c51.py:70-160 on the device buffer."""

    _policy_cls = C51Policy
    _next_at_idx_n = False

    def __init__(self, *, policy: C51Policy, optim: Any, gamma: float = 0.99, n_step_return_horizon: int = 1,
                 target_update_freq: int = 0) -> None:
        super().__init__(policy=policy, optim=optim, gamma=gamma, n_step_return_horizon=n_step_return_horizon,
                         target_update_freq=target_update_freq)
        self.delta_z = (policy.v_max - policy.v_min) / (policy.num_atoms - 1)

    def _head(self, batch: Batch, q, act, weight):
        pol = self.policy
        head = ops.c51_head(q, batch.q_next_online, batch.raw_next, act, batch.mc, batch.gpow, batch.vmask, pol.support,
                            pol.v_min, pol.v_max, mask_next=batch.get("mask_next"), weight=weight)
        return head["d_out"], head["partial"], head["returns"], head["prio"]

    @staticmethod
    def _stats(loss: float) -> TrainingStats:
        return LossSequenceTrainingStats(loss=loss)   # c51.py:160 hands the float itself to this class

    def _constants(self):
        return OrderedDict([("policy.support", self.policy.support)])


class QRDQN(_DistributionalQLearning):
    """qrdqn.py:26-131 on the device buffer."""

    _policy_cls = QRDQNPolicy

    def __init__(self, *, policy: QRDQNPolicy, optim: Any, gamma: float = 0.99, num_quantiles: int = 200,
                 n_step_return_horizon: int = 1, target_update_freq: int = 0) -> None:
        assert num_quantiles > 1, f"num_quantiles should be greater than 1 but got: {num_quantiles}"
        self._check_quantiles(policy, num_quantiles)
        super().__init__(policy=policy, optim=optim, gamma=gamma, n_step_return_horizon=n_step_return_horizon,
                         target_update_freq=target_update_freq)
        self.num_quantiles = int(num_quantiles)
        tau = torch.linspace(0, 1, self.num_quantiles + 1)   # qrdqn.py:87-90, in float32 on the host as there
        self.tau_hat = ((tau[:-1] + tau[1:]) / 2).view(1, -1, 1).to(self.device)

    @staticmethod
    def _check_quantiles(policy, num_quantiles: int) -> None:
        if isinstance(policy, QRDQNPolicy) and policy.num_quantiles != num_quantiles:
            raise ValueError(f"QRDQN: num_quantiles = {num_quantiles}, but the policy's net emits {policy.num_quantiles} "
                             "quantiles per action")

    def _head(self, batch: Batch, q, act, weight):
        head = ops.qrdqn_head(q, batch.q_next_online, batch.raw_next, act, batch.mc, batch.gpow, batch.vmask, self.tau_hat,
                              mask_next=batch.get("mask_next"), weight=weight)
        return head["d_out"], head["partial"], head["returns"], head["prio"]

    @staticmethod
    def _stats(loss: float) -> TrainingStats:
        return SimpleLossTrainingStats(loss=loss)

    def _constants(self):
        return OrderedDict([("tau_hat", self.tau_hat)])
