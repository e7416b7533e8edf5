"""DQN (double / vanilla, optional lagged target network, n-step targets, action masks) on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelfree/dqn.py:
  `DiscreteQLearningPolicy`      :39-174   Q-network -> masked greedy action, per-row epsilon-greedy noise
  `QLearningOffPolicyAlgorithm`  :180-285  n-step return, periodic full copy into the lagged network
  `DQN`                          :288-404  `_target_q`, MSE / Huber TD loss
and of `Algorithm.compute_nstep_return` / `OffPolicyAlgorithm.update` (algorithm_base.py:720-815, 866-905).
The Q-network is a `FlatMLP` (csrc/dense.hip); the n-step walk over the device buffer is one launch
(`tsm_nstep_return`, csrc/nstep.hip); the bootstrap value, the target, the loss and its gradient are one launch
(`tsm_dqn_td_head`, csrc/dqn.hip); the device acting path is `tsm_dqn_egreedy`.  There is no autograd fallback.

Kept quirks: Q15 -- `compute_q_value`'s mask offset is taken over the whole batch tensor; Q16 -- the
lagged network is copied BEFORE the gradient step of calls 0, f, 2f, ... (`_iter` starts at 0), so the first copy changes
nothing; Q17 -- `weight` does not enter the Huber loss, and the vanilla (non-double) target ignores the mask; Q18 -- on AEC
rows the agent's reward column stands in for `buffer.rew` while the n-step walk visits the rows of every agent; Q19 -- the
mask read with obs_next[idx_n] is the one the buffer keeps for row idx_n.
"""
from __future__ import annotations

import logging
from collections import OrderedDict
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch
from torch import nn

from .. import ops
from ..data.batch import Batch
from ..data.stats import TrainingStats
from ..utils.learner import act_result, result_slot, sample_counter, slab_workspace
from ..utils.net import FlatMLP, Recurrent, export_views, import_views, lagged_copy, ref_layer_keys
from ..utils.tensor import to_tensor
from .optim import flat_adam_of

log = logging.getLogger(__name__)


@dataclass(kw_only=True)
class SimpleLossTrainingStats(TrainingStats):
    """reinforce.py `SimpleLossTrainingStats`."""
    loss: float


def _obs_rows(obs):
    """(observation array, mask or None) of `batch.obs` / `batch.obs_next` (dqn.py:135-138)."""
    if isinstance(obs, Batch):
        return (obs.obs if "obs" in obs else obs), (obs.mask if "mask" in obs else None)
    return obs, None


class DiscreteQLearningPolicy(nn.Module):
    """dqn.py:39-174 with a `FlatMLP` Q-network (obs -> ... -> n actions)."""

    _model_cls: type = FlatMLP   # the network class the update kernels of this policy's learner run on

    def __init__(self, *, model: FlatMLP, action_space: Any, observation_space: Any = None, eps_training: float = 0.0,
                 eps_inference: float = 0.0, seed: int = 0, atoms: int = 1) -> None:
        """`atoms`: outputs per action -- 1 here; the distributional policies (algorithm/distq.py) pass their N."""
        super().__init__()
        # the reference's `Recurrent` (utils/net/common.py:372-458) stands where the plain Q-network does: DQN alone takes it
        self.recurrent = type(self) is DiscreteQLearningPolicy and isinstance(model, Recurrent)   # (not the distributional policies)
        self._act_state: tuple | None = None   # (hidden, cell) [rows, layers, H] of the collector's rows, in HBM
        if not (isinstance(model, self._model_cls) or self.recurrent):
            raise TypeError(f"DiscreteQLearningPolicy needs a {self._model_cls.__name__} Q-network: the update runs in HIP, "
                            f"there is no autograd fallback (got {type(model).__name__})")
        self.n_act = self._n_act_of(model, action_space, int(atoms))
        self.model = model
        self.action_space, self.observation_space = action_space, observation_space
        self.seed = int(seed)
        self._sample_ctr = 0
        dev = model.flat.device
        # the epsilon the acting kernel reads: a device scalar, so that a captured collect graph sees every change
        self._eps_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self._zero_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self._within = False
        self.eps_training, self.eps_inference = float(eps_training), float(eps_inference)
        self._push_eps()

    @staticmethod
    def _n_act_of(model, action_space: Any, atoms: int) -> int:
        """The number of actions the acting kernel chooses among, checked against the model's outputs and the kernels' bounds."""
        n = getattr(action_space, "n", None)
        if n is None or int(n) * atoms != model.dims[-1]:
            raise ValueError(f"DiscreteQLearningPolicy: the model has {model.dims[-1]} outputs, the action space "
                             f"{'no size' if n is None else f'{int(n)} actions'}" + (f" of {atoms} atoms each" if atoms != 1 else ""))
        ops.dqn_check(int(n))
        return int(n)

    @property
    def device(self) -> torch.device:
        return self.model.flat.device

    def _eps(self) -> float:
        return self.eps_training if self._within else self.eps_inference

    def _push_eps(self) -> None:
        self._eps_dev.fill_(self._eps())

    @property
    def is_within_training_step(self) -> bool:
        return self._within

    @is_within_training_step.setter
    def is_within_training_step(self, v: bool) -> None:
        self._within = bool(v)
        self._push_eps()

    def set_eps_training(self, eps: float) -> None:
        self.eps_training = float(eps)
        self._push_eps()

    def set_eps_inference(self, eps: float) -> None:
        self.eps_inference = float(eps)
        self._push_eps()

    def compute_q_value(self, logits: torch.Tensor, mask) -> torch.Tensor:
        """dqn.py:145-151: masked entries sink below the smallest logit of the WHOLE tensor (quirk Q15)."""
        if mask is not None:
            min_value = logits.min() - logits.max() - 1.0
            logits = logits + (1 - to_tensor(mask, logits.device, logits.dtype)) * min_value
        return logits

    # The two hooks a subclass overrides: what its network says about rows, as `forward` and `act_device` need it.
    def _forward_values(self, x: torch.Tensor, model):
        """x [..., D] in HBM, `model` as `forward` got it (None: the online net)
        -> (value per action [R, A], `Batch.logits`, further fields of the returned Batch)."""
        model = self.model if model is None else model
        logits = FlatMLP.forward(model, x.reshape(-1, model.dims[0]), save=False)
        return logits, logits, {}

    def _act_values(self, rows: torch.Tensor, ctr: int, offset_dev) -> torch.Tensor:
        """rows [R, D] in HBM, (ctr, offset_dev) the Philox counter of the epsilon draw -> value per action [R, A]."""
        return FlatMLP.forward(self.model, rows, save=False)

    def forward(self, batch: Batch, state: Any = None, model: FlatMLP | None = None) -> Batch:
        """-> Batch(logits in HBM ([B, A]; a subclass: its distribution per action), act = the first argmax of the masked
        value per action (numpy i64), state)."""
        obs, mask = _obs_rows(batch.obs)
        if self.recurrent:   # obs [B, L, D] | [B, D]; state None (zeros) or Batch(hidden, cell) [B, layers, H], handed back
            q, (hid, cell) = (self.model if model is None else model).forward(to_tensor(obs, self.device, torch.float32), state,
                                                                              save=False)
            logits, extra, state = q, {}, Batch(hidden=hid, cell=cell)
        else:
            q, logits, extra = self._forward_values(to_tensor(obs, self.device, torch.float32), model)
        m = None if mask is None else to_tensor(np.asarray(mask, bool) if not isinstance(mask, torch.Tensor) else mask,
                                                 self.device, torch.uint8).reshape(q.shape)
        act = ops.dqn_egreedy(q, self._zero_dev, 0, mask=m)
        return Batch(logits=logits, act=act.to(torch.int64).cpu().numpy(), state=state, **extra)

    def add_exploration_noise(self, act, batch):
        """dqn.py:153-171 on the host RNG: `np.random.rand` for the row coins, then for the candidate actions."""
        eps = self._eps()
        if np.isclose(eps, 0.0):
            return act
        if isinstance(act, np.ndarray):
            batch_size = len(act)
            rand_mask = np.random.rand(batch_size) < eps
            q = np.random.rand(batch_size, int(self.action_space.n))
            if isinstance(batch.obs, Batch) and "mask" in batch.obs:
                q += np.asarray(batch.obs.mask)
            rand_act = q.argmax(axis=1)
            act[rand_mask] = rand_act[rand_mask]
            return act
        raise NotImplementedError(f"Currently only numpy array is supported for action, but got {type(act)}")

    def act_device(self, obs: torch.Tensor, out: dict | None = None, offset_dev: torch.Tensor | None = None,
                   row_offset: int = 0, mask: torch.Tensor | None = None) -> dict:
        """obs [..., D] in HBM -> act i32 [rows] (`_act_values`, then tsm_dqn_egreedy with the epsilon of the current
        phase); logp, value = 0.  The Philox counter is offset_dev (the env's device tick: captured graphs advance it) or
        the policy's own."""
        rows = obs.reshape(-1, self.model.dims[0])
        R = rows.shape[0]
        ctr = sample_counter(self, R, row_offset, offset_dev)
        if self.recurrent:   # the L = 1 step from the kept state, written back in place: a captured graph advances it on replay
            if self._act_state is None or self._act_state[0].shape[0] != R:
                self._act_state = self.model.zero_state(R)
            q, _ = self.model.forward(rows, self._act_state, save=False, state_out=self._act_state)
        else:
            q = self._act_values(rows, ctr, offset_dev)
        m = None if mask is None else mask.reshape(R, self.n_act)
        act = ops.dqn_egreedy(q, self._eps_dev, self.seed, offset=ctr, offset_dev=offset_dev, mask=m,
                              out=None if out is None else out["act"].view(-1))
        return act_result(out, act, q=q)


    def reset_state_device(self, done: torch.Tensor | None = None) -> None:
        """collector.py:977-979 on the device: the kept state rows of the envs with done[e] != 0 restart from zero (None: all
        of them).  One launch, no host read; nothing to do for a policy without a recurrent net or before its first acting step.
        The state is ONE slot per policy, for the rows of one collector: two collectors that act with the same policy object
        (a train and a test collector) would continue and reset one another's state -- give each a policy of its own over the
        same net (`Recurrent(..., storage=net.flat.data)` shares the parameters)."""
        if self._act_state is None:
            return
        hid, cell = self._act_state
        if done is None:
            hid.zero_()
            cell.zero_()
        else:
            ops.lstm_state_reset(hid, cell, done.reshape(-1), rows_per_env=hid.shape[0] // done.numel())


class DeviceOffPolicyRows:
    """What every off-policy learner on the device buffers shares (algorithm_base.py:720-815, 866-905): the n-step walk, the
    successor rows, the sampled batch of a prioritized buffer, the priority write-back and `update`.  A learner supplies
    `device`, `gamma`, `n_step`, `lr_scheduler`, `is_within_training_step`, `_preprocess_batch` and `_update_with_batch`."""

    def _agent_column(self, buffer, agent: int | None) -> tuple[int, int]:
        """-> (k, col): the agent's reward column and the lane its rows are read from (None: the buffer's only column)."""
        n_col = buffer.rew_store.shape[2]
        name = type(self).__name__
        if agent is None:
            if n_col != 1:
                raise ValueError(f"{name}: the buffer holds {n_col} reward columns; say which agent's (agent=k)")
            agent = 0
        if not 0 <= int(agent) < n_col:
            raise ValueError(f"{name}: agent column {agent} outside the buffer's {n_col}")
        k = int(agent)
        return k, (0 if getattr(buffer, "aec", False) else k)  # AEC rows: one observation / flag per row; joint rows: the lane

    # ---- compute_nstep_return (algorithm_base.py:720-815) ---------------------------------------------------------
    def _nstep_rows(self, batch: Batch, buffer, indices, agent: int | None):
        """The n-step walk for `indices` (one launch): the batch leaves with idx_n, mc, gpow, vmask and -- when it came empty,
        as from `update` -- with obs and act gathered from the device stores.  `agent`: the agent's column -- its lane of a
        joint-step buffer, its reward column of an AEC buffer (the walk still visits all rows, quirk Q18).
        -> (idx, idx_n, col): the flat indices, their n-step successors, the lane the rows are read from."""
        dev = self.device
        idx = to_tensor(indices, dev, torch.int64).reshape(-1)
        if len(batch.get_keys()) != 0 and len(batch) != idx.numel():
            raise ValueError(f"Batch size {len(batch)} and indices size {idx.numel()} mismatch.")
        k, col = self._agent_column(buffer, agent)
        idx_n, mc, gpow, vmask = ops.nstep_return(buffer.index, buffer.term_store, buffer.rew_store, idx, self.n_step,
                                                  self.gamma, rew_col=k, term_col=col)
        batch.idx_n, batch.mc, batch.gpow, batch.vmask = idx_n, mc, gpow, vmask
        stacked = getattr(buffer, "stack_num", 1) > 1
        if stacked and not getattr(self, "takes_stacks", False):
            raise ValueError(f"{type(self).__name__}: the buffer stacks {buffer.stack_num} frames, which only a learner around a "
                             f"recurrent net reads (DQN on utils.net.Recurrent); build the buffer with stack_num=1")
        if "obs" not in batch and stacked:  # the stack ending at idx, this agent's lane: [I, L, D] in one launch
            batch.obs = buffer._gather_obs(buffer.obs_store, idx, lane=col)
        elif "obs" not in batch:  # rows straight from the device stores (DQN.update)
            batch.obs = buffer._gather(buffer.obs_store, idx)[:, col].contiguous()
        if "act" not in batch:
            act = buffer._gather(buffer.act_store, idx)[:, col].contiguous()
            batch.act = act if act.is_floating_point() else act.to(torch.int64)  # a Box store (act_dim): f32 [I, k]
        return idx, idx_n, col

    @staticmethod
    def _successor_rows(buffer, rows, col: int):
        """obs_next[rows] (with ignore_obs_next: obs at next(rows), buffer_base.py:612-616) and the mask the buffer keeps for
        those rows (quirk Q19), gathered with tsm_vrb_gather.  -> (obs_next [I, D], mask or None)."""
        store, at = (buffer.obs_next_store, rows) if buffer._save_obs_next else (buffer.obs_store, buffer.index.next(rows))
        mask_store = getattr(buffer, "mask_store", None)
        if getattr(buffer, "stack_num", 1) > 1:   # the stack ending at `rows`: [I, L, D]
            return buffer._gather_obs(store, at, lane=col), (None if mask_store is None else buffer._gather(mask_store, rows))
        nxt = buffer._gather(store, at)
        return nxt[:, col].contiguous(), (None if mask_store is None else buffer._gather(mask_store, rows))

    @staticmethod
    def _sampled_batch(buffer, indices) -> Batch:
        """What `update` keeps of `buffer[indices]`: the rows stay in the device stores (`_preprocess_batch` gathers them); a
        prioritized buffer adds `weight`, its importance-sampling weights (prio.py:103-106) as float32 in HBM -- the TD head's
        `weight` (quirk Q17: the Huber loss ignores it)."""
        batch = Batch()
        if hasattr(buffer, "update_weight"):
            batch.weight = buffer.batch_weight_device(indices)[0]
        return batch

    @staticmethod
    def _pop_weight(batch: Batch):
        """`batch.weight`, taken off the batch, as the heads take it: None, or one weight per row.  A scalar (a batch that did
        not come from a prioritized buffer) is None when it is 1, else that value for every row."""
        weight = batch.pop("weight", None) if "weight" in batch else None
        if weight is not None and not isinstance(weight, (torch.Tensor, np.ndarray)):
            weight = None if float(weight) == 1.0 else np.full(len(batch.mc), float(weight), np.float32)
        return weight

    def _postprocess_batch(self, batch: Batch, buffer, indices) -> None:
        """Algorithm._postprocess_batch (algorithm_base.py:560-582): a prioritized buffer takes `batch.weight` -- after
        `_update_with_batch` the TD errors, still in HBM -- as the new priorities of `indices`."""
        if hasattr(buffer, "update_weight"):
            if "weight" in batch:
                buffer.update_weight(indices, batch.weight)
            else:
                log.warning("batch has no attribute 'weight', but buffer has an update_weight method. This is probably a "
                            "mistake. Prioritized replay is disabled for this batch.")

    def update(self, buffer, sample_size: int | None, agent: int | None = None) -> SimpleLossTrainingStats:
        """OffPolicyAlgorithm.update (algorithm_base.py:889-905): sample, preprocess, update, postprocess.  The sampled rows
        are read from the device stores in place (`buffer.sample` would carry them through the host); with a prioritized
        buffer the indices, the IS weights and the new priorities stay in HBM too, so the loss slot is the only host read."""
        if not self.is_within_training_step:
            raise RuntimeError("update() was called outside of a training step as signalled by "
                               "`is_within_training_step=False`")
        prioritized = hasattr(buffer, "update_weight")
        indices = buffer.sample_indices_device(sample_size) if prioritized else buffer.sample_indices(sample_size)
        batch = self._preprocess_batch(self._sampled_batch(buffer, indices), buffer, indices, agent=agent)
        stats = self._update_with_batch(batch)
        self._postprocess_batch(batch, buffer, indices)
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        return stats


class DQN(DeviceOffPolicyRows, nn.Module):
    """dqn.py:180-404 on the device buffer.  `optim`: an `AdamOptimizerFactory` (its hyper-parameters drive the HIP Adam
    over the model's flat vector) or a `FlatAdam` over that vector."""

    def __init__(self, *, policy: DiscreteQLearningPolicy, optim: Any, gamma: float = 0.99, n_step_return_horizon: int = 1,
                 target_update_freq: int = 0, is_double: bool = True, huber_loss_delta: float | None = None) -> None:
        super().__init__()
        if not isinstance(policy, DiscreteQLearningPolicy):
            raise TypeError(f"DQN needs a DiscreteQLearningPolicy, got {type(policy).__name__}")
        assert 0.0 <= gamma <= 1.0, f"discount factor should be in [0, 1] but got: {gamma}"
        assert n_step_return_horizon > 0, f"n_step_return_horizon should be greater than 0 but got: {n_step_return_horizon}"
        ops.dqn_check(policy.n_act, int(n_step_return_horizon))
        self.policy = policy
        model = policy.model
        self.optim, self.lr_scheduler = flat_adam_of(optim, model, "DQN: optim", True, ("factory", "flat"))
        self.gamma = gamma
        self.n_step = int(n_step_return_horizon)
        self.target_update_freq = int(target_update_freq)
        self.is_double = bool(is_double)
        self.huber_loss_delta = huber_loss_delta
        self._iter = 0
        self.model_old: FlatMLP | None = None
        if self.use_target_network:
            self.model_old = lagged_copy(model)
            self.target_flat = self.model_old.flat.data
        self._ws: dict = {}

    @property
    def device(self) -> torch.device:
        return self.policy.device

    @property
    def use_target_network(self) -> bool:
        return self.target_update_freq > 0

    @property
    def is_within_training_step(self) -> bool:
        return self.policy.is_within_training_step

    @is_within_training_step.setter
    def is_within_training_step(self, v: bool) -> None:
        self.policy.is_within_training_step = v

    def _periodically_update_lagged_network_weights(self) -> None:
        """dqn.py:277-285: a full copy on calls 0, f, 2f, ... -- `_iter` starts at 0 (quirk Q16)."""
        if self.use_target_network and self._iter % self.target_update_freq == 0:
            self.target_flat.copy_(self.policy.model.flat.data)
        self._iter += 1

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The n-step walk, then the networks on obs_next[idx_n] (and mask[idx_n] if the buffer keeps masks).  The batch
        leaves with what the TD head needs; `returns` is set by `_update_with_batch`, where the head runs."""
        _, idx_n, col = self._nstep_rows(batch, buffer, indices, agent)
        nxt, mask_next = self._successor_rows(buffer, idx_n, col)
        batch.q_next_online = self._q_rows(self.policy.model, nxt)
        if self.use_target_network:
            batch.q_next_target = self._q_rows(self.model_old, nxt)
        if mask_next is not None:
            batch.mask_next = mask_next
        return batch

    # ---- DQN._update_with_batch (dqn.py:381-404) --------------------------------------------------------------
    def _update_with_batch(self, batch: Batch) -> SimpleLossTrainingStats:
        """The online forward (saved), the TD head, the backward into slabs, one Adam step, the loss into a pinned slot."""
        self._periodically_update_lagged_network_weights()
        self._after_lagged_copy(batch)
        dev = self.device
        weight = self._pop_weight(batch)
        obs, _ = _obs_rows(batch.obs)
        model = self.policy.model
        x = to_tensor(obs, dev, torch.float32)
        x = x if self.takes_stacks else x.reshape(-1, model.dims[0])   # a recurrent net: [B, L, D] | [B, D]
        B = x.shape[0]
        act = to_tensor(batch.act, dev, torch.int64).reshape(-1)
        w = slab_workspace(self._ws, B, dev, **self._slab_widths())
        q = self._online_forward(batch, x)
        d_out, partial, returns, prio = self._head(batch, q, act, None if weight is None else
                                                   to_tensor(weight, dev, torch.float32).reshape(-1))
        model.backward(d_out, w["n_split"], slabs=w["slabs"])
        self._before_step(batch, w)
        self.optim.step(w["slabs"])
        slot = result_slot(w, self._n_results)
        self._finalize(batch, partial, B, slot["h"])
        slot["event"].record()
        batch.returns = returns
        batch.weight = prio  # prio-buffer
        slot["event"].synchronize()
        return self._stats_of(slot["h"])

    # What a learner with a second loss changes (FQF): its other gradient and step, the slot's size and what lands in it.
    _n_results = 2

    def _slab_widths(self) -> dict:
        """The gradient slab arrays of a batch's workspace, by name."""
        return dict(slabs=self.policy.model.flat.numel())

    def _before_step(self, batch: Batch, w: dict) -> None:
        """Between the model's backward and its Adam step: nothing here."""

    def _finalize(self, batch: Batch, partial, B: int, h) -> None:
        """The head's partials into the pinned slot `h`: {loss, mean q}."""
        ops.qmix_finalize(partial, B, h)

    def _stats_of(self, h) -> TrainingStats:
        return self._stats(float(h[0]))

    def _online_forward(self, batch: Batch, x: torch.Tensor) -> torch.Tensor:
        """The online net on the sampled rows, activations kept for `model.backward`."""
        if self.takes_stacks:
            return self.policy.model.forward(x, None, save=True)[0]
        return FlatMLP.forward(self.policy.model, x, save=True)

    @property
    def takes_stacks(self) -> bool:
        """The Q-network is recurrent: it reads the stacked rows of a `stack_num > 1` buffer, from zero state in every
        forward of an update, as the reference's does with `state=None` (dqn.py:365-379)."""
        return bool(getattr(self.policy, "recurrent", False))

    def _q_rows(self, net, rows: torch.Tensor) -> torch.Tensor:
        """`net` on successor rows, nothing kept."""
        if self.takes_stacks:
            return net.forward(rows, None, save=False)[0]
        return FlatMLP.forward(net, rows, save=False)

    def _after_lagged_copy(self, batch: Batch) -> None:
        """What a learner computes between the lagged copy and its loss (C51's successor forwards); nothing here."""

    def _head(self, batch: Batch, q, act, weight):
        """-> (d loss / d network output, f64 partials for tsm_qmix_finalize, returns, the new priorities)."""
        head = ops.dqn_td_head(q, batch.q_next_online, batch.get("q_next_target"), act, batch.mc, batch.gpow, batch.vmask,
                               mask_next=batch.get("mask_next"), weight=weight, is_double=self.is_double,
                               huber_delta=self.huber_loss_delta)
        return head["dq"], head["partial"], head["returns"], head["td_error"]

    @staticmethod
    def _stats(loss: float) -> TrainingStats:
        return SimpleLossTrainingStats(loss=loss)

    # ---- checkpoints ---------------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = OrderedDict(model=self.policy.model.flat.data.detach().clone().cpu(),
                         model_old=self.target_flat.detach().clone().cpu() if self.use_target_network else None,
                         optim=self.optim.state_dict(), iter=self._iter)
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        self.policy.model.flat.data.copy_(sd["model"])
        if self.use_target_network:
            self.target_flat.copy_(sd["model_old"] if sd.get("model_old") is not None else sd["model"])
        self.optim.load_state_dict(sd["optim"])
        self._iter = int(sd["iter"])

    def _ref_nets(self) -> list:
        """(prefix, net) of a reference checkpoint: `policy.model.`, then `model_old.module.` with a target network."""
        return [("policy.model.", self.policy.model)] + ([("model_old.module.", self.model_old)] if self.use_target_network else [])

    @staticmethod
    def _ref_views(net) -> list:
        """[(key, view)] of a Q-network: a `FlatMLP` is a `Net(hidden_sizes=[...])` used whole (`ref_layer_keys`: "body");
        any other net states its own names."""
        if isinstance(net, FlatMLP):
            return net.named_layers(ref_layer_keys(net.n_layers, "body"))
        return net.reference_named_views()

    def to_reference_state_dict(self) -> OrderedDict:
        """The module state_dict of the reference's learner around its Q-network: `policy.model.*`, then
        `model_old.module.*` when a target network is used (lagged_network.py wraps it in an EvalModeModuleWrapper)."""
        sd = OrderedDict()
        for prefix, net in self._ref_nets():
            export_views(self._ref_views(net), prefix, sd)
        return sd

    def load_reference_state_dict(self, sd) -> None:
        for prefix, net in self._ref_nets():
            import_views(self._ref_views(net), sd, prefix)
