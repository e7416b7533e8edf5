"""ICM: the curiosity wrappers around the on-policy and the off-policy learners, on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelbased/icm.py:
  `ICMTrainingStats`     :22-34    the wrapped statistics plus icm_loss, icm_forward_loss, icm_inverse_loss
  `_ICMMixin`            :37-109   preprocess (`batch.rew += mse_loss * reward_scale`), one optimizer step on
                                   ((1 - w) CE + w mse) * lr_scale, postprocess (the reward is put back)
  `ICMOffPolicyWrapper`  :112-184  `ICMOnPolicyWrapper`  :187-261
The module is `utils.net.IntrinsicCuriosityModule`: three `FlatMLP`s (csrc/dense.hip) around the row-wise head of
csrc/icm.hip; its gradient is taken at preprocess time, on the weights from before the wrapped learner's update, as the
reference's graph is built then.  There is no autograd fallback.

Kept quirks: Q62 -- on-policy, GAE reads `batch.rew`, so the shaped reward drives the advantages; Q63 --
off-policy, the n-step return reads `buffer.rew`, so the intrinsic reward never reaches the TD target: the wrapped learner
updates as it would alone and only the ICM trains.
"""
from __future__ import annotations

from typing import Any

import torch
from torch import nn

from .. import ops
from ..data.batch import Batch
from ..data.stats import TrainingStats
from ..utils.learner import result_slot, slab_workspace
from ..utils.net import IntrinsicCuriosityModule
from ..utils.tensor import to_tensor
from .dqn import DeviceOffPolicyRows
from .optim import flat_adam_of
from .ppo import PPO


class ICMTrainingStats(TrainingStats):
    """icm.py:22-34 (a `TrainingStatsWrapper`): what the wrapped learner reported, read through, plus the ICM's three losses."""

    def __init__(self, wrapped_stats: Any, *, icm_loss: float, icm_forward_loss: float, icm_inverse_loss: float) -> None:
        self._wrapped_stats = wrapped_stats
        self.icm_loss, self.icm_forward_loss, self.icm_inverse_loss = icm_loss, icm_forward_loss, icm_inverse_loss

    @property
    def wrapped_stats(self):
        return self._wrapped_stats

    # the base class's two fields live on the wrapped object, as the reference keeps them in sync
    train_time = property(lambda self: self._wrapped_stats.train_time,
                          lambda self, v: setattr(self._wrapped_stats, "train_time", v))
    smoothed_loss = property(lambda self: self._wrapped_stats.smoothed_loss,
                             lambda self, v: setattr(self._wrapped_stats, "smoothed_loss", v))

    def __getattr__(self, name: str):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._wrapped_stats, name)

    def get_loss_stats_dict(self) -> dict[str, float]:
        out = dict(self._wrapped_stats.get_loss_stats_dict())
        out.update(icm_loss=float(self.icm_loss), icm_forward_loss=float(self.icm_forward_loss),
                   icm_inverse_loss=float(self.icm_inverse_loss))
        return out


class _ICMMixin:
    """icm.py:37-109 on the device: `_icm_forward` is `_icm_preprocess_batch`, `_icm_update` the optimizer step."""

    def _icm_init(self, wrapped, model, optim, lr_scale: float, reward_scale: float, forward_loss_weight: float) -> None:
        who = type(self).__name__
        if not isinstance(model, IntrinsicCuriosityModule):
            raise TypeError(f"{who} needs a utils.net.IntrinsicCuriosityModule: the update runs in HIP, there is no autograd "
                            f"fallback (got {type(model).__name__})")
        if getattr(wrapped, "dispatch", None) == "per_agent":
            raise NotImplementedError(f'{who}: dispatch="per_agent" is not supported: the wrapped learner would be updated once '
                                      'per agent between one ICM preprocess and one ICM step; use dispatch="pooled"')
        space = getattr(getattr(wrapped, "policy", wrapped), "action_space", None)
        if space is not None and not hasattr(space, "n"):
            raise NotImplementedError(f"{who}: the ICM's forward model takes one-hot actions; Box actions are not supported")
        if space is not None and int(space.n) != model.action_dim:
            raise ValueError(f"{who}: the action space has {int(space.n)} actions, the ICM model {model.action_dim}")
        self._refuse_grad_sync(wrapped)
        self.wrapped_algorithm = wrapped
        self.model = model
        self.optim, self.icm_lr_scheduler = flat_adam_of(optim, model, f"{who}: optim", True, ("factory", "flat"))
        self.lr_scale, self.reward_scale, self.forward_loss_weight = float(lr_scale), float(reward_scale), float(forward_loss_weight)
        self._icm_ws: dict = {}

    def _refuse_grad_sync(self, wrapped) -> None:
        if getattr(wrapped, "_grad_sync", None) is not None:
            raise NotImplementedError(f"{type(self).__name__}: a data-parallel wrapped learner (an attached grad_sync) is not "
                                      "supported: the ICM's gradients are not summed over the ranks")

    def _icm_forward(self, x: torch.Tensor, act: torch.Tensor, rew_io=None, ids=None):
        """The module on interleaved rows x [2R, D]: -> (mse_loss [R], act_hat [R, A]); the gradients of the loss are kept in the
        module for `_icm_update`; `rew_io` / `ids`: the rewards shaped in place."""
        return self.model.forward_rows(x, act, save=True, rew_io=rew_io, ids=ids, reward_scale=self.reward_scale,
                                       forward_loss_weight=self.forward_loss_weight, lr_scale=self.lr_scale)

    def _icm_update(self, original_stats) -> ICMTrainingStats:
        """icm.py:90-109: the backward of the graph built at preprocess time, ONE Adam step, the two losses into a pinned slot."""
        model = self.model
        head = model.head
        R = head["mse"].numel()
        w = slab_workspace(self._icm_ws, R, model.flat.device, slabs=model.flat.numel())
        model.backward(w["n_split"], slabs=w["slabs"])
        self.optim.step(w["slabs"])
        slot = result_slot(w, 2)
        ops.qmix_finalize(head["partial"], R, slot["h"])
        slot["event"].record()
        slot["event"].synchronize()
        fwd, inv = float(slot["h"][0]), float(slot["h"][1])
        if self.icm_lr_scheduler is not None:
            self.icm_lr_scheduler.step()
        wf = self.forward_loss_weight
        return ICMTrainingStats(original_stats, icm_loss=((1.0 - wf) * inv + wf * fwd) * self.lr_scale, icm_forward_loss=fwd,
                                icm_inverse_loss=inv)

    # ---- what the trainers and collectors read of an algorithm: the wrapped learner's ----------------------------------------
    @property
    def policy(self):
        return self.wrapped_algorithm.policy

    @property
    def is_within_training_step(self) -> bool:
        return self.wrapped_algorithm.is_within_training_step

    @is_within_training_step.setter
    def is_within_training_step(self, v: bool) -> None:
        self.wrapped_algorithm.is_within_training_step = v

    def __getattr__(self, name: str):
        try:
            return super().__getattr__(name)   # nn.Module: parameters, buffers, submodules
        except AttributeError:
            if name == "wrapped_algorithm":
                raise
            return getattr(self.wrapped_algorithm, name)

    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        return dict(wrapped=self.wrapped_algorithm.state_dict(), icm_model=self.model.flat.data.detach().clone().cpu(),
                    icm_optim=self.optim.state_dict())

    @torch.no_grad()
    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        self.wrapped_algorithm.load_state_dict(sd["wrapped"])
        self.model.flat.data.copy_(sd["icm_model"])
        self.optim.load_state_dict(sd["icm_optim"])


class ICMOnPolicyWrapper(_ICMMixin, nn.Module):
    """icm.py:187-261 around `PPO`, `A2C`, `Reinforce` or `GenericPPO` on the device rollout buffer."""

    def __init__(self, *, wrapped_algorithm: PPO, model: IntrinsicCuriosityModule, optim: Any, lr_scale: float,
                 reward_scale: float, forward_loss_weight: float) -> None:
        super().__init__()
        if not isinstance(wrapped_algorithm, PPO):
            raise TypeError(f"ICMOnPolicyWrapper wraps PPO, A2C, Reinforce or GenericPPO, got {type(wrapped_algorithm).__name__}")
        self._icm_init(wrapped_algorithm, model, optim, lr_scale, reward_scale, forward_loss_weight)

    def _buffer_rows(self, buffer):
        """The buffer's valid rows x agents, interleaved with their successors: -> (x [2R, D], act i64 [R], ids into
        `rew_store` or None when the rows are its first R entries).  `obs_next` comes from its store, or with
        `ignore_obs_next` through the buffer's `next` index (buffer_base.py:612-616)."""
        algo = self.wrapped_algorithm
        T, rows, _, _ = algo._valid_rows(buffer)
        S, B, N, D = buffer.sub_size, buffer.buffer_num, buffer.n_agent, buffer.obs_dim
        dev = algo.device
        if rows is None:
            rows = torch.arange(T * B, device=dev)
            ids = None
        else:
            ids = (rows[:, None] * N + torch.arange(N, device=dev)[None, :]).reshape(-1)
        slot, env = torch.div(rows, B, rounding_mode="floor"), rows % B
        obs = buffer.obs_store[slot, env]                                            # [n, N, D]
        if buffer.obs_next_store is not None:
            nxt = buffer.obs_next_store[slot, env]
        else:
            j = buffer.index.next(env * S + slot)
            nxt = buffer.obs_store[j % S, torch.div(j, S, rounding_mode="floor")]
        x = torch.stack([obs.reshape(-1, D), nxt.reshape(-1, D)], dim=1).reshape(-1, D)
        act = buffer.act_store[slot, env].reshape(-1).to(torch.int64)
        return x, act, ids

    def update(self, buffer, batch_size: int | None, repeat: int):
        """OnPolicyAlgorithm.update around the wrapper's pre- and postprocess (icm.py:236-261): the ICM forward shapes
        `rew_store` in place, so that the wrapped learner's eager and captured paths read it at the same address (quirk Q62);
        the saved rewards are copied back whatever the wrapped update does; then the ICM's one step."""
        algo = self.wrapped_algorithm
        self._refuse_grad_sync(algo)
        if not algo.is_within_training_step:
            raise RuntimeError("update() was called outside of a training step as signalled by `is_within_training_step=False`")
        if getattr(buffer, "act_dim", None) is not None:
            raise NotImplementedError("ICMOnPolicyWrapper: the ICM's forward model takes one-hot actions; Box actions are not supported")
        x, act, ids = self._buffer_rows(buffer)
        saved = buffer.rew_store.clone()
        try:
            self._icm_forward(x, act, rew_io=buffer.rew_store, ids=ids)
            stats = algo.update(buffer, batch_size, repeat)
        finally:
            buffer.rew_store.copy_(saved)   # a bit-exact copy, never a subtraction
        return self._icm_update(stats)


class ICMOffPolicyWrapper(_ICMMixin, DeviceOffPolicyRows, nn.Module):
    """icm.py:112-184 around any `DeviceOffPolicyRows` learner with discrete actions (`DQN` and its descendants,
    `DiscreteSAC`).  Usable as an agent's learner inside `MultiAgentOffPolicyAlgorithm` (`_preprocess_batch(.., agent=k)`,
    `_update_with_batch`, `_postprocess_batch`: the agent's lane of a joint-step buffer)."""

    def __init__(self, *, wrapped_algorithm: DeviceOffPolicyRows, model: IntrinsicCuriosityModule, optim: Any, lr_scale: float,
                 reward_scale: float, forward_loss_weight: float) -> None:
        super().__init__()
        if not isinstance(wrapped_algorithm, DeviceOffPolicyRows):
            raise TypeError(f"ICMOffPolicyWrapper wraps a device off-policy learner (DQN, ..), got {type(wrapped_algorithm).__name__}")
        self._icm_init(wrapped_algorithm, model, optim, lr_scale, reward_scale, forward_loss_weight)

    @property
    def lr_scheduler(self):
        return self.wrapped_algorithm.lr_scheduler

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """icm.py:161-168.  The ICM forward on the sampled rows; `batch.policy` carries orig_rew / act_hat / mse_loss.  The
        shaped reward is the batch's alone: the wrapped learner's n-step return reads the buffer's (quirk Q63), which is untouched."""
        algo = self.wrapped_algorithm
        if getattr(buffer, "act_dim", None) is not None:
            raise NotImplementedError("ICMOffPolicyWrapper: the ICM's forward model takes one-hot actions; Box actions are not supported")
        dev = algo.device
        idx = to_tensor(indices, dev, torch.int64).reshape(-1)
        k, col = algo._agent_column(buffer, agent)
        obs = buffer._gather(buffer.obs_store, idx)[:, col]
        nxt, _ = algo._successor_rows(buffer, idx, col)
        act = buffer._gather(buffer.act_store, idx)[:, col].to(torch.int64)
        orig_rew = buffer._gather(buffer.rew_store, idx)[:, k].contiguous()
        mse, act_hat = self._icm_forward(torch.stack([obs, nxt], dim=1).reshape(-1, obs.shape[-1]), act)
        batch = algo._preprocess_batch(batch, buffer, indices, agent=agent)
        batch.policy = Batch(orig_rew=orig_rew, act_hat=act_hat, mse_loss=mse)
        batch.rew = orig_rew + mse * self.reward_scale
        return batch

    def _update_with_batch(self, batch: Batch):
        return self._icm_update(self.wrapped_algorithm._update_with_batch(batch))

    def _postprocess_batch(self, batch: Batch, buffer, indices) -> None:
        """icm.py:170-177."""
        self.wrapped_algorithm._postprocess_batch(batch, buffer, indices)
        batch.rew = batch.policy.orig_rew

    def update(self, buffer, sample_size: int | None, agent: int | None = None):
        self._refuse_grad_sync(self.wrapped_algorithm)
        return DeviceOffPolicyRows.update(self, buffer, sample_size, agent=agent)
