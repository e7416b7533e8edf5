"""BDQN, the Branching Dueling Q-Network (arXiv 1711.08946), on the HIP path: an action of K discrete components, K * A values.

Mirror of tianshou/algorithm/modelfree/bdqn.py:
  `BDQNPolicy`  :29-103   per-branch greedy action, one exploration coin per row
  `BDQN`        :106-224  its own 1-step return from the branch-mean target, the masked TD loss
around a `BranchingNet` (utils/net.py; common.py:557-678): a `FlatMLP` trunk and value stream (csrc/dense.hip), the K branches as
one grouped ensemble launch per layer (csrc/ensemble.hip), joined by `tsm_dueling_features` and `tsm_bdqn_combine`.  The target,
the return, the loss and the gradient with the combine's backward folded in are one launch (`tsm_bdqn_head`, csrc/bdqn.hip);
the device acting path is `tsm_bdqn_egreedy`.  The lagged network, the prioritized buffer's weight in / priority out, the
multi-agent dispatch and the statistics are `DQN`'s.  There is no autograd fallback.

Kept quirks: Q57 -- the horizon is 1 and the end flag of the return is `done | newest row of its
sub-buffer` (terminated OR truncated OR unfinished), not the `~terminated` of the n-step line; Q58 -- with
`target_update_freq = 0` the online logits are the target values; Q59 -- the priority written back is the SIGNED sum of the TD
errors over the branches; Q16 as DQN (the lagged copy precedes the step).
Not kept: Q60 -- the reference's `.squeeze()` (bdqn.py:171) collapses a batch of ONE row to [K], and line 187 then skips the
branch mean: a one-row learner batch here follows the same formulas as every other batch.  Q61 -- `rand_act += batch.obs.mask`
(bdqn.py:96-97) adds a mask to random actions; observations that carry a mask are refused.
"""
from __future__ import annotations

from typing import Any

import numpy as np
import torch

from .. import ops
from ..data.batch import Batch
from ..utils.learner import act_result, sample_counter
from ..utils.net import BranchingNet
from ..utils.tensor import to_tensor
from .dqn import DQN, DiscreteQLearningPolicy, _obs_rows


class BDQNPolicy(DiscreteQLearningPolicy):
    """bdqn.py:29-103 with a `BranchingNet`: `act` has one entry per branch, [rows, K]."""

    _model_cls = BranchingNet

    def __init__(self, *, model: BranchingNet, action_space: Any, observation_space: Any = None, eps_training: float = 0.0,
                 eps_inference: float = 0.0, seed: int = 0) -> None:
        super().__init__(model=model, action_space=action_space, observation_space=observation_space, eps_training=eps_training,
                         eps_inference=eps_inference, seed=seed)

    @staticmethod
    def _n_act_of(model, action_space: Any, atoms: int) -> int:
        """A, the actions per branch.  A space that says its size must agree: `nvec` (MultiDiscrete) = K entries of A, `n` = A."""
        K, A = model.num_branches, model.action_per_branch
        nvec, n = getattr(action_space, "nvec", None), getattr(action_space, "n", None)
        if nvec is not None and [int(x) for x in np.asarray(nvec).reshape(-1)] != [A] * K:
            raise ValueError(f"BDQNPolicy: the model has {K} branches of {A} actions, the action space nvec = {list(nvec)}")
        if nvec is None and n is not None and int(n) != A:
            raise ValueError(f"BDQNPolicy: the model has {A} actions per branch, the action space {int(n)}")
        ops.bdqn_check(K, A)
        return A

    @staticmethod
    def _unmasked(obs):
        rows, mask = _obs_rows(obs)
        if mask is not None:
            raise NotImplementedError("BDQNPolicy: observations with an action mask are not served (the reference adds the mask "
                                      "to random actions, bdqn.py:96-97)")
        return rows

    def forward(self, batch: Batch, state: Any = None, model: BranchingNet | None = None) -> Batch:
        """-> Batch(logits [B, K, A] in HBM, act = the first maximum per branch (numpy i64 [B, K]), state)."""
        net = self.model if model is None else model
        q, state = net.forward(to_tensor(self._unmasked(batch.obs), self.device, torch.float32), state=state, save=False)
        act = ops.bdqn_egreedy(q, self._zero_dev, 0)
        return Batch(logits=q, act=act.to(torch.int64).cpu().numpy(), state=state)

    def add_exploration_noise(self, act, batch):
        """bdqn.py:80-103 on the host RNG: `np.random.rand` for the row coins, `np.random.randint` for the candidates."""
        eps = self._eps()
        if np.isclose(eps, 0.0):
            return act
        if isinstance(act, np.ndarray):
            self._unmasked(batch.obs)
            bsz = len(act)
            rand_mask = np.random.rand(bsz) < eps
            rand_act = np.random.randint(low=0, high=self.model.action_per_branch, size=(bsz, act.shape[-1]))
            act[rand_mask] = rand_act[rand_mask]
            return act
        raise NotImplementedError(f"Currently only numpy arrays are supported, got {type(act)=}.")

    def act_device(self, obs: torch.Tensor, out: dict | None = None, offset_dev: torch.Tensor | None = None,
                   row_offset: int = 0, mask: torch.Tensor | None = None) -> dict:
        """obs [..., D] in HBM -> act i32 [rows, K] (tsm_bdqn_egreedy with the epsilon of the current phase); logp, value = 0.
        The Philox counter advances by one per row, as DQN's.  With `out` (a collector's buffers) K must be 1."""
        if mask is not None:
            self._unmasked(Batch(obs=obs, mask=mask))
        rows = obs.reshape(-1, self.model.dims[0])
        ctr = sample_counter(self, rows.shape[0], row_offset, offset_dev)
        q, _ = self.model.forward(rows, save=False)
        act = ops.bdqn_egreedy(q, self._eps_dev, self.seed, offset=ctr, offset_dev=offset_dev,
                               out=None if out is None else out["act"].view(-1))
        return act_result(out, act, q=q)


class BDQN(DQN):
    """bdqn.py:106-224 on the device buffer (`act_branches=K`).  One update: the online net on obs (saved) and on obs_next,
    the lagged net on obs_next, `tsm_bdqn_head`, the backward, one `FlatAdam` step."""

    def __init__(self, *, policy: BDQNPolicy, optim: Any, gamma: float = 0.99, target_update_freq: int = 0,
                 is_double: bool = True) -> None:
        if not isinstance(policy, BDQNPolicy):
            raise TypeError(f"BDQN needs a BDQNPolicy, got {type(policy).__name__}")
        # BDQN forms its own return (below), which supports only 1-step returns
        super().__init__(policy=policy, optim=optim, gamma=gamma, n_step_return_horizon=1, target_update_freq=target_update_freq,
                         is_double=is_double)

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The sampled rows from the device stores, the end flag `done | newest row of its sub-buffer` (bdqn.py:184-186; every
        sub-buffer's newest row is its `last_index`) and the networks on obs_next.  The return is formed by the head, in
        `_update_with_batch`."""
        dev = self.device
        idx = to_tensor(indices, dev, torch.int64).reshape(-1)
        if len(batch.get_keys()) != 0 and len(batch) != idx.numel():
            raise ValueError(f"Batch size {len(batch)} and indices size {idx.numel()} mismatch.")
        K = self.policy.model.num_branches
        if getattr(buffer, "aec", False) or getattr(buffer, "act_branches", None) != K:
            raise ValueError(f"BDQN: the buffer must be a joint-step buffer built with act_branches={K}")
        k, col = self._agent_column(buffer, agent)
        batch.obs = buffer._gather(buffer.obs_store, idx)[:, col].contiguous()
        batch.act = buffer._gather(buffer.act_store, idx)[:, col].contiguous()
        batch.rew = buffer._gather(buffer.rew_store, idx)[:, k].contiguous()
        done = buffer._gather(buffer.done_store.unsqueeze(-1), idx).view(-1)
        batch.end = ((done != 0) | (idx == buffer.index.last_index[idx // buffer.sub_size])).to(torch.uint8)
        nxt, _ = self._successor_rows(buffer, idx, col)
        batch.q_next_online, _ = self.policy.model.forward(nxt, save=False)
        if self.use_target_network:
            batch.q_next_target, _ = self.model_old.forward(nxt, save=False)
        return batch

    def _online_forward(self, batch: Batch, x: torch.Tensor) -> torch.Tensor:
        return self.policy.model.forward(x, save=True)[0]

    def _head(self, batch: Batch, q, act, weight):
        B, K = q.shape[0], q.shape[1]
        head = ops.bdqn_head(q, batch.q_next_online, batch.get("q_next_target"), act.reshape(B, K).to(torch.int32),
                             to_tensor(batch.rew, self.device, torch.float32), to_tensor(batch.end, self.device, torch.uint8),
                             self.gamma, weight=weight, is_double=self.is_double)
        return (head["d_adv"], head["d_v"]), head["partial"], head["returns"], head["prio"]
