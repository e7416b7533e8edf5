"""GAIL: PPO whose reward comes from a discriminator on [obs | one_hot(act)] rows, on the HIP path.

Mirror of tianshou/algorithm/imitation/gail.py:
  `GailTrainingStats`  :24-28    A2C's statistics plus disc_loss, acc_pi, acc_exp over the discriminator steps
  `GAIL`               :31-248   `_preprocess_batch` (`batch.rew = -logsigmoid(-disc(batch))`), the discriminator steps against
                                 the expert buffer, then PPO's update
The reference subclasses PPO.  Here `GAIL` HOLDS the learner that `PPO(...)` builds from its arguments (`PPO`, or `GenericPPO`
through `PPO.__new__`), as the ICM wrappers hold theirs: the reward is written into `rew_store` in place, at the address the
wrapped learner's eager and captured paths read, and copied back afterwards.  `PPO.__new__` dispatches on reference modules
(`policy=`) alone; `PPO(net=MLPActorCritic(..))` would put a general net under the fused 64-wide kernels, so for that engine
net `GAIL` names `GenericPPO` itself, the class a caller would name.  The discriminator is a `FlatMLP` (csrc/dense.hip)
around the row-wise kernels of csrc/gail.hip, trained through `FlatAdam`.  There is no autograd fallback.

Kept quirks and stated departures: Q64 -- the reward of an update comes from the discriminator BEFORE that
update's discriminator steps; Q65 -- `split(bsz, merge_last=True)` gives R // bsz steps, not disc_update_num; Q66 -- the action
enters one-hot (the reference concatenates `batch.act` as it is, which serves Box actions only); Q67 -- expert pairs are drawn
with replacement.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, fields
from typing import Any

import torch
from torch import nn

from .. import ops
from ..data.stats import A2CTrainingStats, SequenceSummaryStats
from ..utils.learner import result_slot
from ..utils.net import FlatMLP, MLPActorCritic
from .optim import flat_adam_of
from .ppo import PPO

_PERM_KEY = 0x4741494C5045524D   # folded into the seed of the chunk permutation: a Philox key no other draw uses


@dataclass(kw_only=True)
class GailTrainingStats(A2CTrainingStats):
    """gail.py:24-28."""

    disc_loss: SequenceSummaryStats
    acc_pi: SequenceSummaryStats
    acc_exp: SequenceSummaryStats


class GAIL(nn.Module):
    """gail.py:31-248 around `PPO` / `GenericPPO` on the device rollout buffer."""

    def __init__(self, *, policy=None, critic=None, optim=None, expert_buffer, disc_net: FlatMLP, disc_optim: Any,
                 disc_update_num: int = 4, eps_clip: float = 0.2, dual_clip: float | None = None, value_clip: bool = False,
                 advantage_normalization: bool = True, recompute_advantage: bool = False, vf_coef: float = 0.5,
                 ent_coef: float = 0.01, max_grad_norm: float | None = None, gae_lambda: float = 0.95, max_batchsize: int = 256,
                 gamma: float = 0.99, return_scaling: bool = False, **engine_kwargs) -> None:
        """The reference's arguments (gail.py:34-56) and, in `engine_kwargs`, what `PPO` takes beyond them (`net=`, `seed=`,
        `use_graph=`, `dispatch=`, ..).  `disc_net`: a `FlatMLP([obs_dim + n_act, *hidden, 1])`; `disc_optim`: an
        `AdamOptimizerFactory` or a `FlatAdam` over it; `expert_buffer`: a device buffer of discrete actions with the same
        obs_dim (its n_agent may differ: pairs are pooled)."""
        super().__init__()
        if not isinstance(disc_net, FlatMLP):
            raise TypeError("GAIL needs a utils.net.FlatMLP as disc_net: the discriminator steps run in HIP, there is no autograd "
                            f"fallback (got {type(disc_net).__name__})")
        learner = PPO   # (`net=MLPActorCritic`: see the module docstring)
        if isinstance(engine_kwargs.get("net"), MLPActorCritic):
            from .ppo_generic import GenericPPO as learner
        wrapped = learner(policy=policy, critic=critic, optim=optim, eps_clip=eps_clip, dual_clip=dual_clip, value_clip=value_clip,
                          advantage_normalization=advantage_normalization, recompute_advantage=recompute_advantage, vf_coef=vf_coef,
                          ent_coef=ent_coef, max_grad_norm=max_grad_norm, gae_lambda=gae_lambda, max_batchsize=max_batchsize,
                          gamma=gamma, return_scaling=return_scaling, **engine_kwargs)
        if wrapped.dispatch == "per_agent":
            raise NotImplementedError('GAIL: dispatch="per_agent" is not supported: the wrapped learner would be updated once per '
                                      'agent between one reward pass and one round of discriminator steps; use dispatch="pooled"')
        self._refuse_grad_sync(wrapped)
        D, A = int(wrapped.net.obs_dim), int(wrapped.net.n_act)
        ops.gail_check(D, A)
        if disc_net.dims[0] != D + A or disc_net.dims[-1] != 1:
            raise ValueError(f"GAIL: disc_net maps {disc_net.dims[0]} -> {disc_net.dims[-1]}, the discriminator takes obs_dim + n_act "
                             f"= {D + A} columns ([obs | one_hot(act)]) and gives 1 logit")
        if int(disc_update_num) < 1:
            raise ValueError(f"GAIL: disc_update_num = {disc_update_num} below 1")
        self._refuse_box(expert_buffer, "the expert buffer")
        if not all(hasattr(expert_buffer, a) for a in ("obs_store", "act_store", "index")) and len(expert_buffer) > 0:
            raise TypeError("GAIL: expert_buffer must be a device buffer (DeviceVectorReplayBuffer / VectorReplayBuffer): the "
                            f"discriminator's rows are read from its stores in place (got {type(expert_buffer).__name__})")
        if len(expert_buffer) == 0:
            raise ValueError("GAIL: the expert buffer is empty")
        if int(expert_buffer.obs_dim) != D:
            raise ValueError(f"GAIL: the expert buffer holds observations of {int(expert_buffer.obs_dim)} floats, the policy takes {D}")
        self.wrapped_algorithm = wrapped
        self.disc_net = disc_net
        self.disc_optim, self.disc_lr_scheduler = flat_adam_of(disc_optim, disc_net, "GAIL: disc_optim", True, ("factory", "flat"))
        self.disc_update_num = int(disc_update_num)
        self.expert_buffer = expert_buffer
        self.action_dim = A
        self._expert_rows: tuple | None = None
        self._gail_ws: dict = {}

    # ---- refusals ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _refuse_grad_sync(wrapped) -> None:
        if getattr(wrapped, "_grad_sync", None) is not None:
            raise NotImplementedError("GAIL: a data-parallel wrapped learner (an attached grad_sync) is not supported: the "
                                      "discriminator's gradients are not summed over the ranks")

    @staticmethod
    def _refuse_box(buffer, what: str) -> None:
        if getattr(buffer, "act_dim", None) is not None or getattr(buffer, "act_branches", None) is not None:
            raise NotImplementedError(f"GAIL: {what} holds Box or branching actions (act_dim / act_branches); the discriminator "
                                      "takes one one-hot discrete action per pair")

    # ---- the pairs -----------------------------------------------------------------------------------------------------------
    def _buffer_pairs(self, buffer):
        """The rollout buffer's valid (row, agent) pairs in the wrapped learner's row order: -> (ids i64 [R] into the stores
        viewed as [S B N], or None when they are the first R elements; R)."""
        algo = self.wrapped_algorithm
        T, rows, _, _ = algo._valid_rows(buffer)
        N = buffer.n_agent
        if rows is None:
            return None, T * buffer.buffer_num * N
        ids = (rows[:, None] * N + torch.arange(N, device=rows.device)[None, :]).reshape(-1)
        return ids, ids.numel()

    def _expert_valid_rows(self) -> torch.Tensor:
        """The expert buffer's store rows (slot * B + env) that hold data, re-derived when its length changes."""
        eb = self.expert_buffer
        n = len(eb)
        if self._expert_rows is None or self._expert_rows[0] != n:
            if n == 0:
                raise ValueError("GAIL: the expert buffer is empty")
            idx = eb.index.sample_indices_all().to(torch.int64)   # env * S + slot
            S, B = eb.sub_size, eb.buffer_num
            self._expert_rows = (n, ((idx % S) * B + torch.div(idx, S, rounding_mode="floor")).contiguous())
        return self._expert_rows[1]

    def _disc_plan(self, n_pairs: int):
        """The random choices of one update's discriminator steps: -> (perm i64 [n_pairs], the order in which the rollout's
        pairs are cut into chunks; expert pair ids i64 [steps, bsz] into the expert stores viewed as [S B N]).  Drawn on the
        device, keyed by `seed` and numbered from the discriminator optimizer's step count at the start of the update: step s
        (counted over the learner's life) owns the counters s 2^32 + i, i < bsz, of tsm_gail_draw, and the update that starts
        at step s the permutation at counter s."""
        bsz = n_pairs // self.disc_update_num
        steps = n_pairs // bsz
        dev = self.wrapped_algorithm.device
        s0, seed = self.disc_optim.step_count, self.wrapped_algorithm.seed
        perm = ops.random_permutations(n_pairs, 1, seed ^ _PERM_KEY, counter=s0, device=dev).reshape(-1)
        valid = self._expert_valid_rows()
        out = torch.empty(steps, bsz, dtype=torch.int64, device=dev)
        for k in range(steps):
            ops.gail_draw(valid, valid.numel(), self.expert_buffer.n_agent, bsz, seed, counter=(s0 + k) << 32, out=out[k])
        return perm, out

    # ---- the update ----------------------------------------------------------------------------------------------------------
    def _disc_steps(self, buffer, ids, R: int) -> dict:
        """gail.py:224-235: R // bsz optimizer steps, each on one chunk of the permuted policy pairs and bsz expert pairs; the
        three statistics of every step go to one pinned [steps, 3] slot, whose event is recorded behind the last."""
        A, eb, disc = self.action_dim, self.expert_buffer, self.disc_net
        bsz = R // self.disc_update_num
        steps = R // bsz
        perm, exp_ids = self._disc_plan(R)
        if tuple(exp_ids.shape) != (steps, bsz) or perm.numel() != R:
            raise ValueError(f"GAIL: _disc_plan must give a permutation of {R} and [{steps}, {bsz}] expert pair ids")
        pairs = perm if ids is None else ids[perm]
        w = self._gail_ws.get(R)
        if w is None:
            rows = sorted({2 * bsz, R - (steps - 1) * bsz + bsz})
            w = self._gail_ws[R] = dict(
                x=torch.empty(rows[-1], disc.dims[0], dtype=torch.float32, device=disc.flat.device),
                slabs={n: torch.empty(ops.mlp_n_split(n), disc.flat.numel(), dtype=torch.float32, device=disc.flat.device)
                       for n in rows})
        slot = result_slot(w, steps, 3)
        for k in range(steps):
            lo, hi = k * bsz, (R if k == steps - 1 else (k + 1) * bsz)   # merge_last: the remainder joins the last chunk
            Rp = hi - lo
            x = w["x"][:Rp + bsz]
            ops.gail_rows(buffer.obs_store, buffer.act_store, A, ids=pairs[lo:hi], out=x[:Rp])
            ops.gail_rows(eb.obs_store, eb.act_store, A, ids=exp_ids[k], out=x[Rp:])
            head = ops.gail_head(disc(x), Rp)
            slabs = w["slabs"][Rp + bsz]
            disc.backward(head["d_logits"], slabs.shape[0], slabs=slabs)
            self.disc_optim.step(slabs)
            ops.gail_finalize(head["partial"], Rp, bsz, out=slot["h"][k])
        slot["event"].record()
        return slot

    def update(self, buffer, batch_size: int | None, repeat: int) -> GailTrainingStats:
        """OnPolicyAlgorithm.update in the reference's order (gail.py:193-237): the discriminator of BEFORE this update rewards
        every valid pair, in `rew_store` in place; the discriminator steps; the wrapped update; the saved rewards are copied
        back whatever happened."""
        algo = self.wrapped_algorithm
        self._refuse_grad_sync(algo)
        if not algo.is_within_training_step:
            raise RuntimeError("update() was called outside of a training step as signalled by `is_within_training_step=False`")
        self._refuse_box(buffer, "the rollout buffer")
        t0 = time.time()
        ids, R = self._buffer_pairs(buffer)
        if R // self.disc_update_num == 0:
            raise ValueError(f"GAIL: {R} pairs in the rollout buffer give disc_update_num = {self.disc_update_num} chunks of 0 rows")
        saved = buffer.rew_store.clone()
        try:
            x = ops.gail_rows(buffer.obs_store, buffer.act_store, self.action_dim, ids=ids, R=R)
            ops.gail_reward(self.disc_net(x, save=False), buffer.rew_store, ids=ids)
            slot = self._disc_steps(buffer, ids, R)
            stats = algo.update(buffer, batch_size, repeat)
        finally:
            buffer.rew_store.copy_(saved)   # a bit-exact copy, never arithmetic
        if self.disc_lr_scheduler is not None:
            self.disc_lr_scheduler.step()
        slot["event"].synchronize()
        h = slot["h"].numpy().astype("float64")
        out = GailTrainingStats(**{f.name: getattr(stats, f.name) for f in fields(A2CTrainingStats)},
                                disc_loss=SequenceSummaryStats.from_sequence(h[:, 0]),
                                acc_pi=SequenceSummaryStats.from_sequence(h[:, 1]),
                                acc_exp=SequenceSummaryStats.from_sequence(h[:, 2]))
        out.train_time = time.time() - t0
        return out

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

    def create_trainer(self, params):
        from ..trainer import OnPolicyTrainer

        return OnPolicyTrainer(self, params)

    def run_training(self, params):
        return self.create_trainer(params).run()

    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = dict(wrapped=self.wrapped_algorithm.state_dict(), disc_net=self.disc_net.flat.data.detach().clone().cpu(),
                  disc_optim=self.disc_optim.state_dict())
        if self.disc_lr_scheduler is not None:   # stepped once per update: a restored run continues its schedule
            sd["disc_lr_scheduler"] = self.disc_lr_scheduler.state_dict()
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        self.wrapped_algorithm.load_state_dict(sd["wrapped"])
        self.disc_net.flat.data.copy_(sd["disc_net"])
        self.disc_optim.load_state_dict(sd["disc_optim"])
        if self.disc_lr_scheduler is not None and "disc_lr_scheduler" in sd:
            self.disc_lr_scheduler.load_state_dict(sd["disc_lr_scheduler"])
