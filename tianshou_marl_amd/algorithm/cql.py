"""CQL (arXiv:2006.04779), calibrated as Cal-QL (arXiv:2303.05479) by default: conservative Q-learning for `Box` actions
from a recorded dataset, on the HIP path.

Mirror of tianshou/algorithm/imitation/cql.py (`CQL` :32-400) on actor_critic.py's learner core with cac.py's
`ContinuousActionRows` and the entropy coefficient: SAC's actor step, the one-step soft target from the batch's own `rew`,
`done` and `obs_next`, then the conservative term.  Per critic that term needs Q at 3 B R rows beside the B data rows (R uniform
actions, R policy actions at obs, R at obs_next per transition): `tsm_cql_rows` stacks all of them into ONE row block, so each
critic runs one forward and one backward per update around the one-launch head `tsm_cql_head`; `tsm_cql_finalize` gives the
statistics and steps the Lagrange multiplier (csrc/cql.hip).  The dataset lives in a device `VectorReplayBuffer(act_dim=k)`.
There is no autograd fallback.

Kept quirks: Q70 -- the random actions are drawn by uniform_(-min_action, max_action), the constant 1
with the defaults; Q71 -- the log-sum-exp runs over the THREE entries (random, current, next) of one flat index and the mean
over B R groups (the reshape to [B, R, 1] is discarded); Q72 -- the multiplier is stepped before the critics' backward, which
still sees the old cql_alpha; Q73 -- the multiplier does move (the reference's `.to(device)` is the same tensor on the CPU).
Also as written: the actor's step and the entropy coefficient's come first, so the target and the conservative rows sample
from the MOVED actor and the target reads the new alpha; the gradients that reach the actor through the sampled actions are
dropped (the reference's policy optimizer zeroes them).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import ops
from ..data.batch import Batch
from ..utils.learner import result_slot
from ..utils.net import ContinuousCritic, FlatMLP
from ..utils.tensor import to_tensor
from .actor_critic import ActorDualCriticsOffPolicyAlgorithm, Alpha, EntropyCoefficient
from .cac import ContinuousActionRows, SACPolicy, SACTrainingStats
from .optim import AdamOptimizerFactory


@dataclass(kw_only=True)
class CQLTrainingStats(SACTrainingStats):
    cql_alpha: float | None = None
    cql_alpha_loss: float | None = None


def offline_batch_rows(algo, batch: Batch, buffer, indices, agent: int | None):
    """What an offline learner's `_preprocess_batch` gathers from the device stores (CQL, BCQ): obs, act, rew, done (terminated
    | truncated: the batch's own flag, not the n-step walk's) and obs_next of the sampled rows, read at the agent's column.
    -> (the indices i64 in HBM, the agent's reward column)."""
    idx = to_tensor(indices, algo.device, torch.int64).reshape(-1)
    k, col = algo._agent_column(buffer, agent)
    batch.obs = buffer._gather(buffer.obs_store, idx)[:, col].contiguous()
    batch.act = buffer._gather(buffer.act_store, idx)[:, col].contiguous()
    batch.rew = buffer._gather(buffer.rew_store, idx)[:, k].contiguous()
    batch.done = buffer._gather(buffer.done_store.unsqueeze(-1), idx).reshape(-1)
    batch.obs_next, _ = algo._successor_rows(buffer, idx, col)
    return idx, k


class CQL(EntropyCoefficient, ContinuousActionRows, ActorDualCriticsOffPolicyAlgorithm):
    """cql.py:32-400."""

    _policy_cls = SACPolicy
    uniform_source = None   # (rows, act_dim) -> f32 [rows, act_dim] in HBM: stands in for the Philox uniforms (tests)

    def __init__(self, *, policy: SACPolicy, policy_optim: AdamOptimizerFactory, critic: ContinuousCritic,
                 critic_optim: AdamOptimizerFactory, critic2: ContinuousCritic | None = None,
                 critic2_optim: AdamOptimizerFactory | None = None, cql_alpha_lr: float = 1e-4, cql_weight: float = 1.0,
                 tau: float = 0.005, gamma: float = 0.99, alpha: float | Alpha = 0.2, temperature: float = 1.0,
                 with_lagrange: bool = True, lagrange_threshold: float = 10.0, min_action: float = -1.0,
                 max_action: float = 1.0, num_repeat_actions: int = 10, alpha_min: float = 0.0, alpha_max: float = 1e6,
                 max_grad_norm: float = 1.0, calibrated: bool = True) -> None:
        super().__init__(policy=policy, policy_optim=policy_optim, critic=critic, critic_optim=critic_optim, critic2=critic2,
                         critic2_optim=critic2_optim, tau=tau, gamma=gamma, n_step_return_horizon=1)
        ops.cql_check(policy.act_dim, int(num_repeat_actions))
        self.critic_optim.max_grad_norm = self.critic2_optim.max_grad_norm = max_grad_norm   # cql.py:169-175
        self._init_alpha(alpha)
        self.temperature, self.with_lagrange, self.lagrange_threshold = temperature, with_lagrange, lagrange_threshold
        self.cql_weight, self.cql_alpha_lr = cql_weight, cql_alpha_lr
        self.min_action, self.max_action = min_action, max_action
        self.num_repeat_actions = int(num_repeat_actions)
        self.alpha_min, self.alpha_max = alpha_min, alpha_max
        self.max_grad_norm, self.calibrated = max_grad_norm, calibrated
        dev = self.device
        # cql_log_alpha = torch.tensor([0.0]) under torch.optim.Adam(lr=cql_alpha_lr) (cql.py:188-191), in HBM
        self.cql_log_alpha = torch.zeros(1, dtype=torch.float32, device=dev)
        self._cql_exp_avg = torch.zeros(1, dtype=torch.float32, device=dev)
        self._cql_exp_avg_sq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._cql_step = torch.zeros(1, dtype=torch.int64, device=dev)
        self._uniform_ctr = 0
        self._calib: torch.Tensor | None = None   # calibration returns in the stores' layout [S, B, N]

    # ---- the workspace: the stacked rows, and the critics' slabs for B (1 + 3 R) rows -------------------------------------
    def _slab_widths(self) -> dict:
        return dict(slabs_a=self.policy.actor.flat.numel())

    def _work(self, B: int, **slabs: int) -> dict:
        w = super()._work(B, **slabs)
        if "X" not in w:
            D, Ad, R, dev = self.policy.actor.dims[0], self.policy.act_dim, self.num_repeat_actions, self.device
            f32 = dict(dtype=torch.float32, device=dev)
            n = B + 3 * B * R
            w.update(X=torch.empty(n, D + Ad, **f32), actor_rows=torch.empty(2 * B * R, D, **f32),
                     gpow=torch.full((B,), float(self.gamma), **f32), n_split_c=ops.mlp_n_split(n))
            w.update(slabs_c1=torch.empty(w["n_split_c"], self.critic.flat.numel(), **f32),
                     slabs_c2=torch.empty(w["n_split_c"], self.critic2.flat.numel(), **f32))
        return w

    def _uniform(self, rows: int) -> torch.Tensor:
        """uniform_(-min_action, max_action) f32 [rows, act_dim] (quirk Q70): `uniform_source`'s, or `tsm_cql_uniform` at the
        learner's own Philox counter under the policy's seed."""
        Ad = self.policy.act_dim
        if self.uniform_source is not None:
            return to_tensor(self.uniform_source(rows, Ad), self.device, torch.float32).reshape(rows, Ad).contiguous()
        u = ops.cql_uniform(rows * Ad, -self.min_action, self.max_action, self.policy.seed, offset=self._uniform_ctr,
                            device=self.device).view(rows, Ad)
        self._uniform_ctr += rows * Ad
        return u

    # ---- process_buffer (cql.py:243-266) ----------------------------------------------------------------------------
    def process_buffer(self, buffer):
        """With `calibrated`: the discounted return-to-go of every stored row (compute_episodic_return with gamma,
        gae_lambda = 1 and no value estimate: the GAE scan over the buffer's rows with zero values; an unfinished tail ends
        at its last row), kept in the stores' layout and gathered per batch.  -> buffer."""
        if self.calibrated:
            S, Bn, N = buffer.sub_size, buffer.buffer_num, buffer.n_agent
            dev = self.device
            lens = buffer.index.lengths.cpu().numpy()
            start = (buffer.index.insertion_idx.cpu().numpy() - lens) % S
            zeros = torch.zeros(S, Bn * N, dtype=torch.float32, device=dev)
            ret, _ = ops.gae_lanes(zeros, zeros, buffer.rew_store.reshape(S, Bn * N), buffer.term_store.reshape(S, Bn * N),
                                   buffer.trunc_store.reshape(S, Bn * N), self.gamma, 1.0, lanes_per_env=N,
                                   env_start=torch.as_tensor(start.astype(np.int32)).to(dev),
                                   env_len=torch.as_tensor(lens.astype(np.int32)).to(dev),
                                   out=(torch.zeros_like(zeros), torch.zeros_like(zeros)))
            self._calib = ret.view(S, Bn, N)
        return buffer

    def calibration_returns(self, buffer) -> torch.Tensor:
        """`buffer.calibration_returns` of the reference: f32 by flat buffer row (sub-buffer * sub_size + slot) and reward
        column, [maxsize, N]."""
        if self._calib is None:
            raise RuntimeError("CQL: process_buffer(buffer) has not computed the calibration returns")
        return self._calib.permute(1, 0, 2).reshape(buffer.maxsize, -1)

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The sampled rows from the device stores: obs, act, rew, done (terminated | truncated: the batch's own flag, not the
        n-step walk's), obs_next and, with `calibrated`, the calibration returns."""
        idx, k = offline_batch_rows(self, batch, buffer, indices, agent)
        if self.calibrated:
            if self._calib is None:
                raise RuntimeError("CQL(calibrated=True): call process_buffer(buffer) before the first update")
            batch.calibration_returns = buffer._gather(self._calib, idx)[:, k].contiguous()
        return batch

    # ---- _update_with_batch (cql.py:268-400), in the reference's order --------------------------------------------------
    def _update_with_batch(self, batch: Batch) -> CQLTrainingStats:
        dev, actor = self.device, self.policy.actor
        if "weight" in batch:   # (CQL's losses take no importance weights)
            batch.pop("weight")
        obs, act = self._batch_rows(batch)
        B, R, (D, Ad) = obs.shape[0], self.num_repeat_actions, (obs.shape[1], self.policy.act_dim)
        BR = B * R
        w = self._work(B, **self._slab_widths())
        f = lambda x: to_tensor(x, dev, torch.float32).reshape(B, -1).contiguous()  # noqa: E731
        obs_next, rew = f(batch.obs_next), f(batch.rew).reshape(-1)
        vmask = to_tensor(batch.done, dev, torch.bool).reshape(-1).logical_not()
        calib = f(batch.calibration_returns).reshape(-1) if self.calibrated else None
        alpha_dev = self.alpha.device_scalar(dev)
        slot = result_slot(w, 3, 6)
        h = slot["h"]   # {critic1_loss, critic2_loss, cql_alpha, cql_alpha_loss, ..}, {actor_loss, mean entropy}, {alpha_loss, alpha}

        def critics(x_pi):   # each critic's value at the sampled action, then its gradient to the action columns
            q1a = FlatMLP.forward(self.critic, x_pi, save=True)
            g1 = self.critic.input_grad(w["ones"], D, Ad)
            q2a = FlatMLP.forward(self.critic2, x_pi, save=True)
            return q1a, q2a, g1, self.critic2.input_grad(w["ones"], D, Ad)

        ah = self._sac_actor_step(w, obs, act, B, critics, alpha_dev)   # 1. cql.py:275-276
        ops.qmix_finalize(ah["partial"], B, h[1])
        self._alpha_step(ah["partial"], B, h[2])                        # 2. :278-279
        # 3. the one-step target with the moved actor and the new alpha (:282-291)
        x_next = w["x_next"]
        x_next[:, :D].copy_(obs_next)
        raw = FlatMLP.forward(actor, obs_next, save=False)
        _, logp = ops.sac_action(raw, self._normal(B), actor.max_action, actor.unbounded, sigma_param=actor.sigma_param,
                                 out=x_next, col0=D)
        target = ops.cac_target(FlatMLP.forward(self.critic_old, x_next, save=False),
                                FlatMLP.forward(self.critic2_old, x_next, save=False), rew, w["gpow"], vmask, logp_next=logp,
                                alpha_dev=alpha_dev)
        # 4. the stacked rows: data, uniform actions, policy actions at obs and at obs_next (:295-319)
        X, actor_rows = ops.cql_rows(obs, obs_next, act, self._uniform(BR), R, out=w["X"], actor_rows=w["actor_rows"])
        raw = FlatMLP.forward(actor, actor_rows, save=False)
        _, logp_pi = ops.sac_action(raw, self._normal(2 * BR), actor.max_action, actor.unbounded, sigma_param=actor.sigma_param,
                                    out=X[B + BR:], col0=D)
        q1 = FlatMLP.forward(self.critic, X, save=True)
        q2 = FlatMLP.forward(self.critic2, X, save=True)
        la = self.cql_log_alpha if self.with_lagrange else None
        ch = ops.cql_head(q1, q2, target, logp_pi[:BR], logp_pi[BR:], R, Ad, calib=calib, temperature=self.temperature,
                          cql_weight=self.cql_weight, alpha_min=self.alpha_min, alpha_max=self.alpha_max, log_alpha=la)
        # 5. the statistics and the multiplier's step; the gradients above hold the cql_alpha of before it (quirk Q72)
        state = (self._cql_exp_avg, self._cql_exp_avg_sq, self._cql_step) if self.with_lagrange else (None, None, None)
        ops.cql_finalize(ch["partial"], B, R, h[0], cql_weight=self.cql_weight, lagrange_threshold=self.lagrange_threshold,
                         alpha_min=self.alpha_min, alpha_max=self.alpha_max, log_alpha=la, exp_avg=state[0], exp_avg_sq=state[1],
                         step=state[2], lr=self.cql_alpha_lr)
        # 6. one backward and one clipped Adam step per critic (:387-388)
        self.critic.backward(ch["dq1"], w["n_split_c"], slabs=w["slabs_c1"])
        self.critic_optim.step(w["slabs_c1"])
        self.critic2.backward(ch["dq2"], w["n_split_c"], slabs=w["slabs_c2"])
        self.critic2_optim.step(w["slabs_c2"])
        self._polyak()                                                  # 7. :390
        slot["event"].record()
        slot["event"].synchronize()
        lag = self.with_lagrange
        return CQLTrainingStats(actor_loss=float(h[1, 0]), critic1_loss=float(h[0, 0]), critic2_loss=float(h[0, 1]),
                                cql_alpha=float(h[0, 2]) if lag else None, cql_alpha_loss=float(h[0, 3]) if lag else None,
                                **self._alpha_stats(h[2]))

    # ---- checkpoints: the multiplier, its Adam state and the uniform draws' counter beside the core's entries -------------
    def _cql_alpha_entry(self) -> dict:
        return dict(log_alpha=self.cql_log_alpha.detach().cpu().clone(), exp_avg=self._cql_exp_avg.detach().cpu().clone(),
                    exp_avg_sq=self._cql_exp_avg_sq.detach().cpu().clone(), step=int(self._cql_step.item()))

    @torch.no_grad()
    def _load_cql_alpha_entry(self, e: dict | None) -> None:
        if e is None:
            return
        self.cql_log_alpha.copy_(torch.as_tensor(e["log_alpha"], dtype=torch.float32).reshape(1))
        self._cql_exp_avg.copy_(torch.as_tensor(e.get("exp_avg", 0.0), dtype=torch.float32).reshape(1))
        self._cql_exp_avg_sq.copy_(torch.as_tensor(e.get("exp_avg_sq", 0.0), dtype=torch.float32).reshape(1))
        self._cql_step.fill_(int(e.get("step", 0)))

    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = super().state_dict()
        sd.update(cql_alpha=self._cql_alpha_entry(), uniform_ctr=self._uniform_ctr)
        return sd

    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        super().load_state_dict(sd)
        self._load_cql_alpha_entry(sd.get("cql_alpha"))
        self._uniform_ctr = int(sd.get("uniform_ctr", 0))

    def to_reference_state_dict(self):
        """The reference's module keys, then what its module state_dict does not hold (`cql_log_alpha` is a plain tensor
        there, its optimizer and the generators live outside): the multiplier with its Adam state and both Philox counters."""
        sd = super().to_reference_state_dict()
        sd.update(cql_alpha=self._cql_alpha_entry(), sample_ctr=self.policy._sample_ctr, uniform_ctr=self._uniform_ctr)
        return sd

    def load_reference_state_dict(self, sd) -> None:
        super().load_reference_state_dict(sd)
        self._load_cql_alpha_entry(sd.get("cql_alpha"))
        self.policy._sample_ctr = int(sd.get("sample_ctr", 0))
        self._uniform_ctr = int(sd.get("uniform_ctr", 0))
