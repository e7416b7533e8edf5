"""IQN (implicit quantile network over QR-DQN's n-step / prioritized-replay / dispatch machinery) on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelfree/iqn.py (`IQNPolicy` :21-100, `IQN` :103-183) around
`ImplicitQuantileNetwork` (utils/net/discrete.py:164-217).  The Q-network is an `ImplicitQuantileNet` (utils/net.py): two
`FlatMLP`s around the cosine embedding of csrc/iqn.hip, one flat parameter vector.  A network row is (b, s), so the net's
output is [B * S, A]; `Batch.logits` is its [B, A, S] view.  `tsm_iqn_values` reduces it to one value per action,
`tsm_iqn_head` forms the target, the loss over per-row fractions and its gradient in one launch.  Acting is `tsm_dqn_egreedy`
on those values.  There is no autograd fallback.

Kept quirks: Q21 / Q22 as QR-DQN (a* and the next distribution at idx_n, before the lagged copy; no
`is_double`); Q29 -- the number of fractions depends on the call: `target_sample_size` when a lagged model is passed, else
`online_sample_size` in torch training mode, else `sample_size`; Q30 -- without a target network the next distribution is
the online forward that chose a*, so N' is that forward's count; Q31 -- every forward draws fresh fractions: three draws
per update with a target network (online and lagged on the successor rows, online on the sampled rows), two without;
Q32 -- `tau_hat` for `num_quantiles` leads the state dict and the loss never reads it.
"""
from __future__ import annotations

from typing import Any

import torch

from .. import ops
from ..data.batch import Batch
from ..utils.net import ImplicitQuantileNet
from ..utils.tensor import to_tensor
from .distq import QRDQN, QRDQNPolicy
from .dqn import DiscreteQLearningPolicy

_UPDATE_STREAM = 0x9E3779B97F4A7C15   # added to the seed for the learner's draws: acting and updating never share fractions


class IQNPolicy(QRDQNPolicy):
    """iqn.py:21-100 with an `ImplicitQuantileNet` Q-network."""

    _model_cls = ImplicitQuantileNet

    def __init__(self, *, model: ImplicitQuantileNet, action_space: Any, sample_size: int = 32, online_sample_size: int = 8,
                 target_sample_size: int = 8, observation_space: Any = None, eps_training: float = 0.0,
                 eps_inference: float = 0.0, seed: int = 0) -> None:
        assert sample_size > 1, f"sample_size should be greater than 1 but got: {sample_size}"
        assert online_sample_size > 1, f"online_sample_size should be greater than 1 but got: {online_sample_size}"
        assert target_sample_size > 1, f"target_sample_size should be greater than 1 but got: {target_sample_size}"
        if isinstance(model, ImplicitQuantileNet):
            for s in (sample_size, online_sample_size, target_sample_size):
                ops.iqn_check(model.num_cosines, model.embedding_dim, int(s), model.n_act)
        # the net emits one number per action and fraction: QR-DQN's fixed count does not apply
        DiscreteQLearningPolicy.__init__(self, model=model, action_space=action_space, observation_space=observation_space,
                                         eps_training=eps_training, eps_inference=eps_inference, seed=seed, atoms=1)
        self.sample_size, self.online_sample_size = int(sample_size), int(online_sample_size)
        self.target_sample_size = int(target_sample_size)
        self.n_atoms = self.num_quantiles = None
        self._tau_ctr = 0
        # fractions to use for the coming forwards of the learner, in call order, in place of device draws (parity tests
        # feed the reference's recorded draws; a replayed update feeds its own)
        self.tau_feed: list = []

    def _sample_count(self, is_model_old: bool) -> int:
        """iqn.py:79-85 (quirk Q29)."""
        if is_model_old:
            return self.target_sample_size
        return self.online_sample_size if self.training else self.sample_size

    def net_forward(self, rows: torch.Tensor, model: ImplicitQuantileNet | None = None, save: bool = False):
        """One forward of the learner's: -> (out [R * S, A], taus [R, S], S).  Fractions come from `tau_feed` when it holds
        any, else from the policy's update stream of device draws."""
        S = self._sample_count(model is not None)
        net = self.model if model is None else model
        taus = None
        if self.tau_feed:
            taus = to_tensor(self.tau_feed.pop(0), self.device, torch.float32)
        R = rows.reshape(-1, net.dims[0]).shape[0]
        out, taus = net.forward(rows, S, taus=taus, save=save, seed=(self.seed + _UPDATE_STREAM) & (2**64 - 1),
                                offset=self._tau_ctr)
        self._tau_ctr += R
        return out, taus, S

    def values(self, out: torch.Tensor, sample_size: int) -> torch.Tensor:  # type: ignore[override]
        """out [R * S, A] (or [R, S, A]) in HBM -> the mean over the fractions [R, A], before the mask."""
        return ops.iqn_values(out, sample_size, self.n_act)

    def compute_q_value(self, logits: torch.Tensor, mask) -> torch.Tensor:
        """qrdqn.py:19-20 on `Batch.logits` [R, A, S], then dqn.py:145-151."""
        logits = to_tensor(logits, self.device, torch.float32)
        if logits.dim() != 3 or logits.shape[1] != self.n_act:
            raise ValueError(f"IQNPolicy.compute_q_value: logits must be [R, {self.n_act}, S]")
        q = self.values(logits.transpose(1, 2).contiguous(), logits.shape[2])
        return DiscreteQLearningPolicy.compute_q_value(self, q, mask)

    def _forward_values(self, x: torch.Tensor, model):
        """`Batch.logits` is the [B, A, S] view of the net's output; the Batch also carries `taus`."""
        out, taus, S = self.net_forward(x, model=model)
        return self.values(out, S), out.view(-1, S, self.n_act).transpose(1, 2), dict(taus=taus)

    def _act_values(self, rows: torch.Tensor, ctr: int, offset_dev) -> torch.Tensor:
        """The net under fresh fractions: tsm_iqn_taus at the counter the epsilon draw uses, under its own key."""
        S = self._sample_count(False)
        o, _ = self.model.forward(rows, S, save=False, seed=self.seed, offset=ctr, offset_dev=offset_dev)
        return self.values(o, S)


class IQN(QRDQN):
    """iqn.py:103-183 on the device buffer."""

    _policy_cls = IQNPolicy

    def __init__(self, *, policy: IQNPolicy, optim: Any, gamma: float = 0.99, num_quantiles: int = 200,
                 n_step_return_horizon: int = 1, target_update_freq: int = 0) -> None:
        super().__init__(policy=policy, optim=optim, gamma=gamma, num_quantiles=num_quantiles,
                         n_step_return_horizon=n_step_return_horizon, target_update_freq=target_update_freq)

    @staticmethod
    def _check_quantiles(policy, num_quantiles: int) -> None:
        """The net emits as many quantiles as fractions are drawn; `num_quantiles` only sizes `tau_hat` (quirk Q32)."""

    def _next_forwards(self, batch: Batch) -> None:
        """qrdqn.py:94-106 with iqn.py's forwards: the online net on the successor rows under its own draw (a* from the mean
        over those fractions), then the lagged net under another; without one the online forward is the next distribution
        (quirks Q30, Q31)."""
        pol = self.policy
        A = pol.n_act
        out_on, _, s_on = pol.net_forward(batch.rows_next)
        batch.q_next_online = pol.values(out_on, s_on)
        if self.use_target_network:
            out_tg, _, s_tg = pol.net_forward(batch.rows_next, model=self.model_old)
            batch.out_next = out_tg.view(-1, s_tg, A)
        else:
            batch.out_next = out_on.view(-1, s_on, A)

    def _online_forward(self, batch: Batch, x: torch.Tensor) -> torch.Tensor:
        out, batch.taus, _ = self.policy.net_forward(x, save=True)
        return out

    def _head(self, batch: Batch, q, act, weight):
        N = batch.taus.shape[1]
        head = ops.iqn_head(q.view(-1, N, self.policy.n_act), batch.q_next_online, batch.out_next, batch.taus, act, batch.mc,
                            batch.gpow, batch.vmask, mask_next=batch.get("mask_next"), weight=weight)
        return head["d_out"], head["partial"], head["returns"], head["prio"]

    # ---- checkpoints ---------------------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = super().state_dict(*args, **kwargs)
        sd["tau_ctr"] = self.policy._tau_ctr
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        super().load_state_dict(sd, *args, **kwargs)
        self.policy._tau_ctr = int(sd.get("tau_ctr", 0))
