"""FQF (fully parameterized quantile function over QR-DQN's n-step / prioritized-replay / dispatch machinery) on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelfree/fqf.py (`FQFPolicy` :27-106, `FQF` :109-256) around
`FractionProposalNetwork` and `FullQuantileFunction` (utils/net/discrete.py:220-315).  The Q-network is a `FullQuantileNet`,
the fraction model a `FractionProposalNet` (utils/net.py), each one flat parameter vector under an optimizer of its own.  A
network row is (b, i), so the net's output is [B * N, A]; `Batch.logits` is its [B, A, N] view.  `tsm_fqf_propose` decides
where the quantile function is evaluated, `tsm_fqf_values` weighs the quantiles by the fractions' widths, `tsm_fqf_head` forms
the target, both losses and both gradients in one launch.  Acting is `tsm_dqn_egreedy` on those values.  There is no autograd
fallback.

Kept quirks: Q33 -- the lagged net is evaluated at the ONLINE proposal's fractions on the successor rows;
there is no lagged fraction model; Q34 -- without a target network the online forward that chose a* is the next distribution;
Q35 -- a* comes from the fraction-weighted values of the online net, there is no `is_double`; Q36 -- `quantiles_tau` exists
only in torch training mode, and an update outside it raises; Q37 -- the fraction loss ignores the importance weights;
Q38 -- `taus[:, -1]` is what the cumulative sum gives, not 1; Q39 -- `num_fractions` of `FQF` only sizes `tau_hat` (as Q32): the
fraction model's own count decides every shape.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from .. import ops
from ..data.batch import Batch
from ..utils.net import FractionProposalNet, FullQuantileNet
from ..utils.tensor import to_tensor
from .actor_critic import _Schedulers
from .distq import QRDQN, QRDQNPolicy
from .dqn import DiscreteQLearningPolicy, SimpleLossTrainingStats, _obs_rows
from .optim import flat_adam_of


@dataclass(kw_only=True)
class FQFTrainingStats(SimpleLossTrainingStats):
    """fqf.py:20-24; `loss` = quantile_loss + (fraction_loss - ent_coef * entropy_loss)."""
    quantile_loss: float
    fraction_loss: float
    entropy_loss: float


class FQFPolicy(QRDQNPolicy):
    """fqf.py:27-106 with a `FullQuantileNet` Q-network and a `FractionProposalNet`."""

    _model_cls = FullQuantileNet

    def __init__(self, *, model: FullQuantileNet, fraction_model: FractionProposalNet, action_space: Any,
                 observation_space: Any = None, eps_training: float = 0.0, eps_inference: float = 0.0, seed: int = 0) -> None:
        if not isinstance(fraction_model, FractionProposalNet):
            raise TypeError(f"FQFPolicy needs a FractionProposalNet fraction model: the proposal runs in HIP, there is no "
                            f"autograd fallback (got {type(fraction_model).__name__})")
        # the net emits one number per action and fraction: QR-DQN's fixed count does not apply
        DiscreteQLearningPolicy.__init__(self, model=model, action_space=action_space, observation_space=observation_space,
                                         eps_training=eps_training, eps_inference=eps_inference, seed=seed, atoms=1)
        if fraction_model.embedding_dim != model.embedding_dim or fraction_model.feature_act != model.feature_act:
            raise ValueError(f"FQFPolicy: the fraction model reads features of width {fraction_model.embedding_dim} "
                             f"(feature_act={fraction_model.feature_act}), the model's preprocess net emits "
                             f"{model.embedding_dim} (feature_act={model.feature_act})")
        if fraction_model.flat.device != model.flat.device:
            raise ValueError("FQFPolicy: model and fraction model must live on one device")
        ops.fqf_check(fraction_model.num_fractions, model.embedding_dim, model.n_act)
        self.fraction_model = fraction_model
        self.n_atoms = self.num_quantiles = None

    def net_forward(self, rows: torch.Tensor, model: FullQuantileNet | None = None, fractions: Batch | None = None,
                    save: bool = False, training: bool = False):
        """One forward of the learner's: -> (out [R * N, A], fractions, out_tau [R * (N - 1), A] or None)."""
        net = self.model if model is None else model
        return net.forward(rows, self.fraction_model, fractions=fractions, save=save, training=training)

    def values(self, out: torch.Tensor, taus: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        """out [R * N, A] (or [R, N, A]) and taus [R, N + 1] in HBM -> the fraction-weighted sum [R, A], before the mask."""
        return ops.fqf_values(out, taus, self.n_act)

    def compute_q_value(self, logits: torch.Tensor, mask, fractions: Batch | None = None) -> torch.Tensor:  # type: ignore[override]
        """fqf.py:94-97 on `Batch.logits` [R, A, N] with the `Batch.fractions` they were evaluated at, then dqn.py:145-151."""
        if fractions is None:
            raise ValueError("FQFPolicy.compute_q_value: the value of FQF logits is defined by their fractions; pass "
                             "`fractions` (the Batch that `forward` returned with them)")
        logits = to_tensor(logits, self.device, torch.float32)
        if logits.dim() != 3 or logits.shape[1] != self.n_act:
            raise ValueError(f"FQFPolicy.compute_q_value: logits must be [R, {self.n_act}, N]")
        q = self.values(logits.transpose(1, 2).contiguous(), to_tensor(fractions.taus, self.device, torch.float32))
        return DiscreteQLearningPolicy.compute_q_value(self, q, mask)

    def forward(self, batch: Batch, state: Any = None, model: FullQuantileNet | None = None,  # type: ignore[override]
                fractions: Batch | None = None, **kwargs: Any) -> Batch:
        """-> Batch(logits [B, A, N] view in HBM, act (numpy i64), state, fractions, quantiles_tau [B, A, N - 1] view in torch
        training mode of the online model, else None)."""
        obs, mask = _obs_rows(batch.obs)
        x = to_tensor(obs, self.device, torch.float32)
        out, fractions, out_tau = self.net_forward(x, model=model, fractions=fractions,
                                                   training=model is None and self.model.training)
        A, N = self.n_act, fractions.tau_hats.shape[1]
        q = self.values(out, fractions.taus)
        m = None if mask is None else to_tensor(np.asarray(mask, bool) if not isinstance(mask, torch.Tensor) else mask,
                                                 self.device, torch.uint8).reshape(q.shape)
        act = ops.dqn_egreedy(q, self._zero_dev, 0, mask=m)
        return Batch(logits=out.view(-1, N, A).transpose(1, 2), act=act.to(torch.int64).cpu().numpy(), state=state,
                     fractions=fractions,
                     quantiles_tau=None if out_tau is None else out_tau.view(-1, N - 1, A).transpose(1, 2))

    def _act_values(self, rows: torch.Tensor, ctr: int, offset_dev) -> torch.Tensor:
        """Features, proposal, embedding at tau_hats, `last`, the weighted sum: no interior forward when acting."""
        out, fractions, _ = self.net_forward(rows)
        return self.values(out, fractions.taus)


class FQF(QRDQN):
    """fqf.py:109-256 on the device buffer.  `optim` steps the quantile model's flat vector only (fqf.py:173-176),
    `fraction_optim` the fraction model's."""

    _policy_cls = FQFPolicy
    _n_results = 4

    def __init__(self, *, policy: FQFPolicy, optim: Any, fraction_optim: Any, gamma: float = 0.99, num_fractions: int = 32,
                 ent_coef: float = 0.0, n_step_return_horizon: int = 1, target_update_freq: int = 0) -> None:
        super().__init__(policy=policy, optim=optim, gamma=gamma, num_quantiles=num_fractions,
                         n_step_return_horizon=n_step_return_horizon, target_update_freq=target_update_freq)
        self.ent_coef = ent_coef
        self.fraction_optim, sched = flat_adam_of(fraction_optim, policy.fraction_model, "FQF: fraction_optim", True,
                                                  ("factory", "flat"))
        if sched is not None:
            self.lr_scheduler = _Schedulers([s for s in (self.lr_scheduler, sched) if s is not None])

    @staticmethod
    def _check_quantiles(policy, num_quantiles: int) -> None:
        """`num_fractions` only sizes `tau_hat` (quirk Q39)."""

    def _next_forwards(self, batch: Batch) -> None:
        """fqf.py:178-193: the online net on the successor rows at its own proposal (a* from the weighted values), then the
        lagged net at those same fractions; without one the online forward is the next distribution (quirks Q33 - Q35)."""
        pol = self.policy
        out_on, fractions, _ = pol.net_forward(batch.rows_next)
        batch.q_next_online = pol.values(out_on, fractions.taus)
        if self.use_target_network:
            out_on, _, _ = pol.net_forward(batch.rows_next, model=self.model_old, fractions=fractions)
        batch.out_next = out_on.view(-1, fractions.tau_hats.shape[1], pol.n_act)

    def _update_with_batch(self, batch: Batch) -> FQFTrainingStats:
        if not self.policy.model.training:   # before the lagged copy, `_iter` and `batch.weight` are touched
            raise RuntimeError("FQF: the update needs `quantiles_tau`, which the model computes only in torch training mode "
                               "(quirk Q36); call .train() on the algorithm or its policy before updating")
        return super()._update_with_batch(batch)

    def _online_forward(self, batch: Batch, x: torch.Tensor) -> torch.Tensor:
        out, batch.fractions, batch.quantiles_tau = self.policy.net_forward(x, save=True, training=True)
        return out

    def _head(self, batch: Batch, q, act, weight):
        fr, A = batch.fractions, self.policy.n_act
        N = fr.tau_hats.shape[1]
        head = ops.fqf_head(q.view(-1, N, A), batch.quantiles_tau.view(-1, N - 1, A), batch.q_next_online, batch.out_next,
                            fr.taus, fr.tau_hats, fr.logp, fr.entropies, act, batch.mc, batch.gpow, batch.vmask,
                            mask_next=batch.get("mask_next"), weight=weight, ent_coef=self.ent_coef)
        batch.d_logits, batch.partial_frac = head["d_logits"], head["partial_frac"]
        return head["d_out"], head["partial"], head["returns"], head["prio"]

    def _slab_widths(self) -> dict:
        return dict(super()._slab_widths(), frac_slabs=self.policy.fraction_model.flat.numel())

    def _before_step(self, batch: Batch, w: dict) -> None:
        """Both gradients exist before either step; the fraction model steps first, as fqf.py:248-249."""
        self.policy.fraction_model.backward(batch.pop("d_logits"), w["n_split"], slabs=w["frac_slabs"])
        self.fraction_optim.step(w["frac_slabs"])

    def _finalize(self, batch: Batch, partial, B: int, h) -> None:
        """h = {quantile loss, mean q, fraction loss, entropy loss}."""
        ops.qmix_finalize(partial, B, h[:2])
        ops.qmix_finalize(batch.pop("partial_frac"), B, h[2:])

    def _stats_of(self, h) -> FQFTrainingStats:
        quantile, fraction, entropy = float(h[0]), float(h[2]), float(h[3])
        return FQFTrainingStats(loss=quantile + (fraction - self.ent_coef * entropy), quantile_loss=quantile,
                                fraction_loss=fraction, entropy_loss=entropy)

    # ---- checkpoints ---------------------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = super().state_dict(*args, **kwargs)
        sd["fraction_model"] = self.policy.fraction_model.flat.data.detach().clone().cpu()
        sd["fraction_optim"] = self.fraction_optim.state_dict()
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        super().load_state_dict(sd, *args, **kwargs)
        self.policy.fraction_model.flat.data.copy_(sd["fraction_model"])
        self.fraction_optim.load_state_dict(sd["fraction_optim"])

    def _ref_nets(self) -> list:
        """`policy.model.`, `policy.fraction_model.`, then `model_old.module.` with a target network."""
        nets = super()._ref_nets()
        return nets[:1] + [("policy.fraction_model.", self.policy.fraction_model)] + nets[1:]
