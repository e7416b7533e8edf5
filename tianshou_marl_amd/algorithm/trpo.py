"""TRPO -- trust region policy optimisation (/root/reference/tianshou/algorithm/modelfree/trpo.py) on NPG's device-side
conjugate gradients: the gradient is of -mean(ratio adv), the step size sqrt(2 max_kl / (x F x + damping x.x)) comes from one
more tangent + Fisher-head pass on the solution, and the backtracking line search (trpo.py:162-191) runs on the device --
`max_backtracks` predicated trials (`tsm_flat_axpy_dev`, `tsm_mlp_forward_cond`, `tsm_categorical_kl_surrogate`,
`tsm_trpo_accept`) with ONE host read per minibatch, after the critic's steps have been queued.  A search that fails leaves the
parameters at the last trial and reports step_size 0, as the reference does (its line 186 writes new_flat_params)."""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import torch

from .. import ops
from ..data.stats import SequenceSummaryStats
from ..utils.net import MLPActorCritic
from .npg import NPG, NPGTrainingStats


@dataclass(kw_only=True)
class TRPOTrainingStats(NPGTrainingStats):
    step_size: SequenceSummaryStats


class TRPO(NPG):
    """trpo.py:23-214 with the reference's constructor arguments (`policy=, critic=, optim=`) or `net=MLPActorCritic`."""

    _stats_cls, _stat_names = TRPOTrainingStats, ("actor_loss", "vf_loss", "kl", "step_size")
    _loss_kind = "ratio"  # -mean(exp(logp - logp_old) adv)

    def __init__(self, *, policy=None, critic=None, optim=None, max_kl: float = 0.01, backtrack_coeff: float = 0.8,
                 max_backtracks: int = 10, optim_critic_iters: int = 5, trust_region_size: float = 0.5,
                 advantage_normalization: bool = True, gae_lambda: float = 0.95, max_batchsize: int = 256, gamma: float = 0.99,
                 return_scaling: bool = False, net: MLPActorCritic | None = None, **kw) -> None:
        super().__init__(policy=policy, critic=critic, optim=optim, optim_critic_iters=optim_critic_iters,
                         trust_region_size=trust_region_size, advantage_normalization=advantage_normalization,
                         gae_lambda=gae_lambda, max_batchsize=max_batchsize, gamma=gamma, return_scaling=return_scaling, net=net, **kw)
        if max_backtracks < 1:
            raise ValueError(f"TRPO: max_backtracks = {max_backtracks} must be >= 1")
        self.max_kl, self.backtrack_coeff, self.max_backtracks = float(max_kl), float(backtrack_coeff), int(max_backtracks)
        self._ctor.update(max_kl=max_kl, backtrack_coeff=backtrack_coeff, max_backtracks=max_backtracks)

    def _actor_step(self, mb: dict, st: dict) -> None:
        actor, B = self.net.actor, mb["B"]
        x_in, acts = actor._saved_forward()
        # x F x from one more tangent + head pass, on the solution (trpo.py:153-160); its J^T product is not needed
        jv, st["fvp"]["t_acts"] = ops.mlp_tangent_forward(actor.desc, actor.flat.data, st["x"], x_in, acts, st["fvp"]["t_acts"])
        _, head = ops.fisher_head(mb["logits"], jv, st["fvp"]["u"], st["fvp"]["partial"])
        w = self._ws.get(("trpo", B))   # the search's buffers, kept like the CG's: the old parameters, the trials' activations
        if w is None:                    # and partials, the search state
            w = self._ws[("trpo", B)] = dict(old=torch.empty_like(actor.flat.data), part=torch.zeros_like(mb["part0"]), ls=None,
                                             run=None, acts=torch.empty_like(acts))
        w["ls"], w["run"] = ls, run = ops.trpo_step_size(head, st["x"], mb["part0"], B, self._damping, self.max_kl, w["ls"], w["run"])
        old = w["old"].copy_(actor.flat.data)
        for i in range(self.max_backtracks):   # new_flat_params = flat_params + step_size * (-x), while `run`
            ops.flat_axpy_dev(old, st["x"], -1.0, scale_dev=ls[0:1], run_if=run, out=actor.flat.data)
            new_logits, _ = ops.mlp_forward_cond(actor.desc, actor.flat.data, mb["x"], run, acts=w["acts"])
            ops.categorical_kl_surrogate(mb["logits"], new_logits, mb["act"], mb["logp_old"], mb["adv"], "ratio",
                                         partial=w["part"], run_if=run)
            ops.trpo_accept(w["part"], B, i, self.max_backtracks, self.max_kl, self.backtrack_coeff, ls, run, mb["out"][0:4])

    def _read_stats(self, o: np.ndarray) -> list[float]:
        if o[3] < 0:
            warnings.warn("Line search failed! It seems hyperparamters are poor and need to be changed.")
        elif o[3] > 0:
            warnings.warn(f"Backtracking to step {int(o[3])}.")
        return [float(o[0]), float(o[6]), float(o[1]), float(o[2])]
