"""NPG -- natural policy gradient (/root/reference/tianshou/algorithm/modelfree/npg.py) for categorical policies on
`MLPActorCritic`, without autograd.

The reference solves (F + 0.1 I) x = g by ten conjugate-gradient iterations per minibatch, F v being the second derivative of
mean KL(old || new) through autograd twice (npg.py:195-224).  Here F v = J^T M (J v) / B runs on csrc/fisher.hip and
csrc/dense.hip -- a tangent forward pass, the Fisher head, `tsm_mlp_backward` -- and the CG vectors, scalars and the break
decision stay on the device (`ops.cg_*`): the host queues the ten iterations and reads nothing.

    preprocess   GAE as A2C, logp_old from the current actor (`GenericPPO._preprocess_batch`); the advantages are normalised
                 over the WHOLE batch the update is handed, with the unbiased std (npg.py:136-137) -- under per-agent dispatch
                 that is one agent's rows (marl.py:208-249)
    minibatch    g = d(-mean(logp adv)); x = CG(g), nsteps 10, residual_tol 1e-10, damping 0.1;
                 theta <- theta - trust_region_size x; kl after the step; optim_critic_iters critic-only Adam steps on
                 mse(returns, V)  (npg.py:149-187).  The optimizer holds the critic alone (`optim_include_actor=False`).

Not built: Gaussian policies, action masks, recurrent actors, data-parallel replicas, a captured-graph update (DESIGN.md
section 9).
"""
from __future__ import annotations

import time
from dataclasses import dataclass

import numpy as np
import torch

from .. import ops
from ..data.batch import Batch, split_bounds
from ..data.stats import MapTrainingStats, SequenceSummaryStats, TrainingStats
from ..utils.net import FlatAdam, MLPActorCritic
from ..utils.tensor import to_tensor
from .ppo_generic import GenericPPO


@dataclass(kw_only=True)
class NPGTrainingStats(TrainingStats):
    actor_loss: SequenceSummaryStats
    vf_loss: SequenceSummaryStats
    kl: SequenceSummaryStats


class NPG(GenericPPO):
    """npg.py:27-236 with the reference's constructor arguments (`policy=, critic=, optim=`) or `net=MLPActorCritic`."""

    _fixed = ("eps_clip", "dual_clip", "value_clip", "recompute_advantage", "vf_coef", "ent_coef", "max_grad_norm", "use_graph")
    _stats_cls, _stat_names = NPGTrainingStats, ("actor_loss", "vf_loss", "kl")
    _loss_kind = "logp"   # the actor loss of `ops.categorical_kl_surrogate`: -mean(logp adv)
    _gaussian_ok = False  # the Fisher head and the KL surrogate are categorical: a GaussianActorCritic is refused by name

    def __init__(self, *, policy=None, critic=None, optim=None, optim_critic_iters: int = 5, trust_region_size: float = 0.5,
                 advantage_normalization: bool = True, gae_lambda: float = 0.95, max_batchsize: int = 256, gamma: float = 0.99,
                 return_scaling: bool = False, net: MLPActorCritic | None = None, **kw) -> None:
        for banned in self._fixed:
            if banned in kw:
                raise TypeError(f"{type(self).__name__} has no `{banned}` (that is a PPO option)")
        kw.update(graph=False, fused_actor=False)  # the update is this class's own launch sequence, on the dense kernels
        super().__init__(policy=policy, critic=critic, optim=optim, net=net, advantage_normalization=advantage_normalization,
                         gae_lambda=gae_lambda, max_batchsize=max_batchsize, gamma=gamma, return_scaling=return_scaling,
                         recompute_advantage=False, value_clip=False, dual_clip=None, vf_coef=1.0, ent_coef=0.0,
                         max_grad_norm=None, **kw)
        net = self.net
        if net.n_act > 64:
            raise ValueError(f"{type(self).__name__}: n_act = {net.n_act} above the 64 of the categorical kernels")
        self.optim_critic_iters, self.trust_region_size = int(optim_critic_iters), float(trust_region_size)
        self._damping = 0.1
        self._cfg_mse = ops.make_ppo_cfg(adv_norm=False, vf_coef=1.0, ent_coef=0.0, loss_kind=2)
        self._ctor.update(optim_critic_iters=optim_critic_iters, trust_region_size=trust_region_size)

    def _make_optim(self, net, lr: float, betas, adam_eps: float, weight_decay: float, max_grad_norm) -> FlatAdam:
        """optim_include_actor=False (npg.py:111): Adam's state, and the `_optimizers` entry of a checkpoint, cover the critic's
        segment alone.  (LR schedulers set `self.lr`, which reads and writes whatever `self.optim` is.)"""
        return FlatAdam(net.critic, lr, betas, adam_eps, weight_decay, None,
                        views=lambda flat: [v for _, v in net.critic.reference_named_views(flat)])

    # ---- the update ----------------------------------------------------------------------------------------------------
    def _update(self, buffer, batch_size: int | None, repeat: int, t0: float):
        pb = self._preprocess_batch(buffer)
        if self.dispatch != "per_agent":
            return self._update_with_batch(pb, batch_size, repeat, buffer=buffer)
        per_agent = {}
        for a in range(buffer.n_agent):  # MARLDispatcher.dispatch_update_with_batch (marl.py:251-268)
            st = self._update_with_batch(pb, batch_size, repeat, agent=a, buffer=buffer)
            st.train_time = time.time() - t0
            per_agent[f"agent_{a}"] = st
        return MapTrainingStats(per_agent)

    def _normalized_adv(self, pb: dict, ids: torch.Tensor) -> torch.Tensor:
        """npg.py:136-137 over the rows `ids` of the batch: (adv - mean) / unbiased std, no epsilon."""
        if not self.advantage_normalization:
            return pb["adv"]
        mb = torch.tensor([0, ids.numel()], dtype=torch.int64, device=self.device)
        st = ops.ppo_adv_stats(pb["adv"], mb, perm=ids)[0]
        out = pb["adv"].clone()
        out[ids] = (pb["adv"][ids] - st[0]) / st[1]
        return out

    def _update_with_batch(self, pb: dict, batch_size: int | None, repeat: int, agent: int | None = None, buffer=None,
                           perm_base: int | None = None):
        if self._grad_sync is not None:
            raise NotImplementedError(f"{type(self).__name__} has no data-parallel update")
        dev = self.device
        ids = self._sample_ids(pb, agent)
        if ids is None:
            ids = torch.arange(pb["obs"].shape[0], dtype=torch.int64, device=dev)
        n = ids.numel()
        adv = self._normalized_adv(pb, ids)
        bounds = split_bounds(n, batch_size or -1, merge_last=True)
        base = self.opt_step if perm_base is None else perm_base
        rows = []
        for step in range(repeat):
            if self.shuffle == "numpy":
                perm_local = torch.as_tensor(np.random.permutation(n)).to(dev)
            else:
                perm_local = self._device_perm(n, base, agent, repeat, step)
            perm = ids[perm_local]
            for s, e in bounds:
                rows.append(self._minibatch(pb, adv, perm[s:e].contiguous()))
        self.param_version += 1
        vals = np.asarray(rows, dtype=np.float64).reshape(-1, len(self._stat_names))
        return self._stats_cls(**{k: SequenceSummaryStats.from_sequence(vals[:, j]) for j, k in enumerate(self._stat_names)})

    def _minibatch(self, pb: dict, adv: torch.Tensor, idx: torch.Tensor) -> list[float]:
        """npg.py:149-187 for the rows `idx` -> this minibatch's statistics, in `_stat_names` order (one host read)."""
        net, actor, dev = self.net, self.net.actor, self.device
        B = idx.numel()
        x = ops.gather_rows(pb["obs"], idx)
        mb = dict(x=x, B=B, act=pb["act"][idx].to(torch.int32), logp_old=pb["logp_old"][idx].contiguous(),
                  adv=adv[idx].contiguous(), out=torch.zeros(8, dtype=torch.float32, device=dev))
        mb["logits"] = logits = actor.forward(x, save=True)
        # the actor loss at the old parameters with its gradient down to the logits, then to the parameters
        mb["part0"], d_logits = ops.categorical_kl_surrogate(logits, logits, mb["act"], mb["logp_old"], mb["adv"], self._loss_kind,
                                                             want_grad=True)
        n_split = ops.mlp_n_split(B)
        st = self._conjugate_gradients(actor, actor.backward(d_logits, n_split), n_split)
        self._actor_step(mb, st)
        # optim_critic_iters critic-only steps on mse(returns, V) (npg.py:180-183)
        cx = x if pb.get("joint") is None else ops.gather_rows(pb["joint"], torch.div(idx, pb["n_agent"], rounding_mode="floor"))
        part_v = None
        for _ in range(self.optim_critic_iters):
            value = net.critic.forward(cx, save=True).reshape(-1)
            dvalue, part_v = ops.ppo_value_loss(value, pb["ret"], self._cfg_mse, B, perm=idx)
            self.optim.step(net.critic.backward(dvalue.view(-1, 1), n_split))
        if part_v is not None:
            ops.call("tsm_ppo_loss_finalize", ops.ptr(part_v), B, ops.C.byref(self._cfg_mse), ops.ptr(mb["out"][4:]), ops.stream_ptr())
        return self._read_stats(mb["out"].cpu().numpy())

    def _conjugate_gradients(self, actor, g_slabs: torch.Tensor, n_split: int, nsteps: int = 10,
                             residual_tol: float = 1e-10) -> dict:
        """npg.py:202-224 on the device, at the rows of the actor's last saved forward: -> the CG state, `x` the solution.  Once
        the residual is below `residual_tol` the device flag freezes x, r and p; the launches of the remaining iterations still
        run and change nothing."""
        n = actor.flat.numel()
        B = actor._saved_forward()[0].shape[0]
        w = self._ws.get(("cg", n, B))
        if w is None:
            w = self._ws[("cg", n, B)] = dict(st=ops.cg_state(n, self.device), fvp={},
                                                   slabs=torch.empty(n_split, n, dtype=torch.float32, device=self.device))
        st = w["st"]
        ops.cg_init(st, g_slabs)
        for _ in range(nsteps):
            _, head = ops.fisher_vector_product(actor, st["p"], n_split, slabs=w["slabs"], ws=w["fvp"])
            ops.cg_update(st, w["slabs"], head, self._damping)
            ops.cg_direction(st, residual_tol)
        st["fvp"] = w["fvp"]
        return st

    def _actor_step(self, mb: dict, st: dict) -> None:
        """theta <- theta - trust_region_size x (npg.py:170-175), then the KL of the new policy from the old one (:176-177)."""
        actor = self.net.actor
        ops.flat_axpy_dev(actor.flat.data, st["x"], -self.trust_region_size, out=actor.flat.data)
        new_logits = actor.forward(mb["x"], save=False)
        part1, _ = ops.categorical_kl_surrogate(mb["logits"], new_logits, mb["act"], mb["logp_old"], mb["adv"], self._loss_kind)
        ops.qmix_finalize(mb["part0"], mb["B"], mb["out"][0:2])   # {kl at the old parameters (0), actor_loss}
        ops.qmix_finalize(part1, mb["B"], mb["out"][2:4])         # {kl, the loss after the step}

    def _read_stats(self, o: np.ndarray) -> list[float]:
        return [float(o[1]), float(o[6]), float(o[2])]

    # ---- `.learn(batch)` of the MARL trainers: one time-ordered lane, no captured form --------------------------------------
    learn_steps = None

    def learn_graph_ok(self, repeat: int = 1) -> bool:
        return False

    def learn(self, batch: Batch, batch_size: int | None = None, repeat: int = 1, **kwargs) -> dict[str, float]:
        t = lambda v, dt: to_tensor(v, self.device, dt)  # noqa: E731
        obs = t(batch.obs, torch.float32)
        n = obs.shape[0]
        joint = joint_next = None
        if self.critic_input == "global":
            if "global_obs" not in batch:
                raise ValueError(f"{type(self).__name__}(critic_input='global').learn needs batch.global_obs / global_obs_next")
            joint, joint_next = t(batch.global_obs, torch.float32), t(batch.global_obs_next, torch.float32)
        term = t(batch.terminated, torch.uint8).reshape(n, 1)
        trunc = t(batch.truncated, torch.uint8).reshape(n, 1) if "truncated" in batch else torch.zeros_like(term)
        pb = self._lane_pb(obs, t(batch.act, torch.int32).reshape(n), t(batch.rew, torch.float32).view(n, 1), term, trunc,
                           t(batch.obs_next, torch.float32), joint, joint_next)
        return self._update_with_batch(pb, batch_size, repeat).get_loss_stats_dict()
