"""BCQ (arXiv:1812.02900): batch-constrained Q-learning for `Box` actions from a recorded dataset, on the HIP path.

Mirror of tianshou/algorithm/imitation/bcq.py (`BCQPolicy` :34-116, `BCQ` :119-263) on actor_critic.py's learner core with the
twin critics: the perturbation net is the core's "actor", the VAE (utils/net.py `VAE`, `Perturbation`) steps under an Adam of
its own.  The matrix products are `FlatMLP`s on csrc/dense.hip; what lies between them is csrc/bcq.hip, the critics' mse head
`tsm_cac_critic_head` and the actor's loss head `tsm_cac_det_actor_head` fed `tsm_bcq_perturb`'s factor.  The decoder runs
ONCE per update over B K + B rows -- the K sampled actions of every obs_next for the target, then one action per obs for the
actor step -- where the reference's call shape runs it twice: both decodes follow the VAE's step and carry no gradient.  The
dataset lives in a device `VectorReplayBuffer(act_dim=k)`; `update` and `_preprocess_batch` are CQL's (the batch's own `rew`,
`done`, `obs_next`; the agent column for `MultiAgentOffPolicyAlgorithm`).  There is no autograd fallback.

The normals, per update and in this order at the policy's Philox counter: [B, L] for the VAE's latent, then ONE draw
[B K + B, L] whose first B K rows are the target's `decode(obs_next)` and whose last B rows the actor step's `decode(obs)` --
the reference's order of draws.  Acting draws [n S, L] row-major: observation by observation, as the reference's loop.

Kept quirks: Q74 -- the target's actions are decoded but NOT perturbed (the reference's comment says
otherwise); Q75 -- `actor_perturbation_target` exists, moves by Polyak and is checkpointed, but nothing reads it; Q76 -- the
actor step's gradients into the decoder and into critic 1 are dropped (the reference's optimizers zero them before their next
step); Q77 -- the actor step decodes with the VAE, and reads critic 1, after their steps of the same call.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Literal

import torch

from .. import ops
from ..data.batch import Batch
from ..data.stats import TrainingStats
from ..utils.learner import result_slot, sample_counter, slab_workspace
from ..utils.net import VAE, ContinuousCritic, FlatMLP, Perturbation, lagged_copy
from ..utils.tensor import to_tensor
from .actor_critic import ActorDualCriticsOffPolicyAlgorithm
from .cac import ContinuousActionRows, _ContinuousPolicy
from .cql import offline_batch_rows
from .dqn import _obs_rows
from .optim import AdamOptimizerFactory, flat_adam_of


@dataclass(kw_only=True)
class BCQTrainingStats(TrainingStats):
    actor_loss: float
    critic1_loss: float
    critic2_loss: float
    vae_loss: float


class BCQPolicy(_ContinuousPolicy):
    """bcq.py:34-116.  `forward` / `act_device` run all n S candidate rows in one pass: the decoder's rows with clamped normals,
    the decoder, its tanh beside the observation, the perturbation net and its clamp, critic 1, and the first maximal q per
    observation (the reference loops over the observations on the host).  `seed` keys the Philox normals;
    `normal_source(rows, L)` stands in for them (tests)."""

    _actor_cls = Perturbation
    normal_source = None

    def __init__(self, *, actor_perturbation: Perturbation, action_space: Any, critic: ContinuousCritic, vae: VAE,
                 forward_sampled_times: int = 100, observation_space: Any = None, action_scaling: bool = False,
                 action_bound_method: Literal["clip"] | None = "clip", seed: int = 0) -> None:
        super().__init__(actor_perturbation, None, action_space, observation_space, action_scaling, action_bound_method, seed)
        name, D, Ad, dev = type(self).__name__, actor_perturbation.obs_dim, actor_perturbation.act_dim, self.device
        if not isinstance(vae, VAE):
            raise TypeError(f"{name} needs a VAE (utils/net.py): the update runs in HIP, there is no autograd fallback "
                            f"(got {type(vae).__name__})")
        if (vae.obs_dim, vae.act_dim) != (D, Ad) or vae.flat.device != dev:
            raise ValueError(f"{name}: the VAE models {vae.obs_dim} + {vae.act_dim} on {vae.flat.device}; the perturbation net "
                             f"reads {D} + {Ad} on {dev}")
        if not isinstance(critic, FlatMLP) or critic.dims[0] != D + Ad or critic.dims[-1] != 1 or critic.flat.device != dev:
            raise ValueError(f"{name}: critic must be a ContinuousCritic / FlatMLP mapping {D} + {Ad} -> 1 on {dev}")
        ops.bcq_check(Ad, vae.latent_dim, int(forward_sampled_times))
        self.actor_perturbation, self.critic, self.vae = actor_perturbation, critic, vae
        self.forward_sampled_times = int(forward_sampled_times)
        self.obs_dim = D

    def _obs(self, batch: Batch) -> torch.Tensor:
        """As the base's, with the policy's own observation width: the "actor" here reads [obs | act]."""
        obs, mask = _obs_rows(batch.obs)
        if mask is not None:
            raise NotImplementedError(f"{type(self).__name__}: action masks have no meaning for a Box action")
        return to_tensor(obs, self.device, torch.float32).reshape(-1, self.obs_dim)

    def _normals(self, rows: int, counter: int | None = None, offset_dev=None) -> torch.Tensor:
        """Standard normals f32 [rows, L]: `normal_source`'s, or `tsm_cac_normal` at `counter` (None: the policy's own, which
        then advances)."""
        L = self.vae.latent_dim
        if self.normal_source is not None:
            return to_tensor(self.normal_source(rows, L), self.device, torch.float32).reshape(rows, L).contiguous()
        if counter is None:
            counter = self._sample_ctr
            self._sample_ctr += rows * L
        return ops.cac_normal(rows * L, self.seed, offset=counter, offset_dev=offset_dev, device=self.device).view(rows, L)

    def candidates(self, obs: torch.Tensor, z: torch.Tensor):
        """obs [n, D], z [n S, L] -> (act [n, Ad], index i32 [n], the candidate rows [n S, D + Ad], q [n S])."""
        pert, vae, S, D, Ad = self.actor_perturbation, self.vae, self.forward_sampled_times, self.obs_dim, self.act_dim
        xd = ops.bcq_decode_rows(obs, S, None, z)
        x = ops.bcq_action_rows(vae.decode_rows(xd), xd, D, vae.max_action)
        x_pi, _ = ops.bcq_perturb(FlatMLP.forward(pert, x, save=False), x, pert.phi, pert.max_action, want_factor=False)
        q = FlatMLP.forward(self.critic, x_pi, save=False).reshape(-1)
        act, index = ops.bcq_select(q, x_pi, S, D, Ad)
        return act, index, x_pi, q

    def forward(self, batch: Batch, state: Any = None, **kwargs: Any) -> Batch:
        """-> Batch(act numpy f32 [n, Ad]: per observation the perturbed candidate of the largest q1, index i32 [n] in HBM)."""
        obs = self._obs(batch).contiguous()
        act, index, _, _ = self.candidates(obs, self._normals(obs.shape[0] * self.forward_sampled_times))
        return Batch(act=act.cpu().numpy(), index=index, state=state)

    def act_device(self, obs: torch.Tensor, out: dict | None = None, offset_dev: torch.Tensor | None = None,
                   row_offset: int = 0) -> dict:
        """obs [..., D] in HBM -> act f32 [rows, Ad] through `_emit` (no exploration noise: the clip and the scaling of
        `map_action`)."""
        obs = obs.reshape(-1, self.obs_dim).contiguous()
        rows = obs.shape[0] * self.forward_sampled_times
        ctr = sample_counter(self, rows * self.vae.latent_dim, row_offset, offset_dev)
        act, _, _, _ = self.candidates(obs, self._normals(rows, ctr, offset_dev))
        return self._emit(act, 0.0, out, offset_dev, row_offset)


class BCQ(ContinuousActionRows, ActorDualCriticsOffPolicyAlgorithm):
    """bcq.py:119-263."""

    _policy_cls = BCQPolicy
    normal_source = None   # (rows, latent_dim) -> f32 [rows, latent_dim] in HBM: stands in for the Philox normals (tests)

    def __init__(self, *, policy: BCQPolicy, actor_perturbation_optim: AdamOptimizerFactory, critic_optim: AdamOptimizerFactory,
                 vae_optim: AdamOptimizerFactory, critic2: ContinuousCritic | None = None,
                 critic2_optim: AdamOptimizerFactory | None = None, gamma: float = 0.99, tau: float = 0.005, lmbda: float = 0.75,
                 num_sampled_action: int = 10) -> None:
        super().__init__(policy=policy, policy_optim=actor_perturbation_optim, critic=policy.critic, critic_optim=critic_optim,
                         critic2=critic2, critic2_optim=critic2_optim, tau=tau, gamma=gamma, n_step_return_horizon=1)
        ops.bcq_check(policy.act_dim, policy.vae.latent_dim, int(num_sampled_action))
        self.actor_perturbation_optim = self.policy_optim
        self.actor_perturbation_target = lagged_copy(policy.actor_perturbation)   # moved and saved, never read (quirk Q75)
        self.vae_optim, s = flat_adam_of(vae_optim, policy.vae, f"{type(self).__name__}: vae_optim", True, ("factory",))
        if s is not None:
            self._scheds.append(s)
        self.lmbda, self.num_sampled_action = float(lmbda), int(num_sampled_action)

    # ---- what the core asks of its subclass, with the observation width the policy's (the "actor" reads [obs | act]) -------
    def _check_critic(self, name: str, net) -> None:
        D, Ad, dev = self.policy.obs_dim, self.policy.act_dim, self.device
        if not isinstance(net, FlatMLP) or net.dims[0] != D + Ad or net.dims[-1] != 1 or net.flat.device != dev:
            raise ValueError(f"{type(self).__name__}: {name} must be a ContinuousCritic / FlatMLP mapping {D} + {Ad} -> 1 on {dev}")

    def _slab_widths(self) -> dict:
        return dict(super()._slab_widths(), slabs_v=self.policy.vae.flat.numel())

    def _work(self, B: int, **slabs: int) -> dict:
        D, Ad, L, K, dev = self.policy.obs_dim, self.policy.act_dim, self.policy.vae.latent_dim, self.num_sampled_action, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        n = B * K + B
        return slab_workspace(self._ws, B, dev, more=lambda: dict(
            x=torch.empty(B, D + Ad, **f32), x_pi=torch.empty(B, D + Ad, **f32), ones=torch.ones(B, 1, **f32),
            xd=torch.empty(n, D + L, **f32), X=torch.empty(n, D + Ad, **f32)), **slabs)

    def _lagged(self) -> list:
        return super()._lagged() + [(self.actor_perturbation_target, self.policy.actor_perturbation)]

    def _nets(self):
        """(reference prefix, net) in the reference's module order (the lagged copies sit in an EvalModeModuleWrapper)."""
        p = self.policy
        return [("policy.actor_perturbation.", p.actor_perturbation), ("policy.critic.", self.critic), ("policy.vae.", p.vae),
                ("actor_perturbation_target.module.", self.actor_perturbation_target),
                ("critic_target.module.", self.critic_old), ("critic2.", self.critic2),
                ("critic2_target.module.", self.critic2_old)]

    def _optims(self) -> dict:
        return dict(actor_perturbation_optim=self.policy_optim, critic_optim=self.critic_optim,
                    critic2_optim=self.critic2_optim, vae_optim=self.vae_optim)

    def _preprocess_batch(self, batch: Batch, buffer, indices, agent: int | None = None) -> Batch:
        """The sampled rows from the device stores, as CQL gathers them: obs, act, rew, done, obs_next of the batch itself."""
        offline_batch_rows(self, batch, buffer, indices, agent)
        return batch

    def _normal_rows(self, rows: int) -> torch.Tensor:
        if self.normal_source is not None:
            L = self.policy.vae.latent_dim
            return to_tensor(self.normal_source(rows, L), self.device, torch.float32).reshape(rows, L).contiguous()
        return self.policy._normals(rows)

    def _decode(self, w: dict, obs_next, obs, z) -> torch.Tensor:
        """`vae.decode` of K actions per obs_next and of one per obs, in one pass of the decoder -> the rows [obs | act]
        [B K + B, D + Ad]."""
        vae = self.policy.vae
        xd = ops.bcq_decode_rows(obs_next, self.num_sampled_action, obs, z, out=w["xd"])
        return ops.bcq_action_rows(vae.decode_rows(xd), xd, self.policy.obs_dim, vae.max_action, out=w["X"])

    # ---- _update_with_batch (bcq.py:188-263), in the reference's order --------------------------------------------------
    def _update_with_batch(self, batch: Batch) -> BCQTrainingStats:
        dev, pol = self.device, self.policy
        pert, vae = pol.actor_perturbation, pol.vae
        if "weight" in batch:   # (BCQ's losses take no importance weights)
            batch.pop("weight")
        obs, act = self._batch_rows(batch)
        B, K, D, Ad = obs.shape[0], self.num_sampled_action, pol.obs_dim, pol.act_dim
        BK = B * K
        w = self._work(B, **self._slab_widths())
        obs_next = to_tensor(batch.obs_next, dev, torch.float32).reshape(B, D).contiguous()
        rew = to_tensor(batch.rew, dev, torch.float32).reshape(-1)
        vmask = to_tensor(batch.done, dev, torch.bool).reshape(-1).logical_not()
        slot = result_slot(w, 3, 2)
        h = slot["h"]   # {vae_loss, KL_loss}, {critic1_loss, critic2_loss}, {actor_loss, .}
        # 1. the VAE's loss and step (bcq.py:202-208) on the rows [obs | act], which the critics read again in step 4
        x = ops.maddpg_joint_rows([obs], [act], out=w["x"])
        vae.forward_rows(x, obs, self._normal_rows(B), save=True)
        vh = vae.loss_head(act)
        ops.qmix_finalize(vh["partial"], B, h[0])
        vae.backward(vh["d_raw"], w["n_split"], slabs=w["slabs_v"])
        self.vae_optim.step(w["slabs_v"])
        # 2. ONE decode with the stepped VAE: K actions per obs_next, then one per obs (:213-217, 247)
        X = self._decode(w, obs_next, obs, self._normal_rows(BK + B))
        # 3. the target from the lagged critics on the decoded, NOT perturbed, actions (:219-237, quirk Q74)
        target = ops.bcq_target(FlatMLP.forward(self.critic_old, X[:BK], save=False),
                                FlatMLP.forward(self.critic2_old, X[:BK], save=False), rew, vmask, K, self.gamma, self.lmbda)
        # 4. both critics' mse steps (:239-245)
        ch = self._critic_step(w, x, lambda q1, q2: ops.cac_critic_head(q1, q2, target, None), twin=True)
        ops.qmix_finalize(ch["partial"], B, h[1])
        # 5. the perturbation net's step through critic 1 after its step (:247-253, quirks Q76, Q77)
        x_s = X[BK:]
        raw_p = FlatMLP.forward(pert, x_s, save=True)
        x_pi, factor = ops.bcq_perturb(raw_p, x_s, pert.phi, pert.max_action, out=w["x_pi"])
        q_pi = FlatMLP.forward(self.critic, x_pi, save=True)
        ah = ops.cac_det_actor_head(self.critic.input_grad(w["ones"], D, Ad), factor, q_pi, pert.max_action)
        ops.qmix_finalize(ah["partial"], B, h[2])
        pert.backward(ah["d_raw"], w["n_split"], slabs=w["slabs_a"])
        self.policy_optim.step(w["slabs_a"])
        self._polyak()                                                  # 6. :256
        slot["event"].record()
        slot["event"].synchronize()
        return BCQTrainingStats(actor_loss=float(h[2, 0]), critic1_loss=float(h[1, 0]), critic2_loss=float(h[1, 1]),
                                vae_loss=float(h[0, 0]))

    # ---- checkpoints: the core's nets and Adams (three of them here, and critic2's), the draw counter from the base ----------
    def to_reference_state_dict(self):
        """The reference's module keys, then what its module state_dict does not hold: the normals' Philox counter."""
        sd = super().to_reference_state_dict()
        sd["sample_ctr"] = self.policy._sample_ctr
        return sd

    def load_reference_state_dict(self, sd) -> None:
        super().load_reference_state_dict(sd)
        self.policy._sample_ctr = int(sd.get("sample_ctr", 0))
