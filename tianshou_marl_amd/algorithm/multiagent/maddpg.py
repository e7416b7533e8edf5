"""MADDPG (per-agent actors with per-agent centralized critics, continuous actions) on the HIP path.

Mirror of /root/reference/tianshou/algorithm/multiagent/ctde.py:728-955 (`MADDPGPolicy`).  Actors (D -> ... -> Ad, linear
output: `DecentralizedActor`) and critics (N (D + Ad) -> ... -> 1) are `FlatMLP`s (csrc/dense.hip) on views of one joint
parameter vector
  [actor_0 ... actor_{N-1} | critic_0 ... critic_{N-1}]
with a `target_flat` of the same layout, and two `FlatAdam`s: one over the actor half, one over the critic half (the
reference's 2 N Adams with equal hyper-parameters are elementwise the same update).  The algorithm's own arithmetic --
the critics' joint rows, the TD head, the loss finalize, the acting epilogue and the soft target update -- is
csrc/maddpg.hip; the critic's gradient w.r.t. the agent's action columns is `tsm_mlp_input_grad`.

Agent independence (what lets `learn` run phase by phase over all agents instead of agent by agent, with every number
unchanged): iteration i of the reference's loop (:829-928) reads the batch, the TARGET actors (:868-872), target critic i
(:892), critic i (:888, :918) and actor i (:907-910).  The other agents' actions come from the batch (:845-863) and the
next actions from the targets, so an actor or critic stepped earlier in the loop (:903, :925) is never read by a later
iteration; the targets move only in `update_target_networks`.

Kept quirks: Q12 -- every agent's TD target uses its OWN `terminated` (:885), where QMIX reads agent
0's; Q13 -- `state_dict()` is empty: all four net lists are plain Python lists (:764-765, :787-788), so a checkpoint goes
through `to_reference_state_dict()`; Q14 -- one set of Adam hyper-parameters per half (stepped by `tsm_adam_step_coef64`).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any

import numpy as np
import torch
from torch import nn

from ... import ops
from ...data.batch import Batch
from ...utils.learner import act_result, result_slot, sample_counter, slab_workspace
from ...utils.net import FlatMLP, join_nets, lagged_twins, ref_layer_keys
from ...utils.tensor import to_tensor
from ..optim import flat_adam_of
from .ctde import LazyScalars


class MADDPGScalars(LazyScalars):
    """The per-agent losses a kernel is writing into pinned host memory, plus the two aggregates of ctde.py:931-932 (the
    means of the per-agent f32 values, taken in float64 as `np.mean` does)."""

    def __init__(self, slot: dict, n_agents: int) -> None:
        names = tuple(f"agent_{i}_{k}_loss" for i in range(n_agents) for k in ("actor", "critic"))
        super().__init__(slot, names)

    def resolve(self) -> "MADDPGScalars":
        first = self._slot is not None
        super().resolve()
        if first:
            for k in ("actor_loss", "critic_loss"):
                dict.__setitem__(self, k, float(np.mean([v for name, v in dict.items(self) if k in name])))
        return self

    _force = resolve


class MADDPGPolicy(nn.Module):
    """ctde.py:728-955 with `FlatMLP` actors and critics.  kwargs: seed, async_stats, noise_std, clip_actions."""

    def __init__(self, actors: list, critics: list, observation_space: Any, action_space: Any, n_agents: int,
                 optimizer_actors: Any = None, optimizer_critics: Any = None, discount_factor: float = 0.99,
                 tau: float = 0.01, **kwargs: Any) -> None:
        super().__init__()
        actors, critics = list(actors), list(critics)
        n_agents = int(n_agents)
        if not all(isinstance(m, FlatMLP) for m in actors + critics):
            raise TypeError("MADDPGPolicy needs FlatMLP actors (DecentralizedActor) and critics: the update runs in HIP, "
                            "there is no autograd fallback")
        if hasattr(action_space, "n"):
            raise NotImplementedError("MADDPGPolicy: a Discrete action space is not built (the reference's discrete branch "
                                      "concatenates integer actions with float actor outputs); use a Box")
        if not all(hasattr(action_space, k) for k in ("low", "high", "shape")):
            raise TypeError(f"MADDPGPolicy: action_space must be a Box, got {type(action_space).__name__}")
        ops.maddpg_check(n_agents)
        if len(actors) != n_agents or len(critics) != n_agents:
            raise ValueError(f"MADDPGPolicy: {len(actors)} actors and {len(critics)} critics for n_agents = {n_agents}")
        D, Ad = actors[0].dims[0], actors[0].dims[-1]
        if any(a.dims[0] != D or a.dims[-1] != Ad for a in actors):
            raise ValueError("MADDPGPolicy: every actor needs the same observation width and the same action width")
        if len(action_space.shape) != 1 or int(action_space.shape[0]) != Ad:
            raise ValueError(f"MADDPGPolicy: the actors give {Ad} action components, the Box has shape {tuple(action_space.shape)}")
        W = n_agents * (D + Ad)
        for i, c in enumerate(critics):
            if c.dims[0] != W:
                raise ValueError(f"MADDPGPolicy: critic {i} reads {c.dims[0]} inputs, the joint row [obs | act] has "
                                 f"{n_agents} x ({D} + {Ad}) = {W}")
            if c.dims[-1] != 1:
                raise ValueError(f"MADDPGPolicy: critic {i} has output width {c.dims[-1]}, needs 1")
        self.observation_space, self.action_space = observation_space, action_space
        self.n_agents, self.obs_dim, self.act_dim, self.joint_dim = n_agents, D, Ad, W
        self.discount_factor, self.tau = discount_factor, tau
        self.seed = int(kwargs.pop("seed", 0))
        self.async_stats = bool(kwargs.pop("async_stats", False))
        self.clip_actions = bool(kwargs.pop("clip_actions", False))
        self._sample_ctr = 0
        dev = actors[0].flat.device
        # ONE joint parameter vector: [actor_0 .. actor_{N-1} | critic_0 .. critic_{N-1}], and the targets over a copy of it
        self.flat, self._offs = join_nets(actors + critics, dev)
        na = self.n_actor_params = self._offs[n_agents]
        self.actors, self.critics = actors, critics  # plain lists, as upstream: not registered (quirk Q13)
        self.target_flat, targets = lagged_twins(actors + critics, self.flat, self._offs)
        self.target_actors, self.target_critics = targets[:n_agents], targets[n_agents:]
        # coef64: the actor loss is a mean over the outputs of the critic that was just stepped, where the one-sided error of
        # the f32 difference 1.f - beta2 in the step length shows (include/tsmarl.h: tsm_adam_step_coef64)
        self.optimizer_actors, _ = flat_adam_of(optimizer_actors, self.flat[:na], "MADDPGPolicy: optimizer_actors", True,
                                                ("none", "adams"))
        self.optimizer_critics, _ = flat_adam_of(optimizer_critics, self.flat[na:], "MADDPGPolicy: optimizer_critics", True,
                                                 ("none", "adams"))
        self._sigma_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self.noise_std = float(kwargs.pop("noise_std", 0.0))
        # the Box bounds as device vectors (act_device's clamp)
        self._low = torch.as_tensor(np.broadcast_to(np.asarray(action_space.low, np.float32), (Ad,)).copy(), device=dev)
        self._high = torch.as_tensor(np.broadcast_to(np.asarray(action_space.high, np.float32), (Ad,)).copy(), device=dev)
        self._ws: dict = {}

    @property
    def device(self) -> torch.device:
        return self.flat.device

    @property
    def noise_std(self) -> float:
        return self._noise_std

    @noise_std.setter
    def noise_std(self, value: float) -> None:
        """Also written to the device scalar the acting kernel reads: captured collect graphs see the new value."""
        self._noise_std = float(value)
        self._sigma_dev.fill_(self._noise_std)

    def _t(self, x, dtype) -> torch.Tensor:
        return to_tensor(x, self.device, dtype)

    # ---- host acting path (ctde.py:790-815) ----------------------------------------------------------------
    def forward(self, batch: Batch, state: Any = None, **kwargs: Any) -> Batch:
        """Batch(act=actor_i(obs)) per `agent_*` key, i = the key's position among ALL keys, as upstream; no noise."""
        result = Batch()
        for i, agent_id in enumerate(batch.keys()):
            if agent_id.startswith("agent_"):
                actor = self.actors[i]
                x = self._t(batch[agent_id].obs, torch.float32)
                act = FlatMLP.forward(actor, x.reshape(-1, actor.dims[0]), save=False)
                result[agent_id] = Batch(act=act.cpu())
        return result

    # ---- device acting path (Collector) -----------------------------------------------------------------
    def act_device(self, obs: torch.Tensor, out: dict | None = None, offset_dev: torch.Tensor | None = None,
                   row_offset: int = 0) -> dict:
        """obs [E, N, D] in HBM -> act f32 [E * N, Ad] (agent i's actor on column i, then tsm_maddpg_act: noise_std times a
        standard normal draw, the clamp to the Box with clip_actions); logp, value = 0.  The Philox counter is offset_dev
        (the env's device tick: captured graphs advance it) or the policy's own."""
        N, D, Ad = self.n_agents, self.obs_dim, self.act_dim
        rows = obs.reshape(-1, N, D)
        E = rows.shape[0]
        mu = [FlatMLP.forward(self.actors[i], rows[:, i], save=False) for i in range(N)]
        lo, hi = (self._low, self._high) if self.clip_actions else (None, None)
        act = ops.maddpg_act(mu, self._sigma_dev, self.seed, offset=sample_counter(self, E * N * Ad, row_offset, offset_dev),
                             offset_dev=offset_dev, low=lo, high=hi, out=None if out is None else out["act"])
        return act_result(out, act, mu=mu)

    # ---- learn (ctde.py:817-934) ------------------------------------------------------------------------
    def _workspace(self, B: int) -> dict:
        N, W, na, dev = self.n_agents, self.joint_dim, self.n_actor_params, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        return slab_workspace(self._ws, B, dev, slabs_actor=na, slabs_critic=self.flat.numel() - na, more=lambda: dict(
            x=torch.empty(B, W, **f32), x_next=torch.empty(B, W, **f32), x_pi=torch.empty(N, B, W, **f32),
            dq=[torch.empty(B, **f32) for _ in range(N)], d_act=[torch.empty(B, self.act_dim, **f32) for _ in range(N)],
            partial=torch.empty(ops.maddpg_partial_elems(B, N), dtype=torch.float64, device=dev),
            d_pi=torch.full((B, 1), -1.0 / B, **f32)))  # d (-mean Q) / d Q

    def learn(self, batch: Batch, **kwargs: Any) -> dict[str, float]:
        """One MADDPG step for every agent, phase by phase (the agents are independent within a call, see the module
        docstring): target actors -> joint rows -> critics and target critics -> TD head -> critic backward and Adam ->
        actors -> actor-side rows -> the stepped critics and their gradient w.r.t. the agent's action -> actor backward and
        Adam -> finalize.  Leaves may be numpy or HBM tensors; device leaves are read in place."""
        N, D, Ad = self.n_agents, self.obs_dim, self.act_dim
        ab = [batch[f"agent_{i}"] for i in range(N)]
        obs = [self._t(b.obs, torch.float32).reshape(-1, D) for b in ab]
        B = obs[0].shape[0]
        obs_next = [self._t(b.obs_next, torch.float32).reshape(B, D) for b in ab]
        act = [self._t(b.act, torch.float32).reshape(B, Ad) for b in ab]
        rew = [self._t(b.rew, torch.float32).reshape(B) for b in ab]
        term = [self._t(b.terminated, torch.uint8).reshape(B) for b in ab]  # every agent its own flags (quirk Q12)
        w = self._workspace(B)
        ns, na = w["n_split"], self.n_actor_params
        # 1-2: next actions of the TARGET actors, then X = [obs | act] and X' = [obs_next | a']
        act_next = [FlatMLP.forward(self.target_actors[j], obs_next[j], save=False) for j in range(N)]
        x = ops.maddpg_joint_rows(obs, act, out=w["x"])
        x_next = ops.maddpg_joint_rows(obs_next, act_next, out=w["x_next"])
        # 3-4: critics on X (saved), target critics on X', the TD head of all agents
        q = [FlatMLP.forward(self.critics[i], x, save=True) for i in range(N)]
        q_next = [FlatMLP.forward(self.target_critics[i], x_next, save=False) for i in range(N)]
        dq, partial = ops.maddpg_td(q, q_next, rew, term, self.discount_factor, out=(w["dq"], w["partial"]))
        # 5: critic backward into the critic half's slabs, one Adam step (it lands before the actor gradient is taken)
        slabs_c, Pc = w["slabs_critic"], self.flat.numel() - na
        for i in range(N):
            self.critics[i].backward(dq[i], ns, slabs=slabs_c[:, self._offs[N + i] - na:], slab_stride=Pc)
        self.optimizer_critics.step(slabs_c)
        # 6-7: a_i = actor_i(obs_i) (saved), then X_i = X with a_i in agent i's action slot
        a_pi = [FlatMLP.forward(self.actors[i], obs[i], save=True) for i in range(N)]
        x_pi = ops.maddpg_joint_rows(obs, act, replace=a_pi, out=w["x_pi"])
        # 8: the stepped critic i on X_i and d(-mean Q_i) / d a_i through its action columns
        q_pi = []
        for i in range(N):
            q_pi.append(FlatMLP.forward(self.critics[i], x_pi[i], save=True))
            self.critics[i].input_grad(w["d_pi"], N * D + i * Ad, Ad, out=w["d_act"][i])
        # 9: actor backward into the actor half's slabs, one Adam step
        slabs_a = w["slabs_actor"]
        for i in range(N):
            self.actors[i].backward(w["d_act"][i], ns, slabs=slabs_a[:, self._offs[i]:], slab_stride=na)
        self.optimizer_actors.step(slabs_a)
        # 10: the 2 N losses into the pinned slot
        slot = result_slot(w, 2 * N)
        ops.maddpg_finalize(partial, q_pi, B, slot["h"])
        slot["event"].record()
        res = MADDPGScalars(slot, N)
        slot["pending"] = res
        return res if self.async_stats else dict(res)

    @torch.no_grad()
    def update_target_networks(self) -> None:
        """ctde.py:936-955 with the policy's tau: one pass over the joint vector (the same f32 operations per element)."""
        ops.polyak(self.target_flat, self.flat, self.tau)

    # ---- checkpoints ----------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        """Empty, as upstream (quirk Q13: actors, critics and both target sets are plain lists there)."""
        return OrderedDict()

    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        if len(sd):
            raise KeyError(f"MADDPGPolicy.state_dict() is empty (use load_reference_state_dict); unexpected keys {list(sd)[:4]}")

    def _named_nets(self) -> list[tuple[str, FlatMLP]]:
        return [(f"{name}.{i}", m) for name, nets in (("actors", self.actors), ("critics", self.critics),
                                                      ("target_actors", self.target_actors),
                                                      ("target_critics", self.target_critics)) for i, m in enumerate(nets)]

    def to_reference_state_dict(self) -> OrderedDict:
        """Every net under `actors.{i}.fc{k}.weight` style keys (critics, target_actors, target_critics alike)."""
        sd = OrderedDict()
        for prefix, m in self._named_nets():
            m.export_layers(ref_layer_keys(m.n_layers, "fc"), prefix + ".", sd)
        return sd

    def load_reference_state_dict(self, sd) -> None:
        for prefix, m in self._named_nets():
            m.import_layers(sd, ref_layer_keys(m.n_layers, "fc"), prefix + ".")
