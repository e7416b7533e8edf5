"""QMIX (value decomposition with a monotonic mixing network) on the HIP path.

Mirror of /root/reference/tianshou/algorithm/multiagent/ctde.py:417-725:
  `QMIXMixer`   :417-499  hypernetworks on the global state -> |w1|, b1, |w2|, b2; q_tot = elu(q w1 + b1) w2 + b2
  `QMIXPolicy`  :502-725  per-agent Q-nets + mixer under ONE Adam, deep-copied targets, epsilon-greedy acting
The networks are `FlatMLP`s (csrc/dense.hip) on views of one joint parameter vector
  [actor_0 ... actor_{N-1} | hyper_w1 | hyper_w2 | hyper_b1 | hyper_b2]
in the order of the reference's optimizer (actors' parameters, then `mixer.parameters()`), so the gradients of every
net land in the slabs of that one vector (`slab_stride`) and one `tsm_adam_step` updates everything.  The mixer's
arithmetic on both sides, the TD target, the MSE and the mixer's backward are one launch (`tsm_qmix_mix_td`,
csrc/qmix.hip); the device acting path is `tsm_qmix_egreedy`.

Kept quirks: Q10 -- one epsilon coin per agent per call, shared by the whole batch (:607);
Q11 -- `state_dict()` holds only `mixer.*` and `target_mixer.*`: the actors are a plain Python list (:536) and are saved
by their owner.
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
from ...utils.net import FlatMLP, FlatNet, join_nets, lagged_twins, ref_layer_keys
from ...utils.tensor import to_tensor
from ..optim import flat_adam_of
from .ctde import LazyScalars

_HYPER = ("hyper_w1", "hyper_w2", "hyper_b1", "hyper_b2")


class QMIXMixer(FlatNet):
    """ctde.py:417-499.  The four hypernetworks are `FlatMLP`s on consecutive views of `flat` (registration order)."""

    split_optimizer_state = False

    def __init__(self, n_agents: int, state_dim: int, mixing_embed_dim: int = 32, hypernet_embed_dim: int = 64,
                 enforce_monotonic: bool = True, device: str | torch.device = "cuda", seed: int | None = None,
                 storage: torch.Tensor | None = None) -> None:
        super().__init__()
        ops.qmix_check(int(n_agents), int(mixing_embed_dim))
        self.n_agents, self.state_dim = int(n_agents), int(state_dim)
        self.embed_dim, self.hypernet_embed_dim = int(mixing_embed_dim), int(hypernet_embed_dim)
        self.enforce_monotonic = bool(enforce_monotonic)
        S, E, Hh, N = self.state_dim, self.embed_dim, self.hypernet_embed_dim, self.n_agents
        self._dims = {"hyper_w1": [S, Hh, N * E], "hyper_w2": [S, Hh, E], "hyper_b1": [S, E], "hyper_b2": [S, E, 1]}
        counts = [ops.mlp_param_count(ops.mlp_desc(self._dims[k])) for k in _HYPER]
        self._offs = np.concatenate([[0], np.cumsum(counts)]).tolist()
        storage = self._claim(self._offs[-1], storage, device)
        for i, k in enumerate(_HYPER):   # hypernetwork i draws its init from seed + i
            setattr(self, k, FlatMLP(self._dims[k], "relu", device=storage.device, seed=None if seed is None else seed + i,
                                     storage=storage[self._offs[i]:self._offs[i + 1]]))

    @property
    def nets(self) -> list[FlatMLP]:
        return [getattr(self, k) for k in _HYPER]

    def rebind(self, storage: torch.Tensor) -> None:
        """Move the parameters into `storage` (a slice of a joint vector) and view them there, hypernetwork by hypernetwork."""
        self.flat = nn.Parameter(storage, requires_grad=False)
        for net, o, e in zip(self.nets, self._offs, self._offs[1:]):
            net.rebind(storage[o:e])

    def hyper_forward(self, state: torch.Tensor, save: bool = False) -> tuple:
        """(w1raw [B, N*E], b1 [B, E], w2raw [B, E], b2 [B, 1]): the hypernetworks on the global state."""
        w1, w2, b1, b2 = (FlatMLP.forward(net, state, save=save) for net in self.nets)
        return w1, b1, w2, b2

    def forward(self, q_values: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
        """q_values [B, N], state [B, S] -> q_tot [B, 1] on the device (ctde.py:468-499; tsm_qmix_mix_td's forward)."""
        dev = self.flat.device
        q = q_values.to(dev, torch.float32).reshape(-1, self.n_agents)
        st = state.to(dev, torch.float32).reshape(q.shape[0], self.state_dim).contiguous()
        B = q.shape[0]
        hyper = self.hyper_forward(st)
        cols = [q[:, i:i + 1].contiguous() for i in range(self.n_agents)]
        zero_act = torch.zeros(B, dtype=torch.int64, device=dev)
        zero_rew = torch.zeros(B, dtype=torch.float32, device=dev)
        out = torch.empty(B, dtype=torch.float32, device=dev)
        ops.qmix_mix_td(cols, cols, [zero_act] * self.n_agents, [zero_rew] * self.n_agents, hyper, hyper,
                        torch.zeros(B, dtype=torch.uint8, device=dev), 0.0, self.enforce_monotonic, qtot_out=out)
        return out.view(B, 1)

    # reference module keys (nn.Sequential indices 0 / 2; hyper_b1 is a bare Linear)
    @staticmethod
    def _layer_keys(name: str) -> list[tuple[str, str]]:
        return [("weight", "bias")] if name == "hyper_b1" else ref_layer_keys(2, "seq")

    def reference_named_views(self, flat: torch.Tensor | None = None) -> list[tuple[str, torch.Tensor]]:
        flat = self._vector(flat)
        return [kv for name, net, o, e in zip(_HYPER, self.nets, self._offs, self._offs[1:])
                for kv in net.named_layers(self._layer_keys(name), f"{name}.", flat[o:e])]

    def state_dict(self, *args, destination: OrderedDict | None = None, prefix: str = "", **kwargs):  # type: ignore[override]
        return self.to_reference_state_dict(prefix, destination)

    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        self.load_reference_state_dict(sd)


class QMIXPolicy(nn.Module):
    """ctde.py:502-725 with `FlatMLP` Q-nets (DecentralizedActor) and a `QMIXMixer`.

    optimizer: None -> FlatAdam(lr 1e-3) over the joint vector (the reference's `optim.Adam(params)`); a torch.optim.Adam
    -> its `param_groups[0]` hyper-parameters are taken over (the update runs in HIP on the joint vector)."""

    def __init__(self, actors: list, mixer: QMIXMixer, observation_space: Any = None, action_space: Any = None,
                 n_agents: int | None = None, optimizer: Any = None, discount_factor: float = 0.99, epsilon: float = 0.1,
                 **kwargs: Any) -> None:
        super().__init__()
        actors = list(actors)
        n_agents = len(actors) if n_agents is None else int(n_agents)
        if not all(isinstance(a, FlatMLP) for a in actors) or not isinstance(mixer, QMIXMixer):
            raise TypeError("QMIXPolicy needs FlatMLP Q-networks (DecentralizedActor) and a QMIXMixer: the update runs in "
                            "HIP, there is no autograd fallback")
        if len(actors) != n_agents or mixer.n_agents != n_agents:
            raise ValueError(f"QMIXPolicy: {len(actors)} actors and a mixer for {mixer.n_agents} agents, n_agents = {n_agents}")
        A = actors[0].dims[-1]
        ops.qmix_check(n_agents, mixer.embed_dim, A)
        if any(a.dims[-1] != A for a in actors):
            raise ValueError("QMIXPolicy: every Q-network needs the same number of actions")
        self.observation_space, self.action_space = observation_space, action_space
        self.n_agents, self.n_act = n_agents, A
        self.discount_factor = discount_factor
        self.seed = int(kwargs.pop("seed", 0))
        self.async_stats = bool(kwargs.pop("async_stats", False))
        self._sample_ctr = 0
        dev = mixer.flat.device
        # ONE joint parameter vector: [actor_0 .. actor_{N-1} | mixer], and the targets over a copy of it
        self.flat, self._offs = join_nets(actors + [mixer], dev)
        self.actors = actors  # a plain list, as upstream: not registered (quirk Q11)
        self.mixer = mixer
        self.target_flat, twins = lagged_twins(actors + [mixer], self.flat, self._offs)
        self.target_actors, self.target_mixer = twins[:-1], twins[-1]
        self.optimizer, _ = flat_adam_of(optimizer, self.flat, "QMIXPolicy: optimizer", False, ("none", "adam"))
        self._eps_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self.epsilon = epsilon
        self._ws: dict = {}

    @property
    def device(self) -> torch.device:
        return self.flat.device

    @property
    def epsilon(self) -> float:
        return self._epsilon

    @epsilon.setter
    def epsilon(self, value: float) -> None:
        """Also written to the device scalar the acting kernel reads: captured collect graphs see the new value."""
        self._epsilon = float(value)
        self._eps_dev.fill_(self._epsilon)

    def _t(self, x, dtype) -> torch.Tensor:
        return to_tensor(x, self.device, dtype)

    # ---- host acting path (ctde.py:557-616) ----------------------------------------------------------------
    def _act_host(self, actor: FlatMLP, obs) -> torch.Tensor:
        x = self._t(obs, torch.float32)
        q = FlatMLP.forward(actor, x.reshape(-1, actor.dims[0]), save=False)
        if np.random.random() < self.epsilon:  # one coin per agent per call, shared by the batch (quirk Q10)
            return torch.randint(0, self.action_space.n, (x.shape[0],))
        act, _ = ops.categorical_sample(q, 0, deterministic=True, want_logp=False)  # first argmax
        return act.to(torch.int64).cpu()

    def forward(self, batch: Batch, state: Any = None, **kwargs: Any) -> Batch:
        """Epsilon-greedy actions on the host RNGs (np.random.random for the coin, the CPU torch.randint for the random
        actions), as upstream: under the same seeds the actions are the reference's."""
        if hasattr(batch, "obs") and not any(k.startswith("agent_") for k in batch.keys()):
            return Batch(act=self._act_host(self.actors[0], batch.obs), state=state)
        result = Batch()
        for i, agent_id in enumerate(batch.keys()):  # i: the key's position among ALL keys, as upstream
            if agent_id.startswith("agent_"):
                result[agent_id] = Batch(act=self._act_host(self.actors[i], batch[agent_id].obs))
        return result

    # ---- device acting path (Collector) -----------------------------------------------------------------
    def act_device(self, obs: torch.Tensor, out: dict | None = None, offset_dev: torch.Tensor | None = None,
                   row_offset: int = 0) -> dict:
        """obs [E, N, D] in HBM -> act i32 [E * N] (agent i's Q-net on column i, then tsm_qmix_egreedy); logp, value = 0.
        The Philox counter is offset_dev (the env's device tick: captured graphs advance it) or the policy's own."""
        N, D = self.n_agents, self.actors[0].dims[0]
        rows = obs.reshape(-1, N, D)
        B = rows.shape[0]
        q = [FlatMLP.forward(self.actors[i], rows[:, i], save=False) for i in range(N)]
        act = out["act"].view(B, N) if out is not None else None
        act = ops.qmix_egreedy(q, self._eps_dev, self.seed, offset=sample_counter(self, B * N, row_offset, offset_dev),
                               offset_dev=offset_dev, out=act)
        return act_result(out, act.view(-1), q=q)

    # ---- learn (ctde.py:618-702) ------------------------------------------------------------------------
    def learn(self, batch: Batch, **kwargs: Any) -> dict[str, float]:
        """One QMIX TD step over the joint rows: N online and N target Q-net forwards, 8 hypernetwork forwards, the mixer
        on both sides with its backward in one launch, the networks' backward into the joint gradient slabs, one Adam
        step.  Leaves may be numpy or HBM tensors (agent_batches_from_buffer); device leaves are read in place."""
        N = self.n_agents
        ab = [batch[f"agent_{i}"] for i in range(N)]
        obs = [self._t(b.obs, torch.float32) for b in ab]
        obs_next = [self._t(b.obs_next, torch.float32) for b in ab]
        act = [self._t(b.act, torch.int64).reshape(-1) for b in ab]
        rew = [self._t(b.rew, torch.float32).reshape(-1) for b in ab]
        term = self._t(ab[0].terminated, torch.uint8).reshape(-1)  # agent 0's flag only (ctde.py:688)
        gs = self._t(batch.global_obs, torch.float32)
        gsn = self._t(batch.global_obs_next, torch.float32)
        B = obs[0].shape[0]
        P = self.flat.numel()
        w = slab_workspace(self._ws, B, self.device, slabs=P)
        q = [FlatMLP.forward(self.actors[i], obs[i], save=True) for i in range(N)]
        qn = [FlatMLP.forward(self.target_actors[i], obs_next[i], save=False) for i in range(N)]
        hyper = self.mixer.hyper_forward(gs, save=True)
        hyper_n = self.target_mixer.hyper_forward(gsn, save=False)
        dq, (dw1, db1, dw2, db2), partial = ops.qmix_mix_td(q, qn, act, rew, hyper, hyper_n, term, self.discount_factor,
                                                            self.mixer.enforce_monotonic)
        slabs, ns = w["slabs"], w["n_split"]
        nets = list(self.actors) + self.mixer.nets
        grads = dq + [dw1, dw2, db1, db2]  # (mixer.nets order: hyper_w1, hyper_w2, hyper_b1, hyper_b2)
        o = 0
        for net, d in zip(nets, grads):
            net.backward(d, ns, slabs=slabs[:, o:], slab_stride=P)
            o += net.flat.numel()
        self.optimizer.step(slabs)
        slot = result_slot(w, 2)
        ops.qmix_finalize(partial, B, slot["h"])
        slot["event"].record()
        res = LazyScalars(slot, ("loss", "q_values"))
        slot["pending"] = res
        return res if self.async_stats else dict(res)

    @torch.no_grad()
    def update_target_networks(self, tau: float = 0.005) -> None:
        """ctde.py:704-725: target = tau * p + (1 - tau) * target, actors then mixer -- one elementwise pass over the joint
        vector (the same f32 operations per element)."""
        self.target_flat.copy_(self.flat * tau + self.target_flat * (1 - tau))

    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        """`mixer.*` and `target_mixer.*` only (quirk Q11: the reference's actors live in a plain list)."""
        sd = OrderedDict()
        for name, m in (("mixer", self.mixer), ("target_mixer", self.target_mixer)):
            m.state_dict(destination=sd, prefix=name + ".")
        return sd

    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        for name, m in (("mixer", self.mixer), ("target_mixer", self.target_mixer)):
            m.load_reference_state_dict(sd, name + ".")
