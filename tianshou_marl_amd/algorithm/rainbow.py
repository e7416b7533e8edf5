"""Rainbow (C51 over a network of NoisyLinear layers and dueling streams) on the HIP path.

Mirror of /root/reference/tianshou/algorithm/modelfree/rainbow.py:18-101 (`RainbowDQN`), which is C51 plus a fresh draw of the
factorised noise of every NoisyLinear layer before each update, in the online and in the lagged net.  Everything else a Rainbow
user needs lives in the network: `RainbowNet` (utils/net.py) is the reference's `Net(num_atoms=N, dueling_param=..., linear_layer=
NoisyLinear)` on one flat vector, composed, combined and differentiated by csrc/rainbow.hip around the matrix products of
csrc/dense.hip.  The head, the n-step walk, the prioritized buffer and the multi-agent dispatch are C51's.  There is no autograd
fallback.

Kept quirks: Q20, Q22, Q23 as C51; Q40 -- on the calls where the lagged copy happens the copy follows the
draw and copies every parameter, the noise slots included, so the target net runs with the ONLINE net's noise on those calls;
Q41 -- noise acts only in torch training mode: `forward` / `act_device` in eval mode use mu alone, the lagged net follows the
algorithm's mode (the reference unwraps its eval-mode wrapper), and an update in eval mode silently trains without noise, sigma
getting zero gradient; Q42 -- the noise slots are parameters: they appear in reference checkpoints; Q43 -- `RainbowDQN` around a
net without a noisy layer is legal and equals C51.
"""
from __future__ import annotations

from typing import Any

import torch

from ..data.batch import Batch
from ..utils.net import RainbowNet
from .distq import C51, C51Policy

_NOISE_STREAM = 0xD1B54A32D192ED03   # added to the seed for the learner's noise draws: acting never shares a key with them


class RainbowPolicy(C51Policy):
    """c51.py:16-67 with a `RainbowNet` Q-network: the net's own forward composes its noisy weights and joins its streams."""

    _model_cls = RainbowNet

    def __init__(self, *, model: RainbowNet, action_space: Any, observation_space: Any = None, num_atoms: int = 51,
                 v_min: float = -10.0, v_max: float = 10.0, eps_training: float = 0.0, eps_inference: float = 0.0,
                 seed: int = 0) -> None:
        if isinstance(model, RainbowNet) and model.num_atoms != int(num_atoms):
            raise ValueError(f"RainbowPolicy: num_atoms = {num_atoms}, but the net emits {model.num_atoms} atoms per action")
        super().__init__(model=model, action_space=action_space, observation_space=observation_space, num_atoms=num_atoms,
                         v_min=v_min, v_max=v_max, eps_training=eps_training, eps_inference=eps_inference, seed=seed)

    def _forward_values(self, x: torch.Tensor, model):
        net = self.model if model is None else model
        q, logits = self._logits(net.forward(x, save=False))
        return q, logits, {}

    def _act_values(self, rows: torch.Tensor, ctr: int, offset_dev) -> torch.Tensor:
        return self.values(self.model.forward(rows, save=False))


class RainbowDQN(C51):
    """rainbow.py:18-101 on the device buffer."""

    _policy_cls = RainbowPolicy

    def __init__(self, *, policy: RainbowPolicy, optim: Any, gamma: float = 0.99, n_step_return_horizon: int = 1,
                 target_update_freq: int = 0) -> None:
        super().__init__(policy=policy, optim=optim, gamma=gamma, n_step_return_horizon=n_step_return_horizon,
                         target_update_freq=target_update_freq)
        if policy.model.n_slots and self.optim.weight_decay != 0:
            raise ValueError("RainbowDQN: weight_decay != 0 on a noisy net is not served: torch skips the noise vectors "
                             "(they take no gradient), the flat Adam would decay them")
        self._noise_ctr = 0
        # noise to load for the coming draws, in call order (online, then lagged, per update), in place of device draws: parity
        # tests feed the reference's recorded noise
        self.noise_feed: list = []

    def _sample_noise(self, net: RainbowNet) -> bool:
        """rainbow.py:76-91: a fresh draw for every noisy layer of `net`; the Philox counter advances per draw."""
        if not net.n_slots:
            return False
        if self.noise_feed:
            net.set_noise(self.noise_feed.pop(0))
        else:
            net.sample((self.policy.seed + _NOISE_STREAM) & (2**64 - 1), offset=self._noise_ctr)
        self._noise_ctr += 1
        return True

    def _update_with_batch(self, batch: Batch):
        self._sample_noise(self.policy.model)
        if self.use_target_network:
            self._sample_noise(self.model_old)
        return super()._update_with_batch(batch)

    def _next_forwards(self, batch: Batch) -> None:
        raw_on = self.policy.model.forward(batch.rows_next, save=False)
        batch.q_next_online = self.policy.values(raw_on)
        batch.raw_next = self.model_old.forward(batch.rows_next, save=False) if self.use_target_network else raw_on

    def _online_forward(self, batch: Batch, x: torch.Tensor) -> torch.Tensor:
        return self.policy.model.forward(x, save=True)

    # ---- checkpoints ---------------------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):  # type: ignore[override]
        sd = super().state_dict(*args, **kwargs)
        sd["noise_ctr"] = self._noise_ctr
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, *args, **kwargs):  # type: ignore[override]
        super().load_state_dict(sd, *args, **kwargs)
        self._noise_ctr = int(sd.get("noise_ctr", 0))

    def _ref_nets(self) -> list:
        """`policy.model.`, then `model_old.`: Rainbow holds the lagged module itself, not its eval-mode wrapper
        (rainbow.py:72-74), so no `.module` stands in its keys."""
        return [("policy.model.", self.policy.model)] + ([("model_old.", self.model_old)] if self.use_target_network else [])
