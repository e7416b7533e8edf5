"""The flat-parameter networks of utils/net.py and the QMIX mixer at one small shape each, and what tests/golden/flat_nets.npz
pins of them (tests/golden/make_flat_net_fixtures.py writes it, tests/test_host_flat_nets.py reads it).  Two hidden layers of 8
to 16, E = K = 3, 5 atoms, 4 cosines; the mixer's mixing width is 32, the smallest it builds, and the fused actor-critic's hidden
width 64, the only one it has."""
from __future__ import annotations

import json
from collections import OrderedDict

import numpy as np
import torch

from tianshou_marl_amd.algorithm.multiagent.qmix import QMIXMixer
from tianshou_marl_amd.utils import net as N

SEED = 3
_IQN = dict(preprocess_dims=[6, 12, 16], n_act=4, hidden_sizes=(10,), num_cosines=4)
_RAINBOW = dict(obs_dim=6, hidden_sizes=(12, 8), n_act=3, num_atoms=5)


def _icm(seed, device="cpu"):
    # the two models take their init from the global generator: seeded here, so that the case is a function of `seed`
    torch.manual_seed(seed)
    return N.IntrinsicCuriosityModule(feature_net=N.FlatMLP([6, 12, 8], device=device, seed=seed), feature_dim=8, action_dim=4,
                                      hidden_sizes=(10,))


# name -> (make(seed) on the CPU, has a twin: `clone_over` / `lagged_copy` serve it)
CASES = OrderedDict([
    ("FlatMLP", (lambda s: N.FlatMLP([6, 12, 8, 4], device="cpu", seed=s), True)),
    ("ContinuousActorDeterministic", (lambda s: N.ContinuousActorDeterministic(6, 3, (12, 8), max_action=2.0, device="cpu", seed=s), True)),
    ("ContinuousCritic", (lambda s: N.ContinuousCritic(6, 3, (12, 8), device="cpu", seed=s), True)),
    ("ContinuousActorProbabilistic", (lambda s: N.ContinuousActorProbabilistic(6, 3, (12, 8), device="cpu", seed=s), True)),
    ("ContinuousActorProbabilistic-conditioned", (lambda s: N.ContinuousActorProbabilistic(6, 3, (12, 8), conditioned_sigma=True,
                                                                                          device="cpu", seed=s), True)),
    ("EnsembleCritic", (lambda s: N.EnsembleCritic(6, 3, 3, (12, 8), device="cpu", seed=s), True)),
    ("ImplicitQuantileNet", (lambda s: N.ImplicitQuantileNet(**_IQN, device="cpu", seed=s), True)),
    ("FractionProposalNet", (lambda s: N.FractionProposalNet(5, 16, device="cpu", seed=s), True)),
    ("FullQuantileNet", (lambda s: N.FullQuantileNet(**_IQN, device="cpu", seed=s), True)),
    ("RainbowNet-dueling", (lambda s: N.RainbowNet(**_RAINBOW, q_hidden=(8,), v_hidden=(8,), device="cpu", seed=s), True)),
    ("RainbowNet-plain", (lambda s: N.RainbowNet(**_RAINBOW, dueling=False, noisy_std=None, device="cpu", seed=s), True)),
    ("BranchingNet", (lambda s: N.BranchingNet(state_shape=(6,), num_branches=3, action_per_branch=4, common_hidden_sizes=[12, 8],
                                               value_hidden_sizes=[8], action_hidden_sizes=[8], device="cpu", seed=s), True)),
    ("MLPActorCritic", (lambda s: N.MLPActorCritic(6, 4, (12, 8), device="cpu", seed=s), True)),
    ("MLPActorCritic-uniform", (lambda s: N.MLPActorCritic(6, 4, (12, 8), device="cpu", seed=s, init="uniform"), True)),
    ("DiscreteActorCritic", (lambda s: N.DiscreteActorCritic(6, 4, 64, device="cpu", seed=s), True)),
    ("DiscreteActorCritic-uniform", (lambda s: N.DiscreteActorCritic(6, 4, 64, device="cpu", seed=s, init="uniform"), True)),
    ("IntrinsicCuriosityModule", (_icm, False)),
    ("QMIXMixer", (lambda s: QMIXMixer(3, 10, 32, 16, device="cpu", seed=s), True)),
])


def checkpoint(net) -> OrderedDict:
    """The net's checkpoint under the reference's names."""
    return net.to_reference_state_dict()


def adam_shapes(net) -> list[list[int]]:
    """The ordered shapes of `FlatAdam(net).state_dict()["state"]` once a step has been taken."""
    opt = N.FlatAdam(net)
    opt.step_count = 1
    return [list(e["exp_avg"].shape) for e in opt.state_dict()["state"].values()]


def record(name: str, checkpoint_of=checkpoint) -> tuple[dict, dict]:
    """-> (arrays, meta) of one case: the flat vector and that of its lagged copy; checkpoint keys and shapes, Adam shapes."""
    make, has_twin = CASES[name]
    net = make(SEED)
    sd = checkpoint_of(net)
    arrays = {f"{name}/flat": net.flat.data.numpy().copy()}
    if has_twin:
        arrays[f"{name}/lagged"] = N.lagged_copy(net).flat.data.numpy().copy()
    return arrays, dict(keys=list(sd), shapes=[list(v.shape) for v in sd.values()], adam=adam_shapes(net))


def load_fixture(path: str) -> tuple[dict, dict]:
    with np.load(path) as z:
        return {k: z[k] for k in z.files if k != "meta"}, json.loads(str(z["meta"]))
