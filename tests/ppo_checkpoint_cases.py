"""The on-policy learners at one small shape each, built on the CPU with a planted optimizer state, and what
tests/golden/ppo_checkpoint_layout.npz pins of their `state_dict()` (tests/golden/make_ppo_checkpoint_fixtures.py writes it,
tests/test_host_ppo_checkpoint.py reads it).  The fused net is 6 -> 64 -> 64 -> (4 | 1), the only hidden width it has; the general
one 6 -> 12 -> 8 -> (4 | 1)."""
from __future__ import annotations

import json
from collections import OrderedDict

import numpy as np
import torch

from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory, LRSchedulerFactoryLinear
from tianshou_marl_amd.algorithm.pg import A2C, Reinforce
from tianshou_marl_amd.algorithm.ppo import PPO
from tianshou_marl_amd.algorithm.ppo_generic import GenericPPO
from tianshou_marl_amd.utils.net import DiscreteActorCritic, MLPActorCritic

SEED = 3


def _fused(seed):
    return DiscreteActorCritic(6, 4, 64, device="cpu", seed=seed)


def _scheduled(seed):
    optim = AdamOptimizerFactory(lr=3e-4).with_lr_scheduler_factory(LRSchedulerFactoryLinear(2, 100, 50))
    return PPO(net=_fused(seed), optim=optim, device="cpu")


# name -> make(seed) on the CPU
CASES = OrderedDict([
    ("PPO", lambda s: PPO(net=_fused(s), lr=3e-4, device="cpu")),
    ("PPO-scheduled", _scheduled),
    ("GenericPPO", lambda s: GenericPPO(net=MLPActorCritic(6, 4, (12, 8), device="cpu", seed=s), lr=3e-4, device="cpu")),
])
# the learners a snapshot (`copy.deepcopy`) is checked of: one of every class, a subclass with constructor arguments of its own
# (a snapshot is built without the scheduler factory: it is an opponent, not a learner)
SNAPSHOT_CASES = OrderedDict({k: CASES[k] for k in ("PPO", "GenericPPO")}, **{
    "A2C": lambda s: A2C(net=_fused(s), lr=3e-4, vf_coef=0.25, max_grad_norm=0.5, device="cpu"),
    "Reinforce": lambda s: Reinforce(net=_fused(s), lr=3e-4, gamma=0.9, return_standardization=True, device="cpu"),
})


def plant(algo):
    """A state no constructor gives: moments that differ in every element, three optimizer steps, counters, return statistics,
    a scheduler (where there is one) that has moved."""
    n = algo.net.flat.numel()
    ramp = torch.arange(n, dtype=torch.float32)
    algo.exp_avg.copy_(ramp / n - 0.5)
    algo.exp_avg_sq.copy_((ramp + 1.0) / (4 * n))
    algo.opt_step = 3
    algo._sample_ctr = 11
    algo._perm_ctr.fill_(5)
    algo.ret_rms.dev.copy_(torch.tensor([0.25, 2.0, 7.0], dtype=torch.float64))
    for s in algo.lr_schedulers:   # one update into the schedule: `lr` has left `initial_lr`
        s.step()
    return algo


def layout(sd) -> tuple[dict, dict]:
    """-> (arrays, meta) of a learner's `state_dict()`: the ordered keys with the parameter shapes; of `_optimizers[0]` the state's
    indices, step counts and moments (arrays), `param_groups[0]` whole, and `tsm_engine` with `ret_rms` as an array."""
    opt, = sd["_optimizers"]
    assert list(opt) == ["state", "param_groups", "tsm_engine"] and len(opt["param_groups"]) == 1
    arrays = {"ret_rms": opt["tsm_engine"]["ret_rms"].numpy().copy()}
    for i, e in opt["state"].items():
        assert list(e) == ["step", "exp_avg", "exp_avg_sq"]
        arrays[f"exp_avg/{i}"], arrays[f"exp_avg_sq/{i}"] = e["exp_avg"].numpy().copy(), e["exp_avg_sq"].numpy().copy()
    meta = dict(keys=list(sd), shapes=[list(v.shape) for k, v in sd.items() if k != "_optimizers"],
                state=[[i, float(e["step"])] for i, e in opt["state"].items()], group=opt["param_groups"][0],
                engine={k: v for k, v in opt["tsm_engine"].items() if k != "ret_rms"})
    return arrays, json.loads(json.dumps(meta))   # (as the fixture holds it: tuples are lists)


def record(name: str) -> tuple[dict, dict]:
    arrays, meta = layout(plant(CASES[name](SEED)).state_dict())
    return {f"{name}/{k}": v for k, v in arrays.items()}, meta


def load_fixture(path: str) -> tuple[dict, dict]:
    with np.load(path) as z:
        return {k: z[k] for k in z.files if k != "meta"}, json.loads(str(z["meta"]))
