"""REDQ's update at the reference's mujoco configuration (examples/mujoco/mujoco_redq.py: E 10, M 2, hidden 256-256, B 256, obs 17,
act 6, actor_delay 20) for a kernel trace, and the same critic-side work expressed as E separate `ContinuousCritic`s through
`tsm_mlp_*` -- what the learner would launch without the grouped ensemble product.

    python tools/bench_redq.py redq  [--updates 10] [--warmup 2]   # `REDQ.update` on a filled device buffer
    python tools/bench_redq.py split [--updates 10] [--warmup 2]   # per update: E lagged forwards, E forwards, E backwards,
                                                                   # E Adam steps, E Polyak moves on rows of the same shape

Run each under `rocprofv3 --kernel-trace --stats` in a run of its own; every count is then warmup + updates calls.  Prints the
wall time per update by device events as well (launch-bound: it includes the host's share)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tianshou_marl_amd import ops  # noqa: E402
from tianshou_marl_amd.algorithm import REDQ, REDQPolicy  # noqa: E402
from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou_marl_amd.data import Batch  # noqa: E402
from tianshou_marl_amd.data.buffer import VectorReplayBuffer  # noqa: E402
from tianshou_marl_amd.utils.net import (ContinuousActorProbabilistic, ContinuousCritic, EnsembleCritic, FlatAdam,  # noqa: E402
                                         lagged_copy)

E, M, HID, B, D, AD, DEV = 10, 2, (256, 256), 256, 17, 6, "cuda"


class _Box:
    def __init__(self, n):
        self.shape, self.low, self.high = (n,), np.full(n, -1.0, np.float32), np.full(n, 1.0, np.float32)


def timed(fn, warmup: int, updates: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(updates):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / updates


def redq_update():
    opt = lambda: AdamOptimizerFactory(lr=1e-3)  # noqa: E731
    actor = ContinuousActorProbabilistic(D, AD, HID, conditioned_sigma=True, device=DEV, seed=0)
    algo = REDQ(policy=REDQPolicy(actor=actor, action_space=_Box(AD)), policy_optim=opt(),
                critic=EnsembleCritic(D, AD, E, HID, device=DEV, seed=1), critic_optim=opt(), ensemble_size=E, subset_size=M)
    algo.is_within_training_step = True
    n_env, S = 8, 256
    buf = VectorReplayBuffer(n_env * S, n_env, n_agent=1, obs_dim=D, device=DEV, act_dim=AD)
    rs = np.random.RandomState(0)
    for _ in range(S - 1):
        f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
        buf.add(Batch(obs=f(n_env, 1, D), act=np.tanh(f(n_env, 1, AD)), rew=f(n_env, 1), terminated=rs.rand(n_env) < 0.02,
                      truncated=np.zeros(n_env, bool), obs_next=f(n_env, 1, D)), buffer_ids=np.arange(n_env))
    np.random.seed(0)
    return lambda: algo.update(buf, B)


def split_update():
    nets = [ContinuousCritic(D, AD, HID, device=DEV, seed=1 + e) for e in range(E)]
    olds = [lagged_copy(n) for n in nets]
    adams = [FlatAdam(n, lr=1e-3, coef64=True) for n in nets]
    g = torch.Generator(device=DEV).manual_seed(0)
    x, x_next = torch.randn(B, D + AD, device=DEV, generator=g), torch.randn(B, D + AD, device=DEV, generator=g)
    dq = torch.randn(B, 1, device=DEV, generator=g) / B
    slabs = [torch.empty(ops.mlp_n_split(B), n.flat.numel(), device=DEV) for n in nets]

    def update():
        for o in olds:
            o.forward(x_next, save=False)
        for n, a, s in zip(nets, adams, slabs):
            n.forward(x, save=True)
            n.backward(dq, slabs=s)
            a.step(s)
        for o, n in zip(olds, nets):
            ops.polyak(o.flat.data, n.flat.data, 0.005)

    return update


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["redq", "split"])
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    fn = redq_update() if args.mode == "redq" else split_update()
    ms = timed(fn, args.warmup, args.updates)
    print(f"{args.mode}: E {E} M {M} hidden {HID} B {B} obs {D} act {AD}: {ms:.4f} ms per update by device events "
          f"({args.updates} updates after {args.warmup})")


if __name__ == "__main__":
    main()
