"""CQL's update at the reference's mujoco configuration (examples/offline/d4rl_cql.py: hidden 256-256, B 256, num_repeat_actions
10, obs 17, act 6, Lagrange multiplier on, calibrated) on a filled device buffer, and the same critic-side work as the four
separate forwards and backwards per critic that a call-by-call port would launch (data rows, uniform actions, policy actions at
obs and at obs_next), through the same `FlatMLP`s.

    python tools/bench_cql.py cql   [--updates 10] [--warmup 2]   # `CQL.update`: one stacked forward / backward per critic
    python tools/bench_cql.py split [--updates 10] [--warmup 2]   # per critic 4 forwards and 4 backwards on rows of the same shapes

Prints the entry points of include/tsmarl.h called per update (each is one launch, or one launch per layer for the dense
products; tsm_td3bc_actor_head is two) and the wall time per update by device events (launch-bound: it includes the host's
share).  For per-kernel durations run either mode under `rocprofv3 --kernel-trace --stats` in a run of its own; every count is
then warmup + updates calls."""
from __future__ import annotations

import argparse
import os
import sys
from collections import Counter

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tianshou_marl_amd import ops  # noqa: E402
from tianshou_marl_amd.algorithm import CQL, SACPolicy  # noqa: E402
from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou_marl_amd.data import Batch  # noqa: E402
from tianshou_marl_amd.data.buffer import VectorReplayBuffer  # noqa: E402
from tianshou_marl_amd.utils.net import ContinuousActorProbabilistic, ContinuousCritic, FlatAdam  # noqa: E402

HID, B, R, D, AD, DEV = (256, 256), 256, 10, 17, 6, "cuda"


class _Box:
    def __init__(self, n):
        self.shape, self.low, self.high = (n,), np.full(n, -1.0, np.float32), np.full(n, 1.0, np.float32)


def timed(fn, warmup: int, updates: int) -> tuple[float, Counter]:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    calls, real = Counter(), ops.call

    def counting(name, *args):
        calls[name] += 1
        return real(name, *args)

    ops.call = counting
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        a.record()
        for _ in range(updates):
            fn()
        b.record()
        b.synchronize()
    finally:
        ops.call = real
    return a.elapsed_time(b) / updates, calls


def cql_update():
    opt = lambda: AdamOptimizerFactory(lr=3e-4)  # noqa: E731
    actor = ContinuousActorProbabilistic(D, AD, HID, conditioned_sigma=True, device=DEV, seed=0)
    algo = CQL(policy=SACPolicy(actor=actor, action_space=_Box(AD)), policy_optim=opt(),
               critic=ContinuousCritic(D, AD, HID, device=DEV, seed=1), critic_optim=opt(),
               critic2=ContinuousCritic(D, AD, HID, device=DEV, seed=2), num_repeat_actions=R)
    algo.is_within_training_step = True
    n_env, S = 8, 256
    buf = VectorReplayBuffer(n_env * S, n_env, n_agent=1, obs_dim=D, device=DEV, act_dim=AD)
    rs = np.random.RandomState(0)
    for _ in range(S):
        f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
        buf.add(Batch(obs=f(n_env, 1, D), act=np.tanh(f(n_env, 1, AD)), rew=f(n_env, 1), terminated=rs.rand(n_env) < 0.02,
                      truncated=np.zeros(n_env, bool), obs_next=f(n_env, 1, D)), buffer_ids=np.arange(n_env))
    algo.process_buffer(buf)
    return lambda: algo.update(buf, B)


def split_update():
    nets = [ContinuousCritic(D, AD, HID, device=DEV, seed=1 + e) for e in range(2)]
    adams = [FlatAdam(n, lr=3e-4, coef64=True, max_grad_norm=1.0) for n in nets]
    g = torch.Generator(device=DEV).manual_seed(0)
    xs = [torch.randn(n, D + AD, device=DEV, generator=g) for n in (B, B * R, B * R, B * R)]
    dqs = [torch.randn(x.shape[0], 1, device=DEV, generator=g) / x.shape[0] for x in xs]
    slabs = [[torch.empty(ops.mlp_n_split(x.shape[0]), n.flat.numel(), device=DEV) for x in xs] for n in nets]

    def update():
        for n, a, sl in zip(nets, adams, slabs):
            for x, dq, s in zip(xs, dqs, sl):   # autograd keeps every forward's activations; here each backward follows its forward
                n.forward(x, save=True)
                n.backward(dq, slabs=s)
            a.step(sl[0])

    return update


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["cql", "split"])
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    fn = cql_update() if args.mode == "cql" else split_update()
    ms, calls = timed(fn, args.warmup, args.updates)
    per = {k: v / args.updates for k, v in sorted(calls.items())}
    print(f"{args.mode}: hidden {HID} B {B} R {R} obs {D} act {AD}: {ms:.4f} ms per update by device events "
          f"({args.updates} updates after {args.warmup}); {sum(per.values()):g} entry-point calls per update")
    for k, v in per.items():
        print(f"  {k:28s} {v:g}")


if __name__ == "__main__":
    main()
