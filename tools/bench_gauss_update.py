#!/usr/bin/env python
"""Update time of a Gaussian GenericPPO over 64-64 nets: the one-launch gradient step (csrc/ppo_gauss.hip, `fused_actor=True`)
against the non-fused chain of general kernels (`fused_actor=False`: gathers, dense forwards, head, value loss, dense backwards,
sigma fold -- about twenty launches per minibatch), in the same process.

Job: continuous simple_spread, N = 3, E = 1024, one collect of T = 25 vector steps (76 800 rows), then on that buffer
  step     one gradient step (`_grad_step_gauss` on a fixed minibatch: the launches up to and including Adam and the loss
           statistics), eager launches, `--steps-per-window` of them between two device events
  update   one whole `update(buffer, batch_size, repeat=1)` as a user runs it (graph=True: replayed from the second call on)
at batch_size = None (the whole batch as one minibatch) and at batch_size = 64.  The two paths alternate within a round, so drift
of the machine falls on both alike.  Warm-up: 3 windows / updates per path and size (first launches, workspaces, the capture).
Prints per figure median / min / max over the rounds and one JSON line; --out appends both to a file."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tianshou_marl_amd import ops  # noqa: E402
from tianshou_marl_amd.algorithm import GenericPPO, policy_within_training_step  # noqa: E402
from tianshou_marl_amd.data import Collector, VectorReplayBuffer  # noqa: E402
from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv  # noqa: E402
from tianshou_marl_amd.utils.net import GaussianActorCritic  # noqa: E402


def make(fused: bool, E: int, N: int, T: int):
    env = DeviceSimpleSpreadVectorEnv(E, N, max_cycles=25, device="cuda", seed=1, continuous_actions=True)
    net = GaussianActorCritic(env.obs_dim, env.act_dim, (64, 64), act="tanh", device="cuda", seed=5)
    algo = GenericPPO(net=net, dispatch="pooled", shuffle="device", seed=11, lr=1e-4, value_clip=True, action_scaling=True,
                      action_bound_method="clip", action_space=env.action_space[0], fused_actor=fused)
    assert algo.fused_gauss == fused
    buf = VectorReplayBuffer(E * T, E, act_dim=env.act_dim, device="cuda")
    col = Collector(algo, env, buf)
    col.reset()
    with policy_within_training_step(algo):
        col.collect(n_step=E * T)
    return algo, buf


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed_steps(algo, buf, batch_size, k: int) -> float:
    """us per gradient step over k eager steps on one fixed minibatch."""
    pb = algo._preprocess_batch(buf)
    n = pb["obs"].shape[0]
    M = n if not batch_size else batch_size
    idx = torch.randperm(n, device="cuda", generator=torch.Generator("cuda").manual_seed(3))[:M].contiguous()
    stats = ops.ppo_adv_stats(pb["adv"], torch.tensor([0, M], device="cuda"), perm=idx)[0]
    t0, t1 = events()
    t0.record()
    for _ in range(k):
        algo._grad_step_gauss(pb, idx, stats, None, None)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / k


def timed_update(algo, buf, batch_size) -> float:
    """ms per update(buffer, batch_size, repeat=1)."""
    t0, t1 = events()
    t0.record()
    with policy_within_training_step(algo):
        st = algo.update(buf, batch_size, 1)
    t1.record()
    torch.cuda.synchronize()
    assert st.gradient_steps >= 1
    return t0.elapsed_time(t1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--steps", type=int, default=25, help="vector steps of the collect")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps-per-window", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gauss_update.py measures on the GPU; there is none here")
    paths, sizes = ("fused", "chain"), (None, 64)
    jobs = {p: make(p == "fused", a.envs, a.agents, a.steps) for p in paths}
    figs = {(kind, bs, p): [] for kind in ("step_us", "update_ms") for bs in sizes for p in paths}
    for rnd in range(-3, a.rounds):   # (negative rounds: warm-up, not recorded)
        for bs in sizes:
            for p in paths:
                s, u = timed_steps(*jobs[p], bs, a.steps_per_window), timed_update(*jobs[p], bs)
                if rnd >= 0:
                    figs[("step_us", bs, p)].append(s)
                    figs[("update_ms", bs, p)].append(u)
    lines = [f"Gaussian GenericPPO 64-64 (tanh), continuous simple_spread N = {a.agents}, E = {a.envs}, T = {a.steps}: "
             f"{a.envs * a.agents * a.steps} rows; {torch.cuda.get_device_name(0)}; device events, {a.rounds} rounds, "
             f"{a.steps_per_window} gradient steps per window"]
    res = {}
    for (kind, bs, p), v in figs.items():
        key = f"{kind}/batch_{bs or 'all'}/{p}"
        res[key] = dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))
        lines.append(f"  {key:32s} median {res[key]['median']:10.3f}  min {res[key]['min']:10.3f}  max {res[key]['max']:10.3f}")
    lines.append(json.dumps(dict(envs=a.envs, agents=a.agents, steps=a.steps, **res)))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
