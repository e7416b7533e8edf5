#!/usr/bin/env python
"""Collect time under Box actions: the persistent Gaussian rollout and the per-step device loop (eager launches, captured graph)
against the host loop.

Job: Collector.collect(n_step = 25 * E) on continuous simple_spread, N = 3, E = 1024, a 64-64 Gaussian GenericPPO sampling within
a training step.  Four ways to run it:
  device-fused     the whole collect in one launch of the persistent Gaussian rollout (csrc/rollout_gauss.hip; the default)
  device-eager     the per-step loop (fused_rollout=False, as the two modes below): env.step_device fed from the policy's env_act
                   in HBM, use_graph=False
  device-captured  the same loop replayed as one captured graph (use_graph=True; engaged from the second collect)
  host-loop        what a Gaussian policy had before the Box step kernels: the Collector's host loop over the env's numpy
                   `step()` -- per vector step one D2H copy of the actions, one H2D copy into the env, D2H of its results and
                   an H2D add into the buffer (the env is hidden behind a view without `step_device`)
Every collect is timed with device events around the call and a synchronise behind it; the modes alternate within a round, so
drift of the machine falls on all of them alike.  Warm-up: 3 collects per mode (first launches, the graph's capture).
Prints one line per mode (median / min / max over the rounds) and one JSON line; --out appends both to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tianshou_marl_amd.algorithm import GenericPPO, policy_within_training_step  # noqa: E402
from tianshou_marl_amd.data import Collector, VectorReplayBuffer  # noqa: E402
from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv  # noqa: E402
from tianshou_marl_amd.utils.net import GaussianActorCritic  # noqa: E402


class HostView:
    """The env's reference-style numpy API alone (no `step_device`): the Collector takes its host loop.  Observations go as
    plain [rows, N, D] arrays."""

    def __init__(self, env) -> None:
        self._env, self.n_agent, self.obs_dim, self.action_space = env, env.n_agent, env.obs_dim, env.action_space
        env._obs_dicts = lambda obs, ids: np.ascontiguousarray(obs[ids])

    def __len__(self) -> int:
        return len(self._env)

    def reset(self, env_id=None, **kw):
        return self._env.reset(env_id, **kw)

    def step(self, action, id=None):  # noqa: A002
        return self._env.step(action, id)


def make(mode: str, E: int, N: int, T: int):
    env = DeviceSimpleSpreadVectorEnv(E, N, max_cycles=25, device="cuda", seed=1, continuous_actions=True,
                                      auto_reset=mode != "host-loop")
    net = GaussianActorCritic(env.obs_dim, env.act_dim, (64, 64), act="tanh", device="cuda", seed=5)
    algo = GenericPPO(net=net, dispatch="pooled", seed=11, action_scaling=True, action_bound_method="clip",
                      action_space=env.action_space[0])
    buf = VectorReplayBuffer(E * T, E, act_dim=env.act_dim, device="cuda")
    col = Collector(algo, HostView(env) if mode == "host-loop" else env, buf, use_graph=mode == "device-captured",
                    fused_rollout=mode == "device-fused")
    col.reset()
    assert col._can_fuse() == (mode == "device-fused")
    return algo, buf, col


def timed_collect(algo, buf, col, n_step: int) -> float:
    buf.reset()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    with policy_within_training_step(algo):
        st = col.collect(n_step=n_step)
    t1.record()
    torch.cuda.synchronize()
    assert st.n_collected_steps == n_step and buf.act_store.abs().sum() > 0
    return t0.elapsed_time(t1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--steps", type=int, default=25, help="vector steps per collect")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--host-rounds", type=int, default=3, help="the host loop is timed in the first so many rounds")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_collect.py measures on the GPU; there is none here")
    modes = ("device-fused", "device-eager", "device-captured", "host-loop")
    n_step = a.steps * a.envs
    jobs = {m: make(m, a.envs, a.agents, a.steps) for m in modes}
    for m in modes:
        for _ in range(3 if m != "host-loop" else 1):
            timed_collect(*jobs[m], n_step)
    ms = {m: [] for m in modes}
    for r in range(a.rounds):
        for m in modes:
            if m != "host-loop" or r < a.host_rounds:
                ms[m].append(timed_collect(*jobs[m], n_step))
    lines = [f"collect(n_step = {a.steps} * {a.envs}), simple_spread N = {a.agents}, Box(5) actions, Gaussian GenericPPO 64-64, "
             f"{torch.cuda.get_device_name(0)}; ms per collect, device events"]
    res = {}
    for m in modes:
        res[m] = dict(median_ms=statistics.median(ms[m]), min_ms=min(ms[m]), max_ms=max(ms[m]), n=len(ms[m]))
        lines.append(f"  {m:16s} median {res[m]['median_ms']:9.3f}  min {res[m]['min_ms']:9.3f}  max {res[m]['max_ms']:9.3f}  "
                     f"(n = {len(ms[m])}; {res[m]['median_ms'] * 1e3 / a.steps:8.1f} us per vector step)")
    lines.append(json.dumps(dict(envs=a.envs, agents=a.agents, steps=a.steps, **res)))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
