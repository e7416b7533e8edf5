"""MADDPG timings at N 8, D 48, Ad 5, H 128: `MADDPGPolicy.learn` at B 4096 and `act_device` per vector step at 4096 envs,
against the float32 torch-autograd restatement of the same step on the same GPU (tests/maddpg_restatement.py).  Device
events after a warm-up; 7 runs, HIP and torch alternating, in one process.

    python tools/bench_maddpg.py [--iters 20] [--runs 7] [--one-learn]

--one-learn: warm up, then run a single `learn` (for a kernel trace of one call)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from maddpg_restatement import MaddpgRestatement  # noqa: E402
from tianshou_marl_amd.algorithm.multiagent.ctde import DecentralizedActor, MADDPGPolicy  # noqa: E402
from tianshou_marl_amd.data import Batch  # noqa: E402
from tianshou_marl_amd.utils.net import FlatMLP  # noqa: E402


class _Box:
    def __init__(self, n):
        self.shape, self.low, self.high = (n,), np.full(n, -1.0, np.float32), np.full(n, 1.0, np.float32)


def timed(fn, iters: int) -> float:
    """ms per call over `iters` calls, by device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--one-learn", action="store_true")
    args = ap.parse_args()
    N, D, Ad, H, B = 8, 48, 5, 128, 4096
    W, dev = N * (D + Ad), "cuda"
    pol = MADDPGPolicy([DecentralizedActor(D, Ad, H, device=dev, seed=i) for i in range(N)],
                       [FlatMLP([W, H, H, 1], device=dev, seed=50 + i) for i in range(N)], None, _Box(Ad), N,
                       noise_std=0.1, clip_actions=True,
                       async_stats=True)  # (neither side waits for its statistics inside the timed loop)
    g = torch.Generator(device=dev).manual_seed(0)
    obs = torch.randn(N, B, D, device=dev, generator=g)
    obs_next = torch.randn(N, B, D, device=dev, generator=g)
    act = torch.rand(N, B, Ad, device=dev, generator=g) * 2 - 1
    rew = torch.randn(N, B, device=dev, generator=g)
    term = torch.rand(N, B, device=dev, generator=g) < 0.1
    batch = Batch(**{f"agent_{i}": Batch(obs=obs[i], act=act[i], rew=rew[i], obs_next=obs_next[i], terminated=term[i])
                     for i in range(N)})
    R = MaddpgRestatement(pol.flat, N, [D, H, H, Ad], [W, H, H, 1], dtype=torch.float32, device=dev)

    def hip_learn():
        pol.learn(batch)

    def torch_learn():  # (no gradient export, no host synchronisation)
        R.learn(obs, act, rew, obs_next, term, want_grads=False)

    if args.one_learn:
        for _ in range(3):
            hip_learn()
        torch.cuda.synchronize()
        hip_learn()
        torch.cuda.synchronize()
        return

    env_obs = obs.transpose(0, 1).contiguous()  # [E, N, D]: the Collector's layout
    out = dict(act=torch.empty(B * N, Ad, device=dev), logp=torch.empty(B * N, device=dev), value=torch.empty(B * N, device=dev))
    tick = torch.zeros(1, dtype=torch.int64, device=dev)

    def hip_act():
        pol.act_device(env_obs, out=out, offset_dev=tick)

    def torch_act():  # the reference's forward on the device plus the caller's noise and clamp
        with torch.no_grad():
            for i in range(N):
                mu = R._mlp(R.params[i], env_obs[:, i])
                out["act"].view(B, N, Ad)[:, i] = (mu + 0.1 * torch.randn_like(mu)).clamp_(-1.0, 1.0)

    lines = []
    for label, fh, ft in (("learn B 4096", hip_learn, torch_learn), ("act_device per step, 4096 envs", hip_act, torch_act)):
        for f in (fh, ft, fh, ft):  # warm-up
            f()
        torch.cuda.synchronize()
        th, tt = [], []
        for _ in range(args.runs):
            th.append(timed(fh, args.iters))
            tt.append(timed(ft, args.iters))
        mh, mt = float(np.median(th)), float(np.median(tt))
        lines.append(f"{label}: HIP median {mh:.4f} ms (spread {max(th) - min(th):.4f}; runs "
                     + " ".join(f"{x:.4f}" for x in th) + f")  torch-f32 restatement median {mt:.4f} ms (spread "
                     f"{max(tt) - min(tt):.4f}; runs " + " ".join(f"{x:.4f}" for x in tt) + f")  ratio HIP/torch {mh / mt:.3f}")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
