"""BCQ's update at the reference test's shape raised to the mujoco size (examples/offline/offline_bcq.py: hidden 256-256, VAE
hidden 512-512, B 256, num_sampled_action 10, obs 17, act 6, latent 12) on a filled device buffer, and acting at 10 observations
with forward_sampled_times 100.

    python tools/bench_bcq.py stacked [--updates 10] [--warmup 2]   # `BCQ.update`: ONE decoder pass over the B K + B rows
    python tools/bench_bcq.py split   [--updates 10] [--warmup 2]   # the target's rows and the actor's rows in two decoder calls
    python tools/bench_bcq.py act     [--updates 10] [--warmup 2]   # `BCQPolicy.act_device` on 10 observations, S = 100

Prints the entry points of include/tsmarl.h called per update (each is one launch, or one launch per layer for the dense
products) and the wall time per update by device events (launch-bound: it includes the host's share).  For per-kernel durations
run a mode under `rocprofv3 --kernel-trace --stats` in a run of its own; every count is then warmup + updates calls."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cql import _Box, timed  # noqa: E402
from tianshou_marl_amd import ops  # noqa: E402
from tianshou_marl_amd.algorithm import BCQ, BCQPolicy  # noqa: E402
from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou_marl_amd.data import Batch  # noqa: E402
from tianshou_marl_amd.data.buffer import VectorReplayBuffer  # noqa: E402
from tianshou_marl_amd.utils.net import VAE, ContinuousCritic, Perturbation  # noqa: E402

HID, VHID, B, K, D, AD, L, N_ACT, S, DEV = (256, 256), (512, 512), 256, 10, 17, 6, 12, 10, 100, "cuda"


class SplitBCQ(BCQ):
    """The reference's call shape: `decode(obs_next)` and `decode(obs)` as two passes of the decoder, on the same rows."""

    def _decode(self, w, obs_next, obs, z):
        vae, D_, BK = self.policy.vae, self.policy.obs_dim, obs_next.shape[0] * self.num_sampled_action
        for sl, src, rep in ((slice(0, BK), obs_next, self.num_sampled_action), (slice(BK, None), obs, 1)):
            xd = ops.bcq_decode_rows(src, rep, None, z[sl], out=w["xd"][sl])
            ops.bcq_action_rows(vae.decode_rows(xd), xd, D_, vae.max_action, out=w["X"][sl])
        return w["X"]


def make(cls):
    opt = lambda: AdamOptimizerFactory(lr=1e-3)  # noqa: E731
    policy = BCQPolicy(actor_perturbation=Perturbation(obs_dim=D, act_dim=AD, hidden_sizes=HID, device=DEV, seed=0),
                       action_space=_Box(AD), critic=ContinuousCritic(D, AD, HID, device=DEV, seed=1),
                       vae=VAE(encoder_hidden_sizes=VHID, decoder_hidden_sizes=VHID, obs_dim=D, act_dim=AD, latent_dim=L, device=DEV,
                               seed=3), forward_sampled_times=S)
    algo = cls(policy=policy, actor_perturbation_optim=opt(), critic_optim=opt(), vae_optim=opt(),
               critic2=ContinuousCritic(D, AD, HID, device=DEV, seed=2), num_sampled_action=K)
    algo.is_within_training_step = True
    return algo


def update_fn(cls):
    algo = make(cls)
    n_env, steps = 8, 256
    buf = VectorReplayBuffer(n_env * steps, n_env, n_agent=1, obs_dim=D, device=DEV, act_dim=AD)
    rs = np.random.RandomState(0)
    for _ in range(steps):
        f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
        buf.add(Batch(obs=f(n_env, 1, D), act=np.tanh(f(n_env, 1, AD)), rew=f(n_env, 1), terminated=rs.rand(n_env) < 0.02,
                      truncated=np.zeros(n_env, bool), obs_next=f(n_env, 1, D)), buffer_ids=np.arange(n_env))
    return lambda: algo.update(buf, B)


def act_fn():
    policy = make(BCQ).policy
    obs = torch.randn(N_ACT, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    return lambda: policy.act_device(obs)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["stacked", "split", "act"])
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    fn = act_fn() if args.mode == "act" else update_fn(BCQ if args.mode == "stacked" else SplitBCQ)
    ms, calls = timed(fn, args.warmup, args.updates)
    per = {k: v / args.updates for k, v in sorted(calls.items())}
    shape = f"n {N_ACT} S {S}" if args.mode == "act" else f"B {B} K {K}"
    print(f"{args.mode}: hidden {HID} VAE hidden {VHID} {shape} obs {D} act {AD} latent {L}: {ms:.4f} ms per call by device events "
          f"({args.updates} calls after {args.warmup}); {sum(per.values()):g} entry-point calls per call")
    for k, v in per.items():
        print(f"  {k:28s} {v:g}")


if __name__ == "__main__":
    main()
