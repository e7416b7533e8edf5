"""BDQN's update at the reference's BipedalWalker configuration (examples/box2d/bipedal_bdq.py: obs 24, K 4 branches of A 25
actions, common 512-256, value 128, action 128, B 512, target_update_freq 1000) for a kernel trace, and the same branch-side
work expressed as K separate `FlatMLP`s through `tsm_mlp_*` -- what the net would launch without the grouped ensemble product.

    timeout -k 10 120 python tools/bench_bdqn.py bdqn  [--updates 20] [--warmup 5]   # `BDQN.update` on a filled device buffer
    timeout -k 10 120 python tools/bench_bdqn.py split [--updates 20] [--warmup 5]   # per update: the K branches' three forwards,
                                                                                     # K backwards and K input gradients

Every GPU step runs under a time limit of its own, as above.  Run each under `rocprofv3 --kernel-trace --stats` in a run of its
own; every count is then warmup + updates calls.  Prints the wall time per update by device events as well (launch-bound: it
includes the host's share)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tianshou_marl_amd.algorithm import BDQN, BDQNPolicy  # noqa: E402
from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou_marl_amd.data import Batch  # noqa: E402
from tianshou_marl_amd.data.buffer import VectorReplayBuffer  # noqa: E402
from tianshou_marl_amd.env.spaces import Discrete  # noqa: E402
from tianshou_marl_amd.utils.net import BranchingNet, FlatMLP  # noqa: E402

D, K, A, COMMON, VALUE, ACTION, B, DEV = 24, 4, 25, [512, 256], [128], [128], 512, "cuda"


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


def bdqn_update():
    net = BranchingNet(state_shape=(D,), num_branches=K, action_per_branch=A, common_hidden_sizes=COMMON, value_hidden_sizes=VALUE,
                       action_hidden_sizes=ACTION, device=DEV, seed=0)
    algo = BDQN(policy=BDQNPolicy(model=net, action_space=Discrete(A)), optim=AdamOptimizerFactory(lr=1e-4), gamma=0.99,
                target_update_freq=1000)
    algo.is_within_training_step = True
    n_env, S = 8, 256
    buf = VectorReplayBuffer(n_env * S, n_env, n_agent=1, obs_dim=D, device=DEV, act_branches=K)
    rs = np.random.RandomState(0)
    for _ in range(S - 1):
        f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
        buf.add(Batch(obs=f(n_env, 1, D), act=rs.randint(0, A, (n_env, 1, K)), rew=f(n_env, 1), terminated=rs.rand(n_env) < 0.02,
                      truncated=np.zeros(n_env, bool), obs_next=f(n_env, 1, D)), buffer_ids=np.arange(n_env))
    return lambda: algo.update(buf, B)


def split_update():
    H = COMMON[-1]
    nets = [FlatMLP([H, *ACTION, A], device=DEV, seed=1 + k) for k in range(K)]
    g = torch.Generator(device=DEV).manual_seed(0)
    f, f_next = torch.randn(B, H, device=DEV, generator=g), torch.randn(B, H, device=DEV, generator=g)
    d_adv = torch.randn(B, A, device=DEV, generator=g) / B

    def update():
        for n in nets:
            n.forward(f_next, save=False)   # the online net on obs_next
            n.forward(f_next, save=False)   # the lagged net on obs_next (a net of the same shape)
            n.forward(f, save=True)
            n.backward(d_adv)
            n.input_grad(d_adv, 0, H)

    return update


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bdqn", "split"])
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    fn = bdqn_update() if args.mode == "bdqn" else split_update()
    ms = timed(fn, args.warmup, args.updates)
    print(f"{args.mode}: K {K} A {A} common {COMMON} value {VALUE} action {ACTION} B {B} obs {D}: {ms:.4f} ms per update by "
          f"device events ({args.updates} updates after {args.warmup})")


if __name__ == "__main__":
    main()
