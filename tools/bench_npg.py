"""NPG's hot path at the two actor shapes of the MPE jobs, B 4096: one Fisher-vector product (tangent forward, Fisher head,
backward: `ops.fisher_vector_product`) and one minibatch update (`NPG._minibatch`: gradient, ten CG iterations, the step, the KL
and optim_critic_iters = 5 critic steps).

    python tools/bench_npg.py [--updates 100] [--warmup 3]   # the product is timed over 50 x as many calls as the update

Prints, per shape, the entry points of include/tsmarl.h called per call (each is one launch, or one launch per layer for the
dense products) and the wall time per call by device events (launch-bound: it includes the host's share).  For per-kernel
durations run it under `rocprofv3 --kernel-trace --stats` in a run of its own."""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cql import timed  # noqa: E402
from tianshou_marl_amd import ops  # noqa: E402
from tianshou_marl_amd.algorithm import NPG  # noqa: E402
from tianshou_marl_amd.utils.net import MLPActorCritic  # noqa: E402

B, DEV = 4096, "cuda"
SHAPES = [(18, (64, 64), 5), (48, (128, 128), 5)]


def cases(D: int, hidden, A: int):
    g = torch.Generator(device=DEV).manual_seed(0)
    net = MLPActorCritic(D, A, hidden, act="tanh", device=DEV, seed=1)
    algo = NPG(net=net, lr=1e-3, dispatch="pooled")
    obs = torch.randn(B, D, device=DEV, generator=g)
    act = torch.randint(0, A, (B,), device=DEV, generator=g).to(torch.int32)
    adv, ret = torch.randn(B, device=DEV, generator=g), torch.randn(B, device=DEV, generator=g)
    logp_old, _ = ops.categorical_logp_entropy(net.actor.forward(obs, save=True), act)
    pb = dict(obs=obs, act=act, adv=adv, ret=ret, logp_old=logp_old, joint=None, n_agent=1)
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    v = torch.randn(net.actor.flat.numel(), device=DEV, generator=g)
    n_split, ws = ops.mlp_n_split(B), {}
    slabs = torch.empty(n_split, v.numel(), dtype=torch.float32, device=DEV)
    theta = net.flat.data.clone()

    def update():
        net.flat.data.copy_(theta)   # every call steps from the same parameters
        algo._minibatch(pb, adv, idx)

    return {"fvp": lambda: ops.fisher_vector_product(net.actor, v, n_split, slabs=slabs, ws=ws), "update": update}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for D, hidden, A in SHAPES:
        for name, fn in cases(D, hidden, A).items():
            n = args.updates * (50 if name == "fvp" else 1)   # (a product is 0.1 ms: time enough of them)
            ms, calls = timed(fn, args.warmup, n)
            per = {k: v / n for k, v in sorted(calls.items())}
            print(f"{name}: {D}-{'-'.join(map(str, hidden))}-{A} tanh B {B}: {ms:.4f} ms per call by device events "
                  f"({n} calls after {args.warmup}); {sum(per.values()):g} entry-point calls per call")
            for k, c in per.items():
                print(f"  {k:30s} {c:g}")


if __name__ == "__main__":
    main()
