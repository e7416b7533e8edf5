"""The learned global states of CTDE at the C3 shape (N 8 agents, obs 48, hidden 64) on B joint rows: `AttentionStateNet` and
`GraphStateNet` forward, and forward + backward (gradient slabs of the whole vector), by device events; beside them torch's own
`nn.MultiheadAttention(48, 4, batch_first=True)` + mean over agents + `nn.Linear(48, 64)`, forward and forward + autograd
backward, on the same device -- the only yardstick there is: the reference has no GPU path.

    timeout -k 10 120 python tools/bench_gstate.py attention [--rows 4096] [--iters 50] [--warmup 10]
    timeout -k 10 120 python tools/bench_gstate.py graph     [--rows 102400]
    timeout -k 10 120 python tools/bench_gstate.py torch     [--rows 4096]
    timeout -k 10 120 python tools/bench_gstate.py kernels   [--rows 4096]    # the four kernels of csrc/gstate.hip alone

Every GPU step runs under a time limit of its own, as above.  For per-kernel durations and launch counts run a mode under
`rocprofv3 --kernel-trace --stats` in a run of its own; every count is then (warmup + iters) calls of each timed function.  The
inputs are fixed normal draws, far from zero-filled, so data-dependent power states see ordinary operands."""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tianshou_marl_amd import ops  # noqa: E402
from tianshou_marl_amd.utils.net import AttentionStateNet, GraphStateNet  # noqa: E402

N, D, H, DEV = 8, 48, 64, "cuda"


def timed(fn, warmup: int, iters: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def inputs(B: int):
    g = torch.Generator(device=DEV).manual_seed(0)
    return torch.randn(B, N, D, device=DEV, generator=g), torch.randn(B, H, device=DEV, generator=g) / B


def net_cases(net, B: int) -> dict:
    obs, d_state = inputs(B)

    def both():
        net.forward(obs, save=True)
        net.backward(d_state)

    return {"forward": lambda: net.forward(obs, save=False), "forward + backward": both}


def torch_cases(B: int) -> dict:
    torch.manual_seed(0)
    mha = torch.nn.MultiheadAttention(D, 4, batch_first=True).to(DEV)
    proj = torch.nn.Linear(D, H).to(DEV)
    obs, d_state = inputs(B)
    params = list(mha.parameters()) + list(proj.parameters())

    def fwd():
        return proj(mha(obs, obs, obs, need_weights=False)[0].mean(dim=1))

    def no_grad():
        with torch.no_grad():
            fwd()

    def both():
        for p in params:
            p.grad = None
        (fwd() * d_state).sum().backward()

    return {"forward": no_grad, "forward + backward": both}


def kernel_cases(B: int) -> dict:
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv, d_ctx = torch.randn(B, N, 3 * D, device=DEV, generator=g), torch.randn(B, D, device=DEV, generator=g)
    h, d = torch.randn(B, N, H, device=DEV, generator=g), torch.randn(B, H, device=DEV, generator=g)
    c = torch.full((N,), 1.0 / N, device=DEV)
    _, P = ops.attn_pool_forward(qkv, N)
    return {"tsm_attn_pool_forward": lambda: ops.attn_pool_forward(qkv, N),
            "tsm_attn_pool_backward": lambda: ops.attn_pool_backward(d_ctx, qkv, P),
            "tsm_agent_pool_forward": lambda: ops.agent_pool_forward(h, c, relu=True),
            "tsm_agent_pool_backward": lambda: ops.agent_pool_backward(d, c, N, h_relu=h)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["attention", "graph", "torch", "kernels"])
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    B = args.rows
    if args.mode == "attention":
        cases = net_cases(AttentionStateNet(D, N, H, device=DEV, seed=0), B)
    elif args.mode == "graph":
        cases = net_cases(GraphStateNet(D, N, H, device=DEV, seed=0), B)
    elif args.mode == "torch":
        cases = torch_cases(B)
    else:
        cases = kernel_cases(B)
    for name, fn in cases.items():
        ms = timed(fn, args.warmup, args.iters)
        print(f"{args.mode} N {N} D {D} hidden {H} B {B}: {name}: {ms:.4f} ms by device events ({args.iters} calls after "
              f"{args.warmup})", flush=True)


if __name__ == "__main__":
    main()
