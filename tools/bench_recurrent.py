"""The recurrent net at the reference's shape (`Recurrent`: hidden 128, 1 layer; obs 18, 5 actions) on B rows of L steps:
forward, and forward + backward (gradient slabs of the whole vector), by device events; beside them torch's own
`nn.Linear -> nn.LSTM(128, 128, 1, batch_first=True) -> nn.Linear` with the same weights on the same device, forward and
forward + autograd backward -- the only yardstick there is: the reference has no GPU path of its own.

    timeout -k 10 120 python tools/bench_recurrent.py hip     [--rows 64] [--steps 4] [--iters 50] [--warmup 10]
    timeout -k 10 120 python tools/bench_recurrent.py torch   [--rows 4096] [--steps 16]
    timeout -k 10 120 python tools/bench_recurrent.py update  [--rows 4096] [--steps 16]   # DQN.update on Recurrent
    timeout -k 10 120 python tools/bench_recurrent.py kernels [--rows 4096] [--steps 16]   # the two kernels of csrc/lstm.hip alone

Every GPU step runs under a time limit of its own, as above.  The inputs are fixed normal draws, far from zero-filled, so
data-dependent power states see ordinary operands.  `update`: a full `DQN.update(buffer, B)` on `Recurrent` (double-Q, lagged
net, n_step 3) over a `stack_num = L` buffer of 64 envs x 256 slots x 3 agents, agent 0: the sampling, the stacked gathers, three
forwards, the head, the backward, Adam and the loss read."""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tianshou_marl_amd import ops  # noqa: E402
from tianshou_marl_amd.utils.net import Recurrent  # noqa: E402

D, H, A, LAYERS, DEV = 18, 128, 5, 1, "cuda"


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


def inputs(B: int, L: int):
    g = torch.Generator(device=DEV).manual_seed(0)
    return torch.randn(B, L, D, device=DEV, generator=g), torch.randn(B, A, device=DEV, generator=g) / B


def hip_cases(B: int, L: int) -> dict:
    net = Recurrent(layer_num=LAYERS, state_shape=D, action_shape=A, hidden_layer_size=H, device=DEV, seed=0)
    obs, d_out = inputs(B, L)

    def both():
        net.forward(obs, save=True)
        net.backward(d_out)

    return {"forward": lambda: net.forward(obs, save=False), "forward + backward": both}


def torch_cases(B: int, L: int) -> dict:
    net = Recurrent(layer_num=LAYERS, state_shape=D, action_shape=A, hidden_layer_size=H, device=DEV, seed=0)
    sd = net.to_reference_state_dict()
    fc1, fc2 = torch.nn.Linear(D, H).to(DEV), torch.nn.Linear(H, A).to(DEV)
    lstm = torch.nn.LSTM(H, H, LAYERS, batch_first=True).to(DEV)
    lstm.load_state_dict({k[3:]: v for k, v in sd.items() if k.startswith("nn.")})
    fc1.load_state_dict({"weight": sd["fc1.weight"], "bias": sd["fc1.bias"]})
    fc2.load_state_dict({"weight": sd["fc2.weight"], "bias": sd["fc2.bias"]})
    obs, d_out = inputs(B, L)
    params = [*fc1.parameters(), *lstm.parameters(), *fc2.parameters()]

    def fwd():
        return fc2(lstm(fc1(obs))[0][:, -1])

    def no_grad():
        with torch.no_grad():
            fwd()

    def both():
        for p in params:
            p.grad = None
        (fwd() * d_out).sum().backward()

    return {"forward": no_grad, "forward + backward": both}


def kernel_cases(B: int, L: int) -> dict:
    g = torch.Generator(device=DEV).manual_seed(0)
    proj = torch.randn(B, L, 4 * H, device=DEV, generator=g)
    w_hh = torch.randn(4 * H, H, device=DEV, generator=g) / H ** 0.5
    d_h = torch.randn(B, L, H, device=DEV, generator=g)
    fw = ops.lstm_forward(proj, w_hh)
    return {"tsm_lstm_forward": lambda: ops.lstm_forward(proj, w_hh),
            "tsm_lstm_backward": lambda: ops.lstm_backward(d_h, w_hh, fw["gates"], fw["c"])}


def update_cases(B: int, L: int) -> dict:
    from tianshou_marl_amd.algorithm.dqn import DQN, DiscreteQLearningPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data.buffer import VectorReplayBuffer

    class Discrete:
        n = A

    E, S, N = 64, 256, 3
    buf = VectorReplayBuffer(E * S, E, n_agent=N, obs_dim=D, device=DEV, stack_num=L)
    g = torch.Generator(device=DEV).manual_seed(0)
    for t in range(S):
        buf.add_device(torch.randn(E, N, D, device=DEV, generator=g), torch.randint(0, A, (E, N), device=DEV, dtype=torch.int32, generator=g),
                       torch.randn(E, N, device=DEV, generator=g), (torch.rand(E, 1, device=DEV, generator=g) < 0.04).expand(E, N).to(torch.uint8).contiguous(),
                       torch.zeros(E, N, dtype=torch.uint8, device=DEV), torch.randn(E, N, D, device=DEV, generator=g))
    net = Recurrent(layer_num=LAYERS, state_shape=D, action_shape=A, hidden_layer_size=H, device=DEV, seed=0)
    algo = DQN(policy=DiscreteQLearningPolicy(model=net, action_space=Discrete()), optim=AdamOptimizerFactory(lr=1e-4),
               n_step_return_horizon=3, target_update_freq=100)
    algo.is_within_training_step = True
    return {"DQN.update": lambda: algo.update(buf, B, agent=0)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["hip", "torch", "kernels", "update"])
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    cases = {"hip": hip_cases, "torch": torch_cases, "kernels": kernel_cases, "update": update_cases}[args.mode](args.rows, args.steps)
    for name, fn in cases.items():
        ms = timed(fn, args.warmup, args.iters)
        print(f"{args.mode} hidden {H} layers {LAYERS} L {args.steps} B {args.rows}: {name}: {ms:.4f} ms by device events "
              f"({args.iters} calls after {args.warmup})", flush=True)


if __name__ == "__main__":
    main()
