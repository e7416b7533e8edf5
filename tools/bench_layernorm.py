#!/usr/bin/env python3
"""Forward + backward of FlatMLP([23, 256, 256, 1], norm="layer") (csrc/layernorm.hip) at B = 256 and 4096 against (a) the
un-normalised FlatMLP of the same dims (csrc/dense.hip: what the norm layers cost) and (b) torch.nn.Sequential(Linear,
LayerNorm, ReLU, ..., Linear) with the same weights and autograd on the same GPU.  Times are device events around ITERS calls,
the three variants alternating inside every repeat; the median over the repeats and the spread (min .. max) are recorded.
Launch counts are torch.profiler's device-kernel events of one forward and one backward, taken in a pass of its own.

    python tools/bench_layernorm.py [out.md]     # default: profiles/layernorm_kernel_stats.md"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tianshou_marl_amd.utils.net import FlatMLP  # noqa: E402

DIMS, ITERS, REPEATS, DEV = [23, 256, 256, 1], 2000, 7, "cuda"


def variants(B):
    """{name: (forward(), backward())} on one set of weights and inputs."""
    ln = FlatMLP(DIMS, "relu", device=DEV, seed=0, norm="layer")
    plain = FlatMLP(DIMS, "relu", device=DEV, seed=0)
    mods = []
    for k, o in zip(DIMS[:-2], DIMS[1:-1]):
        mods += [torch.nn.Linear(k, o), torch.nn.LayerNorm(o), torch.nn.ReLU()]
    seq = torch.nn.Sequential(*mods, torch.nn.Linear(DIMS[-2], DIMS[-1])).to(DEV)
    for p, v in zip(seq.parameters(), ln.mlp_views()):
        p.data.copy_(v)
    x, d = torch.randn(B, DIMS[0], device=DEV), torch.randn(B, 1, device=DEV)
    out = {}

    def torch_fwd():
        out["y"] = seq(x)

    def torch_bwd():
        seq.zero_grad(set_to_none=True)
        out["y"].backward(d)

    err = float((ln(x) - seq(x).detach()).abs().max())
    assert err < 1e-4, err   # the three compute one net
    return {"layernorm.hip": (lambda: ln(x), lambda: ln.backward(d)), "dense.hip, no norm": (lambda: plain(x), lambda: plain.backward(d)),
            "torch eager": (torch_fwd, torch_bwd)}


def event_time(fn):
    """us per call of `fn` over ITERS calls."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / ITERS


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if ev.device_type == DeviceType.CUDA and "memcpy" not in ev.name.lower())


def main():
    assert torch.cuda.is_available(), "bench_layernorm needs a GPU"
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "layernorm_kernel_stats.md")
    lines = ["# LayerNorm MLP: forward and backward against the un-normalised net and torch eager", "",
             f"`tools/bench_layernorm.py` on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}): FlatMLP({DIMS}, relu), us per call by device events "
             f"over {ITERS} calls, median of {REPEATS} repeats (min .. max), variants alternating inside a repeat.  fwd+bwd is a "
             "forward that keeps what the backward needs, then the backward.", "",
             "| B | variant | forward us | fwd+bwd us | launches fwd | launches bwd |", "|---|---|---|---|---|---|"]
    verdict = []
    for B in (256, 4096):
        vs = variants(B)
        for f, b in vs.values():   # warm every shape
            for _ in range(20):
                f()
                b()
        t = {k: ([], []) for k in vs}
        for _ in range(REPEATS):
            for k, (f, b) in vs.items():
                t[k][0].append(event_time(f))
                t[k][1].append(event_time(lambda: (f(), b())))
        med, both = {}, {}
        for k, (f, b) in vs.items():
            f()
            n_f, n_b = launches(f), launches(b)
            med[k], both[k] = statistics.median(t[k][0]), statistics.median(t[k][1])
            cell = [f"{statistics.median(a):.1f} ({min(a):.1f} .. {max(a):.1f})" for a in t[k]]
            lines.append(f"| {B} | {k} | {cell[0]} | {cell[1]} | {n_f} | {n_b} |")
        slower = med["layernorm.hip"] > med["torch eager"]
        verdict.append(f"B = {B}: the one-launch forward is {'SLOWER' if slower else 'faster'} than torch eager's forward "
                       f"({med['layernorm.hip']:.1f} us against {med['torch eager']:.1f} us) and costs "
                       f"{med['layernorm.hip'] - med['dense.hip, no norm']:+.1f} us over the un-normalised forward; forward + backward "
                       f"costs {both['layernorm.hip'] - both['dense.hip, no norm']:+.1f} us over the un-normalised net's (one more "
                       "launch per hidden layer: the row kernel, one workgroup per slab).")
    lines += [""] + verdict
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
