"""GPU tests (`-m gpu`) of the grouped ensemble MLP (csrc/ensemble.hip) against a float64 numpy einsum at the smallest shapes
where its tiling can go wrong: E in {1, 3}; B in {1, 63, 65, 130} (one row, either side of the 64-row tile, three row tiles);
dims [9, 17, 65, 1] (no width a multiple of 4: every load takes the guarded path; 17 crosses the 16-wide k tile, 65 the
64-wide output tile, the output is one column) and [8, 64, 2] (the aligned fast path); n_split in {1, 3}; an odd col0 with
n_col 3 for the input gradient.

Bar: max |hip - ref64| <= 1e-5 max |ref64| (test_gpu_distq.py's `_bar` with e_ref = 0): the products are exact f32 FMAs on
inputs that are f32 values, so the distance is accumulation rounding, some 1e-7 relative at these k.  The float64 reference is
computed once per (dims, E, B) and shared."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

from redq_restatement import ens_forward, ens_layers  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops

DIMS = {"ragged": [9, 17, 65, 1], "aligned": [8, 64, 2]}
COL0, N_COL = 5, 3


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, torch.float32)


def _n(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(kind: str, E: int, B: int) -> dict:
    """Inputs (f32 values) and the float64 forward, parameter gradient and input gradient of sum(out * d_out), from the first
    seed that keeps every ReLU pre-activation 2e-6 away from its kink, where an f32 rounding could flip the mask."""
    dims = DIMS[kind]
    P = sum(E * (dims[i] * dims[i + 1] + dims[i + 1]) for i in range(len(dims) - 1))
    for seed in range(20):
        rs = np.random.RandomState(100000 * seed + 1000 * E + B + len(dims))
        flat = (rs.standard_normal(P) * 0.4).astype(np.float32)
        x = rs.standard_normal((B, dims[0])).astype(np.float32)
        d_out = rs.standard_normal((E, B, dims[-1])).astype(np.float32)
        acts = ens_forward(flat, dims, E, x)
        layers = ens_layers(flat.astype(np.float64), dims, E)
        ins = [np.broadcast_to(x.astype(np.float64), (E, B, dims[0]))] + acts[:-1]
        if all(np.abs(np.einsum("ebk,ekm->ebm", ins[l], layers[l][0]) + layers[l][1]).min() > 2e-6 for l in range(len(dims) - 2)):
            break
    else:
        raise AssertionError("no seed keeps the pre-activations off the kink")
    grad, dz = [], d_out.astype(np.float64)
    for l in range(len(dims) - 2, -1, -1):
        grad = [np.einsum("ebk,ebm->ekm", ins[l], dz).reshape(-1), dz.sum(1).reshape(-1)] + grad
        dz = np.einsum("ebm,ekm->ebk", dz, layers[l][0])
        if l > 0:
            dz = dz * (acts[l - 1] > 0)
    return dict(dims=dims, flat=flat, x=x, d_out=d_out, out=acts[-1], grad=np.concatenate(grad), dx=dz.sum(0)[:, COL0:COL0 + N_COL])


def run(kind, E, B, n_split, flat=None):
    r = reference(kind, E, B)
    desc = ops.mlp_desc(r["dims"], "relu")
    params = _d(r["flat"] if flat is None else flat)
    out, acts = ops.ens_mlp_forward(desc, E, params, _d(r["x"]))
    slabs = torch.full((n_split, params.numel()), float("nan"), device=DEV)   # every entry of every slab must be written
    ops.ens_mlp_backward(desc, E, params, _d(r["x"]), acts, _d(r["d_out"]), n_split, slabs=slabs)
    dx = ops.ens_mlp_input_grad(desc, E, params, _d(r["x"]), acts, _d(r["d_out"]), COL0, N_COL)
    return out, slabs, dx


@pytest.mark.parametrize("kind", ["ragged", "aligned"])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_forward_slabs_and_input_gradient_match_the_float64_einsum(kind, E, B):
    r = reference(kind, E, B)
    for n_split in (1, 3):
        out, slabs, dx = run(kind, E, B, n_split)
        tag = f"{kind} E={E} B={B} n_split={n_split}"
        assert tuple(out.shape) == (E, B, r["dims"][-1]) and tuple(dx.shape) == (B, N_COL)
        _bar(f"forward {tag}", _n(out), r["out"], 0.0)
        _bar(f"slabs summed {tag}", _n(slabs).sum(0), r["grad"], 0.0)
        _bar(f"input gradient {tag}", _n(dx), r["dx"], 0.0)
        again = run(kind, E, B, n_split)   # two runs give the same bits
        for a, b in zip((out, slabs, dx), again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), tag


@pytest.mark.parametrize("kind", ["ragged", "aligned"])
def test_perturbing_one_member_moves_that_member_alone(kind):
    E, B, n_split, e = 3, 65, 3, 1
    r = reference(kind, E, B)
    dims = r["dims"]
    flat2 = r["flat"].copy()
    mine = np.zeros(flat2.size, bool)   # member e's entries of the flat vector
    o = 0
    for i in range(len(dims) - 1):
        k, m = dims[i], dims[i + 1]
        mine[o + e * k * m:o + (e + 1) * k * m] = True
        o += E * k * m
        mine[o + e * m:o + (e + 1) * m] = True
        o += E * m
    flat2[mine] *= 1.25
    (out, slabs, dx), (out2, slabs2, dx2) = run(kind, E, B, n_split), run(kind, E, B, n_split, flat=flat2)
    others = [i for i in range(E) if i != e]
    assert torch.equal(out[others].view(torch.int32), out2[others].view(torch.int32)) and not torch.equal(out[e], out2[e])
    keep = torch.as_tensor(~mine, device=DEV)
    assert torch.equal(slabs[:, keep].view(torch.int32), slabs2[:, keep].view(torch.int32))
    assert not torch.equal(slabs[:, ~keep], slabs2[:, ~keep]) and not torch.equal(dx, dx2)


def test_unaligned_pointers_take_the_guarded_path_with_the_same_bits():
    """The aligned net read through views that start one float into their allocations: no alignment is asked of the caller, and
    the guarded loads feed the same FMAs in the same order."""
    E, B = 3, 65
    r = reference("aligned", E, B)
    desc = ops.mlp_desc(r["dims"], "relu")
    off = lambda a: torch.cat([torch.zeros(1, device=DEV), _d(a).reshape(-1)])[1:].view(a.shape)  # noqa: E731
    out0, acts0 = ops.ens_mlp_forward(desc, E, _d(r["flat"]), _d(r["x"]))
    params, x = off(r["flat"]), off(r["x"])
    assert params.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 4
    out1, acts1 = ops.ens_mlp_forward(desc, E, params, x, acts=torch.empty(acts0.numel() + 1, device=DEV)[1:])
    assert torch.equal(out0.view(torch.int32), out1.view(torch.int32))
    s0 = ops.ens_mlp_backward(desc, E, _d(r["flat"]), _d(r["x"]), acts0, _d(r["d_out"]), 1)
    s1 = ops.ens_mlp_backward(desc, E, params, x, acts1, off(r["d_out"]), 1)
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32))


def test_bounds_are_refused_before_any_launch():
    desc = ops.mlp_desc([9, 17, 1], "relu")
    x, one = torch.zeros(4, 9, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(ValueError, match=r"ensemble size 65 outside \[1, 64\]"):
        _abi.call("tsm_ens_mlp_forward", desc, 65, one.data_ptr(), x.data_ptr(), 4, one.data_ptr(), None)
    with pytest.raises(ValueError, match="null pointer"):   # a mismatched pointer set
        _abi.call("tsm_ens_mlp_backward", desc, 3, one.data_ptr(), x.data_ptr(), 4, one.data_ptr(), None, one.data_ptr(), 1,
                  one.data_ptr(), 0, None)
    with pytest.raises(ValueError, match="d_acts workspace required"):
        _abi.call("tsm_ens_mlp_input_grad", desc, 3, one.data_ptr(), x.data_ptr(), 4, one.data_ptr(), one.data_ptr(), None, 0, 3,
                  one.data_ptr(), 3, None)
    with pytest.raises(ValueError, match="params must hold"):
        ops.ens_mlp_forward(desc, 3, one, x)
    torch.cuda.synchronize()
