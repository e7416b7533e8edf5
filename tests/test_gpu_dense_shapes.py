"""GPU tests (`-m gpu`) of the dense MLP engine (csrc/dense.hip: gemm_kernel behind tsm_mlp_forward, tsm_mlp_backward and
tsm_mlp_input_grad) against the float64 restatement of tests/dense_restatement.py, at the cases of tests/dense_cases.py: the
smallest shapes that reach each branch of the kernel -- guarded and unconditional loads, alone and mixed in one k loop; the
virtual ones column at, before and behind a tile edge; empty and ragged k ranges of slabs and wave groups; both sides of the
1024-workgroup rule; act = none; eight layers; a unit that is dead on every row; input-gradient windows of every alignment, with a
pitch wider than the window; slabs inside a joint vector; pointers one float off 16-byte alignment.

Bar: max |hip - ref64| <= 1e-5 max |ref64| (test_gpu_distq.py's `_bar` with e_ref = 0), applied per BLOCK: each layer's
activation, each dW_l, each db_l, each slab's own blocks, the input gradient.  A whole flat vector is never judged together, so a
small layer cannot hide under a large one's scale.  The products are exact f32 FMAs on inputs that are f32 values, so the
distance is accumulation rounding (and tanhf's few ulp).  The row ranges of the slabs come from dense_cases, not from the
kernel.  The float64 references are computed once per (dims, act, B) and shared.

Measured on an MI355X (worst ratio to the bar over all cases): activations 0.039 (mixed_k), slabs summed 0.064 (deep), per slab
0.064 (deep), input gradient 0.044 (rule_*), windows 0.018; the 99 tests of the file take 1.6 s."""
import contextlib
import ctypes as C
import functools
import io
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import dense_cases as dc  # noqa: E402
from dense_restatement import block_slices, layers, param_count  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops

CASE_IDS = [c["id"] for c in dc.CASES]
NAN = float("nan")


def _d(x):
    return torch.as_tensor(np.array(x, np.float32)).to(DEV)   # a copy: the cases' inputs are read-only


def _off(a):
    """The same values starting one float into their allocation: what a slice of a joint parameter vector looks like."""
    a = np.asarray(a)
    t = torch.cat([torch.zeros(1, device=DEV), _d(a).reshape(-1)])[1:].view(a.shape)
    assert t.data_ptr() % 16 == 4
    return t


def _n(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a: dict, b: dict, tag):
    for k in ("out", "acts", "slabs", "dx"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), (tag, k)


def _bars(name, pairs):
    """`_bar` (e_ref = 0) on every (got, ref64) pair; prints one PARITY line, the worst ratio."""
    worst, quiet = 0.0, io.StringIO()
    with contextlib.redirect_stdout(quiet):
        for got, ref in pairs:
            worst = max(worst, _bar(name, got, ref, 0.0))
    print(f"PARITY {name}: worst of {len(pairs)}: max |hip - ref64| / (1e-5 max |ref64|) = {worst:.3g}")
    return worst


def _layer_acts(acts, dims, B):
    out, o = [], 0
    for w in dims[1:]:
        out.append(acts[o:o + B * w].view(B, w))
        o += B * w
    assert o == acts.numel()
    return out


def run(c, flat=None, shift=False, n_split=None) -> dict:
    """Forward, slabs and whole input gradient of a case through ops; every output buffer starts as NaN."""
    r, dims, B = dc.inputs(c), c["dims"], c["B"]
    n_split = c["n_split"] if n_split is None else n_split
    put = _off if shift else _d
    desc = ops.mlp_desc(dims, c["act"])
    params, x, d_out = put(r["flat"] if flat is None else flat), put(r["x"]), put(r["d_out"])
    n_act = B * sum(dims[1:])
    assert _abi.call("tsm_mlp_act_elems", C.byref(desc), B) == n_act and ops.mlp_param_count(desc) == param_count(dims)
    acts = torch.full((n_act + 1,), NAN, device=DEV)[1:] if shift else torch.full((n_act,), NAN, device=DEV)
    assert not shift or acts.data_ptr() % 16 == 4
    out, acts = ops.mlp_forward(desc, params, x, acts=acts)
    slabs = torch.full((n_split, params.numel()), NAN, device=DEV)
    got = ops.mlp_backward(desc, params, x, acts, d_out, n_split, slabs=slabs)
    assert got is slabs
    dx = ops.mlp_input_grad(desc, params, x, acts, d_out, 0, dims[0], out=torch.full((B, dims[0]), NAN, device=DEV))
    return dict(desc=desc, params=params, x=x, d_out=d_out, out=out, acts=acts, slabs=slabs, dx=dx)


@functools.lru_cache(maxsize=None)
def _first(case_id: str) -> dict:
    return run(dc.BY_ID[case_id])


def first(c) -> dict:
    """The first run of a case, shared by the tests that only read it."""
    return _first(c["id"])


@pytest.mark.parametrize("c", dc.CASES, ids=CASE_IDS)
def test_forward_slabs_and_input_gradient_meet_float64_block_by_block(c):
    ref, g, dims, B = dc.reference(c), first(c), c["dims"], c["B"]
    assert tuple(g["out"].shape) == (B, dims[-1]) and tuple(g["dx"].shape) == (B, dims[0])
    _bars(f"activations {c['id']}", [(_n(a), ref["acts"][l]) for l, a in enumerate(_layer_acts(g["acts"], dims, B))])
    assert torch.equal(_bits(g["out"]), _bits(_layer_acts(g["acts"], dims, B)[-1]))
    slabs = g["slabs"]
    assert bool(torch.isfinite(slabs).all()), "an entry of a slab was not written"
    for s, (r0, r1) in enumerate(dc.slab_rows(B, c["n_split"])):
        if r0 == r1:   # a slab without rows is written all the same, as +0.0
            assert not bool(_bits(slabs[s]).any()), (c["id"], s)
    total = _n(slabs).sum(0)
    _bars(f"slabs summed {c['id']}", [(total[s], ref["grad"][s]) for _, s in dc.blocks(dims)])
    _bar(f"input gradient {c['id']}", _n(g["dx"]), ref["dx"], 0.0)


@pytest.mark.parametrize("c", dc.CASES, ids=CASE_IDS)
def test_every_slab_holds_the_gradient_of_its_own_rows(c):
    """The rows of slab s are dense_cases.slab_rows' -- no 16-row tile straddles two slabs, no row is counted twice."""
    want, got = dc.slab_reference(c), _n(first(c)["slabs"])
    assert got.shape == want.shape
    _bars(f"per slab {c['id']}", [(got[s][b], want[s][b]) for s in range(c["n_split"]) for _, b in dc.blocks(c["dims"])])


@pytest.mark.parametrize("c", dc.CASES, ids=CASE_IDS)
def test_two_runs_give_the_same_bits(c):
    _same_bits(first(c), run(c), c["id"])


@pytest.mark.parametrize("cid", ["ragged-B130-s1", "aligned-B130-s1", "mixed_k-B65-s2"])
def test_adding_rows_leaves_the_earlier_rows_forward_bits_unchanged(cid):
    c = dc.BY_ID[cid]
    g, dims = first(c), c["dims"]
    full = _layer_acts(g["acts"], dims, c["B"])
    for n in (1, 63, 64, c["B"] - 1):
        _, acts = ops.mlp_forward(g["desc"], g["params"], g["x"][:n].contiguous())
        for l, a in enumerate(_layer_acts(acts, dims, n)):
            assert torch.equal(_bits(a), _bits(full[l][:n])), (cid, n, l)


def test_a_dead_unit_gets_exactly_zero_gradient_and_passes_none_on():
    c = dc.BY_ID["dead_unit-B40-s2"]
    (layer, unit, _), dims = c["dead"], c["dims"]
    g, ref = first(c), dc.reference(c)
    assert not bool(_layer_acts(g["acts"], dims, c["B"])[layer][:, unit].any())
    w, b = block_slices(dims)[layer]
    K = dims[layer]
    row = g["slabs"][:, w.start + unit * K:w.start + (unit + 1) * K]
    assert row.shape == (c["n_split"], K) and not bool(_bits(row).any())            # +0.0, not -0.0, in every slab
    assert not bool(_bits(g["slabs"][:, b.start + unit]).any())
    assert bool((g["slabs"][:, w] != 0).any(0).view(dims[layer + 1], K).any(1).sum() == dims[layer + 1] - 1)   # and only that unit
    _bar("input gradient dead_unit", _n(g["dx"]), ref["dx"], 0.0)
    # the unit's outgoing weights carry nothing back: twice as large, the input gradient keeps its bits
    flat2 = dc.inputs(c)["flat"].copy()
    layers(flat2, dims)[layer + 1][0][:, unit] *= 2.0
    assert not np.array_equal(flat2, dc.inputs(c)["flat"])
    g2 = run(c, flat=flat2)
    assert torch.equal(_bits(g["dx"]), _bits(g2["dx"])) and torch.equal(_bits(g["out"]), _bits(g2["out"]))


@functools.lru_cache(maxsize=None)
def _window_net(dims: tuple) -> dict:
    return run(next(w for w in dc.ALL_WINDOWS if tuple(w["dims"]) == dims))


@pytest.mark.parametrize("w", dc.ALL_WINDOWS, ids=[w["id"] for w in dc.ALL_WINDOWS])
def test_input_gradient_windows_meet_float64_and_the_whole_width_bit_for_bit(w):
    g, ref, col0, n_col, B = _window_net(tuple(w["dims"])), dc.reference(w), w["col0"], w["n_col"], w["B"]
    dx = ops.mlp_input_grad(g["desc"], g["params"], g["x"], g["acts"], g["d_out"], col0, n_col,
                            out=torch.full((B, n_col), NAN, device=DEV))
    assert tuple(dx.shape) == (B, n_col)
    _bar(f"input gradient {w['id']}", _n(dx), ref["dx"][:, col0:col0 + n_col], 0.0)
    # an element's products and their order do not depend on where its column sits in a tile or how its tile was loaded
    assert torch.equal(_bits(dx), _bits(g["dx"][:, col0:col0 + n_col]))
    # a pitch wider than the window (allowed by the ABI): the window is the same, the pad columns are left alone
    wide = torch.full((B, n_col + 3), NAN, device=DEV)
    d_acts = torch.empty_like(g["acts"])
    _abi.call("tsm_mlp_input_grad", C.byref(g["desc"]), _abi.ptr(g["params"]), _abi.ptr(g["x"]), B, _abi.ptr(g["acts"]),
              _abi.ptr(g["d_out"]), _abi.ptr(d_acts), col0, n_col, _abi.ptr(wide), n_col + 3, _abi.stream_ptr())
    assert torch.equal(_bits(wide[:, :n_col]), _bits(dx)) and bool(torch.isnan(wide[:, n_col:]).all())


@pytest.mark.parametrize("cid", ["aligned-B65-s3", "ragged-B65-s3"])
def test_slabs_inside_a_joint_vector_are_written_and_nothing_around_them(cid):
    c = dc.BY_ID[cid]
    g, P, n_split, lead = first(c), param_count(c["dims"]), c["n_split"], 11
    stride = P + lead
    joint = torch.full((n_split * stride,), NAN, device=DEV)
    ops.mlp_backward(g["desc"], g["params"], g["x"], g["acts"], g["d_out"], n_split, slabs=joint[lead:], slab_stride=stride)
    rows = joint.view(n_split, stride)
    assert torch.equal(_bits(rows[:, lead:]), _bits(g["slabs"]))
    assert bool(torch.isnan(rows[:, :lead]).all())


@pytest.mark.parametrize("cid", ["aligned-B65-s1", "aligned-B65-s3", "mixed_k-B65-s2"])
def test_unaligned_pointers_take_the_guarded_path_with_the_same_bits(cid):
    """Params as joint[1:] of a vector one float longer -- what FlatMLP(storage=slice) produces at an odd offset --, and x, acts
    and d_out one float into their allocations too: no alignment is asked of the caller, and the guarded loads feed the same
    FMAs in the same order as the 16-byte loads of the aligned run."""
    c = dc.BY_ID[cid]
    g, s = first(c), run(c, shift=True)
    for k in ("params", "x", "d_out", "acts"):
        assert g[k].data_ptr() % 16 == 0 and s[k].data_ptr() % 16 == 4, k
    _same_bits(g, s, cid)


def test_mis_sized_arguments_are_refused_before_any_launch():
    c = dc.BY_ID["ragged-B65-s3"]
    g, dims, B = first(c), c["dims"], c["B"]
    desc, params, x, acts, d_out, P = g["desc"], g["params"], g["x"], g["acts"], g["d_out"], param_count(c["dims"])
    slabs = torch.full((3, P), NAN, device=DEV)
    out = torch.full((B, 3), NAN, device=DEV)

    def refused(match, f, *a, **k):
        with pytest.raises(ValueError, match=match):
            f(*a, **k)

    more = torch.zeros(acts.numel() + 1, device=DEV)
    for bad_acts in (acts[:-1], more, acts.double()):
        refused("acts must be", ops.mlp_backward, desc, params, x, bad_acts, d_out, 3, slabs=slabs)
        refused("acts must be", ops.mlp_input_grad, desc, params, x, bad_acts, d_out, 0, 3, out=out)
        refused("acts must be", ops.mlp_forward, desc, params, x, acts=bad_acts)
        refused("acts must be", ops.mlp_forward_cond, desc, params, x, torch.ones(1, dtype=torch.int32, device=DEV), acts=bad_acts)
    for bad_d in (d_out[:-1], torch.zeros(B, dims[-1] + 1, device=DEV)):
        refused("d_out must be", ops.mlp_backward, desc, params, x, acts, bad_d, 3, slabs=slabs)
        refused("d_out must be", ops.mlp_input_grad, desc, params, x, acts, bad_d, 0, 3, out=out)
    refused("params: expected dtype", ops.mlp_forward, desc, params.double(), x)
    for bad_p in (params[:-1], params[:1]):
        refused("params must hold", ops.mlp_forward, desc, bad_p, x)
        refused("params must hold", ops.mlp_backward, desc, bad_p, x, acts, d_out, 3, slabs=slabs)
        refused("params must hold", ops.mlp_input_grad, desc, bad_p, x, acts, d_out, 0, 3, out=out)
    refused("x must be", ops.mlp_backward, desc, params, x[:, :-1], acts, d_out, 3, slabs=slabs)
    refused("slabs reach", ops.mlp_backward, desc, params, x, acts, d_out, 3, slabs=slabs[:, :-1])
    refused("slabs reach", ops.mlp_backward, desc, params, x, acts, d_out, 3, slabs=slabs.view(-1)[1:])
    refused("slabs reach", ops.mlp_backward, desc, params, x, acts, d_out, 3, slabs=slabs, slab_stride=P + 1)
    refused("slabs must be", ops.mlp_backward, desc, params, x, acts, d_out, 3, slabs=slabs.double())
    refused("n_split 4 exceeds the 3 rows of slabs", ops.mlp_backward, desc, params, x, acts, d_out, 4, slabs=slabs)
    refused("n_split 65536", ops.mlp_backward, desc, params, x, acts, d_out, 65536)
    refused(f"slab_stride {P - 1} smaller than the parameter count", ops.mlp_backward, desc, params, x, acts, d_out, 3,
            slabs=slabs, slab_stride=P - 1)
    refused("out must be", ops.mlp_input_grad, desc, params, x, acts, d_out, 0, 3, out=torch.zeros(B, 4, device=DEV))
    refused("out must be", ops.mlp_input_grad, desc, params, x, acts, d_out, 0, 3, out=torch.zeros(B - 1, 3, device=DEV))
    refused("d_acts must be", ops.mlp_input_grad, desc, params, x, acts, d_out, 0, 3, out=out, d_acts=acts[:-1])
    refused("leave the input width", ops.mlp_input_grad, desc, params, x, acts, d_out, dims[0] - 1, 2, out=out)
    # host tensors
    for f in (lambda: ops.mlp_forward(desc, params.cpu(), x), lambda: ops.mlp_forward(desc, params, x, acts=acts.cpu()),
              lambda: ops.mlp_forward_cond(desc, params, x, torch.ones(1, dtype=torch.int32)),
              lambda: ops.mlp_backward(desc, params, x.cpu(), acts, d_out, 3, slabs=slabs),
              lambda: ops.mlp_backward(desc, params, x, acts, d_out.cpu(), 3, slabs=slabs),
              lambda: ops.mlp_backward(desc, params, x, acts, d_out, 3, slabs=slabs.cpu()),
              lambda: ops.mlp_input_grad(desc, params, x, acts, d_out, 0, 3, out=out.cpu()),
              lambda: ops.mlp_input_grad(desc, params, x, acts, d_out, 0, 3, out=out, d_acts=acts.cpu())):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()
    # the descriptor: 9 layers, a width of 0
    refused("between 1 and 8 layers", ops.mlp_desc, [4] * 10)
    refused(r"dims\[1\] = 0 out of range", ops.mlp_forward, ops.mlp_desc([4, 0, 2]), torch.zeros(2, device=DEV),
            torch.zeros(3, 4, device=DEV))
    nine = ops.mlp_desc([4, 2])
    nine.n_layers = 9
    refused(r"n_layers must be in \[1, 8\]", ops.mlp_forward, nine, torch.zeros(10, device=DEV), torch.zeros(3, 4, device=DEV))
    torch.cuda.synchronize()
    # nothing was launched: the outputs offered above still hold what they held
    assert bool(torch.isnan(slabs).all()) and bool(torch.isnan(out).all())
    # and the same arguments, sized right, go through
    ops.mlp_backward(desc, params, x, acts, d_out, 3, slabs=slabs)
    ops.mlp_input_grad(desc, params, x, acts, d_out, 0, 3, out=out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(slabs), _bits(g["slabs"])) and torch.equal(_bits(out), _bits(g["dx"][:, :3]))
    # a vector that holds more than the net (an actor's sigma_param behind its layers) is read at its head; fresh slabs are as
    # wide as the vector, or as the pitch asked for
    longer = torch.cat([params, torch.ones(5, device=DEV)])
    assert torch.equal(_bits(ops.mlp_forward(desc, longer, x)[0]), _bits(g["out"]))
    fresh = ops.mlp_backward(desc, longer, x, acts, d_out, 3)
    assert tuple(fresh.shape) == (3, P + 5) and torch.equal(_bits(fresh[:, :P]), _bits(g["slabs"]))
    fresh = ops.mlp_backward(desc, params, x, acts, d_out, 3, slab_stride=P + 2)
    assert tuple(fresh.shape) == (3, P + 2) and torch.equal(_bits(fresh[:, :P]), _bits(g["slabs"]))
