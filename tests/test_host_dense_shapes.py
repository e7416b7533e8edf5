"""CPU checks of what tests/test_gpu_dense_shapes.py stands on: the float64 restatement of the dense MLP engine equals torch
float64 autograd on every case, the per-row-range gradients add up, every relu case finds its kink-free seed inside the search
limit, and every claim of the case table (tests/dense_cases.py) holds in arithmetic.  No GPU, no library.

The bar against autograd is max |restatement - autograd| <= 1e-12 max |autograd| per block (each layer's activation, each
dW_l, each db_l, the input gradient): both sides are float64 sums of the same products in different orders, 2736 terms at the
most, so they differ by some 1e-14 of the block's scale; an entry that cancels to near zero is held to its block's scale like
every other."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_cases as dc  # noqa: E402
from dense_restatement import (KINK_MARGIN, SEED_LIMIT, block_slices, dense_reference, first_kink_free, kink_distance,  # noqa: E402
                               param_count, param_grad_rows)

RTOL = 1e-12
EVERY = dc.CASES + dc.ALL_WINDOWS
IDS = [c["id"] for c in EVERY]


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= RTOL * scale, (name, err, scale)


def _autograd(c):
    """torch float64 autograd of sum(out * d_out) over the flat layout (W [out, in] then b, per layer)."""
    r, dims = dc.inputs(c), c["dims"]
    p = torch.tensor(r["flat"].astype(np.float64), requires_grad=True)
    x = torch.tensor(r["x"].astype(np.float64), requires_grad=True)
    h, acts = x, []
    for i, (w, b) in enumerate(block_slices(dims)):
        h = h @ p[w].view(dims[i + 1], dims[i]).T + p[b]
        if i + 2 < len(dims):
            h = {"relu": torch.relu, "tanh": torch.tanh, "none": lambda t: t}[c["act"]](h)
        acts.append(h)
    (h * torch.tensor(r["d_out"].astype(np.float64))).sum().backward()
    return [a.detach().numpy() for a in acts], p.grad.numpy(), x.grad.numpy()


@pytest.mark.parametrize("c", EVERY, ids=IDS)
def test_the_restatement_equals_float64_autograd(c):
    ref, (acts, grad, dx) = dc.reference(c), _autograd(c)
    assert len(ref["acts"]) == len(c["dims"]) - 1 and ref["out"] is ref["acts"][-1]
    for l, a in enumerate(acts):
        _same(f"activation {l}", ref["acts"][l], a)
    for l, (w, b) in enumerate(block_slices(c["dims"])):
        _same(f"dW_{l}", ref["dW"][l].reshape(-1), grad[w])
        _same(f"db_{l}", ref["db"][l], grad[b])
        assert np.array_equal(ref["grad"][w], ref["dW"][l].reshape(-1)) and np.array_equal(ref["grad"][b], ref["db"][l])
    _same("input gradient", ref["dx"], dx)
    assert ref["dx"].shape == (c["B"], c["dims"][0])


@pytest.mark.parametrize("c", dc.CASES, ids=[c["id"] for c in dc.CASES])
def test_row_range_gradients_of_a_partition_sum_to_the_whole(c):
    ref, slabs = dc.reference(c), dc.slab_reference(c)
    assert slabs.shape == (c["n_split"], param_count(c["dims"]))
    for name, s in dc.blocks(c["dims"]):
        _same(name, slabs[:, s].sum(0), ref["grad"][s])
    r, B = dc.inputs(c), c["B"]
    cuts = sorted({0, B // 3, B // 2, B})   # a partition that is not the slabs'
    parts = [param_grad_rows(c["dims"], c["act"], r["flat"], r["x"], r["d_out"], a, b) for a, b in zip(cuts, cuts[1:])]
    for name, s in dc.blocks(c["dims"]):
        _same(name, np.sum(parts, axis=0)[s], ref["grad"][s])
    assert not param_grad_rows(c["dims"], c["act"], r["flat"], r["x"], r["d_out"], B, B).any()


@pytest.mark.parametrize("c", [c for c in EVERY if c["act"] == "relu"], ids=[c["id"] for c in EVERY if c["act"] == "relu"])
def test_every_relu_case_finds_a_kink_free_seed_within_the_limit(c):
    r = dc.inputs(c)   # raises past SEED_LIMIT
    assert 0 <= r["seed"] < SEED_LIMIT
    assert kink_distance(c["dims"], c["act"], r["flat"], r["x"]) >= KINK_MARGIN
    k, _ = first_kink_free(c["dims"], c["act"], lambda k: dc.make_inputs(c, k))
    assert k == r["seed"]
    # every earlier seed was refused for the kink and nothing else
    assert all(kink_distance(c["dims"], "relu", *dc.make_inputs(c, j)[:2]) < KINK_MARGIN for j in range(k))


def test_the_seed_search_gives_up_at_its_limit():
    c = dc.BY_ID["linear-B17-s1"]
    zero = lambda k: tuple(np.zeros_like(a) for a in dc.make_inputs(c, k))  # noqa: E731  every pre-activation on the kink
    with pytest.raises(AssertionError, match="off the kink"):
        first_kink_free(c["dims"], "relu", zero)
    assert first_kink_free(c["dims"], "none", zero)[0] == 0   # no kink to meet


@pytest.mark.parametrize("c", EVERY, ids=IDS)
def test_the_slab_rule_in_plain_python(c):
    B, n = c["B"], c["n_split"]
    kp = dc.k_per(B, n)
    assert kp % 16 == 0 and kp * n >= B and kp - 16 < -(-B // n) <= kp
    rows = dc.slab_rows(B, n)
    assert len(rows) == n and rows[0][0] == 0 and max(r1 for _, r1 in rows) == B
    covered = np.zeros(B, int)
    for s, (r0, r1) in enumerate(rows):
        assert (r0, r1) == (min(s * kp, B), min((s + 1) * kp, B)) and r0 <= r1
        assert r0 % 16 == 0 or r0 == B   # a 16-row tile never straddles two slabs
        covered[r0:r1] += 1
        groups = dc.group_rows(r0, r1)
        assert len(groups) == 4 and groups[0][0] == r0 and max(g1 for _, g1 in groups) == r1
        assert all((g0 - r0) % 16 == 0 or g0 == r1 for g0, _ in groups)
        assert sum(g1 - g0 for g0, g1 in groups) == r1 - r0
    assert (covered == 1).all()   # every row in exactly one slab


def test_the_claims_of_the_table():
    by = dc.BY_ID
    assert len(dc.CASES) == 27 and all(c["reason"] for c in dc.CASES + dc.ALL_WINDOWS)
    # ragged: no width is a multiple of 4; aligned: every one is
    assert all(d % 4 for d in by["ragged-B1-s1"]["dims"]) and not any(d % 4 for d in by["aligned-B64-s1"]["dims"])
    # mixed_k: one whole 16-wide sub-tile, then a ragged one
    assert by["mixed_k-B65-s2"]["dims"][0] // 16 == 1 and by["mixed_k-B65-s2"]["dims"][0] % 16 == 4
    # the bias column K against the 64-wide tile of the K + 1 wide output
    assert [(K % 64, -(-(K + 1) // 64)) for K in (63, 64, 65)] == [(63, 1), (0, 2), (1, 2)]
    # deep reaches the layer limit
    assert len(by["deep-B5-s1"]["dims"]) - 1 == dc.MAX_LAYERS and 1 in by["deep-B5-s1"]["dims"]
    # empty_slabs: k_per = 16, slabs 2..4 cover no rows
    assert dc.k_per(17, 5) == 16 and dc.slab_rows(17, 5) == [(0, 16), (16, 17), (17, 17), (17, 17), (17, 17)]
    # groups (and aligned at B = 130, n_split = 1): 48 / 48 / 34 / 0
    assert [g1 - g0 for g0, g1 in dc.group_rows(*dc.slab_rows(130, 1)[0])] == [48, 48, 34, 0]
    assert dc.wgrad_groups(by["groups-B130-s1"]["dims"], 1) == [4, 4]
    # a LAST group that holds rows (what a fold that stops early would lose): B = 63 and 64 at n_split = 1
    assert [g1 - g0 for g0, g1 in dc.group_rows(0, 63)] == [16, 16, 16, 15]
    assert [g1 - g0 for g0, g1 in dc.group_rows(0, 64)] == [16, 16, 16, 16]
    assert [g1 - g0 for g0, g1 in dc.group_rows(0, 65)] == [32, 32, 1, 0]
    # either side of the 1024-workgroup rule
    lo, hi = by["rule_below-B2736-s170"], by["rule_above-B2736-s171"]
    assert dc.wgrad_tiles(lo["dims"]) == [6]
    assert 6 * 170 == 1020 < dc.MIN_WORKGROUPS <= 6 * 171 == 1026
    assert dc.wgrad_groups(lo["dims"], 170) == [4] and dc.wgrad_groups(hi["dims"], 171) == [1]
    assert dc.k_per(2736, 170) == 32 and sum(r1 > r0 for r0, r1 in dc.slab_rows(2736, 170)) == 86   # 84 slabs are empty
    assert dc.k_per(2736, 171) == 16 and all(r1 - r0 == 16 for r0, r1 in dc.slab_rows(2736, 171))
    # every other case stays below the rule, as every net of the older tests does
    assert all(set(dc.wgrad_groups(c["dims"], c["n_split"])) == {4} for c in dc.CASES if c["name"] != "rule_above")
    # the largest slab allocation is about 6 MB
    assert max(c["n_split"] * param_count(c["dims"]) * 4 for c in dc.CASES) == 171 * 8580 * 4 < 6 << 20
    # the dead unit is dead: its pre-activation is negative on every row, in float64
    dead = by["dead_unit-B40-s2"]
    layer, unit, bias = dead["dead"]
    ref = dc.reference(dead)
    assert dc.inputs(dead)["flat"][block_slices(dead["dims"])[layer][1]][unit] == np.float32(bias)
    assert (ref["pre"][layer][:, unit] < -900).all() and not ref["acts"][layer][:, unit].any()
    assert not ref["dW"][layer][unit].any() and ref["db"][layer][unit] == 0
    assert (ref["acts"][layer] > 0).any(0).sum() == dead["dims"][1] - 1   # and it is the only one


def test_the_windows_and_their_load_paths():
    assert [(w["col0"], w["n_col"]) for w in dc.WINDOWS] == [(0, 130), (4, 64), (5, 64), (63, 3), (129, 1)]
    for w in dc.ALL_WINDOWS:
        assert 0 <= w["col0"] and w["n_col"] >= 1 and w["col0"] + w["n_col"] <= w["dims"][0]
        assert w["B"] == 65 and w["act"] == "relu"
    # a pitch of 130 floats is no multiple of 4: none of the issue's windows can take the unconditional load
    assert [dc.window_fast_tiles(w["dims"], w["col0"], w["n_col"]) for w in dc.WINDOWS] == [0] * 5
    assert [dc.window_fast_tiles(w["dims"], w["col0"], w["n_col"]) for w in dc.WINDOWS_FAST] == [1, 1, 0]


def test_the_restatement_on_a_net_small_enough_to_do_by_hand():
    # 1 -> 1 -> 1 relu: out = w1 * relu(w0 x + b0) + b1
    flat = np.array([2.0, -1.0, 3.0, 0.5], np.float32)   # w0 b0 w1 b1
    x, d = np.array([[1.0], [0.25]], np.float32), np.array([[1.0], [10.0]], np.float32)
    r = dense_reference([1, 1, 1], "relu", flat, x, d)
    assert r["out"].reshape(-1).tolist() == [3.5, 0.5]   # row 1: 2 * 0.25 - 1 < 0, the unit is off
    assert r["grad"].tolist() == [3.0, 3.0, 1.0, 11.0] and r["dx"].reshape(-1).tolist() == [6.0, 0.0]
    t = dense_reference([1, 1, 1], "tanh", flat, x, d)
    y = np.tanh(np.array([1.0, -0.5]))
    assert np.allclose(t["dx"].reshape(-1), np.array([1.0, 10.0]) * 3.0 * (1 - y * y) * 2.0, rtol=1e-15)
    n = dense_reference([1, 1, 1], "none", flat, x, d)
    assert n["out"].reshape(-1).tolist() == [3.5, -1.0] and n["dx"].reshape(-1).tolist() == [6.0, 60.0]
