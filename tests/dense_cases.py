"""The case table of the shape sweep over the dense MLP engine (csrc/dense.hip: one templated f32-MFMA GEMM behind
tsm_mlp_forward, tsm_mlp_backward and tsm_mlp_input_grad), one deterministic input builder and the float64 yardsticks.
tests/test_gpu_dense_shapes.py runs the kernels on these inputs; tests/test_host_dense_shapes.py checks on the CPU that every
claim a case makes below holds in arithmetic and that the yardstick (tests/dense_restatement.py) equals torch float64 autograd.
Plain numpy module.

Every size is the smallest that reaches its branch.  The kernel's constants are restated here (BM = BN = 64, BK = 16, four wave
groups, the 1024-workgroup rule) so that the row range of every slab and of every wave group comes from this file and never
from the kernel under test:
  * slab s of n_split covers the rows [s * k_per, min((s + 1) * k_per, B)), k_per = ceil(ceil(B / n_split) / 16) * 16;
  * a weight-gradient launch has ceil((K + 1) / 64) * ceil(O / 64) output tiles (K + 1: the virtual ones column that yields the
    bias gradient); with tiles * n_split < 1024 four wave groups split a slab's rows in whole 16-row tiles and fold through
    LDS in group order, otherwise one group walks them all;
  * a load takes the unconditional 16-byte path when its pointer is 16-byte aligned, its pitch a multiple of 4 floats and its
    64 x 16 piece inside the operand; everything else is guarded element by element.

The relu cases take the first of their seeds that keeps every pre-activation 2e-6 from the kink (dense_restatement.
first_kink_free); the inputs depend on (dims, act, B) alone, so the n_split variants of a case share one reference.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dense_restatement import block_slices, dense_reference, first_kink_free, param_count, param_grad_rows  # noqa: E402

BM = BN = 64
BK = 16
GROUPS = 4
MIN_WORKGROUPS = 1024    # fewer (output tiles x slabs) than this: the four-group kernel
MAX_LAYERS = 8
WEIGHT_SCALE = 0.4


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def _case(name, dims, act, B, n_split, reason, dead=None) -> dict:
    return dict(id=f"{name}-B{B}-s{n_split}", name=name, dims=list(dims), act=act, B=B, n_split=n_split, reason=reason, dead=dead)


CASES = (
    [_case("ragged", [9, 17, 65, 1], "relu", B, s,
           "no width % 4: every load guarded; 17 crosses BK, 65 crosses BN; one output column")
     for B in (1, 63, 64, 65, 130) for s in (1, 3)]
    + [_case("aligned", [16, 64, 64, 4], "relu", B, s, "all-fast interior tiles, edge row tile at 65")
       for B in (64, 65, 130) for s in (1, 3)]
    + [_case("mixed_k", [20, 64, 2], "tanh", 65, 2, "fast then guarded sub-tile within one k loop")]
    + [_case(f"ones_{K}", [K, 64, 1], "relu", 33, 1, why) for K, why in (
        (63, "the bias column is the last column of a data tile"),
        (64, "the bias column is alone in a tile of its own"),
        (65, "the bias column shares a guarded tile with one data column"))]
    + [_case("linear", [7, 5, 3], "none", 17, 1, "act = 0 forward and derivative"),
       _case("deep", [3, 2, 1, 2, 3, 1, 2, 3, 2], "tanh", 5, 1, "8 layers, widths of 1"),
       _case("empty_slabs", [9, 17, 1], "relu", 17, 5, "k_per = 16: slabs 2..4 cover no rows"),
       _case("groups", [9, 17, 1], "relu", 130, 1, "G = 4: groups of 48/48/34/0 rows"),
       _case("rule_below", [65, 130], "none", 2736, 170, "6 tiles: 1020 < 1024 takes G = 4"),
       _case("rule_above", [65, 130], "none", 2736, 171, "6 tiles: 1026 takes G = 1"),
       _case("dead_unit", [8, 16, 4], "relu", 40, 2, "a unit that is 0 on every row", dead=(0, 3, -1e3))]
)
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def _window(dims, col0, n_col, reason) -> dict:
    c = _case("window", dims, "relu", 65, 1, reason)
    c.update(id=f"window-{dims[0]}-c{col0}-n{n_col}", col0=col0, n_col=n_col)
    return c


# Input-gradient windows: dX[:, col0 : col0 + n_col] = dZ_0 . W_0[:, col0 : col0 + n_col], W_0 read at W + col0 with pitch
# dims[0].  On [130, 64, 2] the pitch is no multiple of 4 floats, so every one of these runs guarded, aligned col0 or not.
WINDOWS = [
    _window([130, 64, 2], 0, 130, "whole width: two column tiles and two guarded columns"),
    _window([130, 64, 2], 4, 64, "col0 % 4 = 0, exactly one column tile"),
    _window([130, 64, 2], 5, 64, "unaligned col0, one column tile"),
    _window([130, 64, 2], 63, 3, "straddles the 64-column boundary of W_0"),
    _window([130, 64, 2], 129, 1, "the last column"),
]
# The same on a pitch of 132 floats, where the unconditional load of the window is reachable (n_col >= 64 and col0 % 4 = 0).
WINDOWS_FAST = [
    _window([132, 64, 2], 4, 64, "aligned: exactly one fast column tile"),
    _window([132, 64, 2], 4, 68, "aligned: one fast column tile, then a guarded tile of 4 columns"),
    _window([132, 64, 2], 5, 64, "the same tile from an odd col0: guarded"),
]
ALL_WINDOWS = WINDOWS + WINDOWS_FAST


# ---- the rules, in plain Python ---------------------------------------------------------------------------------------------
def k_per(B: int, n_split: int) -> int:
    return _ceil_div(_ceil_div(B, n_split), BK) * BK


def slab_rows(B: int, n_split: int) -> list:
    """[(r0, r1)] per slab; r0 == r1 for a slab that covers no rows."""
    kp = k_per(B, n_split)
    return [(min(s * kp, B), min((s + 1) * kp, B)) for s in range(n_split)]


def group_rows(r0: int, r1: int) -> list:
    """[(g0, g1)] per wave group of the four-group kernel on a slab's rows [r0, r1): whole 16-row tiles per group."""
    span = max(r1 - r0, 0)
    per = _ceil_div(_ceil_div(span, GROUPS), BK) * BK
    return [(min(r0 + q * per, r1), min(r0 + (q + 1) * per, r1)) for q in range(GROUPS)]


def wgrad_tiles(dims) -> list:
    """Output tiles of each layer's weight-gradient launch."""
    return [_ceil_div(dims[l] + 1, BN) * _ceil_div(dims[l + 1], BM) for l in range(len(dims) - 1)]


def wgrad_groups(dims, n_split: int) -> list:
    """Wave groups of each layer's weight-gradient launch: 4 below the rule, 1 from it on."""
    return [GROUPS if t * n_split < MIN_WORKGROUPS else 1 for t in wgrad_tiles(dims)]


def window_fast_tiles(dims, col0: int, n_col: int) -> int:
    """Column tiles of an input-gradient window that take the unconditional load, for 16-byte aligned parameters."""
    return n_col // BN if dims[0] % 4 == 0 and col0 % 4 == 0 else 0


# ---- inputs and yardsticks --------------------------------------------------------------------------------------------------
def _key(c: dict):
    return (tuple(c["dims"]), c["act"], c["B"], c["dead"])


def make_inputs(c: dict, k: int):
    """(flat, x, d_out) in float32 of the k-th seed of a case."""
    dims, B = c["dims"], c["B"]
    rs = np.random.RandomState(100000 * k + 1000 * len(dims) + 7 * sum(dims) + B)
    flat = (rs.standard_normal(param_count(dims)) * WEIGHT_SCALE).astype(np.float32)
    x = rs.standard_normal((B, dims[0])).astype(np.float32)
    d_out = rs.standard_normal((B, dims[-1])).astype(np.float32)
    if c["dead"] is not None:
        layer, unit, bias = c["dead"]
        flat[block_slices(dims)[layer][1]][unit] = bias
    return flat, x, d_out


@functools.lru_cache(maxsize=None)
def _inputs(key) -> dict:
    c = dict(dims=list(key[0]), act=key[1], B=key[2], dead=key[3])
    k, (flat, x, d_out) = first_kink_free(c["dims"], c["act"], lambda k: make_inputs(c, k))
    for a in (flat, x, d_out):
        a.setflags(write=False)
    return dict(seed=k, flat=flat, x=x, d_out=d_out)


def inputs(c: dict) -> dict:
    return _inputs(_key(c))


@functools.lru_cache(maxsize=None)
def _reference(key) -> dict:
    r = _inputs(key)
    return dense_reference(list(key[0]), key[1], r["flat"], r["x"], r["d_out"])


def reference(c: dict) -> dict:
    """The float64 forward, activations, dW / db / flat gradient and whole input gradient of a case; computed once."""
    return _reference(_key(c))


@functools.lru_cache(maxsize=None)
def _slab_reference(key, n_split: int) -> np.ndarray:
    r = _inputs(key)
    return np.stack([param_grad_rows(list(key[0]), key[1], r["flat"], r["x"], r["d_out"], r0, r1)
                     for r0, r1 in slab_rows(key[2], n_split)])


def slab_reference(c: dict) -> np.ndarray:
    """[n_split, n_param]: the float64 gradient of each slab's own rows."""
    return _slab_reference(_key(c), c["n_split"])


def blocks(dims) -> list:
    """[(name, slice into the flat vector)]: dW_0, db_0, dW_1, ..."""
    return [(f"{n}_{l}", s) for l, ws in enumerate(block_slices(dims)) for n, s in zip(("dW", "db"), ws)]
