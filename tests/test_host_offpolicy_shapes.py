"""CPU tests of the shape sweeps that tests/test_gpu_offpolicy_shapes.py runs on the device (inputs and yardsticks:
tests/offpolicy_cases.py).  For every case: the preconditions on the reference hold for every row and element (the greedy
choice is clear of 64 float32 ulp, the IQN embedding's ReLU is clear of its kink by 1e-5), the reference's own float32 error
`e_ref` is finite, the float32 restatement alone stays inside the bar the device test applies to the kernel, the scripts and
index draws have the properties the sweep is about, and the C-ABI's argument checks accept every case's sizes (the calls pass
null pointers: they return the size error, if any, before the null-pointer error and before any launch)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import offpolicy_cases as oc  # noqa: E402
from per_restatement import bound_of  # noqa: E402

TINY = float(np.finfo(np.float32).tiny)


def _inside_bar(name, e_ref, ref):
    """test_gpu_distq._bar with the float32 restatement in the kernel's place: e_ref <= 1e-5 max |ref64| + e_ref."""
    assert np.isfinite(e_ref) and e_ref >= 0.0, (name, e_ref)
    scale = max(float(np.abs(np.asarray(ref, np.float64)).max()), TINY)
    assert np.isfinite(scale), name
    tol = 1e-5 * scale + e_ref
    assert e_ref <= tol, (name, e_ref, tol)
    return e_ref / tol


def _inside_rel(name, e_ref, ref):
    """test_gpu_dqn._rel with the float32 restatement in the kernel's place: e_ref <= 1e-5 max |ref64|."""
    scale = max(float(np.abs(np.asarray(ref, np.float64)).max()), TINY)
    assert np.isfinite(e_ref) and e_ref <= 1e-5 * scale, (name, e_ref, scale)
    return e_ref / (1e-5 * scale)


def _variants(name, variants, keys):
    worst = 0.0
    for v, r in variants.items():
        for k in keys:
            worst = max(worst, _inside_bar(f"{name} {v} {k}", r["e_ref"][k], r[k]))
    return worst


# ---- the heads --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.DQN_CASES, ids=oc.case_id)
def test_dqn_case(c):
    ref = oc.dqn_reference(c)
    assert ref["greedy_margin"] > 1.0, ref["greedy_margin"]
    assert set(ref["variants"]) == set(oc.DQN_VARIANTS) and len(oc.DQN_VARIANTS) == 24
    worst = _variants("dqn", ref["variants"], ("returns", "td_error", "dq", "loss"))
    _inside_bar("mean q", ref["mean_q_eref"], [ref["mean_q"]])
    d = oc.dqn_inputs(c)
    assert d["mask"].any(1).all() and d["q"].shape == (c["B"], c["A"])
    print(f"dqn {oc.case_id(c)}: greedy margin {ref['greedy_margin']:.3g} x 64 ulp, worst e_ref / bar {worst:.3g}")


@pytest.mark.parametrize("c", oc.DISTQ_CASES, ids=oc.case_id)
def test_distq_case(c):
    ref = oc.distq_reference(c)
    assert ref["greedy_margin"] > 1.0, ref["greedy_margin"]
    assert len(ref["variants"]) == 16
    worst = _variants("distq", ref["variants"], ("returns", "prio", "d_out", "loss", "mean_q"))
    for kind, v in ref["values"].items():
        _inside_bar(kind + " q", v["e_ref"]["q"], v["q"])
        if kind == "c5":
            _inside_bar("probs", v["e_ref"]["probs"], v["probs"])
    d = oc.distq_inputs(c)
    if c["B"] >= 15:   # C51's clamp is met at each end, QR-DQN's Huber on both sides of its kink
        sup = oc.support_of(oc.V_MIN, oc.V_MAX, c["N"])
        ret = sup[None, :] * d["vmask"][:, None] * d["gpow"][:, None] + d["mc"][:, None]
        assert (ret > oc.V_MAX).any() and (ret < oc.V_MIN).any()
    print(f"distq {oc.case_id(c)}: greedy margin {ref['greedy_margin']:.3g} x 64 ulp, worst e_ref / bar {worst:.3g}")


@pytest.mark.parametrize("c", oc.IQN_CASES, ids=oc.case_id)
def test_iqn_case(c):
    ref = oc.iqn_reference(c)
    assert ref["greedy_margin"] > 1.0, ref["greedy_margin"]
    assert len(ref["variants"]) == 8
    worst = _variants("iqn", ref["variants"], ("returns", "prio", "d_out", "loss", "mean_q"))
    _inside_bar("iqn q", ref["values"]["e_ref"]["q"], ref["values"]["q"])
    for (tgt, _, _), r in ref["variants"].items():
        assert r["returns"].shape == (c["B"], c["Np"] if tgt else c["N"])
    print(f"iqn {oc.case_id(c)}: greedy margin {ref['greedy_margin']:.3g} x 64 ulp, worst e_ref / bar {worst:.3g}")


@pytest.mark.parametrize("c", oc.EMBED_CASES, ids=oc.case_id)
def test_embed_case(c):
    r = oc.embed_reference(c)
    assert r["min_abs_pre"] >= oc.MIN_ABS_PRE, r["min_abs_pre"]
    assert r["same_gate32"]                          # so far from the kink, the float32 restatement opens the same gates
    assert r["pre"].shape == (c["B"] * c["S"], c["H"]) and (r["pre"] > 0).any() and (r["pre"] < 0).any()
    worst = max(_inside_bar(k, r["e_ref"][k], r[k]) for k in ("e", "d_f", "dWe", "dbe"))
    print(f"embed {oc.case_id(c)}: min |pre| {r['min_abs_pre']:.3g}, worst e_ref / bar {worst:.3g}")


def test_embed_cases_cover_the_partial_waves_and_the_limits():
    shapes = set(oc.EMBED_SHAPES)
    assert {s[2] % 16 for s in shapes} >= {4, 0} and {20, 36, 52} <= {s[2] for s in shapes}
    assert {512, 496} <= {s[3] for s in shapes} and max(s[1] for s in shapes) == 64
    assert (3, 5, 64, 512) in shapes and 3 * 5 == 15
    assert len(oc.EMBED_CASES) == 2 * len(oc.EMBED_SHAPES)


@pytest.mark.parametrize("c", oc.DSAC_CASES, ids=oc.case_id)
def test_dsac_case(c):
    ref = oc.dsac_reference(c)
    assert set(ref) == set(oc.DSAC_VARIANTS)
    worst = 0.0
    for v, r in ref.items():
        for k, e in r["e_ref"].items():
            worst = max(worst, _inside_bar(f"dsac {v} {k}", e, r[k]))
        # the alpha step's deficit is far from a cancellation: target entropy 0.3 against a mean entropy of 0 (A = 1) or > 1
        assert abs(oc.DSAC_TARGET_ENTROPY - r["mean_entropy"]) > 0.25
    print(f"dsac {oc.case_id(c)}: worst e_ref / bar {worst:.3g}")


# ---- the n-step walk --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buffer_num,sub_size", oc.NSTEP_BUFFERS)
def test_nstep_scripts_cover_the_cases_asked_for(buffer_num, sub_size):
    rb, script, idx = oc.nstep_restated(buffer_num, sub_size)
    S, total = sub_size, buffer_num * sub_size
    assert len(idx) > 256 and idx.min() < 0 and idx.max() < total and idx.min() >= -total
    assert set(idx % total) == set(rb.sample_indices_all())
    per_env = np.bincount([r[0] for r in script], minlength=buffer_num)
    assert per_env.max() >= 2 * S + 1                                  # a sub-buffer written past its end twice
    assert len(rb.unfinished_index()) >= 1                             # a newest row that ended nothing
    if buffer_num >= 3:
        assert per_env[1] == 0 and rb.size[1] == 0 and (rb.size == S).any()           # an empty one beside full ones
        assert rb.done[S - 1] and 0 < rb.size[buffer_num - 1] < S                     # an end on the last slot; a partly filled one
    if S > 1:
        assert rb.done.any() and rb.term.any()
    assert oc.nstep_horizons(S)[-1] == 40 and S + 3 in oc.nstep_horizons(S)
    worst = 0.0
    for n_step in oc.nstep_horizons(S):
        for gamma in oc.NSTEP_GAMMAS:
            for col in oc.NSTEP_COLS:
                r = oc.nstep_reference(rb, idx, n_step, gamma, col)
                assert r["idx_n"].shape == idx.shape and np.isfinite(r["mc"]).all()
                worst = max(worst, _inside_rel("mc", r["e_ref"]["mc"], r["mc"]), _inside_rel("gpow", r["e_ref"]["gpow"], r["gpow"]))
    print(f"nstep ({buffer_num}, {sub_size}): {len(script)} adds, {len(idx)} indices, worst e_ref / bar {worst:.3g}")


# ---- the sum tree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", oc.TREE_SIZES)
def test_tree_calls_cover_the_strided_loop(size):
    assert bound_of(size) == {1500: 2048, 70000: 131072}[size] and oc.TREE_NS == [1024, 1025, 4099]
    for (idx, val), n in zip(oc.tree_set_calls(size), oc.TREE_NS):
        assert len(idx) == len(val) == n and idx.min() >= 0 and idx.max() < size
        assert np.bincount(idx, minlength=size).max() >= 2              # duplicates: the last one wins
        if size == 1500 and n == 4099:
            assert np.bincount(idx, minlength=size).min() >= 2          # every leaf has duplicates
    trees = oc.tree_after(size)
    assert len(trees) == 3 and not np.array_equal(trees[0], trees[2])
    inner = np.arange(1, bound_of(size))
    assert np.array_equal(trees[-1][inner], trees[-1][2 * inner] + trees[-1][2 * inner + 1])


def test_prefix_values_meet_the_strict_comparison_exactly():
    t = oc.prefix_tree()
    vals, nodes, firsts = oc.prefix_values(t)
    assert len(vals) == 4099 and len(nodes) == 64 and (t.tree[t.bound:t.bound + t.size] > 0).all()
    assert np.array_equal(t.tree * 8, np.round(t.tree * 8))             # the lattice: every sum is exact
    out = t.prefix_sum_idx(vals)
    assert out.min() >= 0 and out.max() < t.size
    for v, k, first, leaf in zip(vals[-64:], nodes, firsts, out[-64:]):
        # replay the descent to node k: the value left in hand there equals the left child's sum, bit for bit ...
        node, rest = 1, float(v)
        while node != k:
            node *= 2
            if t.tree[node] < rest:
                rest -= t.tree[node]
                node += 1
            assert node <= k
        assert rest == t.tree[2 * k]
        # ... and the strict `<` sends it left: the answer is the last leaf left of the right child that holds weight
        assert leaf == first - 1 and leaf < first


@pytest.mark.parametrize("size", oc.TREE_SIZES)
@pytest.mark.parametrize("alpha", oc.PRIO_ALPHAS)
def test_priority_calls(size, alpha):
    p, after = oc.prio_after(size, alpha)
    assert len(after) == 2 * len(oc.TREE_NS) and p.max_prio > 1.0 and p.min_prio < 1.0
    leaves = after[-1][0][p.t.bound:]
    assert (leaves[:size] > 0).sum() >= min(size, 4000) and not leaves[size:].any()
    # float32 restatement of the leaves: (|td| + eps) ** alpha is float32 already; the IS weights are float64 in the reference
    idx = oc.prio_calls(size)[-2][1]
    for norm in (True, False):
        p.weight_norm = norm
        w = p.batch_weight(idx)
        assert np.isfinite(w).all() and (not norm or w.max() == 1.0)
        _inside_rel("IS weights", float(np.abs(w.astype(np.float32).astype(np.float64) - w).max()), w)


# ---- the C-ABI accepts every case's sizes ---------------------------------------------------------------------------------
def test_entry_points_accept_every_case_without_a_device():
    from tianshou_marl_amd import _abi, ops

    def passes_the_size_checks(fn):
        with pytest.raises(ValueError, match="null pointer"):   # the last check of every entry point, after the sizes
            fn()

    for c in oc.DQN_CASES:
        ops.dqn_check(c["A"])
        passes_the_size_checks(lambda: _abi.call("tsm_dqn_td_head", *[None] * 9, c["B"], c["A"], 1, 0.0, None, None, None, None, None))
        assert _abi.call("tsm_dqn_partial_elems", c["B"]) == 2 * -(-c["B"] // 256)
    for c in oc.DISTQ_CASES:
        ops.distq_check(c["A"], c["N"])
        B, A, N = c["B"], c["A"], c["N"]
        passes_the_size_checks(lambda: _abi.call("tsm_distq_values", None, None, B, A, N, 1, None, None, None))
        passes_the_size_checks(lambda: _abi.call("tsm_c51_head", *[None] * 10, B, A, N, oc.V_MIN, oc.V_MAX, None, None, None, None, None))
        passes_the_size_checks(lambda: _abi.call("tsm_qrdqn_head", *[None] * 10, B, A, N, None, None, None, None, None))
    for c in oc.IQN_CASES:
        B, A, N, Np = c["B"], c["A"], c["N"], c["Np"]
        ops.iqn_check(4, 16, N, A)
        ops.iqn_check(4, 16, Np, A)
        passes_the_size_checks(lambda: _abi.call("tsm_iqn_values", None, B, N, A, None, None))
        passes_the_size_checks(lambda: _abi.call("tsm_iqn_head", *[None] * 10, B, A, N, Np, None, None, None, None, None))
    for c in oc.EMBED_CASES:
        B, S, C, H = c["B"], c["S"], c["C"], c["H"]
        ops.iqn_check(C, H, S)
        passes_the_size_checks(lambda: _abi.call("tsm_iqn_embed_forward", None, None, None, None, B, S, C, H, c["relu_f"], None, None, None))
        for n_split, stride, w_off in ((1, H * C + H, 0), (3, H * C + H, 0), (B + 2, H * C + H, 0), (3, H * C + H + 24, 16)):
            passes_the_size_checks(lambda: _abi.call("tsm_iqn_embed_backward", None, None, None, None, B, S, C, H, c["relu_f"], None,
                                                     n_split, None, stride, w_off, w_off + H * C, None))
    for c in oc.DSAC_CASES:
        ops.dsac_check(c["A"])
        B, A = c["B"], c["A"]
        passes_the_size_checks(lambda: _abi.call("tsm_dsac_target", *[None] * 7, B, A, None, None))
        passes_the_size_checks(lambda: _abi.call("tsm_dsac_critic_head", *[None] * 5, B, A, None, None, None, None, None))
        passes_the_size_checks(lambda: _abi.call("tsm_dsac_actor_head", *[None] * 4, B, A, None, None, None, None))
    for size in oc.TREE_SIZES:
        assert _abi.call("tsm_segtree_bound", size) == bound_of(size)
