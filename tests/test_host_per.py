"""CPU tests of prioritized replay: the numpy restatement (tests/per_restatement.py) against the reference's own runs
(tests/golden/per.npz), the import surface, the constructor checks of PrioritizedVectorReplayBuffer, the argument checks of
tsm_segtree_bound / tsm_segtree_set / tsm_segtree_prefix_sum_idx / tsm_segtree_reduce / tsm_segtree_check / tsm_per_sample /
tsm_per_update_weight / tsm_per_init_weight / tsm_per_get_weight that fail before touching a device, and the wrappers'
refusal of CPU tensors."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "per.npz")

from per_restatement import RestatedPrio, RestatedTree, bound_of  # noqa: E402

SIZES = (1, 2, 24, 32, 5000)


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def tree_calls(g, size):
    """[(index, value (one entry: broadcast), expected tree)] of the `ts_*` script of one size."""
    return [(g[f"ts_{size}_c{k}_idx"], g[f"ts_{size}_c{k}_val"], g[f"ts_{size}_c{k}_tree"]) for k in range(int(g[f"ts_{size}_ncalls"]))]


def pa_case(name):
    a, b, n = name.split("_")
    return float(a[1:]), float(b[1:]), n[1:] == "1"


def pa_batch(g, k):
    from tianshou_marl_amd.data import Batch

    return Batch(**{f: g[f"pa_add{k}_{f}"] for f in ("obs", "act", "rew", "terminated", "truncated", "obs_next")})


# ---- the restatement against the reference's runs -------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_restatement_reproduces_the_tree(g, size):
    calls = tree_calls(g, size)
    R = RestatedTree(size)
    assert R.bound == bound_of(size) and len(calls[0][2]) == 2 * R.bound
    for idx, val, tree in calls:
        R.set(idx, val if len(val) == len(idx) else float(val[0]))
        assert np.array_equal(R.tree, tree)
    assert np.array_equal(R.prefix_sum_idx(g[f"ps_{size}_value"]), g[f"ps_{size}_index"])
    if size == 24:
        assert [R.reduce(int(s), int(e)) for s, e in g["rd_spans"]] == list(g["rd_sums"])


def test_fixture_covers_the_cases_asked_for(g):
    for size in SIZES:
        calls = tree_calls(g, size)
        assert len(calls[0][0]) == 300 and any(len(c[0]) == 1 for c in calls)
        assert any(len(c[1]) == 1 and len(c[0]) > 1 for c in calls)                                    # one value for all
        assert any(np.bincount(c[0]).max() >= 3 and len(set(c[1])) == len(c[1]) for c in calls[1:2])   # thrice, values differ
        assert any(0 in c[0] and size - 1 in c[0] for c in calls)
        if size > 1:
            assert any(len(c[0]) == 2 and c[0][0] % 2 == 0 and c[0][1] == c[0][0] + 1 for c in calls)  # two siblings
        tree, v = calls[-1][2], g[f"ps_{size}_value"]
        total = tree[1]
        assert v[0] == 0.0 and np.nextafter(total, 0.0) in v and (v < total).all()
        if size > 1:
            assert tree[2] in v                                                                        # a left sum, exactly
    tree = tree_calls(g, 24)[-1][2]
    leaves = tree[32:32 + 24]
    assert (leaves[8:12] == 0).all() and leaves[:8].all() and leaves[12:].any()                        # zero leaves in the middle


@pytest.mark.parametrize("case", range(8))
def test_restatement_reproduces_the_priorities(g, case):
    alpha, beta, norm = pa_case(str(g["pa_cases"][case]))
    R = RestatedPrio(24, alpha, beta, norm)
    ptr = {0: [0, 8, 16], 1: [1, 9, 17], 2: [2, 10, 18], 3: [3, 11, 19]}   # every add fills the next slot of each sub-buffer
    for s, step in enumerate(g["pa_script"]):
        k = int(step[3:])
        if step.startswith("add"):
            R.init_weight(ptr[k])
        else:
            R.update_weight(g[f"pa_upd{k}_idx"], g[f"pa_upd{k}_td"])
        assert np.array_equal(R.t.tree, g[f"pa_c{case}_trees"][s]), step
        assert [R.max_prio, R.min_prio] == list(g[f"pa_c{case}_prio"][s])
    assert np.array_equal(R.get_weight(g["pa_query"]), g[f"pa_c{case}_get_weight"])
    assert np.array_equal(R.batch_weight(g["pa_query"]), g[f"pa_c{case}_batch_weight"])
    assert np.bincount(g["pa_upd0_idx"]).max() == 3 and (g[f"pa_c{case}_prio"][-1] != 1.0).all()


def test_numpy_draws_meet_the_binomial_bound(g):
    """The bound test_gpu_per.py holds the device draws to, on numpy's own draws through the restated tree."""
    prio, n = g["sm_prio"], int(g["sm_n"])
    assert len(prio) == 37 and (prio == 0).sum() == 3
    R = RestatedTree(37)
    R.set(np.arange(37), prio)
    rs = np.random.RandomState(5)
    cnt = np.bincount(R.prefix_sum_idx(rs.rand(n) * R.reduce()), minlength=37)
    p = prio / prio.sum()
    assert (np.abs(cnt - n * p) <= 5.0 * np.sqrt(n * p * (1 - p))).all() and not cnt[prio == 0].any()


# ---- the class and the entry points without a device -------------------------------------------------------------------
def test_class_exists_and_validates():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.data import DeviceVectorReplayBuffer, PrioritizedVectorReplayBuffer, VectorReplayBuffer
    from tianshou_marl_amd.data.buffer import PrioritizedVectorReplayBuffer as P2

    assert PrioritizedVectorReplayBuffer is P2 and issubclass(P2, VectorReplayBuffer) and issubclass(P2, DeviceVectorReplayBuffer)
    with pytest.raises(AssertionError):
        P2(40, 3, alpha=0.0, beta=0.4, device="cpu")
    with pytest.raises(AssertionError):
        P2(40, 3, alpha=0.6, beta=-0.1, device="cpu")
    buf = P2(40, 3, alpha=0.6, beta=0.4, device="cpu")
    assert (buf.maxsize, buf.weight.size, buf.weight.bound, len(buf.weight.tree)) == (42, 42, 64, 128)
    assert buf.options["alpha"] == 0.6 and buf.options["beta"] == 0.4 and buf._weight_norm
    assert buf.prio.tolist() == [1.0, 1.0] and buf.prio.dtype == torch.float64 and not buf.weight.tree.any()
    assert (buf.weight.mark == -1).all() and len(buf) == 0
    buf.set_beta(0.7)
    assert buf._beta == 0.7
    assert buf.unfused_adds_only and not DeviceVectorReplayBuffer.unfused_adds_only and not VectorReplayBuffer.unfused_adds_only
    for name in ("update_weight", "init_weight", "get_weight", "sample_indices_device", "batch_weight_device"):
        assert callable(getattr(buf, name)), name
    assert not hasattr(VectorReplayBuffer(40, 3), "update_weight")
    with pytest.raises(AssertionError, match="outside the segment tree"):
        buf.init_weight(np.array([42]))
    for name in ("segtree_set", "segtree_prefix_sum_idx", "segtree_reduce", "segtree_check", "per_sample", "per_update_weight",
                 "per_init_weight", "per_get_weight", "segtree_bound", "DeviceSegmentTree"):
        assert hasattr(ops, name), name


def test_entry_points_reject_bad_arguments_without_a_device():
    from tianshou_marl_amd import _abi, ops

    assert [ops.segtree_bound(s) for s in (1, 2, 3, 24, 32, 33, 5000)] == [1, 2, 4, 32, 32, 64, 8192]
    with pytest.raises(ValueError, match="outside"):
        ops.segtree_bound(0)
    assert _abi.call("tsm_segtree_bound", (1 << 30) + 1) == -1
    p = 1   # a non-null address that a failing call never reads
    with pytest.raises(ValueError, match="size = 0"):
        _abi.call("tsm_segtree_set", p, p, 0, p, 4, p, 4, p, None)
    with pytest.raises(ValueError, match="3 values for 4 indices"):
        _abi.call("tsm_segtree_set", p, p, 8, p, 4, p, 3, p, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_segtree_set", p, None, 8, p, 4, p, 4, p, None)
    _abi.call("tsm_segtree_set", p, None, 8, None, 0, None, 0, None, None)   # nothing to do
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_segtree_prefix_sum_idx", p, 8, None, 4, None, None)
    with pytest.raises(ValueError, match="negative"):
        _abi.call("tsm_segtree_prefix_sum_idx", p, 8, p, -1, p, None)
    with pytest.raises(ValueError, match=r"\[3, 9\) outside \[0, 8\)"):
        _abi.call("tsm_segtree_reduce", p, 8, 3, 9, p, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_segtree_check", None, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_per_sample", p, 8, 4, 0, 0, None, None, None)
    _abi.call("tsm_per_sample", p, 8, 0, 0, 0, None, None, None)
    with pytest.raises(ValueError, match="alpha = 0 must be positive"):
        _abi.call("tsm_per_update_weight", p, p, 8, p, p, 4, 0.0, p, p, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_per_update_weight", p, p, 8, p, None, 4, 0.6, p, p, None)
    with pytest.raises(ValueError, match="must be positive"):
        _abi.call("tsm_per_init_weight", p, p, 8, p, 4, -1.0, p, p, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_per_init_weight", p, p, 8, p, 4, 0.6, None, p, None)
    with pytest.raises(ValueError, match="beta = -0.5 is negative"):
        _abi.call("tsm_per_get_weight", p, 8, p, 4, -0.5, 1, p, p, p, p, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_per_get_weight", p, 8, p, 4, 0.4, 1, p, None, p, p, None)


def test_ops_refuse_cpu_tensors():
    from tianshou_marl_amd import ops

    t = ops.DeviceSegmentTree(8, device="cpu")
    idx, val = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.float64)
    # a Python float handed to the class keeps all of its float64 bits on the way to the device (not torch's default float32)
    assert t._dev(0.1, torch.float64).item() == 0.1 and t._dev([0.1, 0.7], torch.float64).tolist() == [0.1, 0.7]
    assert t._dev(np.array([3, 5]), torch.int64).tolist() == [3, 5] and t._dev(7, torch.int64).shape == (1,)
    prio = torch.ones(2, dtype=torch.float64)
    for fn in (lambda: ops.segtree_set(t, idx, val), lambda: ops.segtree_prefix_sum_idx(t, val),
               lambda: ops.per_update_weight(t, idx, torch.zeros(4), 0.6, prio), lambda: ops.per_init_weight(t, idx, 0.6, prio),
               lambda: ops.per_get_weight(t, idx, 0.4, True, prio), lambda: ops.per_sample(t, 4, 0), lambda: ops.segtree_reduce(t, 0, 4),
               lambda: ops.segtree_check(t), lambda: t.__setitem__([1], [2.0])):
        with pytest.raises(RuntimeError, match="no CPU path|device \\(HIP\\) tensors"):
            fn()
