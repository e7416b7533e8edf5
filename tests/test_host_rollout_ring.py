"""The numpy expectations of tests/rollout_ring_cases.py against answers that do not come from them: the reference's own trace
(tests/golden/vrb_trace.npz) and a hand-written 2-env, 3-slot trace whose answers are spelled out below.  Runs on the CPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollout_ring_cases as rc  # noqa: E402


def test_expected_index_replays_the_reference_trace(golden_dir):
    """Sub-buffers are independent (manager.py:159-177), so the adds of the trace that touch sub-buffer e are a one-env run of
    `expected_index`: ptr / ep_idx / ep_len / ep_rew of every add, with the trace's reset(keep_statistics=True), and the manager's
    last_index where the trace recorded it.  Sub-buffers of 5 to 8 slots, 40 adds: every one wraps."""
    g = np.load(os.path.join(golden_dir, "vrb_trace.npz"), allow_pickle=True)
    n_checked = wrapped = 0
    for ci in range(int(g["n_cfg"])):
        p = f"c{ci}_"
        total, num, rew_dim = (int(x) for x in g[p + "cfg"])
        S, n_add, reset_at = int(g[p + "sub_size"]), int(g[p + "n_add"]), int(g[p + "reset_at"])
        for e in range(num):
            adds = [(ai, int(np.nonzero(g[f"{p}a{ai}_ids"] == e)[0][0])) for ai in range(n_add) if e in g[f"{p}a{ai}_ids"]]
            rew = np.stack([np.asarray(g[f"{p}a{ai}_rew"][r], np.float64).reshape(-1) for ai, r in adds]).astype(np.float32)
            done = np.array([bool(g[f"{p}a{ai}_term"][r] | g[f"{p}a{ai}_trunc"][r]) for ai, r in adds])
            resets = [k for k, (ai, _) in enumerate(adds) if ai >= reset_at][:1]
            exp = rc.expected_index(done[:, None], rew[:, None, :], S, resets)
            off = e * S
            for k, (ai, r) in enumerate(adds):
                q = f"{p}a{ai}_"
                assert exp["ptr"][k, 0] + off == g[q + "ptr"][r] and exp["ep_idx"][k, 0] + off == g[q + "ep_idx"][r], (ci, e, ai)
                assert exp["ep_len"][k, 0] == g[q + "ep_len"][r], (ci, e, ai)
                assert np.array_equal(exp["ep_rew"][k, 0], np.asarray(g[q + "ep_rew"][r], np.float64).reshape(-1)), (ci, e, ai)
                n_checked += 1
            # the last recorded last_index at or before this sub-buffer's last add is still its last_index
            rec = [ai for ai in range(adds[-1][0], n_add) if f"{p}a{ai}_last_index" in g]
            if rec and not adds[-1][0] < reset_at <= rec[0]:   # (a reset behind the last add moves last_index: not replayed here)
                assert exp["state"]["last_index"][0] + off == g[f"{p}a{rec[0]}_last_index"][e], (ci, e)
            wrapped += len(adds) > S
    assert n_checked > 300 and wrapped >= 15


# the hand-written trace: 2 envs, S = 3, N = 2 agents, 8 steps.
#   env 0: episodes end at t = 2 (slot 2, the LAST slot: the next episode starts at slot 0) and t = 7 (5 steps: longer than the ring)
#   env 1: episodes end at t = 0 (slot 0), t = 3 (slot 0, started at slot 1: wrapped) and t = 5 (slot 2, the last slot); t = 6, 7 run on
#   rew[t][e] = (t + 1 + e / 2, -(t + 1) + e / 2)
_DONE = np.zeros((8, 2), bool)
_DONE[[2, 7], 0] = True
_DONE[[0, 3, 5], 1] = True
_REW = np.array([[[t + 1 + 0.5 * e, -(t + 1) + 0.5 * e] for e in range(2)] for t in range(8)], np.float32)


def test_expected_index_on_the_hand_written_trace():
    exp = rc.expected_index(_DONE, _REW, 3)
    assert np.array_equal(exp["ptr"], [[0, 3], [1, 4], [2, 5], [0, 3], [1, 4], [2, 5], [0, 3], [1, 4]])
    assert np.array_equal(exp["ep_idx"], [[0, 3], [0, 4], [0, 4], [0, 4], [0, 4], [0, 4], [0, 3], [0, 3]])
    assert np.array_equal(exp["ep_len"], [[0, 1], [0, 0], [3, 0], [0, 3], [0, 0], [0, 2], [0, 0], [5, 0]])
    want_rew = np.zeros((8, 2, 2))
    want_rew[0, 1], want_rew[2, 0], want_rew[3, 1], want_rew[5, 1], want_rew[7, 0] = (1.5, -0.5), (6, -6), (10.5, -7.5), (12, -10), (30, -30)
    assert np.array_equal(exp["ep_rew"], want_rew)
    # episodes in (step, env) order; lens = rows in the buffer: the 5-step episode of env 0 ends at slot 1 having started at slot 0
    assert np.array_equal(exp["step"], [0, 2, 3, 5, 7]) and np.array_equal(exp["env"], [1, 0, 1, 1, 0])
    assert np.array_equal(exp["lens"], [1, 3, 3, 2, 2])
    assert np.array_equal(exp["returns"], [[1.5, -0.5], [6, -6], [10.5, -7.5], [12, -10], [30, -30]])
    st = exp["state"]
    assert np.array_equal(st["ins"], [2, 2]) and np.array_equal(st["size"], [3, 3]) and np.array_equal(st["lengths"], [3, 3])
    assert np.array_equal(st["ep_len"], [0, 2]) and np.array_equal(st["ep_start"], [2, 0]) and np.array_equal(st["last_index"], [1, 4])
    assert np.array_equal(st["ep_return"], [[0, 0], [16, -14]])
    lens, rets = rc.episodes_between(exp, 3, 6)
    assert np.array_equal(lens, [3, 2]) and np.array_equal(rets, [[10.5, -7.5], [12, -10]])
    words = rc.pack_state(st)
    assert words.dtype == np.int64 and len(words) == 6 * 2 + 2 * 2 + 1 and words[-1] == 0
    assert np.array_equal(words[:12], [2, 2, 3, 3, 0, 2, 2, 0, 1, 4, 3, 3])
    assert np.array_equal(words[12:16].view(np.float64), [0, 0, 16, -14])


def test_expected_index_with_a_statistics_keeping_reset():
    """reset(keep_statistics=True) before step 4: insertion, size and episode start go back to 0, the running episode keeps its
    length and return -- `lens` then counts rows since the reset (modulo the ring), the return stays whole."""
    exp = rc.expected_index(_DONE, _REW, 3, resets=[4])
    assert np.array_equal(exp["ptr"], [[0, 3], [1, 4], [2, 5], [0, 3], [0, 3], [1, 4], [2, 5], [0, 3]])
    assert np.array_equal(exp["ep_idx"], [[0, 3], [0, 4], [0, 4], [0, 4], [0, 3], [0, 3], [0, 5], [0, 5]])
    assert np.array_equal(exp["ep_len"], [[0, 1], [0, 0], [3, 0], [0, 3], [0, 0], [0, 2], [0, 0], [5, 0]])
    assert np.array_equal(exp["lens"], [1, 3, 3, 2, 1])
    assert np.array_equal(exp["returns"], [[1.5, -0.5], [6, -6], [10.5, -7.5], [12, -10], [30, -30]])
    st = exp["state"]
    assert np.array_equal(st["ins"], [1, 1]) and np.array_equal(st["size"], [3, 3]) and np.array_equal(st["ep_len"], [0, 2])
    assert np.array_equal(st["ep_start"], [1, 2]) and np.array_equal(st["last_index"], [0, 3])
    assert np.array_equal(st["ep_return"], [[0, 0], [16, -14]])


def test_expected_ring():
    rows = np.arange(8 * 2 * 2).reshape(8, 2, 2)   # row of step t, env e: [4 t + 2 e, 4 t + 2 e + 1]
    ring = rc.expected_ring(rows, 3)               # steps 6, 7, 5 are the last at slots 0, 1, 2
    assert ring.shape == (3, 2, 2) and np.array_equal(ring, rows[[6, 7, 5]])
    assert np.array_equal(rc.expected_ring(rows, 3, resets=[4]), rows[[7, 5, 6]])   # steps 4.. restart at slot 0
    assert np.array_equal(rc.expected_ring(rows, 1), rows[[7]]) and np.array_equal(rc.expected_ring(rows, 8), rows)
    short = rc.expected_ring(rows[:2], 3, init=-1)  # a slot never written keeps the initial value
    assert np.array_equal(short[:2], rows[:2]) and (short[2] == -1).all()
    assert np.array_equal(rc.slot_of_step(8, 3, [4]), [0, 1, 2, 0, 0, 1, 2, 0])


def test_expected_next_on_the_hand_written_trace():
    """Ring after the 8 steps: env 0 holds steps 6, 7 (done, newest), 5; env 1 holds steps 6, 7 (newest), 5 (done)."""
    exp = rc.expected_index(_DONE, _REW, 3)
    done_ring = rc.expected_ring(_DONE, 3)
    assert np.array_equal(done_ring, [[False, False], [True, False], [False, True]])
    nxt = rc.expected_next(done_ring, exp["state"]["last_index"], exp["state"]["lengths"], 3)
    assert np.array_equal(nxt, [1, 1, 0, 4, 4, 5])
    # a part-filled sub-buffer wraps at its length (manager.py:353): 2 rows of 3, the newest at slot 1
    assert np.array_equal(rc.expected_next(np.zeros((3, 1), bool), [1], [2], 3), [1, 1, 1])
