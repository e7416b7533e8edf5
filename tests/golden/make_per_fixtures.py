"""Generate tests/golden/per.npz by RUNNING THE REFERENCE's SegmentTree, PrioritizedVectorReplayBuffer and DQN
(tianshou/data/utils/segtree.py, data/buffer/prio.py, algorithm_base.py:560-582, 889-905; imported through
oracle/ref_shim.py, whose fake `njit` runs segtree.py un-jitted).  Every array is data: inputs, scripts of calls, expected
outputs.

Sections:
  ts_*   the tree under a script of sets, sizes 1, 2, 24 (bound 32), 32, 5000 (bound 8192): n = 300 random entries; one index
         three times in one call with different values; both children of one parent in one call; leaf 0 and leaf size - 1; one
         broadcast value; n = 1; a run of leaves set to 0 in the middle.  (Size 1 has no siblings: its calls all name leaf 0.)
         After every call the whole `_value` array.
  ps_*   get_prefix_sum_idx on the final tree of each size: 0.0, internal left sums exactly (the strict `<`), sums of
         leading leaves, nextafter(total, 0), random values -> the reference's indices.
  rd_*   reduce(start, end) on the tree of size 24.
  pa_*   PrioritizedVectorReplayBuffer(24, 3): add x2 -> update_weight(indices with repeats, td f32) -> add -> update_weight
         -> add, for alpha in {0.6, 1.0} x beta in {0.4, 1.0} x weight_norm on / off: the tree, max_prio, min_prio after every
         step; get_weight and buffer[indices].weight at the end; reset() leaves the tree as it is.  (The reference's manager
         drops weight_norm when it re-initialises itself from `options`, manager.py:250-255: the generator sets the flag on the
         built object, which is what a PrioritizedReplayBuffer given the flag does.)
  sm_*   37 priorities, three of them 0, and the seed of the device draw; the generator checks that numpy's own 65 536 draws
         through the reference tree stay within 5 sqrt(n p (1 - p)) of n p.
  dq_*   three DQN updates (MSE) through a prioritized buffer: net, rows and hyper-parameters of dqn.npz's up_* section,
         alpha 0.6, beta 0.4; the index sets drawn by the reference buffer, the IS weights fed to the loss, the losses, the
         leaves and max / min priority after each step, from a float64 run, with e_ref = |float32 run - float64 run|.
The generator asserts that tests/per_restatement.py equals the reference on every section.
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import ref_shim  # noqa: E402

ref_shim.install()

import torch  # noqa: E402
from tianshou.algorithm.modelfree.dqn import DQN, DiscreteQLearningPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, SegmentTree  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from dqn_restatement import DqnRestatement, RestatedBuffer, nstep_walk  # noqa: E402
from make_dqn_fixtures import QNet, flat  # noqa: E402
from per_restatement import RestatedPrio, RestatedTree  # noqa: E402

SIZES = (1, 2, 24, 32, 5000)
GAMMA = 0.99


# ---- ts / ps / rd --------------------------------------------------------------------------------------------------
def set_script(rs, size):
    """[(index i64 [n], value f64 [n] or a float)]."""
    pick = lambda n: rs.randint(0, size, n).astype(np.int64)  # noqa: E731
    val = lambda n: (rs.rand(n) * 3.0 + 0.01)  # noqa: E731
    a, b, c = (int(x) for x in (pick(3) if size < 3 else rs.choice(size, 3, replace=False)))
    j = 0 if size < 2 else 2 * int(rs.randint(0, size // 2))
    mid = np.arange(size // 3, size // 3 + max(1, size // 6), dtype=np.int64)
    calls = [(pick(300), val(300)),
             (np.array([a, b, a, c, a], np.int64), val(5)),                       # one index three times
             (np.array([j, min(j + 1, size - 1)], np.int64), val(2)),             # both children of one parent
             (np.array([0, size - 1], np.int64), val(2)),                         # the first and the last leaf
             (pick(7), float(rs.rand() + 0.5)),                                   # one value for all
             (pick(1), val(1)),                                                   # n = 1
             (mid, 0.0)]                                                          # zero-weight leaves in the middle
    if size > 1:
        calls.append((np.array([0, 1, size - 1], np.int64), val(3)))             # (so that the total is positive)
    return calls


def tree_sections(res):
    rs = np.random.RandomState(17)
    for size in SIZES:
        ref, R = SegmentTree(size), RestatedTree(size)
        calls = set_script(rs, size)
        res[f"ts_{size}_ncalls"] = np.int64(len(calls))
        for k, (idx, v) in enumerate(calls):
            ref[idx] = v if isinstance(v, float) else v.copy()
            R.set(idx, v)
            assert np.array_equal(ref._value, R.tree), (size, k)
            res[f"ts_{size}_c{k}_idx"] = idx
            res[f"ts_{size}_c{k}_val"] = np.atleast_1d(np.asarray(v, np.float64))
            res[f"ts_{size}_c{k}_tree"] = ref._value.copy()
        if size == 1:   # its last call set the only leaf to 0: give it weight again
            ref[np.array([0])] = np.array([0.75])
            R.set([0], [0.75])
            res["ts_1_c7_idx"], res["ts_1_c7_val"], res["ts_1_c7_tree"] = np.array([0]), np.array([0.75]), ref._value.copy()
            res["ts_1_ncalls"] = np.int64(8)
        tree, bound, total = ref._value, ref._bound, float(ref.reduce())
        assert total > 0
        vals = [0.0, np.nextafter(total, 0.0)]
        k = 2
        while k < 2 * bound:            # the left sums on the leftmost path and on the path to a middle leaf
            vals.append(tree[k])
            k *= 2
        leaves = tree[bound:bound + size]
        cs = np.cumsum(leaves)
        for cut in {0, size // 3, size // 3 + max(1, size // 6) - 1, size // 2, size - 2}:
            if 0 <= cut < size - 1:
                vals.append(cs[cut])     # a sum of leading leaves (right before / inside / after the zero run)
        if bound >= 4:
            vals.append(tree[2] + tree[6])
        vals += list(rs.rand(40) * total)
        vals = np.array([v for v in vals if 0.0 <= v < total], np.float64)
        out = ref.get_prefix_sum_idx(vals.copy())
        assert np.array_equal(out, R.prefix_sum_idx(vals)) and (out < size).all(), size
        res[f"ps_{size}_value"], res[f"ps_{size}_index"] = vals, out.astype(np.int64)
        if size == 24:
            spans = [(0, 24), (0, 1), (3, 17), (8, 16), (23, 24), (5, 6), (1, 23)]
            red = np.array([ref.reduce(s, e) for s, e in spans])
            assert np.array_equal(red, [R.reduce(s, e) for s, e in spans]) and ref.reduce() == R.reduce()
            res["rd_spans"], res["rd_sums"] = np.array(spans, np.int64), red


# ---- pa -------------------------------------------------------------------------------------------------------------
PA_CASES = [(a, b, wn) for a in (0.6, 1.0) for b in (0.4, 1.0) for wn in (True, False)]


def rows(rs, n_env, D):
    return Batch(obs=rs.standard_normal((n_env, D)).astype(np.float32), act=rs.randint(0, 3, n_env), rew=rs.standard_normal(n_env),
                 terminated=rs.rand(n_env) < 0.2, truncated=np.zeros(n_env, bool),
                 obs_next=rs.standard_normal((n_env, D)).astype(np.float32))


def prio_section(res):
    rs = np.random.RandomState(23)
    n_env, total, D = 3, 24, 2
    adds = [rows(rs, n_env, D) for _ in range(4)]
    for k, b in enumerate(adds):
        res.update({f"pa_add{k}_{f}": np.asarray(b[f]) for f in ("obs", "act", "rew", "terminated", "truncated", "obs_next")})
    upd = [(np.array([0, 8, 1, 8, 16, 8, 9], np.int64), np.array([0.3, -2.5, 0.0, 0.7, -0.05, 1.75, 3.0], np.float32)),
           (np.array([16, 2, 2, 10], np.int64), np.array([-1e-3, 0.4, -0.9, 5.5], np.float32))]
    query = np.array([0, 1, 2, 8, 9, 10, 16, 17, 18, 8, 3, 11], np.int64)
    for k, (i, t) in enumerate(upd):
        res[f"pa_upd{k}_idx"], res[f"pa_upd{k}_td"] = i, t
    res["pa_query"] = query
    res["pa_cases"] = np.array([f"a{a}_b{b}_n{int(wn)}" for a, b, wn in PA_CASES])
    script = ["add0", "add1", "upd0", "add2", "upd1", "add3"]
    res["pa_script"] = np.array(script)
    for c, (alpha, beta, wn) in enumerate(PA_CASES):
        buf = PrioritizedVectorReplayBuffer(total, n_env, alpha=alpha, beta=beta, weight_norm=wn)
        buf._weight_norm = wn      # manager.py:250-255 dropped it
        R = RestatedPrio(total, alpha, beta, wn)
        trees, pairs = [], []
        for step in script:
            k = int(step[3:])
            if step.startswith("add"):
                ptr = buf.add(adds[k], buffer_ids=np.arange(n_env))[0]
                R.init_weight(ptr)
            else:
                buf.update_weight(*upd[k])
                R.update_weight(*upd[k])
            assert np.array_equal(buf.weight._value, R.t.tree), (c, step)
            assert float(buf._max_prio) == R.max_prio and float(buf._min_prio) == R.min_prio, (c, step)
            trees.append(buf.weight._value.copy())
            pairs.append([float(buf._max_prio), float(buf._min_prio)])
        gw, bw = buf.get_weight(query), buf[query].weight
        assert np.array_equal(gw, R.get_weight(query)) and np.array_equal(bw, R.batch_weight(query)), c
        assert gw.dtype == np.float64 and bw.dtype == np.float64
        before = buf.weight._value.copy()
        buf.reset()
        assert np.array_equal(buf.weight._value, before) and len(buf) == 0
        res.update({f"pa_c{c}_trees": np.stack(trees), f"pa_c{c}_prio": np.array(pairs), f"pa_c{c}_get_weight": gw,
                    f"pa_c{c}_batch_weight": bw})


# ---- sm -------------------------------------------------------------------------------------------------------------
def sample_section(res):
    rs = np.random.RandomState(31)
    size, n = 37, 65536
    prio = (rs.rand(size) ** 3 * 4.0 + 1e-3)
    prio[[5, 20, 36]] = 0.0
    ref = SegmentTree(size)
    ref[np.arange(size)] = prio.copy()
    p = prio / prio.sum()
    np.random.seed(31)
    draws = ref.get_prefix_sum_idx(np.random.rand(n) * ref.reduce())
    cnt = np.bincount(draws, minlength=size)
    assert (np.abs(cnt - n * p) <= 5.0 * np.sqrt(n * p * (1 - p))).all() and not cnt[[5, 20, 36]].any()
    res.update(sm_prio=prio, sm_n=np.int64(n), sm_seed=np.int64(20240531))


# ---- dq -------------------------------------------------------------------------------------------------------------
def dqn_section(res):
    g = dict(np.load(os.path.join(HERE, "dqn.npz")))
    d = [int(x) for x in g["up_dims"]]
    dims, (B, n_env, S, n_step, freq, steps, T) = d[:4], d[4:]
    alpha, beta = 0.6, 0.4
    A = dims[-1]
    net = QNet(dims)
    with torch.no_grad():
        o = 0
        for p in net.parameters():
            p.copy_(torch.as_tensor(g["up_init"][o:o + p.numel()]).reshape(p.shape))
            o += p.numel()
    assert np.array_equal(flat(net).astype(np.float32), g["up_init"])
    algos, bufs = {}, {}
    for dbl in (True, False):
        m = copy.deepcopy(net).double() if dbl else copy.deepcopy(net)
        pol = DiscreteQLearningPolicy(model=m, action_space=gym.spaces.Discrete(A))
        algos[dbl] = DQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), gamma=GAMMA, n_step_return_horizon=n_step,
                         target_update_freq=freq)
        dt = np.float64 if dbl else np.float32
        buf = PrioritizedVectorReplayBuffer(n_env * S, n_env, alpha=alpha, beta=beta)
        for t in range(T):
            buf.add(Batch(obs=g["up_rows_obs"][t].astype(dt), act=g["up_rows_act"][t], rew=g["up_rows_rew"][t].astype(np.float64),
                          terminated=g["up_rows_term"][t], truncated=g["up_rows_trunc"][t],
                          obs_next=g["up_rows_obs_next"][t].astype(dt)), buffer_ids=np.arange(n_env))
        bufs[dbl] = buf
    RB = RestatedBuffer(n_env, S, 1)
    for t in range(T):
        for e in range(n_env):
            RB.add(e, g["up_rows_rew"][t, e], bool(g["up_rows_term"][t, e]), bool(g["up_rows_trunc"][t, e]))
    R = DqnRestatement(g["up_init"], dims, target_update_freq=freq)
    RP = RestatedPrio(n_env * S, alpha, beta)
    RP.t.tree[:] = bufs[True].weight._value
    bound = bufs[True].weight._bound
    res.update(dq_alpha=np.float64(alpha), dq_beta=np.float64(beta))
    np.random.seed(41)
    for k in range(steps):
        indices = bufs[True].sample_indices(B).astype(np.int64)     # drawn by the reference buffer from its own tree
        assert len(indices) == B and len(np.unique(indices)) < B     # repeats: the last TD error of a row wins
        out = {}
        for dbl, algo in algos.items():
            buf = bufs[dbl]
            batch = buf[indices]
            w_in = np.asarray(batch.weight, np.float64).copy()
            batch = algo._preprocess_batch(batch, buf, indices)
            stats = algo._update_with_batch(batch)
            algo._postprocess_batch(batch, buf, indices)
            out[dbl] = (stats.loss, w_in, buf.weight._value[bound:bound + n_env * S].copy(),
                        np.array([float(buf._max_prio), float(buf._min_prio)]), buf.weight._value.copy())
        # the restatement, fed float32 TD errors as the device path is (the float64 run's differ from them by e_ref)
        idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
        o_, on_ = bufs[False][indices].obs, bufs[False][idx_n].obs_next
        w_r = RP.batch_weight(indices)
        r = R.update(o_, bufs[False][indices].act, on_, None, mc, gpow, vmask, weight=w_r)
        RP.update_weight(indices, r["td_error"].astype(np.float32))
        assert abs(r["loss"] - out[True][0]) <= 1e-5 * abs(out[True][0]), (k, r["loss"], out[True][0])
        assert np.allclose(w_r, out[True][1], rtol=1e-5) and np.allclose(RP.t.tree, out[True][4], rtol=1e-5, atol=1e-7)
        e = lambda j: np.float64(np.abs(np.asarray(out[True][j], np.float64) - np.asarray(out[False][j], np.float64)).max())  # noqa: E731
        res.update({f"dq_s{k}_indices": indices, f"dq_s{k}_loss": np.array([out[True][0], out[False][0]]),
                    f"dq_s{k}_weight": out[True][1], f"dq_s{k}_weight_eref": e(1), f"dq_s{k}_leaves": out[True][2],
                    f"dq_s{k}_leaves_eref": e(2), f"dq_s{k}_prio": out[True][3], f"dq_s{k}_prio_eref": e(3)})
    print("prioritized dqn losses", [float(res[f"dq_s{k}_loss"][0]) for k in range(steps)])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    res = {}
    tree_sections(res)
    prio_section(res)
    sample_section(res)
    dqn_section(res)
    path = os.path.join(HERE, "per.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
