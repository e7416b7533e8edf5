"""GPU tests (`-m gpu`) of prioritized replay: the device sum tree (csrc/segtree.hip), priority-proportional sampling, the
priority arithmetic of PrioritizedVectorReplayBuffer, DQN through a prioritized buffer, and the Collector's add path.

Reference: tests/golden/per.npz, the reference's own runs (tests/golden/make_per_fixtures.py).  Bars:
  * the tree after every set, the prefix-sum indices, reduce: equal, no tolerance (the same float64 additions);
  * leaves written from float32 TD errors, max_prio / min_prio, IS weights: the project's 1e-5 relative bar (DESIGN.md
    section 6); with alpha = 1 the leaves are bit-exact; every internal node is exactly the sum of its two stored children;
  * the DQN run: test_gpu_dqn.py's  |hip - ref64| <= 4 max(e_ref, 8 ulp(max |ref64|)), e_ref = the reference's own float32
    error, recorded in the fixture;
  * sampling: every count within 5 sqrt(n p (1 - p)) of n p -- the binomial bound.
Every comparison prints `PARITY name: ...` with the worst ratio to its bar."""
import logging
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "per.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")
DEV = "cuda"

from test_gpu_dqn import _check, _d, _dqn, _rel  # noqa: E402
from test_host_dqn import _Env, up_inputs  # noqa: E402
from test_host_per import SIZES, pa_batch, pa_case, tree_calls  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.data import Batch, PrioritizedVectorReplayBuffer
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def trees(g):
    """The `ts_*` scripts replayed on the device, checked after every call; the final trees serve the prefix-sum tests."""
    out = {}
    for size in SIZES:
        t = ops.DeviceSegmentTree(size, device=DEV)
        for k, (idx, val, ref) in enumerate(tree_calls(g, size)):
            ops.segtree_set(t, _d(idx), _d(val))
            out[size, k] = np.array_equal(t.tree.cpu().numpy(), ref)
        t.check()
        assert (t.mark == -1).all()
        out[size] = t
    return out


# ---- 1. the tree ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_tree_set_is_bit_exact(g, trees, size):
    n_calls = int(g[f"ts_{size}_ncalls"])
    bad = [k for k in range(n_calls) if not trees[size, k]]
    assert not bad, f"size {size}: the tree differs from the reference's after calls {bad}"
    t = trees[size]
    assert len(t.tree) == 2 * ops.segtree_bound(size) and t.tree[0] == 0
    print(f"PARITY tree size {size}: {n_calls} calls, whole tree equal after each")


def test_tree_set_through_the_class_and_index_errors(g):
    t = ops.DeviceSegmentTree(24, device=DEV)
    for idx, val, ref in tree_calls(g, 24):
        t[idx] = val if len(val) == len(idx) else float(val[0])      # SegmentTree.__setitem__, a float broadcasts
    ref = tree_calls(g, 24)[-1][2]
    assert np.array_equal(t.tree.cpu().numpy(), ref)
    assert np.array_equal(t[np.arange(24)].cpu().numpy(), ref[32:56]) and float(t.reduce()) == ref[1]
    got = [float(t.reduce(int(s), int(e))) for s, e in g["rd_spans"]]                # tsm_segtree_reduce
    assert got == list(g["rd_sums"]) and float(t.reduce(3)) == float(t.reduce(3, 24)) == float(t.reduce(3, -0 + 24))
    # an index outside [0, size) is skipped, the rest of the call lands, and the error word reports it once
    before = t.tree.clone()
    ops.segtree_set(t, _d(np.array([24, 3, -1, 40], np.int64)), _d(np.array([9.0, 2.5, 9.0, 9.0])))
    now = t.tree.cpu().numpy()
    exp = before.cpu().numpy().copy()
    exp[32 + 3] = 2.5
    for k in (17, 8, 4, 2, 1):
        exp[k] = exp[2 * k] + exp[2 * k + 1]
    assert np.array_equal(now, exp) and (t.mark == -1).all()
    with pytest.raises(ValueError, match="outside"):
        t.check()
    t.check()   # cleared
    with pytest.raises(ValueError, match="2 values for 3 indices"):
        ops.segtree_set(t, _d(np.array([1, 2, 3], np.int64)), _d(np.array([1.0, 2.0])))


# ---- 2. prefix sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_prefix_sum_index_is_bit_exact(g, trees, size):
    t = trees[size]
    v, ref = g[f"ps_{size}_value"], g[f"ps_{size}_index"]
    got = ops.segtree_prefix_sum_idx(t, _d(v)).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, ref), (size, np.nonzero(got != ref)[0])
    assert np.array_equal(t.get_prefix_sum_idx(v).cpu().numpy(), ref)
    print(f"PARITY prefix size {size}: {len(v)} values, indices equal")


# ---- 3. priorities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(8))
def test_priority_arithmetic_matches_reference(g, case):
    alpha, beta, norm = pa_case(str(g["pa_cases"][case]))
    buf = PrioritizedVectorReplayBuffer(24, 3, alpha=alpha, beta=beta, weight_norm=norm, n_agent=1, obs_dim=2, device=DEV)
    assert buf.weight.bound == 32
    worst = {}

    def rel(key, got, ref):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        r = float((np.abs(got - ref) / (1e-5 * np.maximum(np.abs(ref), np.finfo(np.float64).tiny))).max())
        worst[key] = max(worst.get(key, 0.0), r)
        assert r <= 1.0, (key, r)

    for s, step in enumerate(g["pa_script"]):
        k = int(step[3:])
        if step.startswith("add"):
            b = pa_batch(g, k)
            b.obs, b.obs_next, b.act, b.rew = b.obs[:, None], b.obs_next[:, None], b.act[:, None], b.rew[:, None].astype(np.float32)
            ptr = buf.add(b, buffer_ids=np.arange(3))[0]
            assert np.array_equal(ptr, [k, 8 + k, 16 + k])
        else:
            buf.update_weight(g[f"pa_upd{k}_idx"], g[f"pa_upd{k}_td"] if k == 0 else torch.as_tensor(g[f"pa_upd{k}_td"]).to(DEV))
        tree, ref = buf.weight.tree.cpu().numpy(), g[f"pa_c{case}_trees"][s]
        leaves, ref_leaves = tree[32:], ref[32:]
        assert np.array_equal(leaves == 0, ref_leaves == 0)
        rel("leaves", leaves[ref_leaves != 0], ref_leaves[ref_leaves != 0])
        if alpha == 1.0:
            assert np.array_equal(leaves, ref_leaves), step
        inner = np.arange(1, 32)
        assert np.array_equal(tree[inner], tree[2 * inner] + tree[2 * inner + 1]), step    # exactly the sum of its children
        rel("prio", buf.prio.cpu().numpy(), g[f"pa_c{case}_prio"][s])
    q = g["pa_query"]
    gw, bw = buf.get_weight(q), buf[q].weight
    assert gw.dtype == np.float64 and bw.dtype == np.float64 and isinstance(buf.get_weight(8), float)
    rel("get_weight", gw, g[f"pa_c{case}_get_weight"])
    rel("batch_weight", bw, g[f"pa_c{case}_batch_weight"])
    w32, w64 = buf.batch_weight_device(_d(q))
    assert np.array_equal(w64.cpu().numpy(), bw) and np.array_equal(w32.cpu().numpy(), bw.astype(np.float32))
    assert not norm or bw.max() == 1.0
    before = buf.weight.tree.clone()
    pair = buf.prio.clone()
    buf.reset()
    assert len(buf) == 0 and torch.equal(buf.weight.tree, before) and torch.equal(buf.prio, pair)
    assert len(buf.sample_indices(5)) == 0                   # an empty buffer takes the parent's path (prio.py:64)
    buf.weight.check()
    for key, r in worst.items():
        print(f"PARITY pa {g['pa_cases'][case]} {key}: max |hip - ref| / (1e-5 |ref|) = {r:.3g}")


# ---- 4. sampling --------------------------------------------------------------------------------------------------------
def test_device_sampling_follows_the_priorities(g):
    prio, n, seed = g["sm_prio"], int(g["sm_n"]), int(g["sm_seed"])
    assert n == 65536 and len(prio) == 37
    t = ops.DeviceSegmentTree(37, device=DEV)
    t[np.arange(37)] = prio
    a = ops.per_sample(t, n, seed, offset=1000)
    an = a.cpu().numpy()
    assert an.dtype == np.int64 and an.min() >= 0 and an.max() < 37
    cnt = np.bincount(an, minlength=37)
    assert not cnt[prio == 0].any()
    p = prio / prio.sum()
    ratio = np.abs(cnt - n * p)[p > 0] / (5.0 * np.sqrt(n * p * (1 - p)))[p > 0]
    print(f"PARITY sampling: max |count - n p| / (5 sqrt(n p (1 - p))) = {ratio.max():.3g}")
    assert (ratio <= 1.0).all()
    assert torch.equal(ops.per_sample(t, n, seed, offset=1000), a)                       # same seed and counter
    assert not torch.equal(ops.per_sample(t, n, seed, offset=1000 + n), a)               # another counter
    assert not torch.equal(ops.per_sample(t, n, seed + 1, offset=1000), a)
    off = torch.full((1,), 600, dtype=torch.int64, device=DEV)                           # a device counter adds to the offset
    assert torch.equal(ops.per_sample(t, n, seed, offset=400, offset_dev=off), a)
    head, tail = ops.per_sample(t, 100, seed, offset=1000), ops.per_sample(t, n - 100, seed, offset=1100)
    assert torch.equal(torch.cat([head, tail]), a)                                       # drawn in pieces = drawn at once
    one = ops.DeviceSegmentTree(1, device=DEV)                                           # bound 1: no level to descend
    one[[0]] = [0.3]
    assert not ops.per_sample(one, 64, seed).any()


# ---- 5. DQN -------------------------------------------------------------------------------------------------------------
def _up_buffer(gd, cls, **kw):
    dims, B, n_env, S, n_step, freq, steps, T, *_ = up_inputs(gd)
    buf = cls(n_env * S, n_env, n_agent=1, obs_dim=dims[0], device=DEV, **kw)
    for t in range(T):
        buf.add(Batch(obs=gd["up_rows_obs"][t][:, None], act=gd["up_rows_act"][t][:, None], rew=gd["up_rows_rew"][t][:, None],
                      terminated=gd["up_rows_term"][t], truncated=gd["up_rows_trunc"][t],
                      obs_next=gd["up_rows_obs_next"][t][:, None]), buffer_ids=np.arange(n_env))
    return buf


def _up_dqn(gd):
    dims, B, n_env, S, n_step, freq, *_ = up_inputs(gd)
    return _dqn(gd["up_init"], dims, gamma=float(gd["gamma"]), n_step_return_horizon=n_step, target_update_freq=freq)


def test_dqn_through_a_prioritized_buffer_matches_reference(g):
    gd = dict(np.load(DQN_GOLD))
    dims, B, n_env, S, n_step, freq, steps, T, *_ = up_inputs(gd)
    buf = _up_buffer(gd, PrioritizedVectorReplayBuffer, alpha=float(g["dq_alpha"]), beta=float(g["dq_beta"]))
    algo = _up_dqn(gd)
    assert algo.huber_loss_delta is None and (B, steps) == (37, 3)
    for k in range(steps):
        idx = _d(g[f"dq_s{k}_indices"])
        batch = algo._sampled_batch(buf, idx)
        w_in = batch.weight.clone()
        assert w_in.dtype == torch.float32 and w_in.is_cuda
        batch = algo._preprocess_batch(batch, buf, idx)
        stats = algo._update_with_batch(batch)
        assert batch.weight.is_cuda and batch.weight.shape == (B,)      # the TD errors
        algo._postprocess_batch(batch, buf, idx)
        ref64, ref32 = (float(x) for x in g[f"dq_s{k}_loss"])
        _check(f"per s{k} IS weights", w_in.cpu().numpy(), g[f"dq_s{k}_weight"], float(g[f"dq_s{k}_weight_eref"]))
        _check(f"per s{k} loss", [stats.loss], [ref64], abs(ref32 - ref64))
        _check(f"per s{k} leaves", buf.weight[np.arange(n_env * S)].cpu().numpy(), g[f"dq_s{k}_leaves"],
               float(g[f"dq_s{k}_leaves_eref"]))
        _check(f"per s{k} max/min prio", buf.prio.cpu().numpy(), g[f"dq_s{k}_prio"], float(g[f"dq_s{k}_prio_eref"]))
    buf.weight.check()


def test_dqn_update_end_to_end_changes_the_sampled_leaves(g):
    gd = dict(np.load(DQN_GOLD))
    buf = _up_buffer(gd, PrioritizedVectorReplayBuffer, alpha=0.6, beta=0.4, seed=77)
    algo = _up_dqn(gd)
    algo.is_within_training_step = True
    before, ctr = buf.weight.tree.clone(), buf._sample_ctr
    assert torch.equal(before[buf.weight.bound:buf.weight.bound + buf.maxsize], torch.ones(buf.maxsize, dtype=torch.float64, device=DEV))
    sampled = ops.per_sample(buf.weight, 37, buf.seed, offset=ctr)          # what update() is about to draw
    stats = algo.update(buf, 37)
    assert np.isfinite(stats.loss) and buf._sample_ctr == ctr + 37
    leaves = lambda x: x[buf.weight.bound:buf.weight.bound + buf.maxsize]  # noqa: E731
    changed = torch.nonzero(leaves(buf.weight.tree) != leaves(before)).view(-1)
    assert torch.equal(changed, torch.unique(sampled))                      # exactly the sampled leaves
    assert float(buf.prio[0]) > 1.0 and float(buf.prio[1]) < 1.0
    tree = buf.weight.tree.cpu().numpy()
    inner = np.arange(1, buf.weight.bound)
    assert np.array_equal(tree[inner], tree[2 * inner] + tree[2 * inner + 1])
    # the next update draws by the new priorities, and Huber ignores the IS weights (quirk Q17) but still writes back
    algo.huber_loss_delta = 1.0
    mid = buf.weight.tree.clone()
    algo.update(buf, 37)
    assert not torch.equal(buf.weight.tree, mid)
    buf.weight.check()


def test_uniform_buffer_update_is_unchanged(g):
    """`DQN.update` on a uniform buffer against the code path as it was: sample_indices -> _preprocess_batch(Batch()) ->
    _update_with_batch, nothing else.  Same seed: bit-identical weights after three updates."""
    gd = dict(np.load(DQN_GOLD))
    flats = []
    for new in (True, False):
        buf = _up_buffer(gd, DeviceVectorReplayBuffer)
        algo = _up_dqn(gd)
        algo.is_within_training_step = True
        torch.manual_seed(123)
        for _ in range(3):
            if new:
                algo.update(buf, 37)
            else:
                algo._update_with_batch(algo._preprocess_batch(Batch(), buf, buf.sample_indices(37)))
        flats.append((algo.policy.model.flat.data.clone(), algo.target_flat.clone()))
    assert torch.equal(flats[0][0], flats[1][0]) and torch.equal(flats[0][1], flats[1][1])
    assert not hasattr(buf, "update_weight")


def test_multiagent_samples_by_priority_and_warns_once(g, caplog):
    rs = np.random.RandomState(8)
    N, E, T, D, A = 2, 4, 6, 5, 3
    buf = PrioritizedVectorReplayBuffer(E * 8, E, alpha=0.6, beta=0.4, n_agent=N, obs_dim=D, device=DEV)
    for t in range(T):
        buf.add(Batch(obs=rs.randn(E, N, D).astype(np.float32), act=rs.randint(0, A, (E, N)), rew=rs.randn(E, N).astype(np.float32),
                      terminated=rs.rand(E) < 0.2, truncated=rs.rand(E) < 0.1, obs_next=rs.randn(E, N, D).astype(np.float32)))
    buf.update_weight(np.arange(4), np.array([3.0, 0.1, 2.0, 0.5], np.float32))
    algos = [_dqn(None, [D, 16, A], seed=20 + i, n_step_return_horizon=2) for i in range(N)]
    ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=_Env(N))
    ma.is_within_training_step = True
    tree = buf.weight.tree.clone()
    with caplog.at_level(logging.WARNING):
        s1 = ma.update(buf, 9).get_loss_stats_dict()
        ma.update(buf, 9)
        ma.update(buf, 0)
    assert sum("Prioritized replay is disabled" in r.getMessage() for r in caplog.records) == 1
    assert torch.equal(buf.weight.tree, tree) and buf._sample_ctr == 18            # sampled by priority, nothing written back
    assert np.isfinite(s1["agent_0/loss"]) and np.isfinite(s1["agent_1/loss"])


# ---- 6. Collector -------------------------------------------------------------------------------------------------------
def test_collector_adds_rows_at_max_priority_and_does_not_fuse():
    from tianshou_marl_amd.algorithm.ppo import PPO, policy_within_training_step
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.utils.net import DiscreteActorCritic

    n_env, N, T, alpha = 8, 3, 4, 0.6
    env = DeviceSimpleSpreadVectorEnv(n_env, N, max_cycles=25, device=DEV, seed=0)
    algo = PPO(net=DiscreteActorCritic(env.obs_dim, env.n_act, 64, device=DEV, seed=0), seed=0)
    plain = Collector(algo, env, DeviceVectorReplayBuffer(n_env * 16, n_env, N, env.obs_dim, device=DEV))
    assert plain._can_fuse()
    buf = PrioritizedVectorReplayBuffer(n_env * 16, n_env, alpha=alpha, beta=0.4, device=DEV)
    col = Collector(algo, env, buf)
    col.reset()
    assert not col._can_fuse() and not col._can_fuse_actor() and buf.allocated
    buf.prio[0] = 2.5          # as if an update had raised max_prio: new rows start at max_prio ** alpha
    for _ in range(2):         # the second collect of a size may replay a captured graph: the init launch is part of it
        with policy_within_training_step(algo):
            col.collect(n_step=n_env * T)
    assert len(buf) == 2 * n_env * T
    tree = buf.weight.tree.cpu().numpy()
    bound = buf.weight.bound
    leaves = tree[bound:bound + buf.maxsize].reshape(n_env, 16)
    exp = float(np.float32(2.5) ** np.float32(alpha))
    _rel("collector leaves", leaves[:, :2 * T], np.full((n_env, 2 * T), exp))
    assert len(np.unique(leaves[:, :2 * T])) == 1 and not leaves[:, 2 * T:].any()
    inner = np.arange(1, bound)
    assert np.array_equal(tree[inner], tree[2 * inner] + tree[2 * inner + 1])
    assert tree[1] == pytest.approx(leaves.sum(), rel=1e-12)
    idx = buf.sample_indices(64)
    assert idx.dtype == np.int64 and (leaves.reshape(-1)[idx] > 0).all()
    buf.weight.check()
