"""GPU tests (`-m gpu`) of BDQN: `BranchingNet` and BDQN's three-call sequences on a device buffer against
tests/golden/bdqn.npz (the reference's float64 run, with e_ref = max |ref32 - ref64| of its own two runs), one branch alone,
determinism, checkpoints, the `act_branches` buffers, the multi-agent dispatch and the collector.

Bar, everywhere a float is compared: test_gpu_distq.py's `_bar`, max |hip - ref64| <= 1e-5 max |ref64| + e_ref.  Every comparison
prints `PARITY name: ...`."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import bdqn_restatement as R  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_host_bdqn import GOLD, N_CASES, call_rows, cases, chains_of  # noqa: E402
from test_host_dqn import _Env  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import BDQN, BDQNPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.algorithm.ppo import policy_within_training_step
    from tianshou_marl_amd.data import Batch
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer, PrioritizedVectorReplayBuffer, VectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.env.spaces import Discrete
    from tianshou_marl_amd.utils.net import BranchingNet, FlatAdam


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _d(x, dt=None):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dt or torch.float32)


def _n(t):
    return t.detach().cpu().numpy().astype(np.float64)


def make_net(g, c, init=True):
    D, c1, c2, vh, ah = (int(x) for x in g["dims"][:5])
    net = BranchingNet(state_shape=(D,), num_branches=c["K"], action_per_branch=c["A"], common_hidden_sizes=[c1, c2],
                       value_hidden_sizes=[vh], action_hidden_sizes=[ah], device=DEV, seed=1)
    if init:
        net.flat.data.copy_(_d(g[f"c{c['i']}_init"]))
    return net


def make_algo(g, c, freq=None):
    algo = BDQN(policy=BDQNPolicy(model=make_net(g, c), action_space=Discrete(c["A"])), optim=AdamOptimizerFactory(lr=float(g["lr"])),
                gamma=float(g["gamma"]), target_update_freq=c["freq"] if freq is None else freq, is_double=c["is_double"])
    algo.is_within_training_step = True
    return algo


def make_buffer(g, c, lanes=(0,)):
    """The fixture's rows on a device buffer with one lane per entry of `lanes`: lane id 0 holds the fixture's own rows, lane id
    j its observations and rewards times 1 + j and its actions shifted by j."""
    D, n_env, S = int(g["dims"][0]), int(g["dims"][6]), int(g["dims"][7])
    pk = f"c{c['i']}_"
    kw = dict(n_agent=len(lanes), obs_dim=D, device=DEV, act_branches=c["K"])
    if c["prio"]:
        buf = PrioritizedVectorReplayBuffer(n_env * S, n_env, alpha=float(g["per"][0]), beta=float(g["per"][1]), **kw)
    else:
        buf = VectorReplayBuffer(n_env * S, n_env, **kw)
    rows = {n: g[f"{pk}rows_{n}"] for n in ("obs", "act", "obs_next", "rew", "term", "trunc")}
    ids = np.asarray(lanes)
    rep = lambda x: np.repeat(x[:, None], len(lanes), 1)  # noqa: E731
    for t in range(rows["obs"].shape[0]):
        buf.add(Batch(obs=rep(rows["obs"][t]) * (1 + ids)[None, :, None], act=(rep(rows["act"][t]) + ids[None, :, None]) % c["A"],
                      rew=rep(rows["rew"][t]) * (1 + ids), terminated=rows["term"][t], truncated=rows["trunc"][t],
                      obs_next=rep(rows["obs_next"][t]) * (1 + ids)[None, :, None]), buffer_ids=np.arange(n_env))
    return buf


def one_call(algo, buf, idx, agent=None):
    batch = algo._sampled_batch(buf, idx)
    w_in = batch.weight.clone() if "weight" in batch else None
    batch = algo._preprocess_batch(batch, buf, idx, agent=agent)
    stats = algo._update_with_batch(batch)
    algo._postprocess_batch(batch, buf, idx)
    return batch, stats, w_in


def run_calls(g, ci, check=True):
    c = cases(g)[ci]
    pk = f"c{ci}_"
    buf, algo = make_buffer(g, c), make_algo(g, c)
    for k in range(int(g["n_calls"])):
        sk = f"{pk}s{k}_"
        idx = _d(g[sk + "indices"], torch.int64)
        batch, stats, w_in = one_call(algo, buf, idx)
        if not check:
            continue
        if c["prio"]:
            _bar(f"{sk}IS weights", _n(w_in), g[sk + "weight_in"], float(g[sk + "weight_in_eref"]))
        _bar(f"{sk}returns", _n(batch.returns), g[sk + "returns"], float(g[sk + "returns_eref"]))
        _bar(f"{sk}prio", _n(batch.weight), g[sk + "prio"], float(g[sk + "prio_eref"]))
        _bar(f"{sk}loss", stats.loss, g[sk + "loss"][0], abs(g[sk + "loss"][1] - g[sk + "loss"][0]))
        _bar(f"{sk}grad", _n(algo._ws[idx.numel()]["slabs"]).sum(0), g[sk + "grad"], float(g[sk + "grad_eref"]))
    if check:
        last = f"{pk}s{int(g['n_calls']) - 1}_"
        _bar(f"{pk}online weights", _n(algo.policy.model.flat.data), g[last + "w"], float(g[last + "w_eref"]))
        if c["freq"]:
            _bar(f"{pk}lagged weights", _n(algo.target_flat), g[last + "w_old"], float(g[last + "w_old_eref"]))
        if c["prio"]:
            n_rows = int(g["dims"][6]) * int(g["dims"][7])
            _bar(f"{pk}leaves", _n(buf.weight[np.arange(n_rows)]), g[pk + "leaves"], float(g[pk + "leaves_eref"]))
            touched = np.unique(np.concatenate([g[f"{pk}s{k}_indices"] for k in range(int(g["n_calls"]))]))
            assert not np.allclose(g[pk + "leaves"][touched], 1.0)
    return algo, buf


@pytest.mark.parametrize("ci", range(N_CASES))
def test_net_output_and_gradient_slabs_follow_the_reference(g, ci):
    """The first call's online forward and its gradient, from the restated head's d_adv / d_v, at n_split 1 and 2."""
    c = cases(g)[ci]
    net = make_net(g, c)
    rows, _ = call_rows(g, c, 0)
    q, state = net(_d(rows[0]), save=True)
    assert tuple(q.shape) == (len(rows[0]), c["K"], c["A"]) and state is None
    _bar(f"c{ci} logits", _n(q), g[f"c{ci}_s0_q"], float(g[f"c{ci}_s0_q_eref"]))
    Rs = R.BdqnRestatement(g[f"c{ci}_init"], chains_of(g, c["A"]), c["K"], float(g["gamma"]), lr=float(g["lr"]),
                           target_update_freq=c["freq"], is_double=c["is_double"])
    r = Rs.update(*rows, weight=g.get(f"c{ci}_s0_weight_in"))
    for n_split in (1, 2):
        slabs = net.backward((_d(r["d_adv"]), _d(r["d_v"])), n_split)
        assert tuple(slabs.shape) == (n_split, net.flat.numel())
        _bar(f"c{ci} gradient n_split {n_split}", _n(slabs).sum(0), g[f"c{ci}_s0_grad"], float(g[f"c{ci}_s0_grad_eref"]))


@pytest.mark.parametrize("ci", range(N_CASES))
def test_three_update_calls_follow_the_reference(g, ci):
    run_calls(g, ci)


def test_running_twice_gives_the_same_parameter_bits(g):
    (a, _), (b, _) = run_calls(g, 1, check=False), run_calls(g, 1, check=False)
    assert torch.equal(a.policy.model.flat.data.view(torch.int32), b.policy.model.flat.data.view(torch.int32))
    assert torch.equal(a.target_flat.view(torch.int32), b.target_flat.view(torch.int32))
    assert torch.equal(a.optim.exp_avg_sq.view(torch.int32), b.optim.exp_avg_sq.view(torch.int32))


def test_one_branch_alone(g):
    """Perturbing branch k's parameters changes q[:, k, :] and nothing else; a loss that touches only branch k leaves the
    other branches' gradient slabs at +0.0."""
    c = cases(g)[0]
    net = make_net(g, c)
    x = _d(call_rows(g, c, 0)[0][0])
    q0 = net(x, save=False)[0].clone()
    k, K, A, B = 1, c["K"], c["A"], x.shape[0]
    for i in range(len(net._b_offsets)):
        net.branch_weight(i)[k].mul_(1.5)
        net.branch_bias(i)[k].add_(0.25)
    q1, _ = net(x, save=True)
    others = [j for j in range(K) if j != k]
    assert torch.equal(q1[:, others], q0[:, others]) and not torch.equal(q1[:, k], q0[:, k])
    rs = np.random.RandomState(0)
    d_adv = np.zeros((K, B, A), np.float32)
    d_adv[k] = rs.standard_normal((B, A))
    slabs = net.backward((_d(d_adv), torch.zeros(B, device=DEV)), 2)
    bits = slabs.view(torch.int32)
    for i in range(len(net._b_offsets)):
        for view in (net.branch_weight, net.branch_bias):
            for s in range(2):
                gsl = view(i, bits[s])
                assert not gsl[others].any(), "another branch's slab is not +0.0"      # all bits zero: +0.0
            assert view(i, slabs.sum(0))[k].any()   # (a slab of its own may get no rows of so small a batch)
    assert slabs[:, :net.b_off].any()   # the trunk's gradient flows through the one branch


def test_update_checkpoints_round_trip(g):
    """`update` end to end on a prioritized buffer, then the native and the reference checkpoint into fresh learners: the
    weights come back bit for bit, and the FlatAdam state through the reference's per-parameter order."""
    c = cases(g)[1]
    buf, algo = make_buffer(g, c), make_algo(g, c)
    before = algo.policy.model.flat.data.clone()
    leaves = _n(buf.weight[np.arange(64)]).copy()
    s1, s2 = algo.update(buf, 12), algo.update(buf, 12)
    assert np.isfinite([s1.loss, s2.loss]).all() and algo._iter == 2
    assert not torch.equal(before, algo.policy.model.flat.data) and not np.array_equal(leaves, _n(buf.weight[np.arange(64)]))
    other = make_algo(g, c)
    other.load_state_dict(algo.state_dict())
    sd = algo.to_reference_state_dict()
    assert list(sd) == [str(k) for k in g["sd_keys"]]
    third = make_algo(g, c)
    third.policy.model.flat.data.zero_()
    third.load_reference_state_dict(sd)
    for o in (other, third):
        assert torch.equal(o.policy.model.flat.data, algo.policy.model.flat.data) and torch.equal(o.target_flat, algo.target_flat)
    assert torch.equal(other.optim.exp_avg, algo.optim.exp_avg) and other.optim.step_count == 2
    fresh = make_net(g, c, init=False)
    fresh.load_reference_state_dict(algo.policy.model.to_reference_state_dict())
    assert torch.equal(fresh.flat.data, algo.policy.model.flat.data)
    opt = FlatAdam(fresh, lr=float(g["lr"]), coef64=True)
    osd = algo.optim.state_dict()
    assert [tuple(e["exp_avg"].shape) for e in osd["state"].values()] == fresh.param_shapes()
    opt.load_state_dict(osd)
    assert torch.equal(opt.exp_avg, algo.optim.exp_avg) and torch.equal(opt.exp_avg_sq, algo.optim.exp_avg_sq)
    assert opt.step_count == 2 and not opt.exp_avg[fresh.b_off:].eq(0).all()


@pytest.mark.parametrize("cls", ["plain", "prio"])
def test_act_branches_buffer_returns_the_integers_that_went_in(cls):
    n_env, S, N, D, K = 3, 4, 2, 5, 3
    kw = dict(n_agent=N, obs_dim=D, device=DEV, act_branches=K)
    buf = (PrioritizedVectorReplayBuffer(n_env * S, n_env, alpha=0.6, beta=0.4, **kw) if cls == "prio" else
           DeviceVectorReplayBuffer(n_env * S, n_env, N, D, device=DEV, act_branches=K))
    assert buf.unfused_adds_only and buf.act_store.dtype == torch.int32 and tuple(buf.act_store.shape) == (S, n_env, N, K)
    rs = np.random.RandomState(4)
    want = np.zeros((n_env, S, N, K), np.int64)
    for t in range(S + 2):                       # every sub-buffer wraps
        act = rs.randint(0, 1000, (n_env, N, K))
        z = np.zeros((n_env, N), np.float32)
        if t % 2:
            buf.add(Batch(obs=np.zeros((n_env, N, D), np.float32), act=act, rew=z, terminated=np.zeros(n_env, bool),
                          truncated=np.zeros(n_env, bool), obs_next=np.zeros((n_env, N, D), np.float32)), buffer_ids=np.arange(n_env))
        else:
            u8 = torch.zeros(n_env, N, dtype=torch.uint8, device=DEV)
            buf.add_device(torch.zeros(n_env, N, D, device=DEV), _d(act, torch.int32), _d(z), u8, u8, torch.zeros(n_env, N, D, device=DEV))
        want[:, t % S] = act
    idx = np.arange(n_env * S)
    got = buf[idx].act
    assert got.dtype == np.int64 and np.array_equal(got, want.reshape(n_env * S, N, K))
    batch, indices = buf.sample(7)
    assert np.array_equal(batch.act, want.reshape(n_env * S, N, K)[indices])
    assert np.array_equal(buf.act, want.reshape(n_env * S, N, K))


def test_multi_agent_dispatch_equals_the_single_agent_updates(g):
    """Two agents on a joint-lane `act_branches` buffer: each agent's update equals, bit for bit, a single-agent BDQN update fed
    that agent's column."""
    c = cases(g)[0]
    buf = make_buffer(g, c, lanes=(0, 1))
    algos = [make_algo(g, c), make_algo(g, c, freq=0)]
    ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=_Env(2))
    ma.is_within_training_step = True
    idx = g["c0_s0_indices"]
    stats = ma._update_with_batch(ma._preprocess_batch(None, buf, idx))
    for k, agent in enumerate(_Env(2).agents):
        solo = make_algo(g, c, freq=None if k == 0 else 0)
        batch, st, _ = one_call(solo, make_buffer(g, c, lanes=(k,)), _d(idx, torch.int64))
        assert st.loss == stats._agent_id_to_stats[agent].loss, agent
        assert torch.equal(solo.policy.model.flat.data.view(torch.int32), algos[k].policy.model.flat.data.view(torch.int32)), agent
    assert stats._agent_id_to_stats["agent_0"].loss != stats._agent_id_to_stats["agent_1"].loss


def test_collector_fills_an_act_branches_buffer_through_the_unfused_path():
    E, T, A = 8, 6, 5
    env = DeviceSimpleSpreadVectorEnv(E, 3, max_cycles=25, device=DEV, seed=3)
    assert env.n_act == A
    net = BranchingNet(state_shape=(env.obs_dim,), num_branches=1, action_per_branch=A, common_hidden_sizes=[32], value_hidden_sizes=[16],
                       action_hidden_sizes=[16], device=DEV, seed=2)
    pol = BDQNPolicy(model=net, action_space=Discrete(A), eps_training=0.5, seed=9)
    buf = VectorReplayBuffer(E * 16, E, act_branches=1)
    col = Collector(pol, env, buf, use_graph=False)
    col.reset()
    assert not col._can_fuse() and tuple(buf.act_store.shape) == (16, E, 3, 1)
    seen, inner = [], pol.act_device

    def spy(*a, **kw):
        out = inner(*a, **kw)
        seen.append(out["act"].clone())
        return out

    pol.act_device = spy
    with policy_within_training_step(pol):
        col.collect(n_step=E * T)
    assert len(seen) == T and pol._sample_ctr == 0    # the env's device tick supplied the counters
    got = torch.stack(seen).reshape(T, E, 3, 1)
    assert torch.equal(buf.act_store[:T], got) and int(got.min()) >= 0 and int(got.max()) < A
    assert len(torch.unique(got)) > 1
