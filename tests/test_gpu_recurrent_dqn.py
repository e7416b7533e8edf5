"""GPU tests (`-m gpu`) of the recurrent net as a whole (utils/net.Recurrent over csrc/lstm.hip and csrc/dense.hip):
fixtures A and B of tests/golden/recurrent.npz through forward / backward, the acting step against one two-step forward, the
state reset, checkpoints and twins; then the learner and the Collector on it: `act_device` / `reset_state_device`, one DQN step
against the float64 restatement, an eager against a captured-graph collect, and a `FlatMLP` step against the parent commit's.

Bar: max |hip - ref64| <= 1e-5 max |ref64| per block, ref64 = tests/recurrent_restatement.py (held to the reference's recorded
float32 values at 1e-6 on the CPU: tests/test_recurrent_restatement.py)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import recurrent_restatement as rr  # noqa: E402
from test_gpu_dense_shapes import _bars  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.utils.net import FlatAdam, Recurrent, lagged_copy

Z = np.load(os.path.join(HERE, "golden", "recurrent.npz"))
KEYS = [str(k) for k in Z["a_keys"]]


def _d(x):
    return torch.as_tensor(np.array(x, np.float32)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _fixture_net():
    net = Recurrent(layer_num=2, state_shape=6, action_shape=5, hidden_layer_size=32, device=DEV, seed=0)
    net.load_reference_state_dict({k: Z[f"a_p_{k}"] for k in KEYS})
    return net


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_forward_backward(tag):
    net = _fixture_net()
    state = None if tag == "a" else (Z["b_h0"], Z["b_c0"])
    out, (hid, cell) = net(_d(Z["a_obs"]), None if state is None else dict(hidden=_d(state[0]), cell=_d(state[1])))
    grads = dict(net.reference_named_views(net.backward(_d(Z["a_r"]), n_split=2).sum(0)))
    params = {k: Z[f"a_p_{k}"] for k in KEYS}
    rout, (rh, rc), saved = rr.recurrent_forward(params, Z["a_obs"], 2, state)
    rg = rr.recurrent_backward(params, saved, Z["a_r"], 2)
    pairs = [(_n(out), rout), (_n(hid), rh), (_n(cell), rc)] + [(_n(grads[k]), rg[k]) for k in KEYS]
    _bars(f"Recurrent fixture {tag}", pairs)
    # and next to the reference's own float32 run: both sit within float32 rounding of the float64 values
    assert np.abs(_n(out) - Z[f"{tag}_out"]).max() <= 2e-6 * np.abs(rout).max()


def test_two_acting_steps_equal_one_two_step_forward_and_reset_restarts_a_row():
    net = Recurrent(layer_num=2, state_shape=6, action_shape=4, hidden_layer_size=64, device=DEV, seed=3)
    E, N = 3, 2   # rows = envs x agents
    rs = np.random.RandomState(4)
    obs = rs.standard_normal((E * N, 2, 6)).astype(np.float32)
    hid, cell = net.zero_state(E * N)
    q0, _ = net(_d(obs[:, 0]), (hid, cell), save=False, state_out=(hid, cell))   # in place: the state advances where it lies
    q1, (h2, c2) = net(_d(obs[:, 1]), (hid, cell), save=False, state_out=(hid, cell))
    assert h2.data_ptr() == hid.data_ptr() and c2.data_ptr() == cell.data_ptr()
    params = {k: _n(v) for k, v in net.reference_named_views()}
    rq1, (rh, rc), _ = rr.recurrent_forward(params, obs, 2)
    rq0 = rr.recurrent_forward(params, obs[:, :1], 2)[0]
    full, (fh, fc) = net(_d(obs), save=False)
    _bars("acting steps", [(_n(q0), rq0), (_n(q1), rq1), (_n(hid), rh), (_n(cell), rc), (_n(full), rq1), (_n(fh), rh), (_n(fc), rc)])
    # env 1 finishes: its two rows restart from zero, the others carry on
    done = torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV)
    before = hid.clone()
    ops.lstm_state_reset(hid, cell, done, rows_per_env=N)
    assert not hid[2:4].any() and not cell[2:4].any() and torch.equal(hid[:2], before[:2]) and torch.equal(hid[4:], before[4:])
    nxt = rs.standard_normal((E * N, 6)).astype(np.float32)
    q2, _ = net(_d(nxt), (hid, cell), save=False, state_out=(hid, cell))
    fresh = rr.recurrent_forward(params, nxt[:, None], 2)[0]
    carried = rr.recurrent_forward(params, nxt[:, None], 2, (rh, rc))[0]
    want = carried.copy()
    want[2:4] = fresh[2:4]
    assert np.abs(fresh - carried).max() > 1e-3
    _bars("after reset", [(_n(q2), want)])


def test_checkpoint_round_trip_twin_and_optimizer():
    net = _fixture_net()
    sd = net.to_reference_state_dict()
    assert list(sd) == KEYS and all(np.array_equal(sd[k].numpy(), Z[f"a_p_{k}"]) for k in KEYS)
    other = Recurrent(layer_num=2, state_shape=6, action_shape=5, hidden_layer_size=32, device=DEV, seed=9)
    other.load_reference_state_dict(sd)
    assert torch.equal(other.flat.data, net.flat.data)
    twin = lagged_copy(net)
    assert twin.flat.data_ptr() != net.flat.data_ptr() and torch.equal(twin.flat.data, net.flat.data)
    x = _d(Z["a_obs"])
    assert torch.equal(twin(x, save=False)[0], net(x, save=False)[0])
    over = net.clone_over(torch.zeros_like(net.flat.data))
    assert isinstance(over, Recurrent) and (over.layer_num, over.hidden, over.obs_dim, over.n_out) == (2, 32, 6, 5)
    # one Adam step on the slabs moves every parameter block, and only the online net
    opt = FlatAdam(net, lr=1e-2)
    net(x)
    opt.step(net.backward(_d(Z["a_r"]), n_split=2))
    assert all((a != b).any() for (_, a), (_, b) in zip(net.reference_named_views(), twin.reference_named_views()))
    assert [tuple(s) for s in net.param_shapes()] == [Z[f"a_p_{k}"].shape for k in KEYS]


# ---- the learner and the Collector on the recurrent net -------------------------------------------------------------------
class _Discrete:
    def __init__(self, n):
        self.n = n


def _imports():
    from tianshou_marl_amd.algorithm.dqn import DQN, DiscreteQLearningPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data.batch import Batch
    from tianshou_marl_amd.data.buffer import VectorReplayBuffer
    from tianshou_marl_amd.utils.net import FlatMLP

    return DQN, DiscreteQLearningPolicy, AdamOptimizerFactory, Batch, VectorReplayBuffer, FlatMLP


def _filled(buf, Batch, E, N, D, A, T, seed):
    rs = np.random.RandomState(seed)
    rows = []
    for t in range(T):
        row = dict(obs=rs.standard_normal((E, N, D)).astype(np.float32), act=rs.randint(0, A, (E, N)),
                   rew=rs.standard_normal((E, N)).astype(np.float32), terminated=rs.rand(E) < 0.2, truncated=np.zeros(E, bool),
                   obs_next=rs.standard_normal((E, N, D)).astype(np.float32))
        buf.add(Batch(**row))
        rows.append(row)
    return rows


def test_policy_act_device_carries_state_and_reset_state_device_restarts_env_rows():
    """(c) through the policy: two `act_device` calls on consecutive observations equal one L = 2 forward from zeros; after
    `reset_state_device` with done set for env 1 only, env 1's rows restart from zero and the others do not."""
    DQN, Policy, _, Batch, _, _ = _imports()
    E, N, D, A = 3, 2, 6, 4
    net = Recurrent(layer_num=2, state_shape=D, action_shape=A, hidden_layer_size=64, device=DEV, seed=3)
    pol = Policy(model=net, action_space=_Discrete(A))
    assert pol.recurrent and hasattr(pol, "reset_state_device")
    rs = np.random.RandomState(4)
    obs = rs.standard_normal((E, N, 3, D)).astype(np.float32)
    q0 = pol.act_device(_d(obs[:, :, 0]))["q"].clone()
    res = pol.act_device(_d(obs[:, :, 1]))
    q1 = res["q"].clone()
    params = {k: _n(v) for k, v in net.reference_named_views()}
    flat = obs.reshape(E * N, 3, D)
    r0 = rr.recurrent_forward(params, flat[:, :1], 2)[0]
    r1, (rh, rc), _ = rr.recurrent_forward(params, flat[:, :2], 2)
    hid, cell = pol._act_state
    _bars("act_device x 2", [(_n(q0), r0), (_n(q1), r1), (_n(hid), rh), (_n(cell), rc)])
    assert np.array_equal(res["act"].cpu().numpy(), _n(q1).argmax(1))
    pol.reset_state_device(torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV))
    q2 = pol.act_device(_d(obs[:, :, 2]))["q"]
    fresh = rr.recurrent_forward(params, flat[:, 2:3], 2)[0]
    want = rr.recurrent_forward(params, flat[:, 2:3], 2, (rh, rc))[0]
    want[2:4] = fresh[2:4]
    _bars("act_device after reset", [(_n(q2), want)])
    # the host call returns the state as Batch(hidden, cell) [bsz, layers, H] and takes it back
    out = pol(Batch(obs=flat[:, 0], info=Batch()))
    assert tuple(out.state.hidden.shape) == tuple(out.state.cell.shape) == (E * N, 2, 64)
    out2 = pol(Batch(obs=flat[:, 1], info=Batch()), out.state)
    _bars("forward(batch, state)", [(_n(out.logits), r0), (_n(out2.logits), r1)])


def _step_pairs(algo, net, batch, stats, r, n_rows):
    got = dict(net.reference_named_views(algo._ws[n_rows]["slabs"].sum(0)))
    pairs = [(np.array([stats.loss]), np.array([r["loss"]])), (_n(batch.returns), r["returns"])]
    pairs += [(_n(got[k]), r["grads"][k]) for k in r["grads"]]
    return pairs + [(_n(v), r["online"][k]) for k, v in net.reference_named_views()]


def test_fixture_d_dqn_step():
    """(b): fixture d -- the reference's recorded trace, parameters (online, and a lagged net moved off them) and indices --
    through `_preprocess_batch` / `_update_with_batch`: the walk's successors exactly; loss, returns, every parameter's gradient
    and every parameter block AFTER the step within the bar of the float64 restatement of that step, which
    tests/test_recurrent_restatement.py holds to the reference's recorded loss and parameters at 1e-6 on the CPU."""
    DQN, Policy, Adam, Batch, VRB, _ = _imports()
    n_env, S, T, D, A, H, L, n_step, B = (int(x) for x in Z["d_dims"])
    keys = rr.recurrent_keys(1)
    buf = VRB(n_env * S, n_env, device=DEV, stack_num=L)
    for t in range(T):
        buf.add(Batch(obs=Z["d_rows_obs"][t][:, None], act=Z["d_rows_act"][t][:, None], rew=Z["d_rows_rew"][t][:, None],
                      terminated=Z["d_rows_term"][t], truncated=Z["d_rows_trunc"][t], obs_next=Z["d_rows_obs_next"][t][:, None]),
                buffer_ids=np.arange(n_env))
    net = Recurrent(layer_num=1, state_shape=D, action_shape=A, hidden_layer_size=H, device=DEV, seed=0)
    net.load_reference_state_dict({k: Z[f"d_p_{k}"] for k in keys})
    algo = DQN(policy=Policy(model=net, action_space=_Discrete(A)), optim=Adam(lr=float(Z["d_lr"]), eps=float(Z["d_eps"])),
               gamma=float(Z["d_gamma"]), n_step_return_horizon=n_step, target_update_freq=1, is_double=True)
    algo.model_old.load_reference_state_dict({k: Z[f"d_lag_{k}"] for k in keys})
    r = rr.fixture_d_step(Z)
    batch = algo._preprocess_batch(Batch(), buf, Z["d_idx"])
    assert np.array_equal(batch.idx_n.cpu().numpy(), r["idx_n"]) and np.array_equal(batch.obs.cpu().numpy(), r["obs"])
    stats = algo._update_with_batch(batch)
    _bars("fixture d DQN step", _step_pairs(algo, net, batch, stats, r, B))
    assert torch.equal(algo.target_flat, _d(np.concatenate([Z[f"d_p_{k}"].reshape(-1) for k in keys])))   # the copy of call 0
    # next to the reference's own float32 numbers
    assert abs(stats.loss - float(Z["d_loss"])) <= 2e-6 * abs(r["loss"])


def test_recurrent_dqn_step_on_an_agent_lane():
    """The same step on a joint-row buffer of two agents, agent = 1, stack_num = 3, the lagged net moved off the online one (so
    a mix-up of the three forwards shows): loss, returns, gradients and the parameters after the step against
    `recurrent_dqn_step` at the bar."""
    DQN, Policy, Adam, Batch, VRB, _ = _imports()
    E, N, D, A, T, L, gamma, lr = 4, 2, 6, 5, 7, 3, 0.97, 1e-3
    buf = VRB(E * 8, E, device=DEV, stack_num=L)
    _filled(buf, Batch, E, N, D, A, T, 21)
    net = Recurrent(layer_num=1, state_shape=D, action_shape=A, hidden_layer_size=32, device=DEV, seed=13)
    algo = DQN(policy=Policy(model=net, action_space=_Discrete(A)), optim=Adam(lr=lr), gamma=gamma, n_step_return_horizon=2,
               target_update_freq=1)
    algo.target_flat.add_(0.05 * torch.randn(algo.target_flat.shape, generator=torch.Generator().manual_seed(1)).to(DEV))
    online = {k: _n(v) for k, v in net.reference_named_views()}
    lagged = {k: _n(v) for k, v in algo.model_old.reference_named_views()}
    idx = buf.sample_indices(0)
    batch = algo._preprocess_batch(Batch(), buf, idx, agent=1)
    assert tuple(batch.obs.shape) == (len(idx), L, D)
    obs, act = batch.obs.cpu().numpy(), batch.act.cpu().numpy()
    nxt = buf.get(batch.idx_n.cpu().numpy(), "obs_next")[:, :, 1]
    stats = algo._update_with_batch(batch)
    r = rr.recurrent_dqn_step(online, lagged, obs, act, nxt, _n(batch.mc), _n(batch.gpow), batch.vmask.cpu().numpy().astype(bool), 1, lr)
    assert r["top2_gap"] > 1e-4
    _bars("recurrent DQN step, agent lane", _step_pairs(algo, net, batch, stats, r, len(idx)))
    swapped = rr.recurrent_dqn_step(lagged, online, obs, act, nxt, _n(batch.mc), _n(batch.gpow), batch.vmask.cpu().numpy().astype(bool), 1, lr)
    assert np.abs(swapped["returns"] - r["returns"]).max() > 1e-3   # the nets are told apart
    # a learner around a plain net refuses the stacking buffer instead of training on single frames
    _, _, _, _, _, FlatMLP = _imports()
    plain = DQN(policy=Policy(model=FlatMLP([D, 16, A], device=DEV, seed=1), action_space=_Discrete(A)), optim=Adam(lr=lr))
    with pytest.raises(ValueError, match="stack"):
        plain._preprocess_batch(Batch(), buf, idx, agent=1)


def test_collector_eager_and_captured_graph_fill_the_buffer_alike():
    """(d): 4 envs of simple_spread with N = 2, a recurrent DQN policy, 6 steps per collect: the first collect runs eagerly, the
    second captures the graph, the third replays it; a second collector runs all three eagerly.  Buffers and kept state are equal bit for bit."""
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv

    _, Policy, _, _, VRB, _ = _imports()
    got = []
    for use_graph in (False, True):
        env = DeviceSimpleSpreadVectorEnv(4, n_agent=2, max_cycles=7, device=DEV, seed=5)
        net = Recurrent(layer_num=1, state_shape=env.obs_dim, action_shape=5, hidden_layer_size=32, device=DEV, seed=2)
        pol = Policy(model=net, action_space=_Discrete(5), eps_inference=0.3, seed=9)
        buf = VRB(4 * 32, 4, n_agent=2, obs_dim=env.obs_dim, device=DEV, stack_num=2)
        col = Collector(pol, env, buf)
        col.use_graph = use_graph
        col.reset()
        assert col._can_fuse() is False and col._can_fuse_actor() is False
        for _ in range(3):
            col.collect(n_step=6 * 4)
        torch.cuda.synchronize()
        assert not use_graph or any(isinstance(k, tuple) and k[0] == "graph" for k in col._ws)
        got.append([buf.obs_store.clone(), buf.obs_next_store.clone(), buf.act_store.clone(), buf.rew_store.clone(),
                    buf.done_store.clone(), buf.index.state.clone(), *pol._act_state])
        assert pol._act_state[0].abs().sum() > 0 and len(buf) == 72 and buf.done_store.sum() >= 4   # episodes ended on the way
    for a, b in zip(*got):
        assert torch.equal(a, b)


# (rows, loss, sha256 of the parameters, their float64 sum) of the test's script run on the parent commit (7e26c3f) on an MI355X
PARENT_STEP = (28, "0x1.60834e0000000p+0", "da9c7516376a592befdade41235ba8127dbf9fad8c1a4402853ccdf3e6216906",
               "0x1.c7521706b0000p+2")


def test_flat_mlp_dqn_step_is_the_parent_commit_s_bit_for_bit():
    """(f): one seeded DQN step on a `FlatMLP` with a stack_num = 1 buffer gives the loss and the parameters that the parent
    commit gave for the same script on the same GPU type (recorded from a run of the parent, not of this branch)."""
    import hashlib

    DQN, Policy, Adam, Batch, VRB, FlatMLP = _imports()
    E, N, D, A, T = 4, 2, 6, 5, 7
    buf = VRB(E * 8, E, device=DEV)
    _filled(buf, Batch, E, N, D, A, T, 21)
    assert buf.stack_num == 1
    net = FlatMLP([D, 32, 32, A], "relu", device=DEV, seed=13)
    algo = DQN(policy=Policy(model=net, action_space=_Discrete(A)), optim=Adam(lr=1e-3), gamma=0.97, n_step_return_horizon=2,
               target_update_freq=1)
    idx = buf.sample_indices(0)
    stats = algo._update_with_batch(algo._preprocess_batch(Batch(), buf, idx, agent=1))
    w = net.flat.data.cpu().numpy()
    rows, loss, sha, total = PARENT_STEP
    assert len(idx) == rows and float(stats.loss).hex() == loss and float(w.astype(np.float64).sum()).hex() == total
    assert hashlib.sha256(w.tobytes()).hexdigest() == sha
