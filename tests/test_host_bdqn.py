"""CPU tests of BDQN: the float64 restatement (tests/bdqn_restatement.py) against the reference's own float64 run in
tests/golden/bdqn.npz at 1e-10, constructor signatures and checkpoint keys against the reference's, the flat layout of
`BranchingNet` and the optimizer state's reference order, the host-side refusals of the new wrappers, entry points and buffer
arguments, and the word plan of the restated epsilon-greedy draw.  Nothing is launched."""
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "bdqn.npz")

import bdqn_restatement as R  # noqa: E402
import sampling_restatement as sr  # noqa: E402
from test_host_sampling import BIT63, _disjoint, _policy_counter  # noqa: E402

from tianshou_marl_amd import _abi, _build, ops  # noqa: E402

N_CASES = 4


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def cases(g):
    out = []
    for i, c in enumerate(g["cases"]):
        K, A, dbl, freq, prio = (int(x) for x in str(c).split("|"))
        out.append(dict(i=i, K=K, A=A, is_double=bool(dbl), freq=freq, prio=bool(prio)))
    return out


def chains_of(g, A):
    D, c1, c2, vh, ah = (int(x) for x in g["dims"][:5])
    return R.chains(D, [c1, c2], [vh], [ah], A)


def call_rows(g, c, k):
    """(obs, act, obs_next, rew, end) of call k: the rows at the recorded indices, with the end flag `done | newest row`."""
    pk, S = f"c{c['i']}_", int(g["dims"][7])
    idx = g[f"{pk}s{k}_indices"]
    slot, env = idx % S, idx // S
    rows = {n: g[f"{pk}rows_{n}"] for n in ("obs", "act", "obs_next", "rew", "term", "trunc")}
    T = rows["obs"].shape[0]
    done = rows["term"] | rows["trunc"]
    newest = (slot == T - 1) & ~done[T - 1, env]        # every sub-buffer got T < S rows: its newest row is slot T - 1
    end = done[slot, env] | newest
    kinds = dict(term=rows["term"][slot, env], trunc_only=rows["trunc"][slot, env] & ~rows["term"][slot, env], newest=newest)
    return (rows["obs"][slot, env], rows["act"][slot, env], rows["obs_next"][slot, env], rows["rew"][slot, env], end), kinds


@pytest.mark.parametrize("ci", range(N_CASES))
def test_restatement_follows_the_reference_float64_run(g, ci):
    c = cases(g)[ci]
    assert len(cases(g)) == N_CASES
    assert [(x["K"], x["A"], int(x["is_double"]), x["freq"], int(x["prio"])) for x in cases(g)] == \
        [(3, 5, 1, 2, 0), (3, 5, 0, 2, 1), (1, 4, 1, 0, 0), (4, 1, 1, 2, 0)]
    pk = f"c{ci}_"
    Rs = R.BdqnRestatement(g[pk + "init"], chains_of(g, c["A"]), c["K"], float(g["gamma"]), lr=float(g["lr"]),
                           target_update_freq=c["freq"], is_double=c["is_double"])
    for k in range(int(g["n_calls"])):
        sk = f"{pk}s{k}_"
        rows, kinds = call_rows(g, c, k)
        assert all(v.any() for v in kinds.values()) and not rows[4].all()   # the end-flag rule is exercised
        r = Rs.update(*rows, weight=g.get(sk + "weight_in"))
        assert abs(r["loss"] - g[sk + "loss"][0]) <= 1e-10 * abs(g[sk + "loss"][0])
        assert np.allclose(r["q"], g[sk + "q"], rtol=1e-10, atol=1e-13)
        assert np.allclose(r["returns"], g[sk + "returns"], rtol=1e-10, atol=1e-13)
        assert np.allclose(r["prio"], g[sk + "prio"], rtol=1e-10, atol=1e-13)
        assert np.allclose(r["grads"], g[sk + "grad"], rtol=1e-10, atol=1e-15), k
    assert np.allclose(Rs.net.flat, g[pk + "s2_w"], rtol=1e-10, atol=1e-13)
    if c["freq"]:
        assert np.allclose(Rs.old.flat, g[pk + "s2_w_old"], rtol=1e-10, atol=1e-13)
    assert Rs.kink > float(g["delta"])


def test_restated_closed_form_gradient_is_the_combines_backward():
    """d_adv = g ((a == act) - 1 / A) and d_v = sum_k g, the closed form the kernel writes, equal the combine's backward of
    d loss / d logits; and a one-row batch follows the same formulas (the reference's squeeze is not kept)."""
    rs = np.random.RandomState(0)
    for B, K, A in ((1, 3, 5), (7, 4, 1), (5, 1, 4)):
        q, on, tg = (rs.standard_normal((B, K, A)) for _ in range(3))
        act, rew, end, w = rs.randint(0, A, (B, K)), rs.standard_normal(B), rs.rand(B) < 0.5, 0.5 + rs.rand(B)
        h = R.head(q, on, tg, act, rew, end, 0.99, w, True)
        td = h["returns"][:, None] - np.take_along_axis(q, act[..., None], -1)[..., 0]
        gk = -2.0 * w[:, None] * td / (K * B)
        onehot = (np.arange(A)[None, None, :] == act[..., None]).astype(np.float64)
        assert np.allclose(h["d_adv"], (gk[..., None] * (onehot - 1.0 / A)).transpose(1, 0, 2), rtol=1e-12, atol=1e-15)
        assert np.allclose(h["d_v"], gk.sum(1), rtol=1e-12, atol=1e-15)
        a_star = on.argmax(-1)
        tq = np.take_along_axis(tg, a_star[..., None], -1)[..., 0].mean(-1)
        assert np.allclose(h["returns"], rew + 0.99 * tq * (1 - end))


def cpu_learner(K=3, A=5, freq=2, **kw):
    from tianshou_marl_amd.algorithm import BDQN, BDQNPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.env.spaces import Discrete
    from tianshou_marl_amd.utils.net import BranchingNet

    net = BranchingNet(state_shape=(6,), num_branches=K, action_per_branch=A, common_hidden_sizes=[16, 16], value_hidden_sizes=[16],
                       action_hidden_sizes=[16], device="cpu", seed=3)
    return BDQN(policy=BDQNPolicy(model=net, action_space=Discrete(A)), optim=AdamOptimizerFactory(lr=1e-3),
                target_update_freq=freq, **kw)


def test_signatures_are_the_reference_ones(g):
    from tianshou_marl_amd.algorithm import BDQN, BDQNPolicy
    from tianshou_marl_amd.utils.net import BranchingNet

    for cls in (BDQNPolicy, BDQN, BranchingNet):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        mine = [f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}" for q in ps]
        ref = [str(x) for x in g[f"sig_{cls.__name__}"]]
        assert mine[:len(ref)] == ref, (cls.__name__, mine, ref)
        assert all(q.default is not inspect.Parameter.empty for q in ps[len(ref):])   # extras (device, seed, storage) have defaults
        assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for q in ps)


def test_checkpoint_keys_shapes_and_round_trip(g):
    K, A = (int(x) for x in g["sd_case"])
    algo = cpu_learner(K, A)
    sd = algo.to_reference_state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [",".join(str(n) for n in v.shape) for v in sd.values()] == [str(x) for x in g["sd_shapes"]]
    other = cpu_learner(K, A)
    other.policy.model.flat.data.add_(1.0)
    other.target_flat.add_(2.0)
    other.load_reference_state_dict(sd)
    assert torch.equal(other.policy.model.flat.data, algo.policy.model.flat.data) and torch.equal(other.target_flat, algo.target_flat)
    # the optimizer's state in the reference's per-parameter order: the shapes are those of `policy.model.*`, and a branch's
    # weight is the transposed slice of the grouped layout
    net, opt = algo.policy.model, algo.optim
    n_model = len(sd) // 2
    assert [",".join(str(n) for n in s) for s in opt._shapes()] == [str(x) for x in g["sd_shapes"]][:n_model]
    opt.exp_avg.copy_(torch.arange(net.flat.numel(), dtype=torch.float32))
    opt.exp_avg_sq.copy_(torch.arange(net.flat.numel(), dtype=torch.float32) * 0.5)
    opt.step_count = 4
    osd = opt.state_dict()
    names = [k for k, _ in net.reference_named_views()]
    i = names.index("branches.1.model.0.weight")
    assert torch.equal(osd["state"][i]["exp_avg"], net.branch_weight(0, opt.exp_avg)[1].t())
    opt2 = other.optim
    opt2.load_state_dict(osd)
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq) and opt2.step_count == 4


def test_branching_net_layout_matches_the_restatement_and_refuses_what_is_not_served():
    from torch import nn

    from tianshou_marl_amd.utils.net import BranchingNet, lagged_copy

    kw = dict(state_shape=(6,), num_branches=3, action_per_branch=5, common_hidden_sizes=[16, 8], value_hidden_sizes=[4],
              action_hidden_sizes=[7], device="cpu")
    net = BranchingNet(seed=1, **kw)
    ch = R.chains(6, [16, 8], [4], [7], 5)
    assert net.flat.numel() == sum(R.sizes(ch, 3)) and (net.v_off, net.b_off) == R.sizes(ch, 3)[:1] + (sum(R.sizes(ch, 3)[:2]),)
    assert net.param_shapes() == R.reference_shapes(ch, 3)
    ref = [v.numpy().astype(np.float64) for _, v in net.reference_named_views()]
    assert np.array_equal(R.flat_from_reference(ref, ch, 3), net.flat.data.numpy().astype(np.float64))
    assert all(np.array_equal(a, b) for a, b in zip(R.reference_from_flat(net.flat.data.numpy(), ch, 3), ref))
    assert torch.equal(BranchingNet(seed=1, **kw).flat.data, net.flat.data)
    state = torch.random.get_rng_state()
    twin = lagged_copy(net)
    assert torch.equal(torch.random.get_rng_state(), state) and torch.equal(twin.flat.data, net.flat.data)
    assert twin.flat.data_ptr() != net.flat.data_ptr()
    for bad, name in ((dict(norm_layer=nn.LayerNorm), "norm_layer"), (dict(activation=nn.Tanh), "activation"),
                      (dict(activation=None), "activation"), (dict(act_args={"inplace": True}), "act_args"),
                      (dict(norm_args={}), "norm_args")):
        with pytest.raises(NotImplementedError, match=name):
            BranchingNet(**{**kw, **bad})
    with pytest.raises(IndexError):
        BranchingNet(**{**kw, "common_hidden_sizes": []})
    with pytest.raises(ValueError, match=r"num_branches = 0 outside \[1, 64\]"):
        BranchingNet(state_shape=(6,), common_hidden_sizes=[16], device="cpu")


def test_policy_refuses_masks_and_a_mismatched_space():
    from tianshou_marl_amd.algorithm import BDQNPolicy
    from tianshou_marl_amd.data.batch import Batch
    from tianshou_marl_amd.env.spaces import Discrete

    algo = cpu_learner()
    pol = algo.policy
    with pytest.raises(ValueError, match="5 actions per branch, the action space 4"):
        BDQNPolicy(model=pol.model, action_space=Discrete(4))
    pol.set_eps_inference(0.5)
    obs = Batch(obs=np.zeros((4, 6), np.float32), mask=np.ones((4, 5), bool))
    with pytest.raises(NotImplementedError, match="action mask"):
        pol.add_exploration_noise(np.zeros((4, 3), np.int64), Batch(obs=obs))
    with pytest.raises(NotImplementedError, match="action mask"):
        pol.forward(Batch(obs=obs))
    np.random.seed(3)
    out = pol.add_exploration_noise(np.full((200, 3), -1, np.int64), Batch(obs=np.zeros((200, 6), np.float32)))
    rnd = (out >= 0).all(1)
    assert 0.35 < rnd.mean() < 0.65 and ((out >= 0).any(1) == rnd).all() and out.max() == 4   # one coin per row
    assert algo.n_step == 1 and algo.use_target_network and algo._iter == 0


def test_wrappers_refuse_cpu_tensors_and_entries_check_bounds_without_a_device():
    _build.build()
    _abi.load()
    assert _abi.BDQN_ROWS_PER_BLOCK == 16
    q, a = torch.zeros(4, 3, 5), torch.zeros(4, 3, dtype=torch.int32)
    for f in (lambda: ops.bdqn_combine(torch.zeros(3, 4, 5), torch.zeros(4)),
              lambda: ops.bdqn_head(q, q, None, a, torch.zeros(4), torch.zeros(4, dtype=torch.uint8), 0.99),
              lambda: ops.bdqn_egreedy(q, torch.zeros(1), 0)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()
    ops.bdqn_check(1, 1)
    ops.bdqn_check(64, 64)
    for K, A, msg in ((0, 5, r"num_branches = 0 outside \[1, 64\]"), (65, 5, r"num_branches = 65 outside \[1, 64\]"),
                      (3, 0, r"n_act = 0 outside \[1, 64\]"), (3, 65, r"n_act = 65 outside \[1, 64\]")):
        with pytest.raises(ValueError, match=msg):
            ops.bdqn_check(K, A)
        with pytest.raises(ValueError, match="tsm_bdqn_check: " + msg):
            _abi.call("tsm_bdqn_check", K, A)
        with pytest.raises(ValueError, match="tsm_bdqn_combine: " + msg):
            _abi.call("tsm_bdqn_combine", 1, 1, 4, K, A, 1, None)
        with pytest.raises(ValueError, match="tsm_bdqn_head: " + msg):
            _abi.call("tsm_bdqn_head", 1, 1, None, 1, 1, 1, None, 4, K, A, 0.99, 1, 1, 1, 1, 1, 1, None)
        with pytest.raises(ValueError, match="tsm_bdqn_egreedy: " + msg):
            _abi.call("tsm_bdqn_egreedy", 1, 4, K, A, 1, 0, 0, None, 1, None)
    for B in (0, 2**25 + 1):
        with pytest.raises(ValueError, match="out of range"):
            _abi.call("tsm_bdqn_combine", 1, 1, B, 3, 5, 1, None)
        with pytest.raises(ValueError, match="out of range"):
            _abi.call("tsm_bdqn_head", 1, 1, None, 1, 1, 1, None, B, 3, 5, 0.99, 1, 1, 1, 1, 1, 1, None)
    for R_ in (-1, 2**25 + 1):
        with pytest.raises(ValueError, match="out of range"):
            _abi.call("tsm_bdqn_egreedy", 1, R_, 3, 5, 1, 0, 0, None, 1, None)
    _abi.call("tsm_bdqn_egreedy", None, 0, 3, 5, None, 0, 0, None, None, None)   # no rows: nothing to do, nothing read
    with pytest.raises(ValueError, match="tsm_bdqn_combine: null pointer"):
        _abi.call("tsm_bdqn_combine", 1, None, 4, 3, 5, 1, None)
    for i in (0, 1, 3, 4, 5, 12, 13, 14, 15, 16):   # every pointer but q_next_target (2) and weight (6), which may be null
        args = [1, 1, None, 1, 1, 1, None, 4, 3, 5, 0.99, 1, 1, 1, 1, 1, 1, None]
        args[i] = None
        with pytest.raises(ValueError, match="tsm_bdqn_head: null pointer"):
            _abi.call("tsm_bdqn_head", *args)
    for i in (0, 4, 8):
        args = [1, 4, 3, 5, 1, 0, 0, None, 1, None]
        args[i] = None
        with pytest.raises(ValueError, match="tsm_bdqn_egreedy: null pointer"):
            _abi.call("tsm_bdqn_egreedy", *args)


def test_buffer_argument_validation():
    from tianshou_marl_amd.data.buffer import DeviceAECReplayBuffer, DeviceVectorReplayBuffer, PrioritizedVectorReplayBuffer

    with pytest.raises(ValueError, match="exclude one another"):
        DeviceVectorReplayBuffer(64, 4, 1, 6, device="cpu", act_dim=2, act_branches=3)
    with pytest.raises(ValueError, match="act_branches = 0"):
        DeviceVectorReplayBuffer(64, 4, 1, 6, device="cpu", act_branches=0)
    with pytest.raises(ValueError, match="exclude one another"):
        PrioritizedVectorReplayBuffer(64, 4, 0.6, 0.4, n_agent=1, obs_dim=6, device="cpu", act_dim=2, act_branches=3)
    with pytest.raises(NotImplementedError, match="act_branches"):
        DeviceAECReplayBuffer(64, 4, ["a", "b"], 6, n_act=5, device="cpu", act_branches=3)
    ps = list(inspect.signature(DeviceVectorReplayBuffer.__init__).parameters.values())
    assert ps[-1].name == "act_branches" and ps[-1].default is None


@pytest.mark.parametrize("K", [1, 3, 4, 5, 9])
def test_counter_advance_and_word_plan(K):
    """Three successive restated draws at the counters `sample_counter` hands out (draws = R, as DQN) own disjoint word sets,
    plain and under a device tick; the coin (word 0 of sub 0) never shares a word with an action (subs 1 ..)."""
    seed, Rr = 0x1234ABCD5678, 37
    pol, ctr = _policy_counter()
    q = np.zeros((Rr, K, 5), np.float32)
    us = [R.bdqn_egreedy(q, 0.5, seed, ctr(Rr))[1] for _ in range(3)]
    assert all(len(u) == Rr * (1 + K) for u in us)
    _disjoint(*us)
    for u in us:
        coin = {w for w in u if w[2] == 0}
        assert len(coin) == Rr and all(w[3] == 0 for w in coin) and all(1 <= w[2] <= 1 + (K - 1) // 4 for w in u - coin)
        assert len(sr.blocks_of(u - coin)) == Rr * ((K + 3) // 4)
    E, N = 7, 3
    before = pol._sample_ctr
    ticks = [2**40 + k * E * N for k in range(3)]
    _disjoint(*[R.bdqn_egreedy(np.zeros((E * N, K, 5), np.float32), 0.5, BIT63, ctr(E * N, 0, t), t)[1] for t in ticks])
    assert pol._sample_ctr == before


@pytest.mark.parametrize("A", [1, 2, 5, 25, 64])
def test_restated_uniform_actions_cover_their_range(A):
    q = np.zeros((400, 3, A), np.float32)
    q[..., A - 1] = 1.0                                   # greedy: the last action
    ref, _ = R.bdqn_egreedy(q, 1.0, 7, 2**32 - 3)
    assert ref["random"].all() and ref["act"].min() == 0 and ref["act"].max() == A - 1
    assert set(np.unique(ref["act"])) == set(range(A))
    ref0, _ = R.bdqn_egreedy(q, 0.0, 7, 2**32 - 3)
    assert not ref0["random"].any() and (ref0["act"] == A - 1).all()
    half, _ = R.bdqn_egreedy(q, 0.5, 7, 2**32 - 3)
    assert 0.4 < half["random"].mean() < 0.6
    assert np.array_equal(half["act"][half["random"]], ref["act"][half["random"]])        # the same words whatever eps
    assert (half["act"][~half["random"]] == A - 1).all()
