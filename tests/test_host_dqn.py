"""CPU tests of the DQN port: the import surface, the argument checks of tsm_nstep_return / tsm_dqn_check /
tsm_dqn_partial_elems / tsm_dqn_td_head / tsm_dqn_egreedy (which fail before touching a device) and of the Python
constructors, `add_exploration_noise` on the host RNG against the reference's actions, the reference-layout checkpoint keys,
and the float64 restatement (tests/dqn_restatement.py) against the reference's own runs (tests/golden/dqn.npz)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "dqn.npz")

from dqn_restatement import DqnRestatement, RestatedBuffer, nstep_walk, td_head  # noqa: E402


class _Discrete:
    def __init__(self, n):
        self.n = n


class _Env:
    def __init__(self, n):
        self.agents = [f"agent_{i}" for i in range(n)]
        self.agent_idx = {a: i for i, a in enumerate(self.agents)}


def _policy(dims=(6, 32, 32, 5), **kw):
    from tianshou_marl_amd.algorithm.dqn import DiscreteQLearningPolicy
    from tianshou_marl_amd.utils.net import FlatMLP

    return DiscreteQLearningPolicy(model=FlatMLP(list(dims), device="cpu", seed=0), action_space=_Discrete(dims[-1]), **kw)


def test_importable_from_algorithm_and_multiagent():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import DQN, DiscreteQLearningPolicy
    from tianshou_marl_amd.algorithm.dqn import DQN as D2
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.multiagent.marl import MultiAgentOffPolicyAlgorithm as M2

    assert DQN is D2 and MultiAgentOffPolicyAlgorithm is M2 and DiscreteQLearningPolicy is not None
    for name in ("nstep_return", "dqn_td_head", "dqn_egreedy", "dqn_check"):
        assert callable(getattr(ops, name)), name


def test_entry_points_reject_bad_arguments_without_a_device():
    from tianshou_marl_amd import _abi, ops

    ns = lambda n_step=1, rs=2, rc=0, ts=1, tc=0, gamma=0.99, I=4, B=3, p=None: _abi.call(  # noqa: E731
        "tsm_nstep_return", p, B, 8, p, p, ts, tc, p, rs, rc, p, I, n_step, gamma, p, p, p, p, None)
    with pytest.raises(ValueError, match="n_step = 0"):
        ns(n_step=0)
    with pytest.raises(ValueError, match="reward column 2"):
        ns(rc=2)
    with pytest.raises(ValueError, match="terminated column 1"):
        ns(tc=1)
    with pytest.raises(ValueError, match="discount factor"):
        ns(gamma=1.5)
    with pytest.raises(ValueError, match="bad sizes"):
        ns(B=0)
    with pytest.raises(ValueError, match="null pointer"):
        ns()
    ns(I=0)  # nothing to do: no pointer is read
    nul = [None] * 9
    with pytest.raises(ValueError, match="n_act = 65"):
        _abi.call("tsm_dqn_td_head", *nul, 37, 65, 1, 0.0, None, None, None, None, None)
    with pytest.raises(ValueError, match="B = 0"):
        _abi.call("tsm_dqn_td_head", *nul, 0, 5, 1, 0.0, None, None, None, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_dqn_td_head", *nul, 37, 5, 1, 0.0, None, None, None, None, None)
    with pytest.raises(ValueError, match="n_act = 0"):
        _abi.call("tsm_dqn_egreedy", None, None, 4, 0, None, 0, 0, None, None, None)
    with pytest.raises(ValueError, match="negative"):
        _abi.call("tsm_dqn_egreedy", None, None, -1, 5, None, 0, 0, None, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_dqn_egreedy", None, None, 4, 5, None, 0, 0, None, None, None)
    _abi.call("tsm_dqn_egreedy", None, None, 0, 5, None, 0, 0, None, None, None)
    with pytest.raises(ValueError, match="n_act = 100"):
        ops.dqn_check(100)
    with pytest.raises(ValueError, match="greater than 0"):
        ops.dqn_check(5, 0)
    ops.dqn_check(64, 1)
    assert _abi.call("tsm_dqn_partial_elems", 0) == -1
    assert _abi.call("tsm_dqn_partial_elems", 257) == 2 * 2  # 256 rows per workgroup
    for B in (1, 256, 257):   # ops.dqn_td_head allocates its partials by _abi.DQN_ROWS_PER_BLOCK
        assert _abi.call("tsm_dqn_partial_elems", B) == 2 * -(-B // _abi.DQN_ROWS_PER_BLOCK)


def test_ops_refuse_cpu_tensors():
    from tianshou_marl_amd import ops

    q = torch.zeros(4, 5)
    v = torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dqn_td_head(q, q, None, v.long(), v, v, v.to(torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dqn_egreedy(q, torch.zeros(1), 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.nstep_return(None, torch.zeros(8, 3, 1, dtype=torch.uint8), torch.zeros(8, 3, 2), v.long(), 3, 0.99)


def test_constructors_validate():
    from tianshou_marl_amd.algorithm.dqn import DQN, DiscreteQLearningPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import FlatAdam, FlatMLP

    with pytest.raises(TypeError, match="FlatMLP"):
        DiscreteQLearningPolicy(model=torch.nn.Linear(6, 5), action_space=_Discrete(5))
    with pytest.raises(ValueError, match="5 outputs"):
        DiscreteQLearningPolicy(model=FlatMLP([6, 5], device="cpu"), action_space=_Discrete(4))
    with pytest.raises(ValueError, match="n_act = 65"):
        DiscreteQLearningPolicy(model=FlatMLP([6, 65], device="cpu"), action_space=_Discrete(65))
    pol = _policy(eps_training=0.25, eps_inference=0.05)
    assert float(pol._eps_dev) == pytest.approx(0.05)
    pol.is_within_training_step = True
    assert float(pol._eps_dev) == pytest.approx(0.25)
    pol.set_eps_training(0.5)
    assert pol.eps_training == 0.5 and float(pol._eps_dev) == 0.5
    pol.set_eps_inference(0.125)
    pol.is_within_training_step = False
    assert float(pol._eps_dev) == 0.125
    with pytest.raises(TypeError, match="DiscreteQLearningPolicy"):
        DQN(policy=torch.nn.Linear(2, 2), optim=AdamOptimizerFactory())
    with pytest.raises(TypeError, match="AdamOptimizerFactory or a FlatAdam"):
        DQN(policy=pol, optim=torch.optim.Adam([torch.zeros(1, requires_grad=True)]))
    with pytest.raises(AssertionError, match="n_step_return_horizon"):
        DQN(policy=pol, optim=AdamOptimizerFactory(), n_step_return_horizon=0)
    with pytest.raises(AssertionError, match="discount factor"):
        DQN(policy=pol, optim=AdamOptimizerFactory(), gamma=1.5)
    with pytest.raises(ValueError, match="own flat parameter vector"):
        DQN(policy=pol, optim=FlatAdam(FlatMLP([6, 5], device="cpu")))
    algo = DQN(policy=pol, optim=AdamOptimizerFactory(lr=3e-4, betas=(0.8, 0.99), eps=1e-6), target_update_freq=2)
    assert (algo.optim.lr, algo.optim.betas, algo.optim.eps) == (3e-4, (0.8, 0.99), 1e-6)
    assert algo.use_target_network and torch.equal(algo.model_old.flat.data, pol.model.flat.data)
    assert algo.model_old.flat.data_ptr() != pol.model.flat.data_ptr()
    assert DQN(policy=_policy(), optim=AdamOptimizerFactory()).model_old is None
    with pytest.raises(RuntimeError, match="outside of a training step"):
        algo.update(None, 8)
    ma = MultiAgentOffPolicyAlgorithm(algorithms=[algo, DQN(policy=_policy(), optim=AdamOptimizerFactory())], env=_Env(2))
    assert ma.get_algorithm("agent_0") is algo and set(ma.state_dict()) == {"agent_0", "agent_1"}
    with pytest.raises(RuntimeError, match="outside of a training step"):
        ma.update(None, 8)
    ma.is_within_training_step = True
    assert pol.is_within_training_step and algo.is_within_training_step


def test_lagged_copy_follows_the_iter_rule():
    """dqn.py:277-285 with `_iter` starting at 0: copies on calls 0, f, 2f, ..."""
    from tianshou_marl_amd.algorithm.dqn import DQN
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory

    algo = DQN(policy=_policy(), optim=AdamOptimizerFactory(), target_update_freq=3)
    copied = []
    for k in range(7):
        algo.policy.model.flat.data.add_(1.0)
        algo._periodically_update_lagged_network_weights()
        copied.append(bool(torch.equal(algo.target_flat, algo.policy.model.flat.data)))
    assert copied == [True, False, False, True, False, False, True] and algo._iter == 7


def test_add_exploration_noise_matches_the_reference():
    from tianshou_marl_amd.data import Batch

    g = np.load(GOLD)
    B = len(g["ex_act"])
    pol = _policy((3, 5), eps_training=float(g["ex_eps"]))
    obs = np.zeros((B, 3), np.float32)
    np.random.seed(int(g["ex_seed"]))
    same = pol.add_exploration_noise(g["ex_act"].copy(), Batch(obs=obs))   # inference epsilon 0: untouched, nothing drawn
    assert np.array_equal(same, g["ex_act"])
    pol.is_within_training_step = True
    out = pol.add_exploration_noise(g["ex_act"].copy(), Batch(obs=obs))
    assert np.array_equal(out, g["ex_out_nomask"]) and not np.array_equal(out, g["ex_act"])
    np.random.seed(int(g["ex_seed"]))
    out = pol.add_exploration_noise(g["ex_act"].copy(), Batch(obs=Batch(obs=obs, mask=g["ex_mask"])))
    assert np.array_equal(out, g["ex_out_mask"])
    assert g["ex_mask"][np.arange(B), out][out != g["ex_act"]].all()
    with pytest.raises(NotImplementedError):
        pol.add_exploration_noise(torch.zeros(3), Batch(obs=obs))


def test_reference_checkpoint_layout():
    from tianshou_marl_amd.algorithm.dqn import DQN
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory

    g = np.load(GOLD)
    algo = DQN(policy=_policy(), optim=AdamOptimizerFactory(), target_update_freq=2)
    sd = algo.to_reference_state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g["sd_shapes"]]
    other = DQN(policy=_policy(), optim=AdamOptimizerFactory(), target_update_freq=2)
    other.policy.model.flat.data.zero_()
    other.load_reference_state_dict(sd)
    assert torch.equal(other.policy.model.flat.data, algo.policy.model.flat.data)
    algo._iter = 5
    other.load_state_dict(algo.state_dict())
    assert other._iter == 5 and torch.equal(other.target_flat, algo.target_flat)


# ---- the restatement against the reference's runs ----------------------------------------------------------------
def replay_ns(g) -> RestatedBuffer:
    B, S, D = (int(x) for x in g["ns_dims"])
    R = RestatedBuffer(B, S, D)
    for k in range(len(g["ns_env"])):
        R.add(int(g["ns_env"][k]), g["ns_rew"][k], bool(g["ns_term"][k]), bool(g["ns_trunc"][k]))
    return R


def test_fixture_buffer_covers_the_cases_asked_for():
    g = np.load(GOLD)
    R = replay_ns(g)
    assert (R.size == R.S).any() and (np.bincount(g["ns_env"]) > R.S).any()          # filled past wrap-around
    assert g["ns_term"].any() and (g["ns_trunc"] & ~g["ns_term"]).any()               # terminated vs truncated ends
    assert len(g["ns_unfinished"]) >= 1 and len(g["ns_unfinished"]) < R.B             # an open tail and a finished one
    assert len(g["ns_indices"]) > len(g["ns_all"]) and np.array_equal(g["ns_indices"][:len(g["ns_all"])], g["ns_all"])
    assert (g["ns_n3_c0_gpow"] > 0.99 ** 3 + 1e-9).any()                               # an episode end inside a window


@pytest.mark.parametrize("n_step", [1, 3, 5])
@pytest.mark.parametrize("col", [0, 1])
def test_restatement_reproduces_the_nstep_walk(n_step, col):
    g = np.load(GOLD)
    R = replay_ns(g)
    assert np.array_equal(R.sample_indices_all(), g["ns_all"]) and np.array_equal(R.unfinished_index(), g["ns_unfinished"])
    idx_n, mc, gpow, vmask = nstep_walk(R, g["ns_indices"], n_step, float(g["gamma"]), col)
    p = f"ns_n{n_step}_c{col}_"
    assert np.array_equal(idx_n, g[p + "idxn"]) and np.array_equal(vmask, g[p + "vmask"])
    np.testing.assert_allclose(mc, g[p + "mc"], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(gpow, g[p + "gpow"], rtol=1e-12, atol=0)
    ret = (g["ns_tq"][idx_n] * vmask).astype(np.float32) * gpow + mc
    np.testing.assert_allclose(ret.astype(np.float32), g[p + "returns"], rtol=2e-7, atol=1e-7)


@pytest.mark.parametrize("A", [2, 5, 9])
def test_restatement_reproduces_the_td_head(A):
    g = np.load(GOLD)
    p = f"hd_A{A}_"
    on = g[p + "on"]
    assert (on[3] == on[3].max()).sum() >= 2  # the tie that pins first-argmax
    for c, case in enumerate(g["hd_cases"]):
        dbl, tgt, loss, msk = case[1] == "1", case[3] == "1", case.split("_")[1], case[-1] == "1"
        h = td_head(g[p + "q"], on, g[p + "tg"] if tgt else None, g[p + "mask"] if msk else None, g[p + "act"], g[p + "mc"],
                    g[p + "gpow"], g[p + "vmask"], g[p + "weight"] if loss == "msew" else None, dbl,
                    float(g["hd_huber_delta"]) if loss == "huber" else None)
        assert h["loss"] == pytest.approx(float(g[p + "loss"][c, 0]), rel=1e-12, abs=0), case
        np.testing.assert_allclose(h["td_error"], g[p + "td"][4 * dbl + 2 * tgt + msk], rtol=1e-11, atol=1e-14, err_msg=case)
        sel = h["dq"][np.arange(len(on)), g[p + "act"]]
        np.testing.assert_allclose(sel, g[p + "dqsel"][c], rtol=1e-12, atol=1e-16, err_msg=case)
        assert np.count_nonzero(h["dq"]) == np.count_nonzero(sel)


def check_digest(g, key, x, rel=1e-10):
    """`x` against the digest of the reference's float64 array: sum, sum of squares and the fixed entries."""
    scale = float(np.abs(x).max())
    assert abs(x.sum() - float(g[f"{key}_dsum"])) <= rel * scale * x.size ** 0.5, key
    assert abs((x * x).sum() - float(g[f"{key}_dsq"])) <= rel * float(g[f"{key}_dsq"]), key
    np.testing.assert_allclose(x[g[f"{key}_didx"]], g[f"{key}_dval"], rtol=rel, atol=rel * scale * 1e-3, err_msg=key)


def up_inputs(g):
    """The `up_*` buffer as the restatement sees it: RestatedBuffer, flat obs / obs_next / act arrays."""
    d = [int(x) for x in g["up_dims"]]
    dims, (B, n_env, S, n_step, freq, steps, T) = d[:4], d[4:]
    RB = RestatedBuffer(n_env, S, 1)
    obs = np.zeros((n_env * S, dims[0]), np.float32)
    obs_next, act = obs.copy(), np.zeros(n_env * S, np.int64)
    for t in range(T):
        for e in range(n_env):
            cur = RB.add(e, g["up_rows_rew"][t, e], bool(g["up_rows_term"][t, e]), bool(g["up_rows_trunc"][t, e]))
            obs[cur], obs_next[cur], act[cur] = g["up_rows_obs"][t, e], g["up_rows_obs_next"][t, e], g["up_rows_act"][t, e]
    return dims, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act


def test_restatement_reproduces_the_updates():
    g = np.load(GOLD)
    dims, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(g)
    R = DqnRestatement(g["up_init"], dims, target_update_freq=freq)
    for k in range(steps):
        idx = g[f"up_s{k}_indices"]
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        assert R.min_kink_gap(np.concatenate([obs[idx], obs_next[idx_n]])) > float(g["delta"])
        r = R.update(obs[idx], act[idx], obs_next[idx_n], None, mc, gpow, vmask)
        assert r["loss"] == pytest.approx(float(g[f"up_s{k}_loss"][0]), rel=1e-11, abs=0)
        np.testing.assert_allclose(r["returns"], g[f"up_s{k}_returns"], rtol=1e-11, atol=1e-13)
        check_digest(g, f"up_s{k}_weights", R.weights())
        check_digest(g, f"up_s{k}_targets", R.targets())
