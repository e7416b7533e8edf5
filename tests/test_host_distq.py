"""CPU tests of the C51 / QR-DQN port: the import surface, the constructors' refusals, the argument checks of
tsm_distq_check / tsm_distq_values / tsm_c51_head / tsm_qrdqn_head (which fail before touching a device), the recorded
reference signatures, the reference-layout checkpoint keys, and the float64 restatement (tests/distq_restatement.py)
against the reference's own runs (tests/golden/distq.npz) to 1e-10 relative."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "distq.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")

from distq_restatement import DistqRestatement, c51_head, dist_values, qr_head, support_of, tau_hat_of  # noqa: E402
from dqn_restatement import nstep_walk  # noqa: E402
from test_host_dqn import _Discrete, _Env, check_digest, up_inputs  # noqa: E402

GRID = [(A, N) for A in (2, 5) for N in (2, 51, 200)]
REL = 1e-10


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def head_inputs(g, A, N):
    """The shared head inputs of one (A, N): the i8 lattice back as float32 logits, the rest as stored."""
    p = f"hd_A{A}_N{N}_"
    d = {k: g[p + k] for k in ("act", "mc", "gpow", "vmask", "weight", "mask")}
    d.update({k: (g[p + k].astype(np.float32) / np.float32(8.0)) for k in ("raw", "on", "tg")})
    return d


def _c51(dims=(6, 32, 32, 255), A=5, N=51, policy_kw=None, **kw):
    from tianshou_marl_amd.algorithm import C51, C51Policy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import FlatMLP

    pol = C51Policy(model=FlatMLP(list(dims), device="cpu", seed=0), action_space=_Discrete(A), num_atoms=N, **(policy_kw or {}))
    return C51(policy=pol, optim=AdamOptimizerFactory(), **kw)


def _qr(dims=(6, 32, 32, 160), A=5, N=32, **kw):
    from tianshou_marl_amd.algorithm import QRDQN, QRDQNPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import FlatMLP

    pol = QRDQNPolicy(model=FlatMLP(list(dims), device="cpu", seed=0), action_space=_Discrete(A), num_quantiles=N)
    return QRDQN(policy=pol, optim=AdamOptimizerFactory(), num_quantiles=N, **kw)


def test_importable_from_algorithm():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import C51, DQN, QRDQN, C51Policy, DiscreteQLearningPolicy, QRDQNPolicy
    from tianshou_marl_amd.algorithm.distq import C51 as C2

    assert C51 is C2 and issubclass(C51Policy, DiscreteQLearningPolicy) and issubclass(QRDQNPolicy, DiscreteQLearningPolicy)
    assert issubclass(C51, DQN) and issubclass(QRDQN, DQN)
    for name in ("distq_check", "distq_values", "c51_head", "qrdqn_head"):
        assert callable(getattr(ops, name)), name


def test_constructors_validate():
    from tianshou_marl_amd.algorithm import C51, QRDQN, C51Policy, QRDQNPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import FlatMLP

    net = lambda w: FlatMLP([6, 16, w], device="cpu", seed=0)  # noqa: E731
    with pytest.raises(AssertionError, match="num_atoms should be greater than 1 but got: 1"):
        C51Policy(model=net(5), action_space=_Discrete(5), num_atoms=1)
    with pytest.raises(AssertionError, match="v_max should be larger than v_min"):
        C51Policy(model=net(255), action_space=_Discrete(5), v_min=3.0, v_max=3.0)
    with pytest.raises(ValueError, match="250 outputs"):
        C51Policy(model=net(250), action_space=_Discrete(5))
    with pytest.raises(ValueError, match="256"):
        C51Policy(model=net(5 * 257), action_space=_Discrete(5), num_atoms=257)
    with pytest.raises(ValueError, match="256"):
        QRDQNPolicy(model=net(5 * 257), action_space=_Discrete(5), num_quantiles=257)
    with pytest.raises(AssertionError, match="num_quantiles should be greater than 1 but got: 1"):
        QRDQNPolicy(model=net(5), action_space=_Discrete(5), num_quantiles=1)
    with pytest.raises(ValueError, match="160 outputs"):
        QRDQNPolicy(model=net(160), action_space=_Discrete(5), num_quantiles=200)
    with pytest.raises(TypeError, match="FlatMLP"):
        C51Policy(model=torch.nn.Linear(6, 255), action_space=_Discrete(5))
    pol = C51Policy(model=net(255), action_space=_Discrete(5), eps_training=0.25)
    assert pol.support.dtype == torch.float32 and torch.equal(pol.support, torch.linspace(-10.0, 10.0, 51)) and pol.n_act == 5
    with pytest.raises(TypeError, match="needs a QRDQNPolicy"):
        QRDQN(policy=pol, optim=AdamOptimizerFactory(), num_quantiles=51)
    qpol = QRDQNPolicy(model=net(160), action_space=_Discrete(5), num_quantiles=32)
    with pytest.raises(TypeError, match="needs a C51Policy"):
        C51(policy=qpol, optim=AdamOptimizerFactory())
    with pytest.raises(ValueError, match="emits 32"):
        QRDQN(policy=qpol, optim=AdamOptimizerFactory())          # the default of 200 quantiles
    with pytest.raises(AssertionError, match="num_quantiles should be greater than 1"):
        QRDQN(policy=qpol, optim=AdamOptimizerFactory(), num_quantiles=1)
    with pytest.raises(AssertionError, match="n_step_return_horizon"):
        C51(policy=pol, optim=AdamOptimizerFactory(), n_step_return_horizon=0)
    algo = C51(policy=pol, optim=AdamOptimizerFactory(lr=3e-4), target_update_freq=2)
    assert algo.delta_z == pytest.approx(0.4) and algo.use_target_network and algo.optim.lr == 3e-4
    assert torch.equal(algo.model_old.flat.data, pol.model.flat.data)
    with pytest.raises(RuntimeError, match="outside of a training step"):
        algo.update(None, 8)
    q = QRDQN(policy=qpol, optim=AdamOptimizerFactory(), num_quantiles=32)
    tau = torch.linspace(0, 1, 33)
    assert q.tau_hat.shape == (1, 32, 1) and torch.equal(q.tau_hat.view(-1), (tau[:-1] + tau[1:]) / 2) and q.model_old is None


def test_lagged_copy_follows_the_iter_rule():
    algo = _qr(target_update_freq=2)
    copied = []
    for _ in range(5):
        algo.policy.model.flat.data.add_(1.0)
        algo._periodically_update_lagged_network_weights()
        copied.append(bool(torch.equal(algo.target_flat, algo.policy.model.flat.data)))
    assert copied == [True, False, True, False, True]


def test_members_of_a_multiagent_algorithm():
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm

    ma = MultiAgentOffPolicyAlgorithm(algorithms=[_c51(), _qr()], env=_Env(2))
    assert set(ma.state_dict()) == {"agent_0", "agent_1"}
    ma.is_within_training_step = True
    assert ma.get_algorithm("agent_1").is_within_training_step


def test_entry_points_reject_bad_arguments_without_a_device():
    from tianshou_marl_amd import _abi, ops

    hdr = int(re.search(r"#define\s+TSM_DISTQ_ROWS_PER_BLOCK\s+(\d+)", open(_abi.HEADER_PATH).read()).group(1))
    assert hdr == _abi.DISTQ_ROWS_PER_BLOCK
    with pytest.raises(ValueError, match=r"n_atoms = 257 outside \[2, 256\]"):
        ops.distq_check(5, 257)
    with pytest.raises(ValueError, match=r"n_atoms = 1 outside \[2, 256\]"):
        _abi.call("tsm_distq_check", 5, 1)
    with pytest.raises(ValueError, match=r"n_act = 65 outside \[1, 64\]"):
        ops.distq_check(65, 51)
    ops.distq_check(64, 256)
    ops.distq_check(1, 2)
    with pytest.raises(ValueError, match="n_atoms = 300"):
        _abi.call("tsm_distq_values", None, None, 4, 5, 300, 1, None, None, None)
    with pytest.raises(ValueError, match="out of range"):
        _abi.call("tsm_distq_values", None, None, -1, 5, 51, 1, None, None, None)
    with pytest.raises(ValueError, match="categorical mode"):
        _abi.call("tsm_distq_values", 8, None, 4, 5, 51, 0, 8, 8, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_distq_values", None, None, 4, 5, 51, 1, None, None, None)
    _abi.call("tsm_distq_values", None, None, 0, 5, 51, 1, None, None, None)   # nothing to do: no pointer is read
    nul = [None] * 10
    c51 = lambda B=37, A=5, N=51, lo=-10.0, hi=10.0: _abi.call("tsm_c51_head", *nul, B, A, N, lo, hi, None, None, None, None, None)  # noqa: E731
    qr = lambda B=37, A=5, N=200: _abi.call("tsm_qrdqn_head", *nul, B, A, N, None, None, None, None, None)  # noqa: E731
    for fn in (c51, qr):
        with pytest.raises(ValueError, match="n_act = 65"):
            fn(A=65)
        with pytest.raises(ValueError, match="n_atoms = 257"):
            fn(N=257)
        with pytest.raises(ValueError, match="B = 0"):
            fn(B=0)
        with pytest.raises(ValueError, match="null pointer"):
            fn()
    with pytest.raises(ValueError, match="v_max should be larger than v_min"):
        c51(lo=1.0, hi=1.0)


def test_ops_refuse_cpu_tensors_and_check_shapes_first():
    from tianshou_marl_amd import ops

    raw, q, v = torch.zeros(4, 10), torch.zeros(4, 5), torch.zeros(4)
    sup = torch.linspace(-1, 1, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.distq_values(raw, 5, 2, support=sup)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.c51_head(raw, q, raw, v.long(), v, v, v.to(torch.uint8), sup, -1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.qrdqn_head(raw, q, raw, v.long(), v, v, v.to(torch.uint8), sup)
    with pytest.raises(ValueError, match="v_max should be larger"):
        ops.c51_head(raw, q, raw, v.long(), v, v, v.to(torch.uint8), sup, 1.0, -1.0)


def test_recorded_signatures_are_accepted(g):
    """Every parameter of the reference's constructors exists here under its name with its default (ours may add more)."""
    from tianshou_marl_amd.algorithm import C51, QRDQN, C51Policy, QRDQNPolicy

    for cls in (C51Policy, C51, QRDQNPolicy, QRDQN):
        mine = inspect.signature(cls.__init__).parameters
        for item in g[f"sig_{cls.__name__}"]:
            name, default = str(item).split("=", 1)
            assert name in mine, (cls.__name__, name)
            ours = "<required>" if mine[name].default is inspect.Parameter.empty else repr(mine[name].default)
            assert ours == default, (cls.__name__, name, ours, default)


def test_reference_checkpoint_layout(g):
    for kind, mk in (("c51", _c51), ("qr", _qr)):
        algo = mk(target_update_freq=2)
        sd = algo.to_reference_state_dict()
        assert list(sd.keys()) == [str(k) for k in g[f"sd_{kind}_keys"]]
        assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g[f"sd_{kind}_shapes"]]
        other = mk(target_update_freq=2)
        other.policy.model.flat.data.zero_()
        other.load_reference_state_dict(sd)
        assert torch.equal(other.policy.model.flat.data, algo.policy.model.flat.data)
        algo._iter = 5
        other.load_state_dict(algo.state_dict())
        assert other._iter == 5 and torch.equal(other.target_flat, algo.target_flat)


# ---- the restatement against the reference's runs --------------------------------------------------------------------
@pytest.mark.parametrize("A,N", GRID)
def test_fixture_rows_cover_the_cases_asked_for(g, A, N):
    d = head_inputs(g, A, N)
    on = d["on"].reshape(-1, A, N)
    assert len(d["act"]) == 37 and np.array_equal(on[3, 0], on[3, 1]) and not d["vmask"][5]
    sup = support_of(-10.0, 10.0, N)
    ret = sup[None, :] * d["vmask"][:, None] * d["gpow"][:, None] + d["mc"][:, None]
    assert (ret > 10.0).any() and (ret < -10.0).any()                       # clamped at each end
    assert N == 2 or (d["mc"][5] in sup and abs(d["mc"][5]) < 10.0)          # exactly on an interior atom
    for kind in ("c51", "qr"):
        q = g[f"dv_A{A}_N{N}_{kind}_q"]
        assert q[3, 0] == q[3, 1] == q[3].max() and g[f"dv_A{A}_N{N}_{kind}_act"][3] == 0


@pytest.mark.parametrize("A,N", GRID)
def test_restatement_reproduces_values_and_actions(g, A, N):
    d = head_inputs(g, A, N)
    for kind, sup in (("c51", support_of(-10.0, 10.0, N)), ("qr", None)):
        p = f"dv_A{A}_N{N}_{kind}_"
        r0, r1 = dist_values(d["on"], A, N, sup), dist_values(d["on"], A, N, sup, d["mask"])
        np.testing.assert_allclose(r0["q"], g[p + "q"], rtol=REL, atol=REL * np.abs(g[p + "q"]).max())
        assert np.array_equal(r0["act"], g[p + "act"]) and np.array_equal(r1["act"], g[p + "act_masked"])
        assert d["mask"][np.arange(37), r1["act"]].all()


@pytest.mark.parametrize("A,N", GRID)
@pytest.mark.parametrize("kind", ["c5", "qr"])
def test_restatement_reproduces_the_heads(g, kind, A, N):
    d = head_inputs(g, A, N)
    p = f"{kind}_A{A}_N{N}_"
    extra = (support_of(-10.0, 10.0, N), -10.0, 10.0) if kind == "c5" else (tau_hat_of(N),)
    fn = c51_head if kind == "c5" else qr_head
    for c, case in enumerate(g["cases"]):
        tgt, wgt, msk = (case[i] == "1" for i in (1, 3, 5))
        h = fn(d["raw"], d["on"], d["tg"] if tgt else None, d["mask"] if msk else None, d["act"], d["mc"], d["gpow"], d["vmask"],
               d["weight"] if wgt else None, *extra, A, N)
        assert h["loss"] == pytest.approx(float(g[p + "loss"][c, 0]), rel=REL, abs=0), case
        np.testing.assert_allclose(h["prio"], g[p + "prio"][c], rtol=REL, atol=REL * np.abs(g[p + "prio"][c]).max(), err_msg=case)
        assert np.array_equal(h["a_star"], g[p + "astar"][c]), case
        check_digest(g, f"{p}c{c}_dout", h["d_out"].reshape(-1))
        check_digest(g, f"{p}c{c}_ret", h["returns"].reshape(-1))
        if kind == "qr":
            assert (np.abs(h["u"]) > 1.0).any() and (np.abs(h["u"]) < 1.0).any()


def up_rows(gd, kind, idx, idx_n, obs_next):
    """The successor rows each learner reads: the one-step successors (C51, c51.py:124) or those at idx_n (QR-DQN)."""
    return obs_next[idx] if kind == "c51" else obs_next[idx_n]


@pytest.mark.parametrize("kind", ["c51", "qr"])
def test_restatement_reproduces_the_updates(g, kind):
    gd = np.load(DQN_GOLD)
    _, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    dims = [int(x) for x in g[f"up_{kind}_dims"]]
    dims, (A, N) = dims[:4], dims[4:]
    assert (A, N, B, n_step, freq, steps) == (5, 51 if kind == "c51" else 32, 37, 3, 2, 3)
    R = DistqRestatement(g[f"up_{kind}_init"], dims, kind, A, N, target_update_freq=freq)
    for k in range(steps):
        pk = f"up_{kind}_s{k}_"
        idx = g[pk + "indices"]
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        assert not np.array_equal(idx, idx_n)
        r = R.update(obs[idx], act[idx], up_rows(gd, kind, idx, idx_n, obs_next), None, mc, gpow, vmask)
        assert r["loss"] == pytest.approx(float(g[pk + "loss"][0]), rel=REL, abs=0)
        check_digest(g, pk + "returns", r["returns"].reshape(-1))
        check_digest(g, pk + "weights", R.weights())
        check_digest(g, pk + "targets", R.targets())
