"""CPU tests of the Discrete SAC port: the import surface, the constructors' refusals, the argument checks of the
tsm_dsac_* entries (which fail before touching a device), the recorded reference signatures, the reference-layout checkpoint
keys, and the float64 restatement (tests/dsac_restatement.py) against the reference's own runs (tests/golden/dsac.npz) to
1e-10 relative, with its closed-form actor gradient against a central finite difference of the restated loss."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "dsac.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")

from dqn_restatement import nstep_walk  # noqa: E402
from dsac_restatement import (DsacRestatement, actor_head, actor_loss, alpha_state, alpha_step, categorical, critic_head,  # noqa: E402
                              target)
from test_host_dqn import _Discrete, _Env, check_digest, up_inputs  # noqa: E402

ACTS = (2, 5, 64)
REL = 1e-10
NETS = ("actor", "critic", "critic2", "critic_old", "critic2_old")
STAT_KEYS = ("actor_loss", "critic1_loss", "critic2_loss", "alpha", "alpha_loss")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def head_inputs(g, A):
    """The head inputs of one A: the i16 lattice back as float32 values, the rest as stored."""
    p = f"hd_A{A}_"
    d = {k: g[p + k] for k in ("act", "mc", "gpow", "vmask", "weight")}
    d.update({k: (g[p + k].astype(np.float32) / np.float32(8.0)) for k in ("logits", "lnext", "q1", "q2", "q1n", "q2n")})
    return d


def head_alpha(g, auto: bool) -> float:
    """The alpha the head cases run under: the fixed one, or exp(log_alpha) of the fixture's AutoAlpha before its step."""
    return float(np.exp(g["hd_log_alpha"])) if auto else float(g["hd_fixed"])


def up_restatement(g, kind):
    init = g[f"up_{kind}_init"]
    alpha = float(g["up_fixed"]) if kind == "fix" else alpha_state(0.0)
    return DsacRestatement(init[0], init[1], init[2], [6, 32, 32, 5], alpha, float(g["tau"]), lr=float(g["lr"]),
                           target_entropy=float(g["up_target_entropy"]), alpha_lr=float(g["lr"]))


def _sac(dims=(6, 32, 32, 5), alpha=0.2, policy_kw=None, **kw):
    from tianshou_marl_amd.algorithm import DiscreteSAC, DiscreteSACPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import FlatMLP

    pol = DiscreteSACPolicy(actor=FlatMLP(list(dims), device="cpu", seed=0), action_space=_Discrete(dims[-1]), **(policy_kw or {}))
    return DiscreteSAC(policy=pol, policy_optim=AdamOptimizerFactory(), critic=FlatMLP(list(dims), device="cpu", seed=1),
                       critic_optim=AdamOptimizerFactory(lr=3e-4), alpha=alpha, **kw)


def _auto(**kw):
    from tianshou_marl_amd.algorithm import AutoAlpha
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory

    return AutoAlpha(0.98 * float(np.log(5.0)), 0.0, AdamOptimizerFactory(lr=1e-3), **kw)


# ---- surface ----------------------------------------------------------------------------------------------------------------
def test_importable_from_algorithm():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import Alpha, AutoAlpha, DiscreteSAC, DiscreteSACPolicy, DiscreteSACTrainingStats, FixedAlpha
    from tianshou_marl_amd.algorithm.dsac import DiscreteSAC as D2

    assert DiscreteSAC is D2 and issubclass(AutoAlpha, Alpha) and issubclass(FixedAlpha, Alpha) and DiscreteSACPolicy is not None
    assert DiscreteSACTrainingStats(actor_loss=1.0, critic1_loss=2.0, critic2_loss=3.0, alpha=0.2).get_loss_stats_dict() == {
        "actor_loss": 1.0, "critic1_loss": 2.0, "critic2_loss": 3.0, "alpha": 0.2}
    for name in ("dsac_check", "dsac_target", "dsac_critic_head", "dsac_actor_head", "dsac_alpha_step"):
        assert callable(getattr(ops, name)), name


def test_recorded_signatures_match_the_reference(g):
    """Same names, same defaults, same kinds (keyword-only where the reference is); ours may add trailing parameters."""
    from tianshou_marl_amd.algorithm import AutoAlpha, DiscreteSAC, DiscreteSACPolicy, FixedAlpha

    for cls in (DiscreteSACPolicy, DiscreteSAC, AutoAlpha, FixedAlpha):
        mine = inspect.signature(cls.__init__).parameters
        names = [str(x).split("=", 1)[0] for x in g[f"sig_{cls.__name__}"]]
        assert [n for n in mine if n != "self"][:len(names)] == names, cls.__name__
        for item, kind in zip(g[f"sig_{cls.__name__}"], g[f"sigkind_{cls.__name__}"]):
            name, default = str(item).split("=", 1)
            ours = "<required>" if mine[name].default is inspect.Parameter.empty else repr(mine[name].default)
            assert ours == default and mine[name].kind.name == str(kind), (cls.__name__, name, ours, default)


def test_constructors_validate():
    from tianshou_marl_amd.algorithm import Alpha, AutoAlpha, DiscreteSAC, DiscreteSACPolicy, FixedAlpha
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory, LRSchedulerFactoryLinear
    from tianshou_marl_amd.utils.net import FlatMLP

    net = lambda w=5, d=6: FlatMLP([d, 16, w], device="cpu", seed=0)  # noqa: E731
    with pytest.raises(TypeError, match="FlatMLP"):
        DiscreteSACPolicy(actor=torch.nn.Linear(6, 5), action_space=_Discrete(5))
    with pytest.raises(ValueError, match="4 outputs, the action space 5 actions"):
        DiscreteSACPolicy(actor=net(4), action_space=_Discrete(5))
    with pytest.raises(ValueError, match="no size"):
        DiscreteSACPolicy(actor=net(), action_space=object())
    with pytest.raises(ValueError, match=r"n_act = 65 outside \[1, 64\]"):
        DiscreteSACPolicy(actor=net(65), action_space=_Discrete(65))
    with pytest.raises(TypeError):
        DiscreteSACPolicy(net(), True, _Discrete(5))       # keyword-only, as in the reference
    pol = DiscreteSACPolicy(actor=net(), action_space=_Discrete(5))
    assert pol.deterministic_eval is True and pol.n_act == 5 and not pol.is_within_training_step
    with pytest.raises(NotImplementedError, match="action masks are not part of the reference's Discrete SAC"):
        pol.act_device(torch.zeros(3, 6), mask=torch.ones(3, 5, dtype=torch.bool))
    from tianshou_marl_amd.data import Batch
    with pytest.raises(NotImplementedError, match="action masks"):
        pol(Batch(obs=Batch(obs=np.zeros((3, 6), np.float32), mask=np.ones((3, 5), bool)), info=Batch()))
    f = AdamOptimizerFactory()
    with pytest.raises(TypeError, match="needs a DiscreteSACPolicy"):
        DiscreteSAC(policy=net(), policy_optim=f, critic=net(), critic_optim=f)
    with pytest.raises(TypeError, match="critic must be a FlatMLP"):
        DiscreteSAC(policy=pol, policy_optim=f, critic=torch.nn.Linear(6, 5), critic_optim=f)
    with pytest.raises(ValueError, match="critic2 maps 6 -> 4"):
        DiscreteSAC(policy=pol, policy_optim=f, critic=net(), critic_optim=f, critic2=net(4))
    with pytest.raises(AssertionError, match="tau should be in"):
        DiscreteSAC(policy=pol, policy_optim=f, critic=net(), critic_optim=f, tau=1.5)
    with pytest.raises(AssertionError, match="n_step_return_horizon should be greater than 0"):
        DiscreteSAC(policy=pol, policy_optim=f, critic=net(), critic_optim=f, n_step_return_horizon=0)
    with pytest.raises(ValueError, match="Expected float or Alpha instance"):
        DiscreteSAC(policy=pol, policy_optim=f, critic=net(), critic_optim=f, alpha=1)
    with pytest.raises(ValueError, match="Learning rate schedulers are not supported by AutoAlpha"):
        AutoAlpha(1.0, 0.0, AdamOptimizerFactory().with_lr_scheduler_factory(LRSchedulerFactoryLinear(1, 1, 1)))
    crit = net()
    algo = DiscreteSAC(policy=pol, policy_optim=f, critic=crit, critic_optim=AdamOptimizerFactory(lr=3e-4))
    assert isinstance(algo.alpha, FixedAlpha) and algo.alpha.value == 0.2 and algo.tau == 0.005 and algo.gamma == 0.99
    assert algo.critic is crit and algo.critic2 is not crit and torch.equal(algo.critic2.flat.data, crit.flat.data)   # deepcopy
    assert algo.critic2.flat.data.data_ptr() != crit.flat.data.data_ptr()
    assert torch.equal(algo.critic_old.flat.data, crit.flat.data) and torch.equal(algo.critic2_old.flat.data, crit.flat.data)
    assert algo.critic2_optim.lr == 3e-4 and algo.critic_optim.coef64 and algo.policy_optim.lr == 1e-3   # the first factory again
    assert torch.equal(algo.alpha.device_scalar("cpu"), torch.tensor([0.2]))
    with pytest.raises(RuntimeError, match="outside of a training step"):
        algo.update(None, 8)
    auto = _auto()
    assert isinstance(Alpha.from_float_or_instance(auto), AutoAlpha) and auto.value == 1.0
    assert list(auto.state_dict().keys()) == ["_log_alpha"] and auto._log_alpha.shape == ()


def test_members_of_a_multiagent_algorithm():
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm

    ma = MultiAgentOffPolicyAlgorithm(algorithms=[_sac(), _sac(alpha=_auto())], env=_Env(2))
    assert set(ma.state_dict()) == {"agent_0", "agent_1"}
    ma.is_within_training_step = True
    assert ma.get_algorithm("agent_1").is_within_training_step and ma.get_algorithm("agent_1").policy.is_within_training_step


def test_entry_points_reject_bad_arguments_without_a_device():
    from tianshou_marl_amd import _abi, ops

    hdr = int(re.search(r"#define\s+TSM_DSAC_ROWS_PER_BLOCK\s+(\d+)", open(_abi.HEADER_PATH).read()).group(1))
    assert hdr == _abi.DSAC_ROWS_PER_BLOCK
    with pytest.raises(ValueError, match=r"n_act = 65 outside \[1, 64\]"):
        ops.dsac_check(65)
    with pytest.raises(ValueError, match=r"n_act = 0 outside \[1, 64\]"):
        _abi.call("tsm_dsac_check", 0, 1)
    with pytest.raises(ValueError, match="n_step_return_horizon should be greater than 0 but got: 0"):
        ops.dsac_check(5, 0)
    ops.dsac_check(64, 1)
    ops.dsac_check(1, 7)
    tgt = lambda B=37, A=5: _abi.call("tsm_dsac_target", *[None] * 7, B, A, None, None)  # noqa: E731
    cri = lambda B=37, A=5: _abi.call("tsm_dsac_critic_head", *[None] * 5, B, A, None, None, None, None, None)  # noqa: E731
    act = lambda B=37, A=5: _abi.call("tsm_dsac_actor_head", *[None] * 4, B, A, None, None, None, None)  # noqa: E731
    for fn in (tgt, cri, act):
        with pytest.raises(ValueError, match="n_act = 65"):
            fn(A=65)
        with pytest.raises(ValueError, match="B = 0"):
            fn(B=0)
        with pytest.raises(ValueError, match="null pointer"):
            fn()
    step = lambda lr=1e-3, b1=0.9, nb=1: _abi.call("tsm_dsac_alpha_step", None, nb, 37, *[None] * 4, 1.0, lr, b1, 0.999, 1e-8, 0.0,  # noqa: E731
                                                   None, None, None)
    with pytest.raises(ValueError, match="n_blocks = 0"):
        step(nb=0)
    with pytest.raises(ValueError, match="bad Adam hyper-parameters"):
        step(lr=-1.0)
    with pytest.raises(ValueError, match="bad Adam hyper-parameters"):
        step(b1=1.0)
    with pytest.raises(ValueError, match="null pointer"):
        step()


def test_ops_refuse_cpu_tensors():
    from tianshou_marl_amd import ops

    q, v, a = torch.zeros(4, 5), torch.zeros(4), torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dsac_target(q, q, q, a, v, v, v.to(torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dsac_critic_head(q, q, v.long(), v)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dsac_actor_head(q, q, q, a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dsac_alpha_step(torch.zeros(2, dtype=torch.float64), 4, a, a, a, a.long(), 1.0, a, torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _auto().update(torch.zeros(4))


def test_reference_checkpoint_layout(g):
    for kind in ("fix", "auto"):
        algo = _sac(alpha=0.2 if kind == "fix" else _auto())
        sd = algo.to_reference_state_dict()
        assert list(sd.keys()) == [str(k) for k in g[f"sd_{kind}_keys"]]
        assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g[f"sd_{kind}_shapes"]]
    other = _sac(alpha=_auto())
    for _, net in other._nets():
        net.flat.data.zero_()
    sd["alpha._log_alpha"] = torch.tensor(-0.5)
    other.load_reference_state_dict(sd)
    for (_, a), (_, b) in zip(other._nets(), algo._nets()):
        assert torch.equal(a.flat.data, b.flat.data)
    assert other.alpha._log_alpha.item() == -0.5 and other.alpha.device_scalar("cpu").item() == pytest.approx(np.exp(-0.5))
    other.critic_old.flat.data.add_(1.0)
    other.policy_optim.step_count = 3
    algo.load_state_dict(other.state_dict())
    assert torch.equal(algo.critic_old.flat.data, other.critic_old.flat.data) and algo.alpha._log_alpha.item() == -0.5


# ---- the restatement against the reference's runs -----------------------------------------------------------------------
@pytest.mark.parametrize("A", ACTS)
def test_fixture_rows_cover_the_cases_asked_for(g, A):
    d = head_inputs(g, A)
    assert len(d["act"]) == 37 and not d["vmask"][5] and d["vmask"].any()
    for k in ("logits", "lnext"):
        x = d[k]
        top = np.sort(x[3])
        assert top[-1] == top[-2] and (A == 2 or top[-2] > top[-3])                      # two equal top logits
        assert np.sort(x[7])[1] - x[7, 1] >= 40.0 and x[7].argmin() == 1                 # one logit 40 below the rest
        p, _, H = categorical(x)
        assert 0.0 < p[7, 1] < 1e-15 and np.float32(p[7, 1]) > 0 and (H > 0).all()
    assert (d["q1"] != d["q2"]).all() and (d["q1n"] != d["q2n"]).all()
    for k in ("logits", "q1", "q2n"):
        assert np.array_equal(d[k] * 8, np.round(d[k] * 8))                              # eighths: exact in float32


@pytest.mark.parametrize("A", ACTS)
def test_restatement_reproduces_the_heads(g, A):
    d = head_inputs(g, A)
    p = f"A{A}_"
    for auto in (0, 1):
        ret = target(d["lnext"], d["q1n"], d["q2n"], head_alpha(g, auto), d["mc"], d["gpow"], d["vmask"])
        ref = g[f"tg_{p}a{auto}_returns"]
        np.testing.assert_allclose(ret, ref, rtol=REL, atol=REL * np.abs(ref).max())
        assert ret[5] == d["mc"][5]
    for c, case in enumerate(g["hc_cases"]):
        wgt, auto = case[1] == "1", case[3] == "1"
        alpha = head_alpha(g, auto)
        ret = target(d["lnext"], d["q1n"], d["q2n"], alpha, d["mc"], d["gpow"], d["vmask"])
        ch = critic_head(d["q1"], d["q2"], d["act"], ret, d["weight"] if wgt else None)
        ah = actor_head(d["logits"], d["q1"], d["q2"], alpha)
        stats = g[f"hc_{p}stats"][c]
        assert [ah["loss"], ch["loss1"], ch["loss2"]] == pytest.approx(list(stats[:3]), rel=REL, abs=0), case
        np.testing.assert_allclose(ch["prio"], g[f"hc_{p}prio"][c], rtol=REL, atol=REL * np.abs(g[f"hc_{p}prio"][c]).max())
        check_digest(g, f"hc_{p}c{c}_dl", ah["d_logits"].reshape(-1))
        off = ch["dq1"].copy()
        off[np.arange(37), d["act"]] = 0.0
        assert not off.any()
        if auto:   # AutoAlpha.update from the pre-step entropy: the loss, the new log_alpha, the alpha the stats report
            st = alpha_state(float(g["hd_log_alpha"]))
            loss = alpha_step(st, ah["mean_entropy"], float(g["hd_target_entropy"]), lr=float(g["lr"]))
            assert loss == pytest.approx(stats[4], rel=REL) and st["log_alpha"] == pytest.approx(g[f"hc_{p}log_alpha"][c, 0], rel=REL)
            assert np.exp(st["log_alpha"]) == pytest.approx(stats[3], rel=REL)
        else:
            assert np.isnan(stats[4]) and stats[3] == alpha


@pytest.mark.parametrize("A", ACTS)
def test_closed_form_actor_gradient_matches_a_central_difference(g, A):
    d = head_inputs(g, A)
    x = d["logits"].astype(np.float64)
    alpha = 0.37
    grad = actor_head(x, d["q1"], d["q2"], alpha)["d_logits"]
    rs = np.random.RandomState(A)
    eps = 1e-5
    entries = [(3, 0), (3, A - 1), (7, 1), (7, 0)] + [(int(rs.randint(37)), int(rs.randint(A))) for _ in range(24)]
    for b, j in entries:
        up, dn = x.copy(), x.copy()
        up[b, j] += eps
        dn[b, j] -= eps
        fd = (actor_loss(up, d["q1"], d["q2"], alpha) - actor_loss(dn, d["q1"], d["q2"], alpha)) / (2 * eps)
        assert abs(fd - grad[b, j]) <= 1e-8 * np.abs(grad).max() + 1e-7 * abs(grad[b, j]), (b, j, fd, grad[b, j])
    np.testing.assert_allclose(grad.sum(1), 0.0, atol=1e-15)    # a shift of a row's logits changes nothing


@pytest.mark.parametrize("kind", ["fix", "auto"])
def test_restatement_reproduces_the_updates(g, kind):
    gd = np.load(DQN_GOLD)
    _, B, n_env, S, n_step, _, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    R = up_restatement(g, kind)
    for k in range(steps):
        pk = f"up_{kind}_s{k}_"
        idx = g[pk + "indices"]
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        r = R.update(obs[idx], act[idx], obs_next[idx_n], mc, gpow, vmask)
        ref = g[pk + "stats"][0]
        assert R.kink > float(g["delta"])
        assert [r["actor_loss"], r["critic1_loss"], r["critic2_loss"], r["alpha"]] == pytest.approx(list(ref[:4]), rel=REL, abs=0)
        check_digest(g, pk + "returns", r["returns"])
        for n in NETS:
            check_digest(g, pk + n, R.weights(n))
        assert r["mean_entropy"] == pytest.approx(float(g[pk + "mean_entropy"]), rel=REL)
        if kind == "auto":
            assert r["alpha_loss"] == pytest.approx(ref[4], rel=REL, abs=0)
            assert R.alpha["log_alpha"] == pytest.approx(g[pk + "log_alpha"][0], rel=REL)
        else:
            assert r["alpha_loss"] is None and np.isnan(ref[4])
