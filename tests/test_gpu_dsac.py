"""GPU tests (`-m gpu`) of Discrete SAC: tsm_dsac_check, tsm_dsac_target, tsm_dsac_critic_head, tsm_dsac_actor_head and
tsm_dsac_alpha_step (csrc/dsac.hip), updates of the learner on a device buffer, in front of a prioritized buffer and as a
member of MultiAgentOffPolicyAlgorithm, the checkpoint round trip and the sampling policy.

References: tests/golden/dsac.npz (the reference's own float64 and float32 runs) and the float64 restatement
(tests/dsac_restatement.py, pinned to those runs to 1e-10 by tests/test_host_dsac.py; it supplies the full arrays of which
the fixture keeps digests).  Bars:
  * zeros of the gradients off the taken action, greedy actions: exact;
  * returns, priorities, gradients, entropies, losses, log_alpha of the heads and of the alpha step: test_gpu_distq.py's
    max |hip - ref64| <= 1e-5 max |ref64| + e_ref per array, e_ref = max |ref32 - ref64| of the reference's own two runs;
  * losses, returns, gradients and weights of full updates, IS weights and tree leaves: test_gpu_dqn.py's `_check`;
  * sampling: Pearson's chi-square of 4096 draws against softmax(logits), below the 0.999 quantile for A - 1 degrees of
    freedom (the draws are a function of the seed, so the statistic is one fixed number).
Every comparison prints `PARITY name: ...` with the ratio to its bar."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "dsac.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")
DEV = "cuda"

from dqn_restatement import nstep_walk  # noqa: E402
from dsac_restatement import actor_head, categorical, critic_head, target  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_gpu_dqn import _check, _d, _ulp_floor  # noqa: E402
from test_host_dqn import _Discrete, _Env, up_inputs  # noqa: E402
from test_host_dsac import ACTS, NETS, STAT_KEYS, head_alpha, head_inputs, up_restatement  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import AutoAlpha, DiscreteSAC, DiscreteSACPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch, PrioritizedVectorReplayBuffer
    from tianshou_marl_amd.data.buffer import DeviceAECReplayBuffer, DeviceVectorReplayBuffer
    from tianshou_marl_amd.utils.net import FlatMLP

B_HEAD = 37


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def gd():
    return dict(np.load(DQN_GOLD))


def _f32(x):
    return _d(np.asarray(x, np.float64), torch.float32)


def _alpha(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _heads(d, alpha, weight=None, act=None):
    """The three heads on the fixture's inputs: the target, then the critic and actor heads on its returns."""
    a = _alpha(alpha)
    ret = ops.dsac_target(_d(d["lnext"]), _d(d["q1n"]), _d(d["q2n"]), a, _f32(d["mc"]), _f32(d["gpow"]), _d(d["vmask"]))
    ch = ops.dsac_critic_head(_d(d["q1"]), _d(d["q2"]), _d(d["act"]) if act is None else act, ret, weight)
    ah = ops.dsac_actor_head(_d(d["logits"]), _d(d["q1"]), _d(d["q2"]), a)
    return ret, ch, ah


# ---- heads --------------------------------------------------------------------------------------------------------------
def test_check_names_the_limits():
    ops.dsac_check(64, 3)
    with pytest.raises(ValueError, match=r"n_act = 65 outside \[1, 64\]"):
        ops.dsac_check(65)
    with pytest.raises(ValueError, match="greater than 0 but got: 0"):
        ops.dsac_check(5, 0)
    with pytest.raises(ValueError, match="must be"):
        ops.dsac_target(torch.zeros(4, 5, device=DEV), torch.zeros(4, 6, device=DEV), torch.zeros(4, 5, device=DEV), _alpha(0.2),
                        torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), torch.zeros(4, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("A", ACTS)
def test_target_matches_reference(g, A):
    d = head_inputs(g, A)
    for auto in (0, 1):
        ret = _heads(d, head_alpha(g, auto))[0].cpu().numpy()
        key = f"tg_A{A}_a{auto}_returns"
        _bar(key, ret, g[key], g[key + "_eref"])
        assert ret[5] == np.float32(d["mc"][5])   # vmask = 0: the Monte-Carlo part alone


@pytest.mark.parametrize("A", ACTS)
def test_critic_and_actor_heads_match_reference(g, A):
    d = head_inputs(g, A)
    B, p = B_HEAD, f"A{A}_"
    slot = torch.zeros(2, 2, device=DEV)
    worst = {}
    for c, case in enumerate(g["hc_cases"]):
        wgt, auto = case[1] == "1", case[3] == "1"
        alpha = head_alpha(g, auto)
        ret64 = target(d["lnext"], d["q1n"], d["q2n"], alpha, d["mc"], d["gpow"], d["vmask"])
        rc = critic_head(d["q1"], d["q2"], d["act"], ret64, d["weight"] if wgt else None)
        ra = actor_head(d["logits"], d["q1"], d["q2"], alpha)
        _, ch, ah = _heads(d, alpha, _d(d["weight"]) if wgt else None)
        ops.qmix_finalize(ch["partial"], B, slot[0])
        ops.qmix_finalize(ah["partial"], B, slot[1])
        for k in ("dq1", "dq2"):
            off = ch[k].cpu().numpy().copy()
            assert off[np.arange(B), d["act"]].all()
            off[np.arange(B), d["act"]] = 0.0
            assert not off.any(), (case, k)   # exactly zero off the taken action
        s64, s32 = g[f"hc_{p}stats"][c], g[f"hc_{p}stats32"][c]
        checks = [("dq1", ch["dq1"].cpu().numpy(), rc["dq1"], g[f"hc_{p}dq_eref"][c]),
                  ("dq2", ch["dq2"].cpu().numpy(), rc["dq2"], g[f"hc_{p}dq_eref"][c]),
                  ("prio", ch["prio"].cpu().numpy(), g[f"hc_{p}prio"][c], g[f"hc_{p}prio_eref"][c]),
                  ("d_logits", ah["d_logits"].cpu().numpy(), ra["d_logits"], g[f"hc_{p}dl_eref"][c]),
                  ("entropy", ah["entropy"].cpu().numpy(), ra["entropy"], g[f"hc_{p}ent_eref"][c]),
                  ("actor_loss", [float(slot[1, 0])], [s64[0]], abs(s32[0] - s64[0])),
                  ("critic1_loss", [float(slot[0, 0])], [s64[1]], abs(s32[1] - s64[1])),
                  ("critic2_loss", [float(slot[0, 1])], [s64[2]], abs(s32[2] - s64[2])),
                  ("mean entropy", [float(slot[1, 1])], [ra["mean_entropy"]], 0.0)]
        if auto:   # AutoAlpha.update from the actor head's entropy partials, on device scalars
            la = torch.full((), float(g["hd_log_alpha"]), device=DEV)
            m, v, t = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
            a_dev, out = _alpha(alpha), torch.zeros(2, device=DEV)
            ops.dsac_alpha_step(ah["partial"], B, la, m, v, t, float(g["hd_target_entropy"]), a_dev, out, lr=float(g["lr"]))
            la64, la32 = g[f"hc_{p}log_alpha"][c]
            checks += [("log_alpha", [float(la)], [la64], abs(la32 - la64)), ("alpha_loss", [float(out[0])], [s64[4]], abs(s32[4] - s64[4])),
                       ("alpha", [float(out[1])], [s64[3]], abs(s32[3] - s64[3]))]
            assert int(t) == 1 and float(a_dev) == float(out[1]) == pytest.approx(float(torch.exp(la)), rel=1e-6)
        for key, got, ref, e in checks:
            worst[key] = max(worst.get(key, 0.0), _bar(f"hc_{p}{case} {key}", got, ref, e))
    print(f"PARITY hc_{p} worst of {len(g['hc_cases'])} cases:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_heads_poison_an_action_outside_the_range_and_repeat_bit_for_bit(g):
    A = 5
    d = head_inputs(g, A)
    act = _d(d["act"]).clone()
    act[4], act[9] = A, -1
    _, ch, _ = _heads(d, 0.25, _d(d["weight"]), act=act)
    bad = torch.zeros(B_HEAD, dtype=torch.bool, device=DEV)
    bad[4] = bad[9] = True
    assert torch.isnan(ch["prio"][bad]).all() and not torch.isnan(ch["prio"][~bad]).any()
    for k in ("dq1", "dq2"):
        assert not ch[k][bad].any() and ch[k][~bad].any() and not torch.isnan(ch[k]).any()
    assert torch.isnan(ch["partial"][0]) and torch.isnan(ch["partial"][1]) and not torch.isnan(ch["partial"][2:]).any()
    d = head_inputs(g, 64)   # the widest rows: every lane carries an action
    (r0, c0, a0), (r1, c1, a1) = (_heads(d, 0.25, _d(d["weight"])) for _ in range(2))
    assert torch.equal(_bits(r0), _bits(r1))
    for x, y in ((c0, c1), (a0, a1)):
        for key in x:
            assert torch.equal(_bits(x[key]), _bits(y[key])), key


def test_alpha_step_follows_the_reference_over_three_steps(g):
    la = torch.zeros((), device=DEV)
    m, v, t = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    a_dev, out = _alpha(1.0), torch.zeros(2, device=DEV)
    for k in range(3):
        pk = f"up_auto_s{k}_"
        part = _d(np.array([0.0, float(g[pk + "mean_entropy"])]))   # one "workgroup" of one row: the reference's mean entropy
        ops.dsac_alpha_step(part, 1, la, m, v, t, float(g["up_target_entropy"]), a_dev, out, lr=float(g["lr"]))
        la64, la32 = g[pk + "log_alpha"]
        s64, s32 = g[pk + "stats"]
        _bar(pk + "log_alpha", [float(la)], [la64], abs(la32 - la64))
        _bar(pk + "alpha", [float(out[1])], [s64[3]], abs(s32[3] - s64[3]))
        _bar(pk + "alpha_loss", [float(out[0])], [s64[4]], abs(s32[4] - s64[4]))
    assert int(t) == 3 and float(a_dev) == float(out[1]) == pytest.approx(float(torch.exp(la)), rel=1e-6)


def test_alpha_step_sums_many_workgroups_in_a_fixed_order():
    """More partial pairs than lanes: the mean entropy over 200 workgroups against a float64 sum, twice with the same bits."""
    rs = np.random.RandomState(6)
    nb, B, target_entropy = 200, 200 * 16 - 5, 1.5
    part = np.stack([rs.standard_normal(nb), 16 * (1.5 + 0.1 * rs.rand(nb))], 1)
    outs = []
    for _ in range(2):
        la = torch.full((), -0.75, device=DEV)
        m, v, t = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        a_dev, out = _alpha(1.0), torch.zeros(2, device=DEV)
        ops.dsac_alpha_step(_d(part.reshape(-1)), B, la, m, v, t, target_entropy, a_dev, out)
        outs.append((out.clone(), la.clone()))
    ref = -(-0.75 * (target_entropy - part[:, 1].sum() / B))
    _bar("alpha step over 200 workgroups: alpha_loss", [float(outs[0][0][0])], [ref], 0.0)
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert float(outs[0][1]) == pytest.approx(-0.75 + 1e-3 * np.sign(target_entropy - part[:, 1].sum() / B), abs=1e-6)   # Adam's first step: lr * sign


# ---- learners -------------------------------------------------------------------------------------------------------------
def _net(init, dims, seed=0):
    net = FlatMLP(list(dims), "relu", device=DEV, seed=seed)
    if init is not None:
        net.flat.data.copy_(_d(np.asarray(init, np.float32)))
    return net


def _algo(init, dims, alpha, seed=0, lr=1e-3, **kw):
    """init: [actor, critic, critic2] flat vectors, or None for seeded nets."""
    nets = [_net(None if init is None else init[i], dims, seed=seed + i) for i in range(3)]
    pol = DiscreteSACPolicy(actor=nets[0], action_space=_Discrete(dims[-1]))
    f = lambda: AdamOptimizerFactory(lr=lr)  # noqa: E731
    return DiscreteSAC(policy=pol, policy_optim=f(), critic=nets[1], critic_optim=f(), critic2=nets[2], alpha=alpha, **kw)


def _auto(target_entropy, lr=1e-3):
    return AutoAlpha(float(target_entropy), 0.0, AdamOptimizerFactory(lr=lr))


def _up_buffer(gd, cls, **kw):
    dims, B, n_env, S, n_step, freq, steps, T, *_ = up_inputs(gd)
    buf = cls(n_env * S, n_env, n_agent=1, obs_dim=dims[0], device=DEV, **kw)
    for t in range(T):
        buf.add(Batch(obs=gd["up_rows_obs"][t][:, None], act=gd["up_rows_act"][t][:, None], rew=gd["up_rows_rew"][t][:, None],
                      terminated=gd["up_rows_term"][t], truncated=gd["up_rows_trunc"][t],
                      obs_next=gd["up_rows_obs_next"][t][:, None]), buffer_ids=np.arange(n_env))
    return buf


def _up_algo(g, gd, kind):
    n_step = up_inputs(gd)[4]
    alpha = float(g["up_fixed"]) if kind == "fix" else _auto(g["up_target_entropy"], float(g["lr"]))
    return _algo(g[f"up_{kind}_init"], [6, 32, 32, 5], alpha, lr=float(g["lr"]), tau=float(g["tau"]), gamma=float(g["gamma"]),
                 n_step_return_horizon=n_step)


def _stats(name, stats, ref):
    """The five statistics of one update against the reference's float64 run, e_ref from its float32 run."""
    s64, s32 = ref
    for i, k in enumerate(STAT_KEYS):
        got = getattr(stats, k)
        if np.isnan(s64[i]):
            assert got is None, (name, k)
        else:
            _check(f"{name}{k}", [got], [s64[i]], abs(s32[i] - s64[i]))


@pytest.mark.parametrize("kind", ["fix", "auto"])
def test_three_updates_match_reference(g, gd, kind):
    _, B, n_env, S, n_step, _, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    algo = _up_algo(g, gd, kind)
    R = up_restatement(g, kind)
    live = {"actor": (algo.policy.actor, "slabs_a"), "critic": (algo.critic, "slabs_c1"), "critic2": (algo.critic2, "slabs_c2")}
    lagged = {"critic_old": (algo.critic_old, "critic"), "critic2_old": (algo.critic2_old, "critic2")}
    lr = float(g["lr"])
    cond = {n: np.zeros(net.flat.numel()) for n, (net, _) in live.items()}
    grad_tol = {}
    for k in range(steps):
        pk = f"up_{kind}_s{k}_"
        idx = g[pk + "indices"]
        batch = algo._preprocess_batch(Batch(), buf, idx)
        stats = algo._update_with_batch(batch)
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        assert np.array_equal(batch.idx_n.cpu().numpy(), idx_n)
        r = R.update(obs[idx], act[idx], obs_next[idx_n], mc, gpow, vmask)
        _stats(pk, stats, g[pk + "stats"])
        ret = batch.returns.cpu().numpy()
        _check(f"{pk}returns", ret, r["returns"], float(g[pk + "returns_eref"]))
        _check(f"{pk}returns (reference entries)", ret[g[pk + "returns_didx"]], g[pk + "returns_dval"], float(g[pk + "returns_eref"]))
        assert batch.returns.shape == (B,) and batch.weight.shape == (B,) and batch.weight.is_cuda   # the new priorities
        extra = {}
        for n, (net, slabs) in live.items():
            grad = algo._ws[B][slabs].double().sum(0).cpu().numpy()
            e = float(g[pk + n + "_grad_eref"])
            _check(f"{pk}{n} grad", grad, r["grads"][n], e)
            grad_tol.setdefault(n, 4.0 * max(e, _ulp_floor(r["grads"][n])))
            cond[n] += R.adam_cond(n)
            extra[n] = np.minimum(cond[n] * grad_tol[n], 2 * lr * (k + 1))
            w_hip = net.flat.double().cpu().numpy()
            _check(f"{pk}{n} weights", w_hip, R.weights(n), float(g[pk + n + "_eref"]), extra[n])
            didx = g[pk + n + "_didx"]
            _check(f"{pk}{n} weights (reference entries)", w_hip[didx], g[pk + n + "_dval"], float(g[pk + n + "_eref"]), extra[n][didx])
        for n, (net, src) in lagged.items():   # the Polyak-lagged copies: a convex mix of weights held to the bars above
            w_hip = net.flat.double().cpu().numpy()
            _check(f"{pk}{n} weights", w_hip, R.weights(n), float(g[pk + n + "_eref"]), extra[src])
            didx = g[pk + n + "_didx"]
            _check(f"{pk}{n} weights (reference entries)", w_hip[didx], g[pk + n + "_dval"], float(g[pk + n + "_eref"]), extra[src][didx])
        if kind == "auto":
            la64, la32 = g[pk + "log_alpha"]
            _check(f"{pk}log_alpha", [float(algo.alpha._log_alpha)], [la64], abs(la32 - la64))
            assert algo.alpha.value == pytest.approx(stats.alpha, rel=1e-6)
    assert algo.policy_optim.step_count == algo.critic_optim.step_count == algo.critic2_optim.step_count == steps


def test_update_through_a_prioritized_buffer_matches_reference(g, gd):
    _, B, n_env, S, *_ = up_inputs(gd)
    buf = _up_buffer(gd, PrioritizedVectorReplayBuffer, alpha=float(g["pr_alpha"]), beta=float(g["pr_beta"]))
    algo = _up_algo(g, gd, "fix")
    for k in range(2):
        pk = f"pr_s{k}_"
        idx = _d(g[pk + "indices"])
        batch = algo._sampled_batch(buf, idx)
        w_in = batch.weight.clone()
        assert w_in.dtype == torch.float32 and w_in.is_cuda
        batch = algo._preprocess_batch(batch, buf, idx)
        stats = algo._update_with_batch(batch)
        assert batch.weight.is_cuda and batch.weight.shape == (B,) and (batch.weight < 0).any()   # signed: the buffer takes |.|
        algo._postprocess_batch(batch, buf, idx)
        _check(f"{pk}IS weights", w_in.cpu().numpy(), g[pk + "weight"], float(g[pk + "weight_eref"]))
        _stats(pk, stats, g[pk + "stats"])
        _check(f"{pk}leaves", buf.weight[np.arange(n_env * S)].cpu().numpy(), g[pk + "leaves"], float(g[pk + "leaves_eref"]))
        _check(f"{pk}max/min prio", buf.prio.cpu().numpy(), g[pk + "prio"], float(g[pk + "prio_eref"]))
    buf.weight.check()
    algo.is_within_training_step = True
    assert np.isfinite(algo.update(buf, 16).actor_loss)    # sampled on the device, end to end


def _ma_algos(g, n_step, seed0=20):
    dims = [int(x) for x in g["ma_dims"]]
    kinds = [str(k) for k in g["ma_kinds"]]
    assert kinds == ["fix", "auto"]
    return [_algo(g["ma_init"][i], dims, float(g["up_fixed"]) if k == "fix" else _auto(g["ma_target_entropy"], float(g["lr"])),
                  seed=seed0 + 3 * i, lr=float(g["lr"]), tau=float(g["tau"]), gamma=float(g["gamma"]), n_step_return_horizon=n_step)
            for i, k in enumerate(kinds)]


def test_multiagent_update_aec_matches_reference(g, gd):
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    env = _Env(N_AG)
    buf = DeviceAECReplayBuffer(n_env * S, n_env, env.agents, obs_dim=D, device=DEV)   # no n_act: the rows carry no masks
    for t in range(T):
        ids = np.array([env.agents[a] for a in gd["ma_turn"][t]], dtype=object)
        nxt = np.array([env.agents[(a + 1) % N_AG] for a in gd["ma_turn"][t]], dtype=object)
        buf.add(Batch(obs=Batch(agent_id=ids, obs=gd["ma_obs"][t]), act=gd["ma_act"][t], rew=gd["ma_rew"][t],
                      terminated=gd["ma_term"][t], truncated=gd["ma_trunc"][t],
                      obs_next=Batch(agent_id=nxt, obs=gd["ma_obs_next"][t])), buffer_ids=np.arange(n_env))
    ours, alone = _ma_algos(g, n_step), _ma_algos(g, n_step)
    ma = MultiAgentOffPolicyAlgorithm(algorithms=ours, env=env)
    ma.is_within_training_step = True
    stats = ma.update(buf, 0).get_loss_stats_dict()
    idx = buf.sample_indices(0)
    who = buf[idx].obs.agent_id
    for k, agent in enumerate(env.agents):
        rows = idx[np.nonzero(who == agent)[0]]
        s = alone[k]._update_with_batch(alone[k]._preprocess_batch(Batch(), buf, rows, agent=k))
        assert stats[f"{agent}/actor_loss"] == s.actor_loss and stats[f"{agent}/critic2_loss"] == s.critic2_loss
        _stats(f"ma {agent} ", s, g["ma_stats"][:, k])
        for (_, a), (_, b) in zip(ours[k]._nets(), alone[k]._nets()):
            assert torch.equal(a.flat.data, b.flat.data)


def test_multiagent_update_joint_lanes():
    rs = np.random.RandomState(8)
    N_AG, E, T, D, A = 2, 4, 6, 5, 3
    buf = DeviceVectorReplayBuffer(E * 8, E, n_agent=N_AG, obs_dim=D, device=DEV)
    for t in range(T):
        buf.add(Batch(obs=rs.randn(E, N_AG, D).astype(np.float32), act=rs.randint(0, A, (E, N_AG)),
                      rew=rs.randn(E, N_AG).astype(np.float32), terminated=rs.rand(E) < 0.2, truncated=rs.rand(E) < 0.1,
                      obs_next=rs.randn(E, N_AG, D).astype(np.float32)))
    mk = lambda: [_algo(None, [D, 16, A], 0.2 if i == 0 else _auto(1.0), seed=20 + 3 * i, n_step_return_horizon=3)  # noqa: E731
                  for i in range(N_AG)]
    ours, alone = mk(), mk()
    ma = MultiAgentOffPolicyAlgorithm(algorithms=ours, env=_Env(N_AG))
    ma.is_within_training_step = True
    stats = ma.update(buf, 0).get_loss_stats_dict()
    idx = buf.sample_indices(0)
    for k in range(N_AG):
        s = alone[k]._update_with_batch(alone[k]._preprocess_batch(Batch(), buf, idx, agent=k))
        assert stats[f"agent_{k}/actor_loss"] == s.actor_loss and np.isfinite(s.actor_loss) and np.isfinite(s.critic1_loss)
        assert torch.equal(ours[k].policy.actor.flat.data, alone[k].policy.actor.flat.data)
    assert "agent_1/alpha_loss" in stats and "agent_0/alpha_loss" not in stats


def test_a_buffer_with_masks_is_refused(gd):
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    env = _Env(N_AG)
    buf = DeviceAECReplayBuffer(n_env * S, n_env, env.agents, obs_dim=D, n_act=A, device=DEV)
    ids = np.array([env.agents[a] for a in gd["ma_turn"][0]], dtype=object)
    buf.add(Batch(obs=Batch(agent_id=ids, obs=gd["ma_obs"][0], mask=gd["ma_mask"][0]), act=gd["ma_act"][0], rew=gd["ma_rew"][0],
                  terminated=gd["ma_term"][0], truncated=gd["ma_trunc"][0], obs_next=Batch(agent_id=ids, obs=gd["ma_obs_next"][0])),
            buffer_ids=np.arange(n_env))
    algo = _algo(None, [D, 16, A], 0.2)
    with pytest.raises(NotImplementedError, match="action masks are not part of the reference's Discrete SAC"):
        algo._preprocess_batch(Batch(), buf, buf.sample_indices(0), agent=0)


def test_reference_state_dict_round_trip(g, gd):
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    algo = _up_algo(g, gd, "auto")
    algo._update_with_batch(algo._preprocess_batch(Batch(), buf, g["up_auto_s0_indices"]))
    sd = algo.to_reference_state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_auto_keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g["sd_auto_shapes"]]
    other = _up_algo(g, gd, "auto")   # the same hyper-parameters (a checkpoint does not carry them), other weights
    for _, net in other._nets():
        net.flat.data.normal_()
    other.load_reference_state_dict(sd)
    for (n, a), (_, b) in zip(other._nets(), algo._nets()):
        assert torch.equal(a.flat.data, b.flat.data), n
    assert torch.equal(other.alpha._log_alpha, algo.alpha._log_alpha) and other.alpha.value == pytest.approx(algo.alpha.value, rel=1e-6)
    assert not torch.equal(algo.critic_old.flat.data, algo.critic.flat.data)   # one Polyak step behind
    # the full checkpoint carries the optimisers and the alpha step as well: both learners then move alike
    other.load_state_dict(algo.state_dict())
    idx = g["up_auto_s1_indices"]
    s0 = algo._update_with_batch(algo._preprocess_batch(Batch(), buf, idx))
    s1 = other._update_with_batch(other._preprocess_batch(Batch(), buf, idx))
    assert s0 == s1
    for (n, a), (_, b) in zip(other._nets(), algo._nets()):
        assert torch.equal(a.flat.data, b.flat.data), n


# ---- acting -----------------------------------------------------------------------------------------------------------------
CHI2_Q999 = {4: 18.466826952903}   # the 0.999 quantile of chi-square with A - 1 = 4 degrees of freedom


def test_act_device_samples_softmax_within_a_training_step_and_takes_the_mode_outside():
    R, A, D = 4096, 5, 4
    net = FlatMLP([D, A], "relu", device=DEV, seed=3)
    pol = DiscreteSACPolicy(actor=net, action_space=_Discrete(A), seed=11)
    obs = torch.full((R, D), 0.5, device=DEV)                        # one fixed observation: one fixed logit row
    obs_varied = _d(np.random.RandomState(4).standard_normal((130, D)).astype(np.float32))
    logits = FlatMLP.forward(net, obs_varied, save=False).double().cpu().numpy()
    res = pol.act_device(obs_varied)                                  # outside a training step: the argmax
    assert np.array_equal(res["act"].cpu().numpy(), logits.argmax(1)) and res["act"].dtype == torch.int32
    assert not res["value"].any() and pol._sample_ctr == 130
    _bar("act_device logp (mode)", res["logp"].cpu().numpy(), categorical(logits)[1][np.arange(130), logits.argmax(1)], 0.0)
    out = pol(Batch(obs=obs_varied.cpu().numpy(), info=Batch()))
    assert np.array_equal(out.act, logits.argmax(1)) and out.act.dtype == np.int64 and out.logits.shape == (130, A)
    assert pol._sample_ctr == 260   # both acting paths give every row a counter, drawn from or not
    pol.is_within_training_step = True
    res = pol.act_device(obs)
    act = res["act"].cpu().numpy()
    row = FlatMLP.forward(net, obs[:1], save=False).double().cpu().numpy()
    p, ln, _ = categorical(row)
    counts = np.bincount(act, minlength=A).astype(np.float64)
    stat = float(((counts - R * p[0]) ** 2 / (R * p[0])).sum())
    print(f"PARITY act_device chi-square over {R} draws: {stat:.4g} against the 0.999 quantile {CHI2_Q999[A - 1]:.4g}; counts {counts}")
    assert counts.sum() == R and (counts > 0).all() and stat <= CHI2_Q999[A - 1]
    _bar("act_device logp (sample)", res["logp"].cpu().numpy(), ln[0][act], 0.0)
    again = DiscreteSACPolicy(actor=net, action_space=_Discrete(A), seed=11)
    again.is_within_training_step = True
    again._sample_ctr = 260
    halves = torch.cat([again.act_device(obs[:1000])["act"], again.act_device(obs[1000:])["act"]])
    assert torch.equal(halves, res["act"])                            # the draws are a function of (seed, counter)
    stochastic = DiscreteSACPolicy(actor=net, deterministic_eval=False, action_space=_Discrete(A), seed=11)
    assert len(np.unique(stochastic.act_device(obs)["act"].cpu().numpy())) > 1   # no deterministic_eval: sampling everywhere
    with pytest.raises(NotImplementedError, match="action masks"):
        pol.act_device(obs, mask=torch.ones(R, A, dtype=torch.bool, device=DEV))
