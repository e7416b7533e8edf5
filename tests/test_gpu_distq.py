"""GPU tests (`-m gpu`) of C51 and QR-DQN: tsm_distq_values, tsm_c51_head and tsm_qrdqn_head (csrc/distq.hip), updates of
both learners on a device buffer, in front of a prioritized buffer, and as members of MultiAgentOffPolicyAlgorithm.

References: tests/golden/distq.npz (the reference's own float64 and float32 runs) and the float64 restatement
(tests/distq_restatement.py, pinned to those runs to 1e-10 by tests/test_host_distq.py; it supplies the full arrays of which
the fixture keeps digests).  Bars:
  * a*, actions, zeros of the gradient off the taken action: exact;
  * values, probabilities, returns, priorities, gradients and losses of the heads:
    max |hip - ref64| <= 1e-5 max |ref64| + e_ref per array, e_ref = max |ref32 - ref64| of the reference's own two runs
    (the project's 1e-5 relative bar on the array's scale, plus what float32 costs the reference itself);
  * losses, returns, gradients and weights of full updates, IS weights and tree leaves: test_gpu_dqn.py's `_check`.
Every comparison prints `PARITY name: ...` with the ratio to its bar."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "distq.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")
DEV = "cuda"

from distq_restatement import DistqRestatement, c51_head, dist_values, qr_head, support_of, tau_hat_of  # noqa: E402
from dqn_restatement import nstep_walk  # noqa: E402
from test_gpu_dqn import _check, _d, _ulp_floor  # noqa: E402
from test_host_distq import GRID, head_inputs, up_rows  # noqa: E402
from test_host_dqn import _Discrete, _Env, up_inputs  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import C51, QRDQN, C51Policy, QRDQNPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch, PrioritizedVectorReplayBuffer
    from tianshou_marl_amd.data.buffer import DeviceAECReplayBuffer, DeviceVectorReplayBuffer
    from tianshou_marl_amd.utils.net import FlatMLP


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def gd():
    return dict(np.load(DQN_GOLD))


def _bar(name, got, ref, e_ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = 1e-5 * max(float(np.abs(ref).max()), float(np.finfo(np.float32).tiny)) + float(e_ref)
    ratio = float(np.abs(got - ref).max()) / tol
    print(f"PARITY {name}: max |hip - ref64| / (1e-5 max |ref64| + e_ref) = {ratio:.3g}")
    assert ratio <= 1.0, (name, ratio)   # a NaN ratio fails too
    return ratio


def _consts(kind, N):
    return _d(support_of(-10.0, 10.0, N), torch.float32) if kind == "c5" else _d(tau_hat_of(N), torch.float32)


def _head(kind, d, A, N, tgt, wgt, msk, act=None):
    """One launch of the head under test on the fixture's inputs."""
    raw, on, tg = _d(d["raw"]), _d(d["on"]), _d(d["tg"])
    q_next = ops.distq_values(on, A, N, support=_consts("c5", N) if kind == "c5" else None)
    args = (raw, q_next, tg if tgt else on, _d(d["act"]) if act is None else act, _d(d["mc"], torch.float32),
            _d(d["gpow"], torch.float32), _d(d["vmask"]))
    kw = dict(mask_next=_d(d["mask"]) if msk else None, weight=_d(d["weight"]) if wgt else None)
    if kind == "c5":
        return ops.c51_head(*args, _consts(kind, N), -10.0, 10.0, **kw)
    return ops.qrdqn_head(*args, _consts(kind, N), **kw)


# ---- values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N", GRID)
def test_values_and_greedy_actions_match_reference(g, A, N):
    d = head_inputs(g, A, N)
    on, mask, eps0 = _d(d["on"]), _d(d["mask"]), torch.zeros(1, device=DEV)
    for kind, sup in (("c51", support_of(-10.0, 10.0, N)), ("qr", None)):
        p = f"dv_A{A}_N{N}_{kind}_"
        if sup is None:
            q = ops.distq_values(on, A, N)
        else:
            q, probs = ops.distq_values(on, A, N, support=_d(sup, torch.float32), want_probs=True)
            ref = dist_values(d["on"], A, N, sup)["probs"]
            _bar(p + "probs", probs.cpu().numpy(), ref, 0.0)
            assert probs.shape == (37, A, N)
        _bar(p + "q", q.cpu().numpy(), g[p + "q"], g[p + "q_eref"])
        assert np.array_equal(ops.dqn_egreedy(q, eps0, 0).cpu().numpy(), g[p + "act"])
        assert np.array_equal(ops.dqn_egreedy(q, eps0, 0, mask=mask).cpu().numpy(), g[p + "act_masked"])


# ---- heads --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N", GRID)
@pytest.mark.parametrize("kind", ["c5", "qr"])
def test_head_matches_reference(g, kind, A, N):
    d = head_inputs(g, A, N)
    B = 37
    p = f"{kind}_A{A}_N{N}_"
    extra = (support_of(-10.0, 10.0, N), -10.0, 10.0) if kind == "c5" else (tau_hat_of(N),)
    fn = c51_head if kind == "c5" else qr_head
    slot = torch.zeros(2, device=DEV)
    worst = {}
    for c, case in enumerate(g["cases"]):
        tgt, wgt, msk = (case[i] == "1" for i in (1, 3, 5))
        r = fn(d["raw"], d["on"], d["tg"] if tgt else None, d["mask"] if msk else None, d["act"], d["mc"], d["gpow"], d["vmask"],
               d["weight"] if wgt else None, *extra, A, N)
        assert np.array_equal(r["a_star"], g[p + "astar"][c])
        h = _head(kind, d, A, N, tgt, wgt, msk)
        ops.qmix_finalize(h["partial"], B, slot)
        dout = h["d_out"].cpu().numpy().reshape(B, A, N)
        off = dout.copy()
        off[np.arange(B), d["act"]] = 0.0
        assert not off.any(), case   # exactly zero off the taken action
        # a* itself: the rows of the next distribution it selects show in the returns (QR-DQN) and the priorities (both)
        for key, got, ref, e in (("returns", h["returns"].cpu().numpy(), r["returns"], g[p + "ret_eref"][c]),
                                 ("prio", h["prio"].cpu().numpy(), g[p + "prio"][c], g[p + "prio_eref"][c]),
                                 ("d_out", dout, r["d_out"].reshape(B, A, N), g[p + "dout_eref"][c]),
                                 ("loss", [float(slot[0])], [g[p + "loss"][c, 0]], abs(g[p + "loss"][c, 1] - g[p + "loss"][c, 0]))):
            worst[key] = max(worst.get(key, 0.0), _bar(f"{p}{case} {key}", got, ref, e))
        # the second statistic: a mean over the rows, held to 1e-5 of the scale of the values it averages
        assert abs(float(slot[1]) - r["q_taken"].mean()) <= 1e-5 * np.abs(r["q_taken"]).max(), case
    print(f"PARITY {p} worst of {len(g['cases'])} cases:", {k: f"{v:.3g}" for k, v in worst.items()})


@pytest.mark.parametrize("kind", ["c5", "qr"])
def test_head_poisons_an_action_outside_the_range_and_repeats_bit_for_bit(g, kind):
    A, N = 5, 51
    d = head_inputs(g, A, N)
    act = _d(d["act"]).clone()
    act[4], act[9] = A, -1
    h = _head(kind, d, A, N, True, True, True, act=act)
    bad = torch.zeros(37, dtype=torch.bool, device=DEV)
    bad[4] = bad[9] = True
    assert torch.isnan(h["prio"][bad]).all() and not torch.isnan(h["prio"][~bad]).any()
    assert not h["d_out"][bad].any() and h["d_out"][~bad].any() and torch.isnan(h["partial"][0])
    d = head_inputs(g, 5, 200)   # the widest rows: every lane carries several atoms
    a, b = (_head(kind, d, 5, 200, True, True, True) for _ in range(2))
    for key in ("returns", "prio", "d_out", "partial"):
        assert torch.equal(a[key].view(torch.int64 if a[key].dtype == torch.float64 else torch.int32),
                           b[key].view(torch.int64 if b[key].dtype == torch.float64 else torch.int32)), key


# ---- learners -------------------------------------------------------------------------------------------------------------
def _algo(kind, init, dims, A, N, seed=0, **kw):
    net = FlatMLP(list(dims), "relu", device=DEV, seed=seed)
    if init is not None:
        net.flat.data.copy_(_d(np.asarray(init, np.float32)))
    if kind == "c51":
        pol = C51Policy(model=net, action_space=_Discrete(A), num_atoms=N)
        return C51(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), **kw)
    pol = QRDQNPolicy(model=net, action_space=_Discrete(A), num_quantiles=N)
    return QRDQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), num_quantiles=N, **kw)


def _up_buffer(gd, cls, **kw):
    dims, B, n_env, S, n_step, freq, steps, T, *_ = up_inputs(gd)
    buf = cls(n_env * S, n_env, n_agent=1, obs_dim=dims[0], device=DEV, **kw)
    for t in range(T):
        buf.add(Batch(obs=gd["up_rows_obs"][t][:, None], act=gd["up_rows_act"][t][:, None], rew=gd["up_rows_rew"][t][:, None],
                      terminated=gd["up_rows_term"][t], truncated=gd["up_rows_trunc"][t],
                      obs_next=gd["up_rows_obs_next"][t][:, None]), buffer_ids=np.arange(n_env))
    return buf


def _up_algo(g, gd, kind):
    _, B, n_env, S, n_step, freq, *_ = up_inputs(gd)
    d = [int(x) for x in g[f"up_{kind}_dims"]]
    return _algo(kind, g[f"up_{kind}_init"], d[:4], d[4], d[5], gamma=float(g["gamma"]), n_step_return_horizon=n_step,
                 target_update_freq=freq), d[:4], d[4], d[5]


@pytest.mark.parametrize("kind", ["c51", "qr"])
def test_three_updates_match_reference(g, gd, kind):
    _, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    algo, dims, A, N = _up_algo(g, gd, kind)
    R = DistqRestatement(g[f"up_{kind}_init"], dims, kind, A, N, target_update_freq=freq)
    lr, cond, grad_tol = 1e-3, np.zeros(algo.policy.model.flat.numel()), None
    for k in range(steps):
        pk = f"up_{kind}_s{k}_"
        idx = g[pk + "indices"]
        batch = algo._preprocess_batch(Batch(), buf, idx)
        w_before = algo.policy.model.flat.data.clone()
        stats = algo._update_with_batch(batch)
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        assert np.array_equal(batch.idx_n.cpu().numpy(), idx_n)
        r = R.update(obs[idx], act[idx], up_rows(gd, kind, idx, idx_n, obs_next), None, mc, gpow, vmask)
        cond += R.adam_cond()
        ref64, ref32 = (float(x) for x in g[pk + "loss"])
        loss = stats.get_loss_stats_dict()["loss"]
        _check(f"{pk}loss", [loss], [ref64], abs(ref32 - ref64))
        _check(f"{pk}returns", batch.returns.cpu().numpy().reshape(-1), r["returns"].reshape(-1), float(g[pk + "returns_eref"]))
        didx = g[pk + "returns_didx"]   # ... and the entries of the reference's own float64 returns that the fixture keeps
        _check(f"{pk}returns (reference entries)", batch.returns.cpu().numpy().reshape(-1)[didx], g[pk + "returns_dval"],
               float(g[pk + "returns_eref"]))
        assert batch.returns.shape == (B, N) and batch.weight.shape == (B,) and batch.weight.is_cuda   # the new priorities
        grad = algo._ws[B]["slabs"].double().sum(0).cpu().numpy()
        e = float(g[pk + "grad_eref"])
        _check(f"{pk}grad", grad, r["grads"], e)
        if grad_tol is None:
            grad_tol = 4.0 * max(e, _ulp_floor(r["grads"]))
        extra = np.minimum(cond * grad_tol, 2 * lr * (k + 1))
        w_hip = algo.policy.model.flat.double().cpu().numpy()
        _check(f"{pk}weights", w_hip, R.weights(), float(g[pk + "weights_eref"]), extra)
        didx = g[pk + "weights_didx"]
        _check(f"{pk}weights (reference entries)", w_hip[didx], g[pk + "weights_dval"], float(g[pk + "weights_eref"]), extra[didx])
        if k % freq == 0:   # the lagged copy: the weights BEFORE the step of calls 0, 2, ...
            assert torch.equal(algo.target_flat, w_before), k
        tidx = g[pk + "targets_didx"]
        _check(f"{pk}targets (reference entries)", algo.target_flat.double().cpu().numpy()[tidx], g[pk + "targets_dval"],
               float(g[pk + "weights_eref"]), extra[tidx])
    assert algo._iter == steps


@pytest.mark.parametrize("kind", ["c51", "qr"])
def test_update_through_a_prioritized_buffer_matches_reference(g, gd, kind):
    _, B, n_env, S, *_ = up_inputs(gd)
    buf = _up_buffer(gd, PrioritizedVectorReplayBuffer, alpha=float(g["pr_alpha"]), beta=float(g["pr_beta"]))
    algo, *_ = _up_algo(g, gd, kind)
    for k in range(2):
        pk = f"pr_{kind}_s{k}_"
        idx = _d(g[pk + "indices"])
        batch = algo._sampled_batch(buf, idx)
        w_in = batch.weight.clone()
        assert w_in.dtype == torch.float32 and w_in.is_cuda
        batch = algo._preprocess_batch(batch, buf, idx)
        stats = algo._update_with_batch(batch)
        assert batch.weight.is_cuda and batch.weight.shape == (B,) and (batch.weight >= 0).all()
        algo._postprocess_batch(batch, buf, idx)
        ref64, ref32 = (float(x) for x in g[pk + "loss"])
        _check(f"{pk}IS weights", w_in.cpu().numpy(), g[pk + "weight"], float(g[pk + "weight_eref"]))
        _check(f"{pk}loss", [stats.get_loss_stats_dict()["loss"]], [ref64], abs(ref32 - ref64))
        _check(f"{pk}leaves", buf.weight[np.arange(n_env * S)].cpu().numpy(), g[pk + "leaves"], float(g[pk + "leaves_eref"]))
        _check(f"{pk}max/min prio", buf.prio.cpu().numpy(), g[pk + "prio"], float(g[pk + "prio_eref"]))
    buf.weight.check()
    algo.is_within_training_step = True
    assert np.isfinite(algo.update(buf, 16).get_loss_stats_dict()["loss"])    # sampled on the device, end to end


def test_multiagent_update_aec_matches_reference(g, gd):
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    d = [int(x) for x in g["ma_dims"]]
    dims, NA = d[:3], d[4]
    kinds = [str(k) for k in g["ma_kinds"]]
    assert kinds == ["c51", "qr"] and d[3] == A
    env = _Env(N_AG)
    buf = DeviceAECReplayBuffer(n_env * S, n_env, env.agents, obs_dim=D, n_act=A, device=DEV)
    for t in range(T):
        ids = np.array([env.agents[a] for a in gd["ma_turn"][t]], dtype=object)
        nxt = np.array([env.agents[(a + 1) % N_AG] for a in gd["ma_turn"][t]], dtype=object)
        buf.add(Batch(obs=Batch(agent_id=ids, obs=gd["ma_obs"][t], mask=gd["ma_mask"][t]), act=gd["ma_act"][t], rew=gd["ma_rew"][t],
                      terminated=gd["ma_term"][t], truncated=gd["ma_trunc"][t],
                      obs_next=Batch(agent_id=nxt, obs=gd["ma_obs_next"][t])), buffer_ids=np.arange(n_env))
    kw = dict(gamma=float(g["gamma"]), n_step_return_horizon=n_step, target_update_freq=3)
    mk = lambda: [_algo(k, g["ma_init"][i], dims, A, NA, seed=20 + i, **kw) for i, k in enumerate(kinds)]  # noqa: E731
    ours, alone = mk(), mk()
    ma = MultiAgentOffPolicyAlgorithm(algorithms=ours, env=env)
    ma.is_within_training_step = True
    stats = ma.update(buf, 0).get_loss_stats_dict()
    idx = buf.sample_indices(0)
    who = buf[idx].obs.agent_id
    for k, agent in enumerate(env.agents):
        rows = idx[np.nonzero(who == agent)[0]]
        s = alone[k]._update_with_batch(alone[k]._preprocess_batch(Batch(), buf, rows, agent=k)).get_loss_stats_dict()["loss"]
        assert stats[f"{agent}/loss"] == s
        ref64, ref32 = float(g["ma_loss"][0, k]), float(g["ma_loss"][1, k])
        _check(f"ma {agent} ({kinds[k]}) loss", [s], [ref64], abs(ref32 - ref64))
        assert torch.equal(ours[k].policy.model.flat.data, alone[k].policy.model.flat.data)


def test_multiagent_update_joint_lanes():
    rs = np.random.RandomState(8)
    N_AG, E, T, D, A, NA = 2, 4, 6, 5, 3, 8
    buf = DeviceVectorReplayBuffer(E * 8, E, n_agent=N_AG, obs_dim=D, device=DEV)
    for t in range(T):
        buf.add(Batch(obs=rs.randn(E, N_AG, D).astype(np.float32), act=rs.randint(0, A, (E, N_AG)),
                      rew=rs.randn(E, N_AG).astype(np.float32), terminated=rs.rand(E) < 0.2, truncated=rs.rand(E) < 0.1,
                      obs_next=rs.randn(E, N_AG, D).astype(np.float32)))
    kw = dict(n_step_return_horizon=3, target_update_freq=2)
    mk = lambda: [_algo(k, None, [D, 16, A * NA], A, NA, seed=20 + i, **kw) for i, k in enumerate(("c51", "qr"))]  # noqa: E731
    ours, alone = mk(), mk()
    ma = MultiAgentOffPolicyAlgorithm(algorithms=ours, env=_Env(N_AG))
    ma.is_within_training_step = True
    stats = ma.update(buf, 0).get_loss_stats_dict()
    idx = buf.sample_indices(0)
    for k in range(N_AG):
        s = alone[k]._update_with_batch(alone[k]._preprocess_batch(Batch(), buf, idx, agent=k)).get_loss_stats_dict()["loss"]
        assert stats[f"agent_{k}/loss"] == s and np.isfinite(s)
        assert torch.equal(ours[k].policy.model.flat.data, alone[k].policy.model.flat.data)


# ---- acting ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c51", "qr"])
def test_policy_forward_and_act_device_honour_the_mask(kind):
    rs = np.random.RandomState(4)
    R, A, N = 130, 5, 11
    mask = np.zeros((R, A), bool)
    for r in range(R):
        mask[r, rs.choice(A, 1 + r % 4, replace=False)] = True
    net = FlatMLP([4, 16, A * N], "relu", device=DEV, seed=3)
    cls, kw = (C51Policy, dict(num_atoms=N)) if kind == "c51" else (QRDQNPolicy, dict(num_quantiles=N))
    pol = cls(model=net, action_space=_Discrete(A), eps_training=1.0, eps_inference=0.0, seed=11, **kw)
    obs = rs.standard_normal((R, 4)).astype(np.float32)
    out = pol(Batch(obs=Batch(obs=obs, mask=mask), info=Batch()))
    assert out.logits.shape == (R, A, N) and out.act.dtype == np.int64
    logits = out.logits.double().cpu().numpy()
    if kind == "c51":
        np.testing.assert_allclose(logits.sum(2), 1.0, rtol=1e-5)
        q = (logits * pol.support.double().cpu().numpy()).sum(2)
    else:
        q = logits.mean(2)
    assert np.array_equal(out.act, np.where(mask, q, -np.inf).argmax(1))
    raw = FlatMLP.forward(net, _d(obs), save=False)
    assert np.array_equal(out.act, pol.compute_q_value(raw, mask).argmax(1).cpu().numpy())
    assert np.array_equal(pol(Batch(obs=obs, info=Batch())).act, q.argmax(1))
    res = pol.act_device(_d(obs), mask=_d(mask))                       # epsilon 0: the greedy action of forward
    assert np.array_equal(res["act"].cpu().numpy(), out.act) and pol._sample_ctr == R
    assert np.array_equal(pol.act_device(_d(obs))["act"].cpu().numpy(), q.argmax(1))
    pol.is_within_training_step = True                                  # epsilon 1: legal random actions
    a1 = pol.act_device(_d(obs), mask=_d(mask))["act"].cpu().numpy()
    assert mask[np.arange(R), a1].all() and not np.array_equal(a1, out.act)
