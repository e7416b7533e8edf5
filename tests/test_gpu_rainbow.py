"""GPU tests (`-m gpu`) of Rainbow: `RainbowNet` forward and backward in both modes, updates of `RainbowDQN` on a device
buffer, in front of a prioritized buffer and as members of MultiAgentOffPolicyAlgorithm, and the learner's behaviour around its
noise (csrc/rainbow.hip around csrc/dense.hip and csrc/distq.hip).

References: tests/golden/rainbow.npz (the reference's own float64 and float32 runs, its noise stored as data) and the float64
restatement (tests/rainbow_restatement.py, pinned to those runs to 1e-10 by tests/test_host_rainbow.py; it supplies the full
arrays of which the fixture keeps digests).  Bars:
  * actions, structural zeros, noise bits, bit-for-bit equalities: exact;
  * outputs and gradients of the net: max |hip - ref64| <= 1e-5 max |ref64| + e_ref per array, e_ref = max |ref32 - ref64| of the
    reference's own two runs;
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
GOLD = os.path.join(HERE, "golden", "rainbow.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")
DEV = "cuda"

from dqn_restatement import nstep_walk  # noqa: E402
from rainbow_restatement import RainbowNetRestatement, RainbowRestatement  # noqa: E402
from test_gpu_distq import _bar, _up_buffer  # noqa: E402
from test_gpu_dqn import _check, _d, _ulp_floor  # noqa: E402
from test_host_dqn import _Discrete, _Env, up_inputs  # noqa: E402
from test_host_rainbow import net_case, up_case  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd.algorithm import C51, C51Policy, RainbowDQN, RainbowPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch, PrioritizedVectorReplayBuffer
    from tianshou_marl_amd.data.buffer import DeviceAECReplayBuffer, DeviceVectorReplayBuffer
    from tianshou_marl_amd.utils.net import FlatMLP, RainbowNet


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def gd():
    return dict(np.load(DQN_GOLD))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _net(kw, init=None, seed=0, **more):
    net = RainbowNet(device=DEV, seed=seed, **{**kw, **more})
    if init is not None:
        net.flat.data.copy_(_d(np.asarray(init, np.float32)))
    return net


def _algo(kw, init, seed=0, policy_kw=None, **akw):
    net = _net(kw, init, seed=seed)
    pol = RainbowPolicy(model=net, action_space=_Discrete(kw["n_act"]), num_atoms=kw["num_atoms"], seed=seed, **(policy_kw or {}))
    return RainbowDQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), **akw)


# ---- the net ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nl", "du"])
def test_net_forward_and_backward_match_reference(g, tag):
    R, kw = net_case(g, tag)
    net = _net(kw, g[f"{tag}_init"])
    x, d = _d(g[f"{tag}_x"]), _d(g[f"{tag}_d"])
    for mode, training in (("train", True), ("eval", False)):
        net.train(training)
        y_ref, cache = R.forward(g[f"{tag}_init"], g[f"{tag}_x"], training)
        g_ref = R.backward(cache, g[f"{tag}_d"])
        for n_split in (1, 3):
            y = net.forward(x, save=True)
            slabs = net.backward(d, n_split)
            assert y.shape == (x.shape[0], R.A * R.N) and slabs.shape == (n_split, R.P)
            _bar(f"{tag} {mode} out", y.cpu().numpy(), y_ref, g[f"{tag}_{mode}_out_eref"])
            grad = slabs.double().sum(0).cpu().numpy()
            _bar(f"{tag} {mode} grad (n_split {n_split})", grad, g_ref, g[f"{tag}_{mode}_grad_eref"])
            didx = g[f"{tag}_{mode}_grad_didx"]    # ... and the entries of the reference's own float64 gradient the fixture keeps
            _bar(f"{tag} {mode} grad (reference entries)", grad[didx], g[f"{tag}_{mode}_grad_dval"], g[f"{tag}_{mode}_grad_eref"])
            for v in net.layer_views(slabs[n_split - 1]):
                assert not _bits(v["eps_p"]).any() and not _bits(v["eps_q"]).any()           # +0.0 bit for bit
                assert training or not (v["sigma_W"].any() or v["sigma_bias"].any())
    net.forward(x, save=True)
    net.forward(x, save=False)
    with pytest.raises(RuntimeError, match="must follow its forward"):
        net.backward(d)


def test_other_net_forms_match_the_restatement(g):
    rs = np.random.RandomState(6)
    x = rs.standard_normal((37, 6)).astype(np.float32)
    for name, kw in (("dueling=False", dict(hidden_sizes=(32,), dueling=False)), ("noisy_std=None", dict(hidden_sizes=(32,), noisy_std=None)),
                     ("empty q_hidden / v_hidden", dict(hidden_sizes=(16, 24))),
                     ("q_hidden only", dict(hidden_sizes=(16,), q_hidden=(8, 12)))):
        kw = dict(obs_dim=6, n_act=3, num_atoms=11, **kw)
        net = _net(kw, seed=4)
        R = RainbowNetRestatement(6, kw["hidden_sizes"], 3, 11, kw.get("q_hidden", ()), kw.get("v_hidden", ()), kw.get("dueling", True),
                                  kw.get("noisy_std", 0.5) is not None)
        flat = net.flat.data.double().cpu().numpy()
        d = (rs.standard_normal((37, 33)) / 37).astype(np.float32)
        for training in (True, False):
            net.train(training)
            y_ref, cache = R.forward(flat, x, training)
            # what float32 costs a torch run of the same lines is not recorded for these forms: the bar is the plain 1e-5 one
            _bar(f"{name} train={training} out", net.forward(_d(x)).cpu().numpy(), y_ref, 0.0)
            _bar(f"{name} train={training} grad", net.backward(_d(d), 2).double().sum(0).cpu().numpy(), R.backward(cache, d), 0.0)


def test_noise_free_chain_equals_a_flat_mlp_bit_for_bit():
    dims = [6, 32, 24, 55]
    mlp = FlatMLP(dims, "relu", device=DEV, seed=9)
    net = RainbowNet(6, (32, 24), 5, 11, dueling=False, noisy_std=None, device=DEV, seed=1)
    net.flat.data.copy_(mlp.flat.data)
    rs = np.random.RandomState(2)
    x, d = _d(rs.standard_normal((300, 6)).astype(np.float32)), _d(rs.standard_normal((300, 55)).astype(np.float32))
    assert torch.equal(_bits(net.forward(x)), _bits(mlp.forward(x)))
    a, b = net.backward(d, 2), mlp.backward(d, 2)
    assert torch.equal(_bits(a), _bits(b))


# ---- learners -------------------------------------------------------------------------------------------------------------
def _up_algo(g, gd, **more):
    _, B, n_env, S, n_step, freq, *_ = up_inputs(gd)
    R, kw = up_case(g)
    return _algo(kw, g["up_init"], gamma=float(g["gamma"]), n_step_return_horizon=n_step, target_update_freq=freq, **more), R


def test_three_updates_match_reference(g, gd):
    _, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    algo, R = _up_algo(g, gd)
    net, eps = algo.policy.model, g["up_eps"]
    RS = RainbowRestatement(g["up_init"], R, target_update_freq=freq)
    lr, cond, grad_tol = 1e-3, np.zeros(R.P), None
    for k in range(steps):
        pk = f"up_s{k}_"
        idx = g[pk + "indices"]
        batch = algo._preprocess_batch(Batch(), buf, idx)
        algo.noise_feed = [eps[k, 0], eps[k, 1]]
        stats = algo._update_with_batch(batch)
        assert not algo.noise_feed and algo._noise_ctr == 2 * (k + 1)
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        assert np.array_equal(batch.idx_n.cpu().numpy(), idx_n)
        r = RS.update(obs[idx], act[idx], obs_next[idx], None, mc, gpow, vmask, eps_online=eps[k, 0], eps_target=eps[k, 1])
        cond += RS.adam_cond()
        ref64, ref32 = (float(x) for x in g[pk + "loss"])
        _check(f"{pk}loss", [stats.get_loss_stats_dict()["loss"]], [ref64], abs(ref32 - ref64))
        _check(f"{pk}returns", batch.returns.cpu().numpy().reshape(-1), r["returns"].reshape(-1), float(g[pk + "returns_eref"]))
        assert batch.returns.shape == (B, R.N) and batch.weight.shape == (B,) and batch.weight.is_cuda
        grad = algo._ws[B]["slabs"].double().sum(0).cpu().numpy()
        e = float(g[pk + "grad_eref"])
        _check(f"{pk}grad", grad, r["grads"], e)
        didx = g[pk + "grad_didx"]
        _check(f"{pk}grad (reference entries)", grad[didx], g[pk + "grad_dval"], e)
        if grad_tol is None:
            grad_tol = 4.0 * max(e, _ulp_floor(r["grads"]))
        extra = np.minimum(cond * grad_tol, 2 * lr * (k + 1))
        w_hip = net.flat.double().cpu().numpy()
        _check(f"{pk}weights", w_hip, RS.weights(), float(g[pk + "weights_eref"]), extra)
        didx = g[pk + "weights_didx"]
        _check(f"{pk}weights (reference entries)", w_hip[didx], g[pk + "weights_dval"], float(g[pk + "weights_eref"]), extra[didx])
        t_hip = algo.target_flat.double().cpu().numpy()
        _check(f"{pk}targets", t_hip, RS.targets(), float(g[pk + "weights_eref"]), extra)
        tidx = g[pk + "targets_didx"]
        _check(f"{pk}targets (reference entries)", t_hip[tidx], g[pk + "targets_dval"], float(g[pk + "weights_eref"]), extra[tidx])
        # quirk Q40: the copy follows the draw and takes the noise along; the Adam step leaves the noise bits alone
        assert torch.equal(_bits(net.noise()), _bits(_d(eps[k, 0])))
        same = torch.equal(_bits(algo.model_old.noise()), _bits(net.noise()))
        assert same == (k % freq == 0), k
        if k % freq != 0:
            assert torch.equal(_bits(algo.model_old.noise()), _bits(_d(eps[k, 1])))
    assert algo._iter == steps


def test_update_through_a_prioritized_buffer_matches_reference(g, gd):
    _, B, n_env, S, *_ = up_inputs(gd)
    buf = _up_buffer(gd, PrioritizedVectorReplayBuffer, alpha=float(g["pr_alpha"]), beta=float(g["pr_beta"]))
    algo, _ = _up_algo(g, gd)
    for k in range(2):
        pk = f"pr_s{k}_"
        idx = _d(g[pk + "indices"])
        batch = algo._sampled_batch(buf, idx)
        w_in = batch.weight.clone()
        batch = algo._preprocess_batch(batch, buf, idx)
        algo.noise_feed = [g["pr_eps"][k, 0], g["pr_eps"][k, 1]]
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
    assert np.isfinite(algo.update(buf, 16).get_loss_stats_dict()["loss"])    # sampled and drawn on the device, end to end


def test_multiagent_update_aec_matches_reference(g, gd):
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    d = [int(x) for x in g["ma_dims"]]
    assert d[0] == D and d[2] == A
    kw = dict(obs_dim=D, hidden_sizes=(d[1],), n_act=A, num_atoms=d[3])
    env = _Env(N_AG)
    buf = DeviceAECReplayBuffer(n_env * S, n_env, env.agents, obs_dim=D, n_act=A, device=DEV)
    for t in range(T):
        ids = np.array([env.agents[a] for a in gd["ma_turn"][t]], dtype=object)
        nxt = np.array([env.agents[(a + 1) % N_AG] for a in gd["ma_turn"][t]], dtype=object)
        buf.add(Batch(obs=Batch(agent_id=ids, obs=gd["ma_obs"][t], mask=gd["ma_mask"][t]), act=gd["ma_act"][t], rew=gd["ma_rew"][t],
                      terminated=gd["ma_term"][t], truncated=gd["ma_trunc"][t],
                      obs_next=Batch(agent_id=nxt, obs=gd["ma_obs_next"][t])), buffer_ids=np.arange(n_env))
    akw = dict(gamma=float(g["gamma"]), n_step_return_horizon=n_step, target_update_freq=3)

    def mk():
        algos = [_algo(kw, g["ma_init"][i], seed=20 + i, **akw) for i in range(N_AG)]
        for i, a in enumerate(algos):
            a.noise_feed = [g["ma_eps"][i, 0], g["ma_eps"][i, 1]]
        return algos

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
        _check(f"ma {agent} loss", [s], [ref64], abs(ref32 - ref64))
        assert torch.equal(ours[k].policy.model.flat.data, alone[k].policy.model.flat.data)


# ---- behaviour ------------------------------------------------------------------------------------------------------------
def _three_device_drawn_updates(g, gd, buf, seed):
    algo, _ = _up_algo(g, gd, seed=seed)
    noises = []
    for k in range(3):
        algo._update_with_batch(algo._preprocess_batch(Batch(), buf, g[f"up_s{k}_indices"]))
        noises.append(algo.policy.model.noise().clone())
    return algo, noises


def test_device_drawn_updates_are_reproducible_and_draw_fresh_noise(g, gd):
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    (a, na), (b, _), (c, nc) = (_three_device_drawn_updates(g, gd, buf, s) for s in (3, 3, 4))
    assert torch.equal(_bits(a.policy.model.flat.data), _bits(b.policy.model.flat.data))
    assert torch.equal(_bits(a.target_flat), _bits(b.target_flat)) and a._noise_ctr == 6
    assert not torch.equal(a.policy.model.flat.data, c.policy.model.flat.data) and not torch.equal(na[0], nc[0])
    assert not torch.equal(na[0], na[1]) and not torch.equal(na[1], na[2])           # consecutive updates draw fresh noise
    assert torch.equal(_bits(a.model_old.noise()), _bits(na[2]))                     # update 2 is a copy call (quirk Q40)


def test_eval_mode_ignores_the_noise_and_respects_the_mask(g, gd):
    algo, R = _up_algo(g, gd, policy_kw=dict(eps_training=1.0))
    pol, net = algo.policy, algo.policy.model
    rs = np.random.RandomState(4)
    Rw, A = 130, R.A
    obs = rs.standard_normal((Rw, 6)).astype(np.float32)
    mask = np.zeros((Rw, A), bool)
    for r in range(Rw):
        mask[r, rs.choice(A, 1 + r % 4, replace=False)] = True
    algo.eval()
    out0 = pol(Batch(obs=Batch(obs=obs, mask=mask), info=Batch()))
    act0 = pol.act_device(_d(obs), mask=_d(mask))["act"].cpu().numpy()
    net.sample(99)                                                        # other noise: nothing may change in eval mode
    out1 = pol(Batch(obs=Batch(obs=obs, mask=mask), info=Batch()))
    assert torch.equal(_bits(out0.logits), _bits(out1.logits)) and np.array_equal(out0.act, out1.act)
    assert np.array_equal(pol.act_device(_d(obs), mask=_d(mask))["act"].cpu().numpy(), act0) and np.array_equal(act0, out0.act)
    assert out0.logits.shape == (Rw, A, R.N) and mask[np.arange(Rw), out0.act].all()
    q = (out0.logits.double().cpu().numpy() * pol.support.double().cpu().numpy()).sum(2)
    assert np.array_equal(out0.act, np.where(mask, q, -np.inf).argmax(1))
    mu_only = RainbowNetRestatement(6, (32,), A, R.N, (32,), (32,)).forward(net.flat.data.double().cpu().numpy(), obs, False)[0]
    _bar("eval-mode raw output against mu alone", net.forward(_d(obs), save=False).cpu().numpy(), mu_only, 0.0)
    algo.train()
    out2 = pol(Batch(obs=Batch(obs=obs, mask=mask), info=Batch()))
    assert not torch.equal(out2.logits, out0.logits) and mask[np.arange(Rw), out2.act].all()    # training mode: the noise acts
    pol.is_within_training_step = True                                    # epsilon 1: legal random actions
    a1 = pol.act_device(_d(obs), mask=_d(mask))["act"].cpu().numpy()
    assert mask[np.arange(Rw), a1].all() and not np.array_equal(a1, out0.act)


def test_eval_mode_update_leaves_sigma_unchanged(g, gd):
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    algo, _ = _up_algo(g, gd)
    net = algo.policy.model
    before = [{k: v.clone() for k, v in lv.items()} for lv in net.layer_views()]
    algo.eval()
    loss = algo._update_with_batch(algo._preprocess_batch(Batch(), buf, g["up_s0_indices"])).get_loss_stats_dict()["loss"]
    assert np.isfinite(loss)
    for b, a in zip(before, net.layer_views()):
        assert torch.equal(_bits(b["sigma_W"]), _bits(a["sigma_W"])) and torch.equal(_bits(b["sigma_bias"]), _bits(a["sigma_bias"]))
        assert not torch.equal(b["mu_W"], a["mu_W"])


def test_rainbow_over_a_noise_free_net_is_c51_bit_for_bit(g, gd):
    _, B, n_env, S, n_step, freq, *_ = up_inputs(gd)
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    akw = dict(gamma=float(g["gamma"]), n_step_return_horizon=n_step, target_update_freq=freq)
    mlp = FlatMLP([6, 32, 32, 255], "relu", device=DEV, seed=5)
    c51 = C51(policy=C51Policy(model=mlp, action_space=_Discrete(5), num_atoms=51), optim=AdamOptimizerFactory(lr=1e-3), **akw)
    net = RainbowNet(6, (32, 32), 5, 51, dueling=False, noisy_std=None, device=DEV, seed=1)
    net.flat.data.copy_(mlp.flat.data)
    rb = RainbowDQN(policy=RainbowPolicy(model=net, action_space=_Discrete(5), num_atoms=51), optim=AdamOptimizerFactory(lr=1e-3), **akw)
    rb.target_flat.copy_(net.flat.data)
    for k in range(2):
        la, lb = (a._update_with_batch(a._preprocess_batch(Batch(), buf, g[f"up_s{k}_indices"])).get_loss_stats_dict()["loss"]
                  for a in (c51, rb))
        assert la == lb
        assert torch.equal(_bits(mlp.flat.data), _bits(net.flat.data)) and torch.equal(_bits(c51.target_flat), _bits(rb.target_flat))
    assert rb._noise_ctr == 0


def test_reference_checkpoint_round_trips(g, gd):
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    algo, _ = _up_algo(g, gd, seed=2)
    algo._update_with_batch(algo._preprocess_batch(Batch(), buf, g["up_s0_indices"]))
    sd = algo.to_reference_state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    other, _ = _up_algo(g, gd, seed=2)
    other.policy.model.flat.data.zero_()
    other.target_flat.zero_()
    other.load_reference_state_dict(sd)
    assert torch.equal(_bits(other.policy.model.flat.data), _bits(algo.policy.model.flat.data))
    assert torch.equal(_bits(other.target_flat), _bits(algo.target_flat))
    other.load_state_dict(algo.state_dict())
    assert other._iter == 1 and other._noise_ctr == 2 and other.optim.step_count == 1
    idx = g["up_s1_indices"]      # both continue alike: same counter, same noise, same step
    la, lb = (a._update_with_batch(a._preprocess_batch(Batch(), buf, idx)).get_loss_stats_dict()["loss"] for a in (algo, other))
    assert la == lb and torch.equal(_bits(other.policy.model.flat.data), _bits(algo.policy.model.flat.data))
