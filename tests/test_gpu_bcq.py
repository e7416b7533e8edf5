"""GPU tests (`-m gpu`) of BCQ: every entry point of csrc/bcq.hip alone against the float64 restatement
(tests/bcq_restatement.py, pinned to the reference's float64 run at 1e-10 by tests/test_host_bcq.py), BCQ's two-call sequences
and BCQPolicy's acting on a device buffer against tests/golden/bcq.npz, fed the recorded normals, both checkpoint layouts, and
the agent-column path through MultiAgentOffPolicyAlgorithm.

Bar, everywhere: test_gpu_distq.py's `_bar`, max |hip - ref64| <= 1e-5 max |ref64| + e_ref, with e_ref = max |ref32 - ref64| of
the reference's own two runs where the fixture has it (0 for the entry points alone: the restatement is their reference).  The
float32 reference's own relative distance from the float64 one is recorded in the fixture (`ref32_distance`): at most 4.6e-7
for every gradient, weight and action, 2.1e-7 for the statistics.  Every comparison prints `PARITY name: ...`."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import bcq_restatement as R  # noqa: E402
from cac_restatement import det_actor_head  # noqa: E402
from test_gpu_cac import _Box, _d, _final, _n, make_buffer  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_host_bcq import GOLD, N_CASES, STAT_KEYS, cases, dims_of, restatement_of  # noqa: E402
from test_host_cql import buffer_rows, flat_rows  # noqa: E402
from test_host_dqn import _Env  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import BCQ, BCQPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import VAE, ContinuousCritic, Perturbation

NET_OF = {"pert": lambda a: a.policy.actor_perturbation, "critic": lambda a: a.critic, "critic2": lambda a: a.critic2,
          "vae": lambda a: a.policy.vae, "pert_old": lambda a: a.actor_perturbation_target, "critic_old": lambda a: a.critic_old,
          "critic2_old": lambda a: a.critic2_old}


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def inputs(B=12, D=6, Ad=3, L=6, seed=5):
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    head = f(B, 2 * L)
    head[:, L:] = 3.0 * head[:, L:] - 2.0   # raw log_std on both sides of -4
    return dict(head=head, eps=f(B, L), obs=f(B, D), nxt=f(B, D), act=rs.uniform(-1, 1, (B, Ad)).astype(np.float32),
                raw=np.clip(f(B, Ad), -3, 3), dz=f(B, L))


# ---- the entry points alone -----------------------------------------------------------------------------------------------
def test_latent_vae_head_and_latent_grad_match_the_restatement():
    d = inputs()
    B, L, M = 12, 6, 1.5
    assert (d["head"][:, L:] < -4).any() and (d["head"][:, L:] > -4).any()
    x, std = ops.bcq_latent(_d(d["head"]), _d(d["eps"]), _d(d["obs"]))
    rx, rstd = R.latent(d["head"], d["eps"], d["obs"])
    _bar("latent rows", _n(x), rx, 0.0)
    _bar("latent std", _n(std), rstd, 0.0)
    vh = ops.bcq_vae_head(_d(d["raw"]), _d(d["act"]), _d(d["head"]), M)
    rv = R.vae_head(d["raw"], d["act"], d["head"], M)
    _bar("vae d_raw", _n(vh["d_raw"]), rv["d_raw"], 0.0)
    fin = _final(vh["partial"], B)
    _bar("vae_loss", fin[0], rv["vae_loss"], 0.0)
    _bar("KL_loss", fin[1], rv["kl_loss"], 0.0)
    dh = ops.bcq_latent_grad(_d(d["dz"]), _d(d["head"]), _d(d["eps"]))
    _bar("latent d_head", _n(dh), R.latent_grad(d["dz"], d["head"], d["eps"]), 0.0)
    assert torch.equal(vh["partial"], ops.bcq_vae_head(_d(d["raw"]), _d(d["act"]), _d(d["head"]), M)["partial"])   # same bits


def test_decode_rows_action_rows_and_target_match_the_restatement():
    d = inputs()
    B, D, L, K, M = 12, 6, 6, 3, 2.0
    rs = np.random.RandomState(1)
    z = rs.standard_normal((B * K + B, L)).astype(np.float32)
    xd = ops.bcq_decode_rows(_d(d["nxt"]), K, _d(d["obs"]), _d(z))
    rxd = R.decode_rows(d["nxt"], K, d["obs"], z)
    assert np.array_equal(_n(xd), rxd) and (np.abs(rxd[:, D:]) == 0.5).any()
    raw = np.clip(rs.standard_normal((B * K + B, 3)), -3, 3).astype(np.float32)
    X = ops.bcq_action_rows(_d(raw), xd, D, M)
    _bar("action rows", _n(X), R.action_rows(raw, rxd, D, M), 0.0)
    assert torch.equal(X[:, :D], xd[:, :D])
    q1, q2 = (rs.standard_normal(B * K).astype(np.float32) for _ in range(2))
    rew, done = rs.standard_normal(B).astype(np.float32), rs.rand(B) < 0.4
    for lmbda in (0.75, 1.0, 0.0):
        t = ops.bcq_target(_d(q1), _d(q2), _d(rew), _d(~done, torch.bool), K, 0.99, lmbda)
        _bar(f"target lmbda={lmbda}", _n(t), R.target(q1, q2, rew, ~done, K, 0.99, lmbda), 0.0)


def test_perturb_with_the_det_actor_head_and_select_match_the_restatement():
    rs = np.random.RandomState(2)
    n, D, Ad, phi, M, S = 15, 6, 3, 0.5, 1.0, 5
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    x_in = np.concatenate([f(n, D), rs.uniform(-M, M, (n, Ad)).astype(np.float32)], 1)
    raw_p, g1, q = f(n, Ad), f(n, Ad), f(n)
    x_out, factor = ops.bcq_perturb(_d(raw_p), _d(x_in), phi, M)
    rx, rf, u = R.perturb(raw_p, x_in, D, phi, M)
    assert (np.abs(u) > M).any() and (np.abs(u) < M).any()
    _bar("perturbed rows", _n(x_out), rx, 0.0)
    _bar("perturb factor", _n(factor), rf, 0.0)
    assert np.array_equal(_n(factor) == 0.0, np.abs(u) > M)
    ah = ops.cac_det_actor_head(_d(g1), factor, _d(q), M)
    ref = det_actor_head(g1, rf, q, M)
    _bar("actor d_raw", _n(ah["d_raw"]), ref["d_raw"], 0.0)
    _bar("actor_loss", _final(ah["partial"], n)[0], ref["loss"], 0.0)
    act, index = ops.bcq_select(_d(q), x_out, S, D, Ad)
    ra, ri = R.select(q, _n(x_out), S, D, Ad)
    assert np.array_equal(index.cpu().numpy(), ri) and np.array_equal(_n(act), ra) and index.dtype == torch.int32


# ---- the learner and the policy on the fixture's buffer ------------------------------------------------------------------------
def make_bcq(g, c, seed=0):
    d = dims_of(g)
    D, Ad, L, pk, lr = d["D"], d["Ad"], d["L"], f"c{c['i']}_", float(g["lr"])
    opt = lambda: AdamOptimizerFactory(lr=lr)  # noqa: E731

    def load(net, name):
        net.flat.data.copy_(_d(g[pk + "init_" + name]))
        return net

    pert = load(Perturbation(obs_dim=D, act_dim=Ad, hidden_sizes=d["hid"], max_action=c["max_action"], phi=c["phi"], device=DEV), "pert")
    vae = load(VAE(encoder_hidden_sizes=d["vhid"], decoder_hidden_sizes=d["vhid"], obs_dim=D, act_dim=Ad, latent_dim=L,
                   max_action=c["max_action"], device=DEV), "vae")
    c1 = load(ContinuousCritic(D, Ad, d["hid"], device=DEV), "critic")
    c2 = None if c["no_c2"] else load(ContinuousCritic(D, Ad, d["hid"], device=DEV), "critic2")
    policy = BCQPolicy(actor_perturbation=pert, action_space=_Box(Ad, -c["max_action"], c["max_action"]), critic=c1, vae=vae,
                       forward_sampled_times=d["S"], seed=seed)
    algo = BCQ(policy=policy, actor_perturbation_optim=opt(), critic_optim=opt(), vae_optim=opt(), critic2=c2,
               gamma=float(g["gamma"]), tau=float(g["tau"]), lmbda=c["lmbda"], num_sampled_action=d["K"])
    algo.is_within_training_step = True
    return algo


def bcq_buffer(g, c, n_agent=1):
    rows, _ = buffer_rows(g, int(g[f"c{c['i']}_seed"]), dims_of(g)["T"])
    return make_buffer(g, dict(prio=False), rows, n_agent=n_agent)


def bcq_call(g, c, algo, buf, k, agent=None):
    sk = f"c{c['i']}_s{k}_"
    zs = [_d(g[sk + "z_vae"]), _d(np.concatenate([g[sk + "z_next"], g[sk + "z_obs"]], 0))]
    algo.normal_source = lambda rows, L: zs.pop(0)
    idx = _d(g[sk + "indices"], torch.int64)
    stats = algo._update_with_batch(algo._preprocess_batch(algo._sampled_batch(buf, idx), buf, idx, agent=agent))
    assert not zs, "a recorded draw was not consumed"
    algo.normal_source = None
    return stats, idx


@pytest.mark.parametrize("ci", range(N_CASES))
def test_two_update_calls_and_acting_follow_the_reference(g, ci):
    c = cases(g)[ci]
    pk = f"c{ci}_"
    buf, algo = bcq_buffer(g, c), make_bcq(g, c)
    for k in range(2):
        sk = f"{pk}s{k}_"
        stats, idx = bcq_call(g, c, algo, buf, k)
        ref, ref32 = g[sk + "stats"], g[sk + "stats32"]
        for j, key in enumerate(STAT_KEYS):
            _bar(f"{sk}{key}", getattr(stats, key), ref[j], abs(ref32[j] - ref[j]))
        w = algo._ws[idx.numel()]   # the gradient each optimizer stepped with: its slabs, summed
        for n, key in (("vae", "slabs_v"), ("critic", "slabs_c1"), ("critic2", "slabs_c2"), ("pert", "slabs_a")):
            _bar(f"{sk}grad {n}", _n(w[key]).sum(0), g[f"{sk}grad_{n}"], float(g[f"{sk}grad_{n}_eref"]))
    for n, net in NET_OF.items():
        _bar(f"{pk}{n} weights", _n(net(algo).flat.data), g[f"{pk}s1_w_{n}"], float(g[f"{pk}s1_w_{n}_eref"]))
    # acting after the second call: the recorded normals, row-major [n S, L]
    from tianshou_marl_amd.data.batch import Batch

    algo.policy.normal_source = lambda rows, L: _d(g[pk + "act_z"])
    out = algo.policy.forward(Batch(obs=g[pk + "act_obs"]))
    _bar(f"{pk}act", out.act, g[pk + "act"], float(g[pk + "act_eref"]))
    assert np.array_equal(out.index.cpu().numpy(), g[pk + "act_index"])
    act, index, rows, q = algo.policy.candidates(_d(g[pk + "act_obs"]), _d(g[pk + "act_z"]))
    S, D = algo.policy.forward_sampled_times, algo.policy.obs_dim
    pick = rows.view(-1, S, rows.shape[1])[torch.arange(index.numel(), device=DEV), index.long(), D:]
    assert torch.equal(act.view(torch.int32), pick.contiguous().view(torch.int32))   # bit-equal to the device's own candidates
    assert torch.equal(index.long(), q.view(-1, S).argmax(1)) and np.array_equal(out.act, act.cpu().numpy())


def test_state_dict_and_reference_layout_round_trips_continue_bit_identically(g):
    for ci, layout in ((0, "native"), (5, "reference")):
        c = cases(g)[ci]
        buf, a = bcq_buffer(g, c), make_bcq(g, c, seed=7)
        bcq_call(g, c, a, buf, 0)
        idx = _d(g[f"c{ci}_s1_indices"], torch.int64)
        own = lambda algo: algo._update_with_batch(algo._preprocess_batch(algo._sampled_batch(buf, idx), buf, idx))  # noqa: E731
        own(a)   # draws its own normals: the counter moves
        b = make_bcq(g, c, seed=7)
        b.load_state_dict(a.state_dict())   # the Adam states travel in the native layout alone
        if layout == "reference":
            sd = a.to_reference_state_dict()
            assert [k for k in sd if k != "sample_ctr"] == [str(k) for k in g["sd_keys"]]   # exactly the reference's
            for n, net in NET_OF.items():
                net(b).flat.data.zero_()
            b.policy._sample_ctr = 0
            b.load_reference_state_dict(sd)
        assert b.policy._sample_ctr == a.policy._sample_ctr > 0
        sa, sb = own(a), own(b)   # the same rows, each learner's own draws at its restored counter
        for key in STAT_KEYS:
            assert getattr(sa, key) == getattr(sb, key), key
        for n, net in NET_OF.items():
            assert torch.equal(net(a).flat.data.view(torch.int32), net(b).flat.data.view(torch.int32)), n
        st = a.state_dict()
        assert {"actor_perturbation_optim", "critic_optim", "critic2_optim", "vae_optim", "sample_ctr"} <= set(st)


def test_update_draws_its_own_normals_and_moves_every_net(g):
    c = cases(g)[0]
    d = dims_of(g)
    buf, algo = bcq_buffer(g, c), make_bcq(g, c)
    before = {n: net(algo).flat.data.clone() for n, net in NET_OF.items()}
    stats = algo.update(buf, 12)
    assert np.isfinite([getattr(stats, k) for k in STAT_KEYS]).all()
    assert algo.policy._sample_ctr == (12 + 12 * d["K"] + 12) * d["L"]
    for n, w in before.items():
        assert not torch.equal(w, NET_OF[n](algo).flat.data), n
    res = algo.policy.act_device(torch.zeros(3, d["D"], device=DEV))
    assert tuple(res["act"].shape) == (3, d["Ad"]) and bool((res["act"].abs() <= 1.0).all())


def test_agent_column_path_through_the_multi_agent_dispatch(g):
    """Two agents on a joint-step buffer whose agents see the same rows and rewards scaled by (1 + k): agent 0's learner
    follows the fixture, agent 1's sees rewards twice as large."""
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm

    c = cases(g)[0]
    buf = bcq_buffer(g, c, n_agent=2)
    algos = [make_bcq(g, c), make_bcq(g, c)]
    sk = "c0_s0_"
    for a in algos:
        zs = [_d(g[sk + "z_vae"]), _d(np.concatenate([g[sk + "z_next"], g[sk + "z_obs"]], 0))]
        a.normal_source = lambda rows, L, zs=zs: zs.pop(0)
    env = _Env(2)
    ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=env)
    ma.is_within_training_step = True
    idx = g[sk + "indices"]
    stats = ma._update_with_batch(ma._preprocess_batch(None, buf, idx))
    rows, _ = buffer_rows(g, int(g["c0_seed"]), dims_of(g)["T"])
    fr = flat_rows(g, rows)
    for k, agent in enumerate(env.agents):
        Rk = restatement_of(g, c)
        r = Rk.update(fr["obs"][idx], fr["act"][idx], fr["rew"][idx] * (1 + k), fr["done"][idx], fr["obs_next"][idx],
                      g[sk + "z_vae"], g[sk + "z_next"], g[sk + "z_obs"])
        st = stats._agent_id_to_stats[agent]
        for key in STAT_KEYS:
            _bar(f"marl {agent} {key}", getattr(st, key), r[key], 0.0)
    s0, s1 = (stats._agent_id_to_stats[a] for a in env.agents)
    assert s1.vae_loss == s0.vae_loss and s1.critic1_loss != s0.critic1_loss
    with pytest.raises(ValueError, match="say which agent"):
        algos[0]._preprocess_batch(algos[0]._sampled_batch(buf, _d(idx, torch.int64)), buf, _d(idx, torch.int64))
