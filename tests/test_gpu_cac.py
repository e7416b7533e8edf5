"""GPU tests (`-m gpu`) of the continuous-action actor-critics: every entry point of csrc/cac.hip alone against the float64
restatement (tests/cac_restatement.py, pinned to the reference's float64 run at 1e-10 by tests/test_host_cac.py) on the
fixture's inputs, and DDPG / TD3 / SAC's two-call sequences on a device buffer against tests/golden/cac.npz, fed the recorded
noise.

Bar, everywhere: test_gpu_distq.py's `_bar`, max |hip - ref64| <= 1e-5 max |ref64| + e_ref, with e_ref = max |ref32 - ref64| of
the reference's own two runs where the fixture has it (0 for the entry points alone: the restatement is their reference).  The
float32 reference's own relative distance from the float64 one is recorded in the fixture (`ref32_distance`): at most 4.9e-6
(the actor gradient), so no quantity needed the wider conditioning bar.  Every comparison prints `PARITY name: ...`."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import cac_restatement as R  # noqa: E402
from dqn_restatement import nstep_walk  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_host_cac import GOLD, N_CASES, buffer_rows, cases, dims_of, flat_rows, net_names, restatement_of  # noqa: E402
from test_host_dqn import _Env  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import DDPG, SAC, TD3, AutoAlpha, ContinuousDeterministicPolicy, SACPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch
    from tianshou_marl_amd.data.buffer import PrioritizedVectorReplayBuffer, VectorReplayBuffer
    from tianshou_marl_amd.utils.net import ContinuousActorDeterministic, ContinuousActorProbabilistic, ContinuousCritic


class _Box:
    def __init__(self, n, low=-1.0, high=1.0):
        self.low, self.high, self.shape = np.full(n, low, np.float32), np.full(n, high, np.float32), (n,)


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _d(x, dt=None):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dt or torch.float32)


def _n(t):
    return t.detach().cpu().numpy().astype(np.float64)


def head_inputs(g, B=None, Ad=None, seed=5):
    """Rows for the entry points alone: f32-representable raw outputs within +-3, normals, Q values, n-step terms."""
    rs = np.random.RandomState(seed)
    B = int(g["dims"][4]) if B is None else B
    Ad = int(g["dims"][1]) if Ad is None else Ad
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    d = dict(raw=np.clip(f(B, Ad), -3, 3), sraw=np.clip(0.7 * f(B, Ad) - 0.5, -3, 1), z=np.clip(f(B, Ad), -2.5, 2.5),
             q1=f(B), q2=f(B), ret=f(B), g1=f(B, Ad), g2=f(B, Ad), lp=f(B), mc=f(B), weight=(0.5 + rs.rand(B)).astype(np.float32),
             gpow=(0.99 ** rs.randint(1, 4, B)).astype(np.float32), vmask=rs.rand(B) > 0.3)
    return d


def _final(partial, B):
    out = torch.empty(2, device=DEV)
    ops.qmix_finalize(partial, B, out)
    return _n(out)


# ---- the entry points alone -----------------------------------------------------------------------------------------------
def test_normal_is_a_function_of_its_key_with_normal_moments():
    n = 1 << 16
    a, b = ops.cac_normal(n, 7, offset=3, device=DEV), ops.cac_normal(n, 7, offset=3, device=DEV)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(a, ops.cac_normal(n, 8, offset=3, device=DEV)) and not torch.equal(a, ops.cac_normal(n, 7, offset=4, device=DEV))
    x = _n(a)
    # 5 standard errors: of the mean 1 / sqrt(n), of the variance sqrt(2 / n)
    assert abs(x.mean()) < 5 / np.sqrt(n) and abs(x.var() - 1.0) < 5 * np.sqrt(2.0 / n), (x.mean(), x.var())
    assert torch.equal(ops.cac_normal(5, 7, offset=3, device=DEV), a[:5])   # a ragged last block of four


def test_det_action_and_det_actor_head_match_the_restatement(g):
    d = head_inputs(g)
    B, Ad = d["raw"].shape
    for name, kw in (("plain", {}), ("td3", dict(z=d["z"], policy_noise=0.2, noise_clip=0.5))):
        ref, omt2_ref = R.det_action(d["raw"], 1.5, **kw)
        rows = torch.zeros(B, Ad + 2, device=DEV)
        kd = {k: (_d(v) if k == "z" else v) for k, v in kw.items()}
        out, omt2 = ops.cac_det_action(_d(d["raw"]), 1.5, out=rows, col0=2, want_backward=True, **kd)
        assert out is rows and not _n(rows[:, :2]).any()
        _bar(f"det_action {name}", _n(rows[:, 2:]), ref, 0.0)
        _bar(f"1 - tanh^2 {name}", _n(omt2), omt2_ref, 0.0)
    ref = R.det_actor_head(d["g1"], omt2_ref, d["q1"], 1.5)
    ah = ops.cac_det_actor_head(_d(d["g1"]), omt2, _d(d["q1"]), 1.5)
    _bar("det d_raw", _n(ah["d_raw"]), ref["d_raw"], 0.0)
    _bar("det actor_loss", _final(ah["partial"], B)[0], ref["loss"], 0.0)


@pytest.mark.parametrize("unbounded", [False, True])
def test_sac_action_and_actor_head_match_the_restatement(g, unbounded):
    d = head_inputs(g)
    B, Ad = d["raw"].shape
    raw = np.concatenate([d["raw"], d["sraw"]], 1)
    ref = R.sac_action(d["raw"], d["sraw"], d["z"], 1.0, unbounded)
    act, logp = ops.sac_action(_d(raw), _d(d["z"]), 1.0, unbounded)
    _bar("sac act", _n(act), ref["a"], 0.0)
    _bar("sac logp", _n(logp), ref["logp"], 0.0)
    mode = R.sac_action(d["raw"], d["sraw"], None, 1.0, unbounded)
    act0, logp0 = ops.sac_action(_d(raw), None, 1.0, unbounded)
    _bar("sac mode", _n(act0), mode["a"], 0.0)
    _bar("sac mode logp", _n(logp0), mode["logp"], 0.0)
    alpha = torch.tensor([0.3], device=DEV)
    for twin in (True, False):
        q2, g2 = (d["q2"], d["g2"]) if twin else (None, None)
        rh = R.sac_actor_head(d["raw"], d["sraw"], d["z"], d["q1"], q2, d["g1"], g2, np.float32(0.3), 1.0, unbounded)
        ah = ops.sac_actor_head(_d(raw), _d(d["z"]), _d(d["q1"]), None if q2 is None else _d(q2), _d(d["g1"]),
                                None if g2 is None else _d(g2), alpha, 1.0, unbounded)
        _bar(f"sac d_mu twin={twin}", _n(ah["d_raw"][:, :Ad]), rh["d_mu"], 0.0)
        _bar(f"sac d_sigma twin={twin}", _n(ah["d_raw"][:, Ad:]), rh["d_sigma"], 0.0)
        _bar(f"sac head logp twin={twin}", _n(ah["logp"]), rh["logp"], 0.0)
        fin = _final(ah["partial"], B)
        _bar(f"sac actor_loss twin={twin}", fin[0], rh["loss"], 0.0)
        _bar(f"sac mean entropy twin={twin}", fin[1], rh["mean_entropy"], 0.0)
    # a state-independent sigma row
    sp = d["sraw"][0]
    rs = R.sac_action(d["raw"], sp, d["z"], 1.0, unbounded)
    a2, lp2 = ops.sac_action(_d(d["raw"]), _d(d["z"]), 1.0, unbounded, sigma_param=_d(sp))
    _bar("sac act (sigma_param)", _n(a2), rs["a"], 0.0)
    _bar("sac logp (sigma_param)", _n(lp2), rs["logp"], 0.0)
    rh = R.sac_actor_head(d["raw"], sp, d["z"], d["q1"], d["q2"], d["g1"], d["g2"], np.float32(0.3), 1.0, unbounded)
    ah = ops.sac_actor_head(_d(d["raw"]), _d(d["z"]), _d(d["q1"]), _d(d["q2"]), _d(d["g1"]), _d(d["g2"]), alpha, 1.0, unbounded,
                            sigma_param=_d(sp))
    _bar("sac d_mu (sigma_param)", _n(ah["d_raw"]), rh["d_mu"], 0.0)
    _bar("sac d_sigma rows (sigma_param)", _n(ah["d_sigma"]), rh["d_sigma"], 0.0)


def test_target_and_critic_head_match_the_restatement(g):
    d = head_inputs(g)
    B = d["q1"].shape[0]
    alpha = torch.tensor([0.25], device=DEV)
    for name, q2, lp in (("ddpg", None, None), ("td3", d["q2"], None), ("sac", d["q2"], d["lp"])):
        ref = R.target(d["q1"], q2, lp, np.float32(0.25), d["mc"], d["gpow"], d["vmask"])
        got = ops.cac_target(_d(d["q1"]), None if q2 is None else _d(q2), _d(d["mc"]), _d(d["gpow"]), _d(d["vmask"], torch.uint8),
                             logp_next=None if lp is None else _d(lp), alpha_dev=None if lp is None else alpha)
        _bar(f"target {name}", _n(got), ref, 0.0)
    for q2 in (None, d["q2"]):
        for wt in (None, d["weight"]):
            ref = R.critic_head(d["q1"], q2, d["ret"], wt)
            ch = ops.cac_critic_head(_d(d["q1"]), None if q2 is None else _d(q2), _d(d["ret"]), None if wt is None else _d(wt))
            tag = f"twin={q2 is not None} weight={wt is not None}"
            _bar(f"dq1 {tag}", _n(ch["dq1"]), ref["dq1"], 0.0)
            _bar(f"prio {tag}", _n(ch["prio"]), ref["prio"], 0.0)
            fin = _final(ch["partial"], B)
            _bar(f"critic1_loss {tag}", fin[0], ref["loss1"], 0.0)
            if q2 is not None:
                _bar(f"dq2 {tag}", _n(ch["dq2"]), ref["dq2"], 0.0)
                _bar(f"critic2_loss {tag}", fin[1], ref["loss2"], 0.0)
            else:
                assert ch["dq2"] is None


def test_act_dim_none_is_the_old_buffer_and_act_dim_only_changes_the_action_store():
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer

    S, B, N, D, k = 4, 2, 3, 5, 2
    old = DeviceVectorReplayBuffer(S * B, B, N, D, device=DEV)
    new = DeviceVectorReplayBuffer(S * B, B, N, D, device=DEV, act_dim=k)
    assert old.act_dim is None and old.unfused_adds_only is False and new.unfused_adds_only is True
    assert old.act_store.dtype == torch.int32 and tuple(old.act_store.shape) == (S, B, N)
    assert new.act_store.dtype == torch.float32 and tuple(new.act_store.shape) == (S, B, N, k)
    expect = dict(obs_store=(torch.float32, (S, B, N, D)), obs_next_store=(torch.float32, (S, B, N, D)),
                  rew_store=(torch.float32, (S, B, N)), term_store=(torch.uint8, (S, B, N)), trunc_store=(torch.uint8, (S, B, N)),
                  logp_store=(torch.float32, (S, B, N)), vs_store=(torch.float32, (S, B, N)), vnext_store=(torch.float32, (S, B, N)))
    for buf in (old, new):
        for name, want in expect.items():
            t = getattr(buf, name)
            assert (t.dtype, tuple(t.shape)) == want, name
    assert len(old.storage_key()) == len(new.storage_key()) == 11   # the eleven allocations of before: no new one
    # rows go in and come out as they are: integers through the old store, floats through the new one
    rs = np.random.RandomState(0)
    row = dict(obs=rs.standard_normal((B, N, D)).astype(np.float32), rew=np.ones((B, N), np.float32), terminated=np.zeros(B, bool),
               truncated=np.zeros(B, bool), obs_next=rs.standard_normal((B, N, D)).astype(np.float32))
    ai, af = rs.randint(0, 5, (B, N)), rs.uniform(-1, 1, (B, N, k)).astype(np.float32)
    old.add(Batch(act=ai, **row))
    new.add(Batch(act=af, **row))
    bo, bn = old[np.array([0, S])], new[np.array([0, S])]
    assert bo.act.dtype == np.int64 and np.array_equal(bo.act, ai)
    assert bn.act.dtype == np.float32 and np.array_equal(bn.act, af) and np.array_equal(bo.obs, bn.obs)


def test_col_sum_fills_slab_zero_and_clears_the_others():
    for B, Ad, n_slab in ((1, 1, 1), (300, 5, 4), (17, 64, 64)):
        rs = np.random.RandomState(B)
        d = rs.standard_normal((B, Ad)).astype(np.float32)
        slabs = torch.full((n_slab, 7 + Ad), 9.0, device=DEV)
        ops.cac_col_sum(_d(d), slabs[:, 7:])
        _bar(f"col_sum B={B}", _n(slabs[0, 7:]), d.astype(np.float64).sum(0), 0.0)
        assert not _n(slabs[1:, 7:]).any() and bool((slabs[:, :7] == 9.0).all())
    with pytest.raises(ValueError, match=r"n_slab = 65 outside \[1, 64\]"):
        ops.cac_col_sum(torch.zeros(4, 3, device=DEV), torch.zeros(65, 3, device=DEV))


# ---- the learners on the fixture's buffer -----------------------------------------------------------------------------------
def make_buffer(g, c, rows, n_agent=1):
    D, Ad = int(g["dims"][0]), int(g["dims"][1])
    n_env, S = int(g["dims"][5]), int(g["dims"][6])
    kw = dict(n_agent=n_agent, obs_dim=D, device=DEV, act_dim=Ad)
    if c["prio"]:
        buf = PrioritizedVectorReplayBuffer(n_env * S, n_env, alpha=float(g["per"][0]), beta=float(g["per"][1]), **kw)
    else:
        buf = VectorReplayBuffer(n_env * S, n_env, **kw)
    for r in rows:
        rep = lambda x: np.repeat(x[:, None], n_agent, 1)  # noqa: E731
        buf.add(Batch(obs=rep(r["obs"]), act=rep(r["act"]), rew=rep(r["rew"]) * (1 + np.arange(n_agent)), terminated=r["terminated"],
                      truncated=r["truncated"], obs_next=rep(r["obs_next"])), buffer_ids=np.arange(n_env))
    return buf


def make_algo(g, c, pk):
    D, Ad, h1, h2 = (int(x) for x in g["dims"][:4])
    M, lr = float(g["max_action"]), float(g["lr"])
    opt = lambda: AdamOptimizerFactory(lr=lr)  # noqa: E731

    def load(net, name):
        net.flat.data.copy_(_d(g[pk + "init_" + name]))
        return net

    crit = lambda name: load(ContinuousCritic(D, Ad, (h1, h2), device=DEV), name)  # noqa: E731
    c2 = None if c["no_c2"] else crit("critic2")
    common = dict(policy_optim=opt(), critic=crit("critic"), critic_optim=opt(), tau=float(g["tau"]), gamma=float(g["gamma"]),
                  n_step_return_horizon=c["n_step"])
    if c["kind"] == "sac":
        actor = load(ContinuousActorProbabilistic(D, Ad, (h1, h2), max_action=M, unbounded=c["unbounded"], conditioned_sigma=c["cond"],
                                                  device=DEV), "actor")
        fixed, la, te = (float(x) for x in g["sac"])
        alpha = AutoAlpha(te, la, opt()) if c["alpha"] == "auto" else fixed
        algo = SAC(policy=SACPolicy(actor=actor, action_space=_Box(Ad)), critic2=c2, alpha=alpha, **common)
    else:
        actor = load(ContinuousActorDeterministic(D, Ad, (h1, h2), max_action=M, device=DEV), "actor")
        pol = ContinuousDeterministicPolicy(actor=actor, action_space=_Box(Ad))
        if c["kind"] == "ddpg":
            algo = DDPG(policy=pol, **common)
        else:
            pn, nc, freq = g["td3"]
            algo = TD3(policy=pol, critic2=c2, policy_noise=float(pn), noise_clip=float(nc), update_actor_freq=int(freq), **common)
    algo.is_within_training_step = True
    return algo


def hip_net(algo, name):
    return {"actor": lambda: algo.policy.actor, "critic": lambda: algo.critic, "critic2": lambda: algo.critic2,
            "critic_old": lambda: algo.critic_old, "critic2_old": lambda: algo.critic2_old, "actor_old": lambda: algo.actor_old}[name]()


def run_two_calls(g, ci, check=True):
    c = cases(g)[ci]
    pk = f"c{ci}_"
    rows, _ = buffer_rows(g, int(g[pk + "seed"]))
    buf = make_buffer(g, c, rows)
    algo = make_algo(g, c, pk)
    keys = [str(k) for k in g["stat_keys"]]
    for k in range(2):
        sk = f"{pk}s{k}_"
        zs = [_d(g[sk + n]) for n in ("z_target", "z_actor") if sk + n in g]
        algo.noise_source = lambda B, Ad, zs=zs: zs.pop(0)
        idx = _d(g[sk + "indices"], torch.int64)
        batch = algo._sampled_batch(buf, idx)
        if c["prio"] and check:
            _bar(f"{sk}IS weights", _n(batch.weight), g[sk + "weight_in"], float(g[sk + "weight_in_eref"]))
        batch = algo._preprocess_batch(batch, buf, idx)
        stats = algo._update_with_batch(batch)
        algo._postprocess_batch(batch, buf, idx)
        assert not zs, "a recorded draw was not consumed"
        if not check:
            continue
        _bar(f"{sk}returns", _n(batch.returns), g[sk + "returns"], float(g[sk + "returns_eref"]))
        _bar(f"{sk}prio", _n(batch.weight), g[sk + "prio"], float(g[sk + "prio_eref"]))
        ref, ref32 = g[sk + "stats"], g[sk + "stats32"]
        for j, key in enumerate(keys):
            if not np.isnan(ref[j]):
                _bar(f"{sk}{key}", getattr(stats, key), ref[j], abs(ref32[j] - ref[j]))
        w = algo._ws[idx.numel()]   # the gradient each optimizer stepped with: its slabs, summed
        for n, key in (("critic", "slabs_c1"), ("critic2", "slabs_c2"), ("actor", "slabs_a")):
            if f"{sk}grad_{n}" in g:
                _bar(f"{sk}grad {n}", _n(w[key]).sum(0), g[f"{sk}grad_{n}"], float(g[f"{sk}grad_{n}_eref"]))
        if c["alpha"] == "auto":
            la = g[sk + "log_alpha"]
            _bar(f"{sk}log_alpha", float(algo.alpha._log_alpha), la[0], abs(la[1] - la[0]))
    if check:
        for n in net_names(c["kind"]):
            _bar(f"{pk}{n} weights", _n(hip_net(algo, n).flat.data), g[f"{pk}s1_w_{n}"], float(g[f"{pk}s1_w_{n}_eref"]))
        if c["prio"]:
            n_rows = int(g["dims"][5]) * int(g["dims"][6])
            _bar(f"{pk}leaves", _n(buf.weight[np.arange(n_rows)]), g[pk + "leaves"], float(g[pk + "leaves_eref"]))
            touched = np.unique(np.concatenate([g[f"{pk}s{k}_indices"] for k in range(2)]))
            assert not np.allclose(g[pk + "leaves"][touched], 1.0)   # the |td|-based priorities, not the initial ones
    return algo


@pytest.mark.parametrize("ci", range(N_CASES))
def test_two_update_calls_follow_the_reference(g, ci):
    run_two_calls(g, ci)


@pytest.mark.parametrize("ci", [1, 3, 6])
def test_running_twice_gives_the_same_parameter_bits(g, ci):
    a, b = run_two_calls(g, ci, check=False), run_two_calls(g, ci, check=False)
    for n in net_names(cases(g)[ci]["kind"]):
        assert torch.equal(hip_net(a, n).flat.data.view(torch.int32), hip_net(b, n).flat.data.view(torch.int32)), n


def test_update_draws_its_own_noise_and_moves_every_net(g):
    """`update` end to end (sampling, the Philox draws of tsm_cac_normal, the write-back) for TD3 and SAC."""
    for ci in (2, 6):
        c = cases(g)[ci]
        pk = f"c{ci}_"
        rows, _ = buffer_rows(g, int(g[pk + "seed"]))
        buf, algo = make_buffer(g, c, rows), make_algo(g, c, pk)
        before = {n: hip_net(algo, n).flat.data.clone() for n in net_names(c["kind"])}
        stats = algo.update(buf, 12)
        assert np.isfinite([stats.actor_loss, stats.critic1_loss, stats.critic2_loss]).all()
        assert algo.policy._sample_ctr == (12 * 3 if c["kind"] == "td3" else 2 * 12 * 3)
        for n, w in before.items():
            assert not torch.equal(w, hip_net(algo, n).flat.data), n
        sd = algo.state_dict()
        algo2 = make_algo(g, c, pk)
        algo2.load_state_dict(sd)
        ref_sd = algo.to_reference_state_dict()
        algo2.load_reference_state_dict(ref_sd)
        for n in net_names(c["kind"]):
            assert torch.equal(hip_net(algo, n).flat.data, hip_net(algo2, n).flat.data), n
        if c["kind"] == "td3":
            assert (algo2._cnt, algo2._last) == (algo._cnt, algo._last) and algo._cnt == 1


def test_multi_agent_dispatch_over_a_joint_lane_act_dim_buffer(g):
    """Two independent learners (DDPG, SAC) over the two lanes of one joint-step `act_dim` buffer: lane k's rows and reward
    column reach learner k, whose first call equals a single-agent call on the same rows."""
    cs = cases(g)
    ci = [0, 5]
    rows, RB = buffer_rows(g, int(g["c0_seed"]))
    buf = make_buffer(g, dict(prio=False), rows, n_agent=2)
    assert buf.act_store.dtype == torch.float32 and tuple(buf.act_store.shape[2:]) == (2, int(g["dims"][1]))
    algos = [make_algo(g, cs[i], f"c{i}_") for i in ci]
    z = [_d(g["c5_s0_z_target"]), _d(g["c5_s0_z_actor"])]
    algos[1].noise_source = lambda B, Ad: z.pop(0)
    ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=_Env(2))
    ma.is_within_training_step = True
    idx = g["c0_s0_indices"]
    stats = ma._update_with_batch(ma._preprocess_batch(None, buf, idx))
    fr = flat_rows(g, rows)
    for k, agent in enumerate(_Env(2).agents):
        c = cs[ci[k]]
        Rk = restatement_of(g, c)
        RB.rew[:, 0] = flat_rew(g, rows) * (1 + k)
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, c["n_step"], float(g["gamma"]), 0)
        r = Rk.update(fr["obs"][idx], fr["act"][idx], fr["obs_next"][idx_n], mc, gpow, vmask,
                      z_target=g.get("c5_s0_z_target") if k else None, z_actor=g.get("c5_s0_z_actor") if k else None)
        st = stats._agent_id_to_stats[agent]
        _bar(f"marl {agent} actor_loss", st.actor_loss, r["actor_loss"], 0.0)
        _bar(f"marl {agent} critic loss", st.critic_loss if k == 0 else st.critic1_loss, r["critic1_loss"], 0.0)


def flat_rew(g, rows):
    n_env, S = int(g["dims"][5]), int(g["dims"][6])
    out = np.zeros(n_env * S)
    for t, r in enumerate(rows):
        out[np.arange(n_env) * S + t] = r["rew"]
    return out
