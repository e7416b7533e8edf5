"""GPU tests (`-m gpu`) of REDQ: every entry point of csrc/redq.hip alone against the float64 restatement
(tests/redq_restatement.py, pinned to the reference's float64 run at 1e-10 by tests/test_host_redq.py) on fixture-sized rows,
the `EnsembleCritic` against the restated ensemble forward, and REDQ's three-call sequences (a call that does not step the
actor, one that does, the call after it) on a device buffer against tests/golden/redq.npz, fed the recorded noise and subsets.

Bar, everywhere: test_gpu_distq.py's `_bar`, max |hip - ref64| <= 1e-5 max |ref64| + e_ref, with e_ref = max |ref32 - ref64| of
the reference's own two runs where the fixture has it (0 for the entry points alone: the restatement is their reference).
Every comparison prints `PARITY name: ...`."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import redq_restatement as R  # noqa: E402
from dqn_restatement import nstep_walk  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_host_cac import _Box, buffer_rows, flat_rows  # noqa: E402
from test_host_dqn import _Env  # noqa: E402
from test_host_redq import GOLD, N_CASES, NETS, cases, restatement_of  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import REDQ, AutoAlpha, REDQPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch
    from tianshou_marl_amd.data.buffer import PrioritizedVectorReplayBuffer, VectorReplayBuffer
    from tianshou_marl_amd.utils.net import ContinuousActorProbabilistic, EnsembleCritic


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _d(x, dt=None):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dt or torch.float32)


def _n(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _final(partial, n):
    out = torch.empty(2, device=DEV)
    ops.qmix_finalize(partial, n, out)
    return _n(out)


def head_inputs(E, B, seed=5):
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    return dict(q=f(E, B), ret=f(B), lp=f(B), mc=f(B), weight=(0.5 + rs.rand(B)).astype(np.float32),
                gpow=(0.99 ** rs.randint(1, 4, B)).astype(np.float32), vmask=rs.rand(B) > 0.3)


# ---- the entry points alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,B", [(4, 12), (1, 12), (10, 300), (64, 5)])   # the fixture's rows; one member; two workgroups; the mask's last bit
def test_target_critic_head_and_mean_q_match_the_restatement(E, B):
    d = head_inputs(E, B)
    alpha = torch.tensor([0.25], device=DEV)
    subsets = [[E - 1], list(range(E))] + ([[E - 1, 0]] if E > 1 else []) + ([[1, 3, 2]] if E > 3 else [])
    for sub in subsets:
        for mode in ("min", "mean"):
            for lp in (None, d["lp"]):
                ref = R.target(d["q"], sub, mode, lp, np.float32(0.25), d["mc"], d["gpow"], d["vmask"])
                got = ops.redq_target(_d(d["q"]), ops.redq_subset_mask(sub, E), mode, _d(d["mc"]), _d(d["gpow"]),
                                      _d(d["vmask"], torch.uint8), logp_next=None if lp is None else _d(lp),
                                      alpha_dev=None if lp is None else alpha)
                _bar(f"target E={E} B={B} subset={sub} {mode} logp={lp is not None}", _n(got), ref, 0.0)
    for wt in (None, d["weight"]):
        ref = R.critic_head(d["q"], d["ret"], wt)
        ch = ops.redq_critic_head(_d(d["q"]).unsqueeze(-1), _d(d["ret"]), None if wt is None else _d(wt))
        tag = f"E={E} B={B} weight={wt is not None}"
        assert tuple(ch["dq"].shape) == (E, B)
        _bar(f"dq {tag}", _n(ch["dq"]), ref["dq"], 0.0)
        _bar(f"prio {tag}", _n(ch["prio"]), ref["prio"], 0.0)
        fin = _final(ch["partial"], E * B)
        _bar(f"critic_loss {tag}", fin[0], ref["loss"], 0.0)
        assert fin[1] == 0.0
        again = ops.redq_critic_head(_d(d["q"]), _d(d["ret"]), None if wt is None else _d(wt))
        assert torch.equal(again["partial"].view(torch.int64), ch["partial"].view(torch.int64))   # two runs, the same bits
    _bar(f"mean_q E={E} B={B}", _n(ops.redq_mean_q(_d(d["q"]))), R.mean_q(d["q"]), 0.0)
    nan_q = d["q"].copy()
    nan_q[E - 1, 0] = np.nan   # torch.min keeps a NaN
    got = ops.redq_target(_d(nan_q), ops.redq_subset_mask(range(E), E), "min", _d(d["mc"]), _d(d["gpow"]), _d(np.ones(B, bool), torch.uint8))
    assert np.isnan(_n(got)[0]) and not np.isnan(_n(got)[1:]).any()


def test_ensemble_critic_is_the_restated_ensemble_and_its_mean_gradient(g):
    """`EnsembleCritic` on the fixture's first case: forward, the gradient slabs of a recorded d_out, and the input gradient
    with d_out = 1 / E, which is the gradient of the ensemble mean the actor's head is fed."""
    c = cases(g)[0]
    D, Ad, h1, h2, B = (int(x) for x in g["dims"][:5])
    E = c["E"]
    net = EnsembleCritic(D, Ad, E, (h1, h2), device=DEV)
    net.flat.data.copy_(_d(g["c0_init_critic"]))
    rs = np.random.RandomState(2)
    x = rs.standard_normal((B, D + Ad)).astype(np.float32)
    q = net(_d(x), save=True)
    assert tuple(q.shape) == (E, B, 1)
    Rn = R._EnsNet(g["c0_init_critic"], net.dims, E, 1e-3, type("O", (), dict(kink=np.inf))())
    xt = torch.as_tensor(x.astype(np.float64)).requires_grad_(True)
    qr = Rn.fwd(Rn.params, xt)
    _bar("ensemble forward", _n(q), qr.detach().numpy(), 0.0)
    (gx,) = torch.autograd.grad(qr.mean(0).sum(), xt, retain_graph=True)
    got = net.input_grad(torch.full((E, B, 1), 1.0 / E, device=DEV), D, Ad)
    _bar("gradient of the ensemble mean w.r.t. the action", _n(got), gx.numpy()[:, D:], 0.0)
    d_out = rs.standard_normal((E, B, 1)).astype(np.float32)
    slabs = net.backward(_d(d_out), 2)
    _bar("ensemble gradient", _n(slabs).sum(0), Rn.step(qr, d_out), 0.0)


# ---- the learner on the fixture's buffer ------------------------------------------------------------------------------------
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


def make_algo(g, c):
    D, Ad, h1, h2 = (int(x) for x in g["dims"][:4])
    pk = f"c{c['i']}_"
    opt = lambda: AdamOptimizerFactory(lr=float(g["lr"]))  # noqa: E731
    actor = ContinuousActorProbabilistic(D, Ad, (h1, h2), max_action=float(g["max_action"]), conditioned_sigma=True, device=DEV)
    actor.flat.data.copy_(_d(g[pk + "init_actor"]))
    critic = EnsembleCritic(D, Ad, c["E"], (h1, h2), device=DEV)
    critic.flat.data.copy_(_d(g[pk + "init_critic"]))
    fixed, la, te = (float(x) for x in g["sac"])
    algo = REDQ(policy=REDQPolicy(actor=actor, action_space=_Box(Ad)), policy_optim=opt(), critic=critic, critic_optim=opt(),
                ensemble_size=c["E"], subset_size=c["M"], tau=float(g["tau"]), gamma=float(g["gamma"]),
                alpha=AutoAlpha(te, la, opt()) if c["alpha"] == "auto" else fixed, n_step_return_horizon=c["n_step"],
                actor_delay=int(g["actor_delay"]), target_mode=c["mode"])
    algo.is_within_training_step = True
    return algo


def hip_net(algo, name):
    return {"actor": algo.policy.actor, "critic": algo.critic, "critic_old": algo.critic_old}[name]


def run_calls(g, ci, check=True):
    c = cases(g)[ci]
    pk = f"c{ci}_"
    rows, _ = buffer_rows(g, int(g[pk + "seed"]))
    buf, algo = make_buffer(g, c, rows), make_algo(g, c)
    keys = [str(k) for k in g["stat_keys"]]
    for k in range(int(g["n_calls"])):
        sk = f"{pk}s{k}_"
        zs = [_d(g[sk + n]) for n in ("z_target", "z_actor") if sk + n in g]
        subs = [g[sk + "subset"]]
        algo.noise_source = lambda B, Ad, zs=zs: zs.pop(0)
        algo.subset_source = lambda E, M, subs=subs: subs.pop(0)
        idx = _d(g[sk + "indices"], torch.int64)
        batch = algo._sampled_batch(buf, idx)
        if c["prio"] and check:
            _bar(f"{sk}IS weights", _n(batch.weight), g[sk + "weight_in"], float(g[sk + "weight_in_eref"]))
        batch = algo._preprocess_batch(batch, buf, idx)
        stats = algo._update_with_batch(batch)
        algo._postprocess_batch(batch, buf, idx)
        assert not zs and not subs, "a recorded draw was not consumed"
        stepped = bool(g[sk + "actor_stepped"])
        assert algo.critic_gradient_step == k + 1 and (stats.alpha_loss is not None) == (stepped and c["alpha"] == "auto")
        if k == 0:
            assert stats.actor_loss == 0.0   # before the first actor step
        if not check:
            continue
        _bar(f"{sk}returns", _n(batch.returns), g[sk + "returns"], float(g[sk + "returns_eref"]))
        _bar(f"{sk}prio", _n(batch.weight), g[sk + "prio"], float(g[sk + "prio_eref"]))
        ref, ref32 = g[sk + "stats"], g[sk + "stats32"]
        for j, key in enumerate(keys):
            if not np.isnan(ref[j]):
                _bar(f"{sk}{key}", getattr(stats, key), ref[j], abs(ref32[j] - ref[j]))
        w = algo._ws[idx.numel()]   # the gradient each optimizer stepped with: its slabs, summed
        for n, key in (("critic", "slabs_c1"), ("actor", "slabs_a")):
            if f"{sk}grad_{n}" in g:
                _bar(f"{sk}grad {n}", _n(w[key]).sum(0), g[f"{sk}grad_{n}"], float(g[f"{sk}grad_{n}_eref"]))
        if c["alpha"] == "auto":
            la = g[sk + "log_alpha"]
            _bar(f"{sk}log_alpha", float(algo.alpha._log_alpha), la[0], abs(la[1] - la[0]))
    if check:
        last = f"{pk}s{int(g['n_calls']) - 1}_"
        for n in NETS:
            _bar(f"{pk}{n} weights", _n(hip_net(algo, n).flat.data), g[f"{last}w_{n}"], float(g[f"{last}w_{n}_eref"]))
        if c["prio"]:
            n_rows = int(g["dims"][5]) * int(g["dims"][6])
            _bar(f"{pk}leaves", _n(buf.weight[np.arange(n_rows)]), g[pk + "leaves"], float(g[pk + "leaves_eref"]))
            touched = np.unique(np.concatenate([g[f"{pk}s{k}_indices"] for k in range(int(g["n_calls"]))]))
            assert not np.allclose(g[pk + "leaves"][touched], 1.0)   # the |td|-based priorities, not the initial ones
    return algo, buf


@pytest.mark.parametrize("ci", range(N_CASES))
def test_three_update_calls_follow_the_reference(g, ci):
    run_calls(g, ci)


def test_running_twice_gives_the_same_parameter_bits(g):
    (a, _), (b, _) = run_calls(g, 1, check=False), run_calls(g, 1, check=False)
    for n in NETS:
        assert torch.equal(hip_net(a, n).flat.data.view(torch.int32), hip_net(b, n).flat.data.view(torch.int32)), n


def test_update_draws_its_own_noise_and_subset_and_checkpoints_round_trip(g):
    """`update` end to end (sampling, the Philox draws, numpy's subset draw, the write-back to the sum tree), then the native
    and the reference checkpoint into a fresh learner: keys and shapes are the reference's, the weights come back bit for bit."""
    c = cases(g)[1]
    rows, _ = buffer_rows(g, int(g["c1_seed"]))
    buf, algo = make_buffer(g, c, rows), make_algo(g, c)
    before = {n: hip_net(algo, n).flat.data.clone() for n in NETS}
    leaves = _n(buf.weight[np.arange(64)]).copy()
    np.random.seed(3)
    want = [np.random.choice(c["E"], c["M"], replace=False) for _ in range(2)]
    seen = []
    keep = ops.redq_subset_mask
    ops.redq_subset_mask = lambda idx, E: seen.append(np.asarray(idx).copy()) or keep(idx, E)
    try:
        np.random.seed(3)
        s1, s2 = algo.update(buf, 12), algo.update(buf, 12)
    finally:
        ops.redq_subset_mask = keep
    assert all(np.array_equal(a, b) for a, b in zip(seen, want)) and len(seen) == 2
    assert s1.actor_loss == 0.0 and s1.alpha_loss is None and s2.actor_loss != 0.0 and s2.alpha_loss is not None
    assert np.isfinite([s1.critic_loss, s2.critic_loss, s2.actor_loss, s2.alpha]).all()
    assert algo.policy._sample_ctr == 3 * 12 * 3   # two target draws and one actor draw of B * act_dim normals
    for n, w in before.items():
        assert not torch.equal(w, hip_net(algo, n).flat.data), n
    assert not np.array_equal(leaves, _n(buf.weight[np.arange(64)]))
    other = make_algo(g, c)
    other.load_state_dict(algo.state_dict())
    assert (other.critic_gradient_step, other._last_actor_loss, other.policy._sample_ctr) == (2, algo._last_actor_loss, 108)
    assert torch.equal(other.alpha._log_alpha, algo.alpha._log_alpha) and torch.equal(other.alpha._alpha_dev, algo.alpha._alpha_dev)
    assert torch.equal(other.critic_optim.exp_avg, algo.critic_optim.exp_avg) and other.critic_optim.step_count == 2
    sd = algo.to_reference_state_dict()
    assert [k for k in sd] == [str(k) for k in g["sd_redq_keys"]]
    assert [",".join(str(n) for n in v.shape) for v in sd.values()] == [str(x) for x in g["sd_redq_shapes"]]
    third = make_algo(g, c)
    third.load_reference_state_dict(sd)
    for n in NETS:
        assert torch.equal(hip_net(algo, n).flat.data, hip_net(other, n).flat.data), n
        assert torch.equal(hip_net(algo, n).flat.data, hip_net(third, n).flat.data), n


def test_multi_agent_dispatch_with_a_redq_member(g):
    """Two REDQ learners over the two lanes of one joint-step `act_dim` buffer: lane k's rows and reward column reach learner k,
    whose first call equals the restatement's on the same rows."""
    cs = cases(g)
    ci = [0, 2]
    rows, RB = buffer_rows(g, int(g["c0_seed"]))
    buf = make_buffer(g, dict(prio=False), rows, n_agent=2)
    algos = [make_algo(g, cs[i]) for i in ci]
    for a, i in zip(algos, ci):
        a.noise_source = lambda B, Ad, z=[_d(g[f"c{i}_s0_z_target"])]: z.pop(0)
        a.subset_source = lambda E, M, s=g[f"c{i}_s0_subset"]: s
    ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=_Env(2))
    ma.is_within_training_step = True
    idx = g["c0_s0_indices"]
    stats = ma._update_with_batch(ma._preprocess_batch(None, buf, idx))
    fr = flat_rows(g, rows)
    n_env, S = int(g["dims"][5]), int(g["dims"][6])
    rew = np.zeros(n_env * S)
    for t, r in enumerate(rows):
        rew[np.arange(n_env) * S + t] = r["rew"]
    for k, agent in enumerate(_Env(2).agents):
        c = cs[ci[k]]
        Rk = restatement_of(g, c)
        RB.rew[:, 0] = rew * (1 + k)
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, c["n_step"], float(g["gamma"]), 0)
        r = Rk.update(fr["obs"][idx], fr["act"][idx], fr["obs_next"][idx_n], mc, gpow, vmask, g[f"c{ci[k]}_s0_subset"],
                      z_target=g[f"c{ci[k]}_s0_z_target"])
        st = stats._agent_id_to_stats[agent]
        _bar(f"marl {agent} critic_loss", st.critic_loss, r["critic_loss"], 0.0)
        assert st.actor_loss == 0.0 and st.alpha_loss is None and algos[k].critic_gradient_step == 1
