"""CPU tests of the continuous-action actor-critics (DDPG, TD3, SAC): the float64 restatement (tests/cac_restatement.py)
against the reference's own float64 run in tests/golden/cac.npz at 1e-10, a central difference of the closed-form SAC actor
gradient, constructor signatures and checkpoint keys against the reference's, the `act_dim` buffer's host-side contract, and the
host-side refusals of the new wrappers and of `tsm_cac_check`.  Nothing is launched."""
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "cac.npz")

from cac_restatement import CacRestatement, alpha_state, sac_action, sac_actor_head  # noqa: E402
from dqn_restatement import RestatedBuffer, nstep_walk  # noqa: E402

from tianshou_marl_amd import _abi, _build, ops  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def cases(g):
    out = []
    for i, c in enumerate(g["cases"]):
        kind, n_step, prio, alpha, unb, no_c2, *cond = str(c).split("|")
        out.append(dict(i=i, kind=kind, n_step=int(n_step), prio=bool(int(prio)), alpha=alpha, unbounded=bool(int(unb)),
                        no_c2=bool(int(no_c2)), cond=bool(int(cond[0])) if cond else True))
    return out


N_CASES = 11


def dims_of(g, c):
    """(actor dims, critic dims); a SAC actor with sigma_param emits mu_raw alone."""
    D, Ad, h1, h2 = (int(x) for x in g["dims"][:4])
    return [D, h1, h2, 2 * Ad if c["kind"] == "sac" and c["cond"] else Ad], [D + Ad, h1, h2, 1]


def buffer_rows(g, seed):
    """The generator's hand-filled buffer, drawn again from its seed: per time step the rows of every env."""
    D, Ad = int(g["dims"][0]), int(g["dims"][1])
    n_env, S, T = (int(x) for x in g["dims"][5:8])
    rs = np.random.RandomState(seed + 1000)
    rows = []
    RB = RestatedBuffer(n_env, S, 1)
    for _ in range(T):
        term, trunc = rs.rand(n_env) < 0.12, rs.rand(n_env) < 0.08
        rew = rs.standard_normal(n_env).astype(np.float32)
        obs = rs.standard_normal((n_env, D)).astype(np.float32)
        act = rs.uniform(-1, 1, (n_env, Ad)).astype(np.float32)
        nxt = rs.standard_normal((n_env, D)).astype(np.float32)
        rows.append(dict(obs=obs, act=act, rew=rew, terminated=term, truncated=trunc, obs_next=nxt))
        for e in range(n_env):
            RB.add(e, rew[e], bool(term[e]), bool(trunc[e]))
    return rows, RB


def flat_rows(g, rows):
    """obs, act, obs_next by flat index env * S + slot."""
    n_env, S, T = (int(x) for x in g["dims"][5:8])
    out = {k: np.zeros((n_env * S,) + rows[0][k].shape[1:], np.float32) for k in ("obs", "act", "obs_next")}
    for t, r in enumerate(rows):
        for k in out:
            out[k][np.arange(n_env) * S + t] = r[k]
    return out


def restatement_of(g, c):
    a_dims, c_dims = dims_of(g, c)
    pk = f"c{c['i']}_"
    init = {n: g[pk + "init_" + n] for n in ("actor", "critic", "critic2") if pk + "init_" + n in g}
    pn, nc, freq = g["td3"]
    fixed, la, te = g["sac"]
    alpha = alpha_state(float(la)) if c["alpha"] == "auto" else float(fixed)
    return CacRestatement(c["kind"], init, a_dims, c_dims, float(g["tau"]), lr=float(g["lr"]), max_action=float(g["max_action"]),
                          unbounded=c["unbounded"], policy_noise=float(pn), noise_clip=float(nc), update_actor_freq=int(freq),
                          alpha=alpha, target_entropy=float(te), alpha_lr=float(g["lr"]))


def net_names(kind):
    return {"ddpg": ["actor", "critic", "critic_old", "actor_old"],
            "td3": ["actor", "critic", "critic_old", "critic2", "critic2_old", "actor_old"],
            "sac": ["actor", "critic", "critic_old", "critic2", "critic2_old"]}[kind]


def mine_stats(kind, r):
    one = kind == "ddpg"
    return np.array([r["actor_loss"], r["critic1_loss"] if one else np.nan, np.nan if one else r["critic1_loss"],
                     np.nan if one else r["critic2_loss"], r.get("alpha", np.nan) if kind == "sac" else np.nan,
                     np.nan if r["alpha_loss"] is None else r["alpha_loss"]])


@pytest.mark.parametrize("ci", range(N_CASES))
def test_restatement_follows_the_reference_float64_run(g, ci):
    c = cases(g)[ci]
    assert len(cases(g)) == N_CASES
    pk = f"c{ci}_"
    rows, RB = buffer_rows(g, int(g[pk + "seed"]))
    fr = flat_rows(g, rows)
    R = restatement_of(g, c)
    for k in range(2):
        sk = f"{pk}s{k}_"
        idx = g[sk + "indices"]
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, c["n_step"], float(g["gamma"]), 0)
        r = R.update(fr["obs"][idx], fr["act"][idx], fr["obs_next"][idx_n], mc, gpow, vmask,
                     weight=g.get(sk + "weight_in"), z_target=g.get(sk + "z_target"), z_actor=g.get(sk + "z_actor"))
        assert np.allclose(mine_stats(c["kind"], r), g[sk + "stats"], rtol=1e-10, atol=0, equal_nan=True)
        assert np.allclose(r["returns"], g[sk + "returns"], rtol=1e-10, atol=1e-13)
        assert np.allclose(r["prio"], g[sk + "prio"], rtol=1e-10, atol=1e-13)
        assert ("actor" in r["grads"]) == bool(g[sk + "actor_stepped"])
        for n, gv in r["grads"].items():
            assert np.allclose(gv, g[f"{sk}grad_{n}"], rtol=1e-10, atol=1e-15), (k, n)
        if c["alpha"] == "auto":
            assert np.isclose(R.alpha["log_alpha"], g[sk + "log_alpha"][0], rtol=1e-10)
    for n in net_names(c["kind"]):
        assert np.allclose(R.weights(n), g[f"{pk}s1_w_{n}"], rtol=1e-10, atol=1e-13), n
    assert R.kink > float(g["delta"])


@pytest.mark.parametrize("unbounded", [False, True])
def test_closed_form_sac_actor_gradient_matches_a_central_difference(unbounded):
    rs = np.random.RandomState(3)
    B, Ad = 5, 4
    m, s, z = rs.standard_normal((B, Ad)), rs.uniform(-2, 1, (B, Ad)), rs.standard_normal((B, Ad))
    s[0, 0], s[1, 1] = 2.5, -20.5                      # past both clamp ends: no gradient
    c1, c2 = rs.standard_normal((B, Ad)), rs.standard_normal((B, Ad))   # linear critics: q_i = c_i . a + b_i
    b1, b2 = rs.standard_normal(B), rs.standard_normal(B)
    alpha, M = 0.3, 1.5

    def loss(m_, s_):
        o = sac_action(m_, s_, z, M, unbounded)
        return float((alpha * o["logp"] - np.minimum((c1 * o["a"]).sum(1) + b1, (c2 * o["a"]).sum(1) + b2)).mean())

    a = sac_action(m, s, z, M, unbounded)["a"]
    ah = sac_actor_head(m, s, z, (c1 * a).sum(1) + b1, (c2 * a).sum(1) + b2, c1, c2, alpha, M, unbounded)
    assert ah["gap"] > 1e-3 and np.isclose(ah["loss"], loss(m, s), rtol=1e-13)
    h = 1e-6
    for arr, d in ((m, ah["d_mu"]), (s, ah["d_sigma"])):
        for i in range(B):
            for k in range(Ad):
                keep = arr[i, k]
                arr[i, k] = keep + h
                up = loss(m, s)
                arr[i, k] = keep - h
                dn = loss(m, s)
                arr[i, k] = keep
                assert abs((up - dn) / (2 * h) - d[i, k]) < 1e-7 * max(1.0, abs(d[i, k])), (i, k)
    assert ah["d_sigma"][0, 0] == 0.0 and ah["d_sigma"][1, 1] == 0.0


def test_signatures_and_defaults_are_the_reference_ones(g):
    from tianshou_marl_amd.algorithm import DDPG, SAC, TD3, ContinuousDeterministicPolicy, SACPolicy

    for cls in (ContinuousDeterministicPolicy, SACPolicy, DDPG, TD3, SAC):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        mine = [f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}" for q in ps]
        ref = [str(x) for x in g[f"sig_{cls.__name__}"]]
        assert mine[:len(ref)] == ref, (cls.__name__, mine, ref)
        assert all(q.default is not inspect.Parameter.empty for q in ps[len(ref):])   # extras (seed) have defaults
        assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for q in ps)


class _Box:
    def __init__(self, n, low=-1.0, high=1.0):
        self.low, self.high, self.shape = np.full(n, low, np.float32), np.full(n, high, np.float32), (n,)


def cpu_learner(g, kind):
    """A learner of the fixture's sizes on the host (nothing is launched: construction and checkpoints only).
    kind: ddpg | td3 | sac (conditioned sigma, AutoAlpha) | sacp (sigma_param, fixed alpha)."""
    from tianshou_marl_amd.algorithm import DDPG, SAC, TD3, AutoAlpha, ContinuousDeterministicPolicy, SACPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import ContinuousActorDeterministic, ContinuousActorProbabilistic, ContinuousCritic

    D, Ad, h1, h2 = (int(x) for x in g["dims"][:4])
    opt = lambda: AdamOptimizerFactory(lr=1e-3)  # noqa: E731
    crit = lambda s: ContinuousCritic(D, Ad, (h1, h2), device="cpu", seed=s)  # noqa: E731
    common = dict(policy_optim=opt(), critic=crit(1), critic_optim=opt())
    if kind in ("sac", "sacp"):
        actor = ContinuousActorProbabilistic(D, Ad, (h1, h2), conditioned_sigma=kind == "sac", device="cpu", seed=0)
        alpha = AutoAlpha(-float(Ad), -1.0, opt()) if kind == "sac" else 0.2
        return SAC(policy=SACPolicy(actor=actor, action_space=_Box(Ad)), critic2=crit(2), alpha=alpha, **common)
    pol = ContinuousDeterministicPolicy(actor=ContinuousActorDeterministic(D, Ad, (h1, h2), device="cpu", seed=0), action_space=_Box(Ad))
    return DDPG(policy=pol, **common) if kind == "ddpg" else TD3(policy=pol, critic2=crit(2), **common)


@pytest.mark.parametrize("kind", ["ddpg", "td3", "sac", "sacp"])
def test_reference_checkpoint_keys_round_trip(g, kind):
    """`to_reference_state_dict()` of a learner gives the reference's state_dict keys, in its order and with its shapes
    (recorded from the reference's learners around Net + ContinuousActor* / ContinuousCritic), and loads back bit for bit."""
    algo = cpu_learner(g, kind)
    sd = algo.to_reference_state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f"sd_{kind}_keys"]]
    assert [",".join(str(n) for n in v.shape) for v in sd.values()] == [str(x) for x in g[f"sd_{kind}_shapes"]]
    other = cpu_learner(g, kind)
    for _, net in other._nets():
        net.flat.data.add_(1.0)
    other.load_reference_state_dict(sd)
    for (_, a), (_, b) in zip(algo._nets(), other._nets()):
        assert torch.equal(a.flat.data, b.flat.data)
    native = algo.state_dict()
    assert ("_cnt" in native and "_last" in native) == (kind == "td3") and ("alpha" in native) == (kind == "sac")
    assert ("critic2_optim" in native) == (kind != "ddpg")


def test_probabilistic_actor_keeps_the_reference_default_and_a_sigma_param_slot(g):
    from tianshou_marl_amd.utils.net import ContinuousActorProbabilistic, lagged_copy

    sig = inspect.signature(ContinuousActorProbabilistic.__init__).parameters
    assert sig["conditioned_sigma"].default is False and not bool(g["default_conditioned_sigma"])
    net = ContinuousActorProbabilistic(6, 3, (16, 16), device="cpu", seed=0)
    n = net.n_mlp_params
    assert net.dims[-1] == 3 and net.flat.numel() == n + 3 and not net.sigma_param.any()   # zeros, continuous.py:222
    assert net.sigma_param.data_ptr() == net.flat.data[n:].data_ptr() and net.weight(0).data_ptr() == net.flat.data.data_ptr()
    net.sigma_param.copy_(torch.tensor([0.5, -1.0, 0.25]))
    twin = lagged_copy(net)
    assert torch.equal(twin.flat.data, net.flat.data) and twin.flat.data_ptr() != net.flat.data_ptr()
    # what lies behind the layers on the flat vector, as `FlatAdam.state_dict` lists it: sigma_param, or nothing
    layers = [(16, 6), (16,), (16, 16), (16,), (3, 16), (3,)]
    assert twin.param_shapes() == layers + [(3, 1)]
    assert ContinuousActorProbabilistic(6, 3, (16,), conditioned_sigma=True, device="cpu").param_shapes() == [(16, 6), (16,), (6, 16), (6,)]
    from tianshou_marl_amd.utils.net import FlatAdam
    shapes = FlatAdam(net)._shapes()
    assert shapes[-1] == (3, 1) and sum(int(np.prod(x)) for x in shapes) == net.flat.numel()


def test_act_dim_none_is_the_old_buffer_and_aec_refuses():
    from tianshou_marl_amd.data.buffer import DeviceAECReplayBuffer, DeviceVectorReplayBuffer, VectorReplayBuffer

    sig = inspect.signature(DeviceVectorReplayBuffer.__init__).parameters
    assert sig["act_dim"].default is None
    assert DeviceVectorReplayBuffer.unfused_adds_only is False
    # (the stores themselves are HBM allocations made by a launch: test_gpu_cac.py compares them with and without act_dim)
    with pytest.raises(NotImplementedError, match="discrete actions only"):
        DeviceAECReplayBuffer(8, 2, ["a", "b"], 4, act_dim=2)
    with pytest.raises(ValueError, match="at least one component"):
        DeviceVectorReplayBuffer(8, 2, 1, 4, device="cpu", act_dim=0)
    lazy = VectorReplayBuffer(8, 2, act_dim=3)   # passes through to the lazy allocation
    assert lazy._lazy["kwargs"] == dict(act_dim=3) and len(lazy) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    z, q, u = torch.zeros(4, 3), torch.zeros(4), torch.zeros(4, dtype=torch.uint8)
    one = torch.zeros(1)
    calls = [lambda: ops.cac_col_sum(z, z), lambda: ops.cac_det_action(z), lambda: ops.sac_action(torch.zeros(4, 6)), lambda: ops.cac_target(q, q, q, q, u),
             lambda: ops.cac_critic_head(q, q, q), lambda: ops.cac_det_actor_head(z, z, q),
             lambda: ops.sac_actor_head(torch.zeros(4, 6), z, q, q, z, z, one), lambda: ops.cac_normal(8, 0, device="cpu")]
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


def test_cac_check_bounds_through_the_abi():
    _build.build()
    _abi.load()
    assert _abi.CAC_MAX_ACT_DIM == 64 and _abi.CAC_ROWS_PER_BLOCK == 16
    _abi.call("tsm_cac_check", 1, 1)
    _abi.call("tsm_cac_check", _abi.CAC_MAX_ACT_DIM, 3)
    with pytest.raises(ValueError, match=r"act_dim = 65 outside \[1, 64\]"):
        _abi.call("tsm_cac_check", _abi.CAC_MAX_ACT_DIM + 1, 1)
    with pytest.raises(ValueError, match=r"act_dim = 0 outside"):
        ops.cac_check(0)
    with pytest.raises(ValueError, match="greater than 0 but got: 0"):
        ops.cac_check(3, 0)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_cac_target", None, None, None, None, None, None, None, 4, None, None)
    with pytest.raises(ValueError, match="leave the row"):
        _abi.call("tsm_cac_det_action", 1, None, 4, 3, 1.0, 0.0, 0.0, 1, 5, 3, None, None)
