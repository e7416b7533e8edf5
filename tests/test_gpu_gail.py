"""GPU tests (`-m gpu`) of GAIL: the head and the reward (csrc/gail.hip) over the fixture grid, the reference's own PPO + GAIL
updates through `GAIL` with the fixture's permutation and expert indices, the wrapped learner against a bare PPO on the
discriminator rewards, a ragged buffer without an obs_next store, `GenericPPO` behind `GAIL`, the device plan (same seed, same
bits; a state-dict round trip), the constructor's refusals and one OnPolicyTrainer epoch.

References: tests/golden/gail.npz (the reference's own float64 and float32 runs) and the float64 restatement
(tests/gail_restatement.py, pinned to the reference by tests/test_gail_restatement.py).  Bar, per array: max |hip - ref64| <=
1e-5 max |ref64| + e_ref, e_ref = the reference's own float32 error (the restatement's float32 run where the fixture has no
such run).  What the design promises bit for bit is asserted bit for bit: the rewards after an update, the wrapped PPO against a
bare PPO on the discriminator rewards, two learners with one seed, a restored learner against the uninterrupted one."""
import copy
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "gail.npz")
DEV = "cuda"

import gail_restatement as gr  # noqa: E402
from test_gail_restatement import HEAD_CASES, up_case  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import GAIL, PPO, GailTrainingStats, GenericPPO, policy_within_training_step
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch, Collector, VectorReplayBuffer
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.trainer import OnPolicyTrainer, OnPolicyTrainerParams
    from tianshou_marl_amd.utils.net import DiscreteActorCritic, FlatMLP, MLPActorCritic

STATS = ("disc_loss", "acc_pi", "acc_exp")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _d(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _check(name, got, ref, e_ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = 1e-5 * float(np.abs(ref).max()) + float(e_ref)
    err = float(np.abs(got - ref).max())
    print(f"PARITY {name}: max |hip - ref64| = {err:.3g}, bar {tol:.3g}")
    assert err <= tol, (name, err, tol)


# ---- the head and the reward over the fixture grid ---------------------------------------------------------------------------
@pytest.mark.parametrize("Rp,Re", HEAD_CASES)
def test_head_and_reward_match_reference(g, Rp, Re):
    p = f"hd_{Rp}_{Re}_"
    lg = (g[p + "logits"].astype(np.float32) / 8.0)
    o = ops.gail_head(_d(lg), Rp)
    _check(p + "d_logits", o["d_logits"].cpu().numpy(), g[p + "d_logits"], g[p + "d_logits_eref"])
    out = ops.gail_finalize(o["partial"], Rp, Re).cpu().numpy()
    ref64, ref32 = g[p + "stats"]
    for j, name in enumerate(STATS):   # each statistic against its own magnitude
        _check(p + name, out[j:j + 1], ref64[j:j + 1], abs(ref32[j] - ref64[j]))
    p = f"rw_{Rp}_{Re}_"
    for ids in (None, g[p + "ids"]):
        store = _d(g[p + "rew0"])
        ops.gail_reward(_d(lg), store, None if ids is None else _d(ids))
        got, at = store.cpu().numpy(), (np.arange(lg.size) if ids is None else ids)
        _check(p + "rew", got[at], g[p + "rew"], g[p + "rew_eref"])
        keep = np.setdiff1d(np.arange(got.size), at)
        assert np.array_equal(got[keep], g[p + "rew0"][keep])


# ---- the learner against the running reference ---------------------------------------------------------------------------------
def _fill(buf, rows, n_env):
    T = rows["act"].shape[0]
    for t in range(T):
        buf.add(Batch(obs=rows["obs"][t][:, None], act=rows["act"][t][:, None], rew=rows["rew"][t][:, None], terminated=rows["term"][t],
                      truncated=rows["trunc"][t], obs_next=rows["obs_next"][t][:, None]), buffer_ids=np.arange(n_env))
    return buf


def _script(g, prefix, kind):
    return {k: g[f"{prefix}{kind}_{k}"] for k in ("obs", "act", "rew", "term", "trunc", "obs_next")}


class FixturePlan:
    """`_disc_plan` from recorded reference indices: flat index env * S + slot -> store pair (slot * B + env) * 1."""

    def __init__(self, g, prefix, c):
        self.g, self.prefix, self.c, self.k = g, prefix, c, 0

    def __call__(self, n_pairs):
        pk, c = f"{self.prefix}s{self.k}_", self.c
        self.k += 1
        store = lambda idx, S, B: (idx % S) * B + idx // S  # noqa: E731
        idx = self.g[pk + "indices"]
        assert n_pairs == len(idx)
        return _d(store(idx[self.g[pk + "perm"]], c["T"], c["n_env"])), _d(store(self.g[pk + "exp_idx"], c["e_T"], c["e_env"]))


@pytest.mark.parametrize("prefix", ["up_", "um_"])
def test_reference_updates_through_gail(g, prefix):
    """Reference PPO (nets 6-32-32, whole batch, repeat 2) + GAIL (disc_update_num 4): the rewards GAE read, PPO statistics, GAIL
    statistics per step and the weight digests of both nets after every update; the rewards bit-identical after each."""
    c = up_case(g, prefix)
    D, A = c["dims"][0], c["A"]
    net = MLPActorCritic(D, A, tuple(c["dims"][1:]), device=DEV, seed=0)
    net.flat.data.copy_(_d(g[prefix + "init_ppo"]))
    buf = _fill(DeviceVectorReplayBuffer(c["n_env"] * c["T"], c["n_env"], 1, D, device=DEV), _script(g, prefix, "rows"), c["n_env"])
    expert = _fill(DeviceVectorReplayBuffer(c["e_env"] * c["e_T"], c["e_env"], 1, D, device=DEV), _script(g, prefix, "exp"), c["e_env"])
    disc = FlatMLP([int(d) for d in g["disc_dims"]], "relu", device=DEV, seed=0)
    disc.flat.data.copy_(_d(g[prefix + "init_disc"]))
    algo = GAIL(net=net, lr=float(g["lr"]), dispatch="pooled", shuffle="numpy", expert_buffer=expert, disc_net=disc,
                disc_optim=AdamOptimizerFactory(lr=float(g["lr"])), disc_update_num=c["num"])
    assert isinstance(algo.wrapped_algorithm, GenericPPO)
    algo._disc_plan = FixturePlan(g, prefix, c)
    before = buf.rew_store.clone()
    seen = {}
    inner = algo.wrapped_algorithm.update

    def spy(buffer, batch_size, repeat):
        seen["rew"] = buffer.rew_store.clone()
        return inner(buffer, batch_size, repeat)

    algo.wrapped_algorithm.update = spy
    for k in range(c["n_up"]):
        np.random.seed(k)
        with policy_within_training_step(algo.policy):
            stats = algo.update(buf, None, c["repeat"])
        pk = f"{prefix}s{k}_"
        assert torch.equal(buf.rew_store, before), k
        assert isinstance(stats, GailTrainingStats) and stats.gradient_steps == c["repeat"]
        idx = g[pk + "indices"]
        rew = seen["rew"].cpu().numpy()[idx % c["T"], idx // c["T"], 0]
        _check(pk + "rew GAE read", rew, g[pk + "rew"], g[pk + "rew_eref"])
        ref64, ref32 = g[pk + "ppo_stats"]
        _check(pk + "ppo stats", [getattr(stats, s).mean for s in ("loss", "actor_loss", "vf_loss", "ent_loss")], ref64,
               np.abs(ref32 - ref64).max())
        ref64, ref32 = g[pk + "summary"]
        for j, s in enumerate(STATS):
            got = getattr(stats, s)
            _check(pk + s, [got.mean, got.std, got.max, got.min], ref64[j], np.abs(ref32[j] - ref64[j]).max())
        assert set(STATS) | {"loss"} <= set(stats.get_loss_stats_dict())
        assert algo.disc_optim.step_count == (k + 1) * len(gr.chunks(len(idx), c["num"]))
        for name, w in (("ppo", net.flat), ("disc", disc.flat)):
            w = w.double().cpu().numpy()
            _check(pk + name + " weights", w[g[pk + name + "_didx"]], g[pk + name + "_dval"], g[pk + name + "_eref"])
            _check(pk + name + " weight sum", [w.sum()], [g[pk + name + "_dsum"]], w.size * float(g[pk + name + "_eref"]))


# ---- on collected rollouts ---------------------------------------------------------------------------------------------------
def _rollout(n_env=4, T=8, seed=3, net=None, cls=None, **ppo_kw):
    torch.manual_seed(seed)
    net = net or DiscreteActorCritic(18, 5, 64, device=DEV)
    ppo = (cls or PPO)(net=net, dispatch="pooled", shuffle="device", seed=seed, lr=1e-3, **ppo_kw)
    envs = DeviceSimpleSpreadVectorEnv(n_env, 3, device=DEV, seed=seed)
    buf = VectorReplayBuffer(n_env * T, n_env)
    col = Collector(ppo, envs, buf)
    col.reset()
    with policy_within_training_step(ppo):
        col.collect(n_step=n_env * T)
    return ppo, buf, col


def _gail_like(ppo, expert, seed=3, cls_kw=None, disc_optim=None, **kw):
    """A GAIL whose wrapped learner is a copy of `ppo` (same weights, same counters)."""
    disc = FlatMLP([18 + 5, 32, 1], "relu", device=DEV, seed=7)
    # a freshly built net, filled by load_state_dict: deep-copying an MLPActorCritic clones `flat`, `actor.flat` and
    # `critic.flat` each on its own, so the copy's actor and critic would no longer alias the vector Adam steps
    src = ppo.net
    net = (MLPActorCritic(src.obs_dim, src.n_act, tuple(src.actor.dims[1:-1]), act=src.actor.act, critic_obs_dim=src.critic_obs_dim,
                          device=DEV) if isinstance(src, MLPActorCritic) else DiscreteActorCritic(src.obs_dim, src.n_act, src.hidden, device=DEV))
    algo = GAIL(net=net, dispatch="pooled", shuffle="device", seed=seed, lr=1e-3, expert_buffer=expert, disc_net=disc,
                disc_optim=disc_optim or AdamOptimizerFactory(lr=1e-3), **(cls_kw or {}), **kw)
    algo.wrapped_algorithm.load_state_dict(ppo.state_dict())
    return algo


def _disc_rewards(algo, buf, flat):
    """rew_store with the rewards of the discriminator weights `flat` at the buffer's valid pairs."""
    old = FlatMLP(algo.disc_net.dims, "relu", device=DEV, seed=0)
    old.flat.data.copy_(flat)
    ids, R = algo._buffer_pairs(buf)
    x = ops.gail_rows(buf.obs_store, buf.act_store, 5, ids=ids, R=R)
    out = buf.rew_store.clone()
    ops.gail_reward(old(x, save=False), out, ids=ids)
    return out


@pytest.mark.parametrize("use_graph", [False, True])
def test_wrapped_ppo_is_a_bare_ppo_on_the_discriminator_rewards(use_graph):
    _, expert, _ = _rollout(n_env=2, T=8, seed=9)                     # another policy's buffer, another number of envs
    ppo, buf, _ = _rollout(use_graph=use_graph)
    algo = _gail_like(ppo, expert, use_graph=use_graph)
    bare = ppo
    assert torch.equal(algo.wrapped_algorithm.net.flat.data, bare.net.flat.data)
    before = buf.rew_store.clone()
    for k in range(3):
        w_disc = algo.disc_net.flat.data.clone()
        with policy_within_training_step(algo.policy):
            stats = algo.update(buf, 32, 2)
        assert torch.equal(buf.rew_store, before), k              # bit-identical: a copy back, never arithmetic
        assert not torch.equal(algo.disc_net.flat.data, w_disc) and algo.disc_optim.step_count == 4 * (k + 1)
        # Q64: the wrapped PPO saw the rewards of the discriminator from BEFORE this update's steps
        shaped = _disc_rewards(algo, buf, w_disc)
        assert not torch.equal(shaped, before) and (shaped.view(-1)[:96] > 0).all()
        buf.rew_store.copy_(shaped)
        with policy_within_training_step(bare):
            b_stats = bare.update(buf, 32, 2)
        buf.rew_store.copy_(before)
        assert torch.equal(algo.wrapped_algorithm.net.flat.data, bare.net.flat.data), k
        assert stats.get_loss_stats_dict()["loss"] == b_stats.get_loss_stats_dict()["loss"]
        for s in STATS:
            v = getattr(stats, s)
            assert np.isfinite([v.mean, v.std, v.max, v.min]).all() and 0 <= stats.acc_pi.min <= stats.acc_pi.max <= 1


def test_discriminator_steps_match_the_restatement_on_a_collected_rollout():
    """The device plan, read back: rewards, the per-step statistics and the discriminator's weights against the restatement fed
    with the same permutation and expert pairs (N = 3 agents per row on both sides)."""
    _, expert, _ = _rollout(n_env=2, T=8, seed=9)
    ppo, buf, _ = _rollout()
    algo = _gail_like(ppo, expert)
    plans = []
    plan = algo._disc_plan
    algo._disc_plan = lambda n: plans.append(plan(n)) or plans[-1]
    refs = {dt: gr.GailRestatement(algo.disc_net.flat.double().cpu().numpy(), [23, 32, 1], 5, dtype=dt) for dt in (torch.float64, torch.float32)}
    obs, act = buf.obs_store.reshape(-1, 18).cpu().numpy()[:96], buf.act_store.reshape(-1).cpu().numpy()[:96]
    e_obs, e_act = expert.obs_store.reshape(-1, 18).cpu().numpy(), expert.act_store.reshape(-1).cpu().numpy()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buf, 32, 1)
    perm, eids = (x.cpu().numpy() for x in plans[0])
    assert sorted(perm.tolist()) == list(range(96)) and eids.shape == (4, 24) and eids.min() >= 0 and eids.max() < 2 * 8 * 3
    flat = expert.index.sample_indices_all().cpu().numpy()
    valid = (flat % expert.sub_size) * expert.buffer_num + flat // expert.sub_size
    want, _, _ = gr.draw(valid, 16, 3, 24, 3, counter=1 << 32)         # step 1 of the learner's life
    assert np.array_equal(eids[1], want)
    r64, r32 = (refs[dt].update(obs, act, perm, e_obs[eids], e_act[eids], 4) for dt in (torch.float64, torch.float32))
    for s, key in zip(STATS, ("loss", "acc_pi", "acc_exp")):
        v = getattr(stats, s)
        _check(s, [v.mean, v.max, v.min], [r64[key].mean(), r64[key].max(), r64[key].min()], np.abs(r64[key] - r32[key]).max())
    w64, w32 = refs[torch.float64].weights(), refs[torch.float32].weights()
    _check("disc weights", algo.disc_net.flat.double().cpu().numpy(), w64, np.abs(w64 - w32).max())


def test_ragged_buffer_without_obs_next():
    n_env, S, D = 3, 8, 18
    rs = np.random.RandomState(6)
    buf = DeviceVectorReplayBuffer(n_env * S, n_env, 1, D, device=DEV, ignore_obs_next=True)
    for t in range(11):
        ids = np.array([e for e, n in enumerate((11, 5, 8)) if t < n])
        o = rs.standard_normal((len(ids), 1, D)).astype(np.float32)
        buf.add(Batch(obs=o, act=rs.randint(0, 5, (len(ids), 1)), rew=rs.standard_normal((len(ids), 1)).astype(np.float32),
                      terminated=rs.rand(len(ids)) < 0.2, truncated=np.zeros(len(ids), bool), obs_next=o), buffer_ids=ids)
    _, expert, _ = _rollout(n_env=2, T=8, seed=9)
    ppo = PPO(net=DiscreteActorCritic(D, 5, 64, device=DEV), dispatch="pooled", shuffle="device", seed=5)
    algo = _gail_like(ppo, expert, seed=5)
    idx = buf.sample_indices(0)
    ids, R = algo._buffer_pairs(buf)
    assert R == 8 + 5 + 8 and np.array_equal(ids.cpu().numpy(), (idx % S) * n_env + idx // S)
    before, w_disc = buf.rew_store.clone(), algo.disc_net.flat.data.clone()
    with policy_within_training_step(algo.policy):
        stats = algo.update(buf, None, 2)
    assert torch.equal(buf.rew_store, before) and algo.disc_optim.step_count == len(gr.chunks(21, 4)) == 4
    shaped = _disc_rewards(algo, buf, w_disc)
    changed = (shaped != before).view(-1).nonzero().view(-1).cpu().numpy()
    assert np.array_equal(np.sort(changed), np.sort(ids.cpu().numpy()))   # the valid pairs' rewards, and only theirs
    buf.rew_store.copy_(shaped)
    with policy_within_training_step(ppo):
        b_stats = ppo.update(buf, None, 2)
    buf.rew_store.copy_(before)
    assert torch.equal(algo.wrapped_algorithm.net.flat.data, ppo.net.flat.data)
    assert stats.get_loss_stats_dict()["loss"] == b_stats.get_loss_stats_dict()["loss"]


def test_generic_ppo_behind_gail_with_a_wide_actor():
    """GenericPPO (128-wide actor, minibatches) behind GAIL is a bare GenericPPO on the discriminator rewards, bit for bit."""
    _, expert, _ = _rollout(n_env=2, T=8, seed=9)
    ppo, buf, _ = _rollout(net=MLPActorCritic(18, 5, (128, 128), device=DEV, seed=0), cls=GenericPPO)
    algo = _gail_like(ppo, expert)
    wrapped = algo.wrapped_algorithm
    assert isinstance(wrapped, GenericPPO) and torch.equal(wrapped.net.flat.data, ppo.net.flat.data)
    assert wrapped.net.actor.flat.data_ptr() == wrapped.net.flat.data_ptr()      # the actor steps with the joint vector
    bare = copy.deepcopy(wrapped)
    before = buf.rew_store.clone()
    for k in range(2):
        w_disc, w0 = algo.disc_net.flat.data.clone(), wrapped.net.flat.data.clone()
        with policy_within_training_step(algo.policy):
            stats = algo.update(buf, 32, 2)
        assert torch.equal(buf.rew_store, before) and not torch.equal(wrapped.net.flat.data, w0), k
        assert algo.disc_optim.step_count == 4 * (k + 1) and stats.gradient_steps == 2 * 3
        shaped = _disc_rewards(algo, buf, w_disc)
        assert not torch.equal(shaped, before)
        buf.rew_store.copy_(shaped)
        with policy_within_training_step(bare):
            b_stats = bare.update(buf, 32, 2)
        buf.rew_store.copy_(before)
        assert torch.equal(wrapped.net.flat.data, bare.net.flat.data), k
        assert stats.get_loss_stats_dict()["loss"] == b_stats.get_loss_stats_dict()["loss"] and np.isfinite(stats.disc_loss.mean)


def test_same_seed_same_bits_and_a_state_dict_round_trip_mid_run():
    _, expert, _ = _rollout(n_env=2, T=8, seed=9)
    ppo, buf, _ = _rollout()
    a, b, other = _gail_like(ppo, expert), _gail_like(ppo, expert), _gail_like(ppo, expert, seed=4)

    def step(algo):
        with policy_within_training_step(algo.policy):
            return algo.update(buf, 32, 2)

    sa, sb, so = step(a), step(b), step(other)
    assert torch.equal(a.disc_net.flat.data, b.disc_net.flat.data) and torch.equal(a.wrapped_algorithm.net.flat.data, b.wrapped_algorithm.net.flat.data)
    assert sa.disc_loss == sb.disc_loss and sa.acc_exp == sb.acc_exp
    assert not torch.equal(a.disc_net.flat.data, other.disc_net.flat.data) and so.disc_loss != sa.disc_loss
    # restore b's state into a fresh learner mid-run: it continues as the uninterrupted one does
    fresh = _gail_like(ppo, expert)
    fresh.disc_net.flat.data.zero_()
    fresh.load_state_dict(copy.deepcopy(b.state_dict()))
    assert fresh.disc_optim.step_count == a.disc_optim.step_count == 4
    sa, sf = step(a), step(fresh)
    assert torch.equal(a.disc_net.flat.data, fresh.disc_net.flat.data) and sa.disc_loss == sf.disc_loss
    assert torch.equal(a.wrapped_algorithm.net.flat.data, fresh.wrapped_algorithm.net.flat.data)


def test_a_scheduled_discriminator_learning_rate_survives_the_state_dict():
    from tianshou_marl_amd.algorithm.optim import LRSchedulerFactoryLinear

    _, expert, _ = _rollout(n_env=2, T=8, seed=9)
    ppo, buf, _ = _rollout()
    mk = lambda: _gail_like(ppo, expert, disc_optim=AdamOptimizerFactory(lr=1e-3).with_lr_scheduler_factory(  # noqa: E731
        LRSchedulerFactoryLinear(max_epochs=2, epoch_num_steps=64, collection_step_num_env_steps=32)))      # 4 updates
    a, fresh = mk(), mk()
    for algo in (a, a):
        with policy_within_training_step(algo.policy):
            algo.update(buf, 32, 1)
    assert a.disc_optim.lr == pytest.approx(0.5e-3) and fresh.disc_optim.lr == 1e-3
    fresh.load_state_dict(copy.deepcopy(a.state_dict()))
    assert fresh.disc_optim.lr == a.disc_optim.lr and fresh.disc_lr_scheduler.last_epoch == a.disc_lr_scheduler.last_epoch == 2
    for algo in (a, fresh):
        with policy_within_training_step(algo.policy):
            algo.update(buf, 32, 1)
    assert torch.equal(a.disc_net.flat.data, fresh.disc_net.flat.data) and a.disc_optim.lr == fresh.disc_optim.lr == pytest.approx(0.25e-3)


def test_rewards_are_put_back_when_the_wrapped_update_raises():
    _, expert, _ = _rollout(n_env=2, T=8, seed=9)
    ppo, buf, _ = _rollout()
    algo = _gail_like(ppo, expert)
    before = buf.rew_store.clone()
    seen = {}

    def boom(buffer, batch_size, repeat):
        seen["shaped"] = not torch.equal(buffer.rew_store, before)
        raise RuntimeError("wrapped update failed")

    algo.wrapped_algorithm.update = boom
    with policy_within_training_step(algo.policy), pytest.raises(RuntimeError, match="wrapped update failed"):
        algo.update(buf, 32, 1)
    assert seen["shaped"] and torch.equal(buf.rew_store, before)


def test_refusals():
    ppo, buf, _ = _rollout()
    mk = lambda **kw: GAIL(**{**dict(net=DiscreteActorCritic(18, 5, 64, device=DEV), dispatch="pooled", expert_buffer=buf,  # noqa: E731
                                   disc_net=FlatMLP([23, 32, 1], device=DEV, seed=0), disc_optim=AdamOptimizerFactory()), **kw})
    with pytest.raises(NotImplementedError, match="per_agent"):
        mk(dispatch="per_agent")
    with pytest.raises(ValueError, match=r"obs_dim \+ n_act = 23"):
        mk(disc_net=FlatMLP([18, 32, 1], device=DEV, seed=0))
    with pytest.raises(ValueError, match="gives 1 logit"):
        mk(disc_net=FlatMLP([23, 32, 2], device=DEV, seed=0))
    with pytest.raises(NotImplementedError, match="act_dim / act_branches"):
        mk(expert_buffer=DeviceVectorReplayBuffer(16, 2, 3, 18, device=DEV, act_dim=2))
    with pytest.raises(NotImplementedError, match="act_dim / act_branches"):
        mk(expert_buffer=DeviceVectorReplayBuffer(16, 2, 3, 18, device=DEV, act_branches=2))
    with pytest.raises(ValueError, match="expert buffer is empty"):
        mk(expert_buffer=DeviceVectorReplayBuffer(16, 2, 3, 18, device=DEV))
    with pytest.raises(ValueError, match="expert buffer is empty"):
        mk(expert_buffer=VectorReplayBuffer(16, 2))
    class HostBuffer:   # holds rows, but no device stores
        act_dim = act_branches = None

        def __len__(self):
            return 5

    with pytest.raises(TypeError, match="expert_buffer must be a device buffer"):
        mk(expert_buffer=HostBuffer())
    with pytest.raises(TypeError, match="GAIL: disc_optim"):
        mk(disc_optim=torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1))
    with pytest.raises(ValueError, match="disc_update_num = 0"):
        mk(disc_update_num=0)
    short = DeviceVectorReplayBuffer(16, 2, 3, 6, device=DEV)
    short.add(Batch(obs=np.zeros((2, 3, 6), np.float32), act=np.zeros((2, 3), np.int64), rew=np.zeros((2, 3), np.float32),
                    terminated=np.zeros(2, bool), truncated=np.zeros(2, bool), obs_next=np.zeros((2, 3, 6), np.float32)), buffer_ids=np.arange(2))
    with pytest.raises(ValueError, match="expert buffer holds observations of 6 floats, the policy takes 18"):
        mk(expert_buffer=short)
    algo = mk()
    assert algo.policy is algo.wrapped_algorithm and algo.action_dim == 5 and algo.eps_clip == 0.2 and algo.gamma == 0.99
    with pytest.raises(RuntimeError, match="outside of a training step"):
        algo.update(buf, 32, 1)
    with policy_within_training_step(algo.policy):
        assert algo.wrapped_algorithm.is_within_training_step
        with pytest.raises(ValueError, match="chunks of 0 rows"):
            big = mk(disc_update_num=97)      # 96 pairs
            big.is_within_training_step = True
            big.update(buf, 32, 1)
        with pytest.raises(NotImplementedError, match="act_dim / act_branches"):
            algo.update(DeviceVectorReplayBuffer(16, 2, 3, 18, device=DEV, act_dim=2), 32, 1)
        algo.wrapped_algorithm._grad_sync = object()
        with pytest.raises(NotImplementedError, match="data-parallel"):
            algo.update(buf, 32, 1)
    sd = mk().state_dict()
    assert set(sd) == {"wrapped", "disc_net", "disc_optim"} and sd["disc_net"].numel() == 23 * 32 + 32 + 32 + 1


def test_one_trainer_epoch_on_device_simple_spread():
    _, expert, _ = _rollout(n_env=2, T=8, seed=9)                    # collected from a second policy
    ppo, buf, col = _rollout()
    algo = GAIL(net=ppo.net, dispatch="pooled", shuffle="device", seed=3, lr=1e-3, expert_buffer=expert,
                disc_net=FlatMLP([23, 32, 1], device=DEV, seed=7), disc_optim=AdamOptimizerFactory(lr=1e-3))
    envs = DeviceSimpleSpreadVectorEnv(4, 3, device=DEV, seed=3)
    buf2 = VectorReplayBuffer(4 * 8, 4)
    col = Collector(algo, envs, buf2)
    col.reset()
    trainer = OnPolicyTrainer(algo, OnPolicyTrainerParams(train_collector=col, max_epochs=1, epoch_num_steps=64,
                                                          collection_step_num_env_steps=32, batch_size=32,
                                                          update_step_num_repetitions=1, verbose=False))
    trainer.reset()
    epoch = trainer.execute_epoch()
    losses = epoch.training_stat.get_loss_stats_dict()
    assert set(STATS) | {"loss"} <= set(losses) and np.isfinite(list(losses.values())).all()
    assert epoch.info_stat.update_step == 2 and algo.disc_optim.step_count == 8 and len(buf2) == 0
    params = OnPolicyTrainerParams(train_collector=col, max_epochs=1, epoch_num_steps=64, collection_step_num_env_steps=32,
                                   batch_size=32, update_step_num_repetitions=1, verbose=False)
    assert isinstance(algo.create_trainer(params), OnPolicyTrainer) and algo.create_trainer(params).algorithm is algo
