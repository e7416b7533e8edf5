"""GPU tests (`-m gpu`) of ICM: the head (csrc/icm.hip) over the fixture grid, the module's forward and backward, the on-policy
wrapper around PPO on a device rollout buffer (against the reference's own three PPO + ICM updates, and on a ragged buffer
without an obs_next store), the off-policy wrapper around DQN and inside MultiAgentOffPolicyAlgorithm, the reference state dict
and one OnPolicyTrainer epoch.

References: tests/golden/icm.npz (the reference's own float64 and float32 runs) and the float64 restatement
(tests/icm_restatement.py, pinned to the reference by tests/test_icm_restatement.py).  Bar, per array: max |hip - ref64| <=
1e-5 max |ref64| + e_ref, e_ref = the reference's own float32 error (the restatement's float32 run where the fixture has no
such run).  What the design promises bit for bit is asserted bit for bit: the rewards after an update, the wrapped DQN's
parameters against a bare DQN's, the wrapped PPO against a bare PPO on the shaped rewards."""
import copy
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "icm.npz")
DEV = "cuda"

from icm_restatement import IcmRestatement  # noqa: E402
from test_host_dqn import _Discrete, up_inputs  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import (DQN, PPO, DiscreteQLearningPolicy, ICMOffPolicyWrapper, ICMOnPolicyWrapper,
                                             ICMTrainingStats, policy_within_training_step)
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch, Collector, VectorReplayBuffer
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.trainer import OnPolicyTrainer, OnPolicyTrainerParams
    from tianshou_marl_amd.utils.net import DiscreteActorCritic, FlatMLP, IntrinsicCuriosityModule

STATS = ("icm_loss", "icm_forward_loss", "icm_inverse_loss")


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


def _icm(g, init=None, feat_dims=None):
    dims = [int(d) for d in (g["feat_dims"] if feat_dims is None else feat_dims)]
    m = IntrinsicCuriosityModule(feature_net=FlatMLP(dims, "relu", device=DEV, seed=0), feature_dim=dims[-1],
                                 action_dim=int(g["n_act"]), hidden_sizes=tuple(int(h) for h in g["hidden"]))
    if init is not None:
        m.flat.data.copy_(_d(np.asarray(init, np.float32)))
    return m


def _kw(g):
    return dict(lr_scale=float(g["lr_scale"]), reward_scale=float(g["reward_scale"]), forward_loss_weight=float(g["w"]))


# ---- the head over the fixture grid ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 5, 64])
@pytest.mark.parametrize("Fd", [1, 7, 16, 512])
def test_head_matches_reference(g, Fd, A):
    p = f"hd_F{Fd}_A{A}_"
    R = 37
    f = {k: (g[p + k].astype(np.float32) / 8.0) for k in ("phi2_hat", "phi2", "act_hat")}
    phi = np.zeros((R, 2, Fd), np.float32)
    phi[:, 1] = f["phi2"]
    rew = _d(g[p + "rew"])
    o = ops.icm_head(_d(f["phi2_hat"]), _d(phi.reshape(2 * R, Fd)), _d(f["act_hat"]), _d(g[p + "act"]), float(g["hd_reward_scale"]),
                     float(g["hd_w"]), float(g["hd_lr_scale"]), rew_io=rew)
    _check(p + "mse", o["mse"].cpu().numpy(), g[p + "mse"], g[p + "mse_eref"])
    _check(p + "shaped", rew.cpu().numpy(), g[p + "shaped"], g[p + "shaped_eref"])
    _check(p + "d_act_hat", o["d_act_hat"].cpu().numpy(), g[p + "d_act_hat"], g[p + "d_act_hat_eref"])
    dh = o["d_phi2_hat"].cpu().numpy().reshape(-1)
    _check(p + "d_phi2_hat", dh[g[p + "d_phi2_hat_didx"]], g[p + "d_phi2_hat_dval"], g[p + "d_phi2_hat_eref"])
    _check(p + "d_phi2_hat sum", [dh.astype(np.float64).sum()], [g[p + "d_phi2_hat_dsum"]], dh.size * float(g[p + "d_phi2_hat_eref"]))
    assert np.array_equal(o["d_phi2_fwd"].cpu().numpy().reshape(-1), -dh)
    slot = torch.empty(2, device=DEV)
    ops.qmix_finalize(o["partial"], R, slot)
    fwd, inv = (float(x) for x in slot.cpu().numpy())
    ref64, ref32 = g[p + "stats"]
    w, s = float(g["hd_w"]), float(g["hd_lr_scale"])
    _check(p + "losses", [((1 - w) * inv + w * fwd) * s, fwd, inv], ref64, np.abs(ref32 - ref64).max())


# ---- the module -----------------------------------------------------------------------------------------------------------
def test_module_forward_and_backward_match_reference(g):
    m = _icm(g, g["md_init"])
    mse, act_hat = m(g["md_s1"], g["md_act"], g["md_s2"], forward_loss_weight=float(g["w"]), lr_scale=float(g["lr_scale"]))
    _check("md mse", mse.cpu().numpy(), g["md_mse"], g["md_mse_eref"])
    _check("md act_hat", act_hat.cpu().numpy(), g["md_act_hat"], g["md_act_hat_eref"])
    slabs = m.backward()
    assert slabs.shape[1] == m.flat.numel() == g["md_grads"].size
    _check("md grads", slabs.double().sum(0).cpu().numpy(), g["md_grads"], g["md_grads_eref"])
    with pytest.raises(RuntimeError, match="before forward"):
        _icm(g).backward()
    with pytest.raises(TypeError, match="FlatMLP"):
        IntrinsicCuriosityModule(feature_net=torch.nn.Linear(6, 16), feature_dim=16, action_dim=5)
    with pytest.raises(ValueError, match="feature_dim"):
        IntrinsicCuriosityModule(feature_net=FlatMLP([6, 8], device=DEV, seed=0), feature_dim=16, action_dim=5)


def test_reference_state_dict_round_trip(g):
    m = _icm(g, g["md_init"])
    sd = m.to_reference_state_dict()
    assert list(sd.keys()) == list(g["sd_keys"])
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(g["sd_shapes"])
    other = _icm(g)
    assert not torch.equal(other.flat.data, m.flat.data)
    other.load_reference_state_dict(sd)
    assert torch.equal(other.flat.data, m.flat.data)
    assert np.array_equal(torch.cat([v.reshape(-1) for v in sd.values()]).numpy(), g["md_init"])


# ---- off-policy -----------------------------------------------------------------------------------------------------------
def _dqn(init, dims, **kw):
    net = FlatMLP(list(dims), "relu", device=DEV, seed=0)
    net.flat.data.copy_(_d(np.asarray(init, np.float32)))
    return DQN(policy=DiscreteQLearningPolicy(model=net, action_space=_Discrete(dims[-1])), optim=AdamOptimizerFactory(lr=1e-3), **kw)


def test_offpolicy_wrapped_dqn_is_the_bare_dqn_and_the_icm_trains(g):
    gd = dict(np.load(os.path.join(HERE, "golden", "dqn.npz")))
    dims, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    buf = DeviceVectorReplayBuffer(n_env * S, n_env, n_agent=1, obs_dim=dims[0], device=DEV)
    for t in range(T):
        buf.add(Batch(obs=gd["up_rows_obs"][t][:, None], act=gd["up_rows_act"][t][:, None], rew=gd["up_rows_rew"][t][:, None],
                      terminated=gd["up_rows_term"][t], truncated=gd["up_rows_trunc"][t],
                      obs_next=gd["up_rows_obs_next"][t][:, None]), buffer_ids=np.arange(n_env))
    kw = dict(gamma=float(gd["gamma"]), n_step_return_horizon=n_step, target_update_freq=freq)
    bare = _dqn(gd["up_init"], dims, **kw)
    icm = _icm(g, g["off_init"])
    algo = ICMOffPolicyWrapper(wrapped_algorithm=_dqn(gd["up_init"], dims, **kw), model=icm, optim=AdamOptimizerFactory(lr=float(g["lr"])),
                               **_kw(g))
    stores = [x.clone() for x in (buf.rew_store, buf.obs_store, buf.act_store)]
    for k in range(steps):
        idx = gd[f"up_s{k}_indices"]
        batch = algo._preprocess_batch(Batch(), buf, idx)
        _check(f"off s{k} shaped", batch.rew.cpu().numpy(), g[f"off_s{k}_shaped"], g[f"off_s{k}_shaped_eref"])
        assert np.array_equal(batch.policy.orig_rew.cpu().numpy(), RB.rew[idx, 0].astype(np.float32))
        assert batch.policy.act_hat.shape == (B, 5) and batch.policy.mse_loss.shape == (B,)
        stats = algo._update_with_batch(batch)
        algo._postprocess_batch(batch, buf, idx)
        assert torch.equal(batch.rew, batch.policy.orig_rew)
        b2 = bare._update_with_batch(bare._preprocess_batch(Batch(), buf, idx))
        # Q63: the intrinsic reward never reaches the TD target -- the wrapped learner is the bare learner, bit for bit
        assert torch.equal(algo.wrapped_algorithm.policy.model.flat.data, bare.policy.model.flat.data), k
        assert torch.equal(algo.wrapped_algorithm.target_flat, bare.target_flat) and stats.loss == b2.loss
        assert isinstance(stats, ICMTrainingStats) and set(STATS) | {"loss"} <= set(stats.get_loss_stats_dict())
        ref64, ref32 = g[f"off_s{k}_stats"]
        _check(f"off s{k} icm stats", [getattr(stats, s) for s in STATS], ref64, np.abs(ref32 - ref64).max())
        w = icm.flat.double().cpu().numpy()
        _check(f"off s{k} icm weights", w[g[f"off_s{k}_icm_didx"]], g[f"off_s{k}_icm_dval"], g[f"off_s{k}_icm_eref"])
    for x, y in zip(stores, (buf.rew_store, buf.obs_store, buf.act_store)):
        assert torch.equal(x, y)   # the buffer is untouched
    # update(): samples as the wrapped learner does, needs a training step
    with pytest.raises(RuntimeError, match="outside of a training step"):
        algo.update(buf, 16)
    algo.is_within_training_step = True
    assert algo.wrapped_algorithm.is_within_training_step and algo.policy is algo.wrapped_algorithm.policy
    st = algo.update(buf, 16)
    assert np.isfinite([st.loss, st.icm_loss]).all() and algo.optim.step_count == steps + 1


# ---- on-policy ------------------------------------------------------------------------------------------------------------
def _rollout(n_env=4, T=8, seed=3, **ppo_kw):
    torch.manual_seed(seed)
    ppo = PPO(net=DiscreteActorCritic(18, 5, 64, device=DEV), dispatch="pooled", shuffle="device", seed=seed, lr=1e-3, **ppo_kw)
    envs = DeviceSimpleSpreadVectorEnv(n_env, 3, device=DEV, seed=seed)
    buf = VectorReplayBuffer(n_env * T, n_env)
    col = Collector(ppo, envs, buf)
    col.reset()
    with policy_within_training_step(ppo):
        col.collect(n_step=n_env * T)
    return ppo, buf, col


def _on_wrapper(g, ppo, init=None):
    icm = _icm(g, init, feat_dims=[18, 32, 16])
    return ICMOnPolicyWrapper(wrapped_algorithm=ppo, model=icm, optim=AdamOptimizerFactory(lr=float(g["lr"])), **_kw(g))


@pytest.mark.parametrize("use_graph", [False, True])
def test_onpolicy_shaped_reward_drives_ppo_and_is_put_back(g, use_graph):
    ppo, buf, _ = _rollout(use_graph=use_graph)
    bare = copy.deepcopy(ppo)
    algo = _on_wrapper(g, ppo)
    init = algo.model.flat.double().cpu().numpy()
    T, L = 8, 12
    before = buf.rew_store.clone()
    obs = buf.obs_store[:T].reshape(T * L, 18).cpu().numpy()
    nxt = buf.obs_next_store[:T].reshape(T * L, 18).cpu().numpy()
    act = buf.act_store[:T].reshape(-1).cpu().numpy()
    refs = {dt: IcmRestatement(init, [18, 32, 16], 5, (32,), lr=float(g["lr"]), dtype=dt) for dt in (torch.float64, torch.float32)}
    for k in range(3):
        with policy_within_training_step(algo.policy):
            stats = algo.update(buf, 32, 2)
        assert torch.equal(buf.rew_store, before), k   # bit-identical: a copy back, never a subtraction
        r64, r32 = (refs[dt].update(obs, act, nxt, float(g["w"]), float(g["lr_scale"])) for dt in (torch.float64, torch.float32))
        e = max(abs(r64[s] - r32[s]) for s in STATS)
        _check(f"on s{k} icm stats", [getattr(stats, s) for s in STATS], [r64[s] for s in STATS], e)
        _check(f"on s{k} icm weights", algo.model.flat.double().cpu().numpy(), refs[torch.float64].weights(),
               np.abs(refs[torch.float64].weights() - refs[torch.float32].weights()).max())
        # Q62: the wrapped PPO saw the shaped reward -- a bare PPO on a buffer holding rew + mse * reward_scale is the same PPO
        mse = algo.model.head["mse"]
        shaped = before.clone()
        shaped.view(-1)[:T * L] += mse * torch.tensor(float(g["reward_scale"]), dtype=torch.float32, device=DEV)
        assert not torch.equal(shaped, before)
        buf.rew_store.copy_(shaped)
        with policy_within_training_step(bare):
            b_stats = bare.update(buf, 32, 2)
        buf.rew_store.copy_(before)
        assert torch.equal(ppo.net.flat.data, bare.net.flat.data), k
        assert stats.get_loss_stats_dict()["loss"] == b_stats.get_loss_stats_dict()["loss"]
        assert set(STATS) <= set(stats.get_loss_stats_dict())


def test_onpolicy_rewards_are_put_back_when_the_wrapped_update_raises(g, monkeypatch):
    ppo, buf, _ = _rollout()
    algo = _on_wrapper(g, ppo)
    before, w0 = buf.rew_store.clone(), algo.model.flat.data.clone()
    seen = {}

    def boom(buffer, batch_size, repeat):
        seen["shaped"] = not torch.equal(buffer.rew_store, before)
        raise RuntimeError("wrapped update failed")

    monkeypatch.setattr(ppo, "update", boom)
    with policy_within_training_step(ppo), pytest.raises(RuntimeError, match="wrapped update failed"):
        algo.update(buf, 32, 1)
    assert seen["shaped"] and torch.equal(buf.rew_store, before) and torch.equal(algo.model.flat.data, w0)
    with pytest.raises(RuntimeError, match="outside of a training step"):
        algo.update(buf, 32, 1)


def test_refusals(g):
    ppo = PPO(net=DiscreteActorCritic(18, 5, 64, device=DEV), dispatch="per_agent")
    with pytest.raises(NotImplementedError, match="per_agent"):
        _on_wrapper(g, ppo)
    pooled = PPO(net=DiscreteActorCritic(18, 5, 64, device=DEV), dispatch="pooled")
    pooled._grad_sync = object()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        _on_wrapper(g, pooled)
    with pytest.raises(TypeError, match="IntrinsicCuriosityModule"):
        ICMOnPolicyWrapper(wrapped_algorithm=PPO(net=DiscreteActorCritic(18, 5, 64, device=DEV), dispatch="pooled"),
                           model=FlatMLP([18, 16], device=DEV, seed=0), optim=AdamOptimizerFactory(), **_kw(g))


def test_one_trainer_epoch_on_device_simple_spread(g):
    ppo, buf, col = _rollout()
    col.reset_buffer()
    algo = _on_wrapper(g, ppo)
    trainer = OnPolicyTrainer(algo, OnPolicyTrainerParams(train_collector=col, max_epochs=1, epoch_num_steps=64,
                                                          collection_step_num_env_steps=32, batch_size=32,
                                                          update_step_num_repetitions=1, verbose=False))
    trainer.reset()
    epoch = trainer.execute_epoch()
    losses = epoch.training_stat.get_loss_stats_dict()
    assert set(STATS) <= set(losses) and np.isfinite(list(losses.values())).all()
    assert epoch.info_stat.update_step == 2 and algo.optim.step_count == 2 and len(buf) == 0


# ---- on-policy against the running reference (icm.npz on_*) ----------------------------------------------------------------
def test_three_onpolicy_updates_match_reference(g):
    """Reference PPO (nets 6-32-32) + ICMOnPolicyWrapper (F 16), whole batch, repeat 2: PPO statistics, ICM statistics and the
    weight digests of both after each of three updates; the rewards bit-identical after each."""
    from tianshou_marl_amd.algorithm import GenericPPO
    from tianshou_marl_amd.utils.net import MLPActorCritic

    *dims, A, n_env, T, repeat, steps = (int(x) for x in g["on_dims"])
    net = MLPActorCritic(dims[0], A, tuple(dims[1:]), device=DEV, seed=0)
    assert net.flat.numel() == g["on_init_ppo"].size
    net.flat.data.copy_(_d(g["on_init_ppo"]))
    ppo = GenericPPO(net=net, lr=float(g["lr"]), dispatch="pooled", shuffle="numpy")
    buf = DeviceVectorReplayBuffer(n_env * T, n_env, 1, dims[0], device=DEV)
    for t in range(T):
        buf.add(Batch(obs=g["on_rows_obs"][t][:, None], act=g["on_rows_act"][t][:, None], rew=g["on_rows_rew"][t][:, None],
                      terminated=g["on_rows_term"][t], truncated=g["on_rows_trunc"][t], obs_next=g["on_rows_obs_next"][t][:, None]),
                buffer_ids=np.arange(n_env))
    algo = ICMOnPolicyWrapper(wrapped_algorithm=ppo, model=_icm(g, g["on_init_icm"]), optim=AdamOptimizerFactory(lr=float(g["lr"])),
                              **_kw(g))
    before = buf.rew_store.clone()
    for k in range(steps):
        np.random.seed(k)
        with policy_within_training_step(algo.policy):
            stats = algo.update(buf, None, repeat)
        assert torch.equal(buf.rew_store, before), k
        assert stats.gradient_steps == repeat
        pk = f"on_s{k}_"
        ref64, ref32 = g[pk + "ppo_stats"]
        _check(pk + "ppo stats", [getattr(stats, s).mean for s in ("loss", "actor_loss", "vf_loss", "ent_loss")], ref64,
               np.abs(ref32 - ref64).max())
        ref64, ref32 = g[pk + "icm_stats"]
        _check(pk + "icm stats", [getattr(stats, s) for s in STATS], ref64, np.abs(ref32 - ref64).max())
        for name, w in (("ppo", net.flat), ("icm", algo.model.flat)):
            w = w.double().cpu().numpy()
            _check(pk + name + " weights", w[g[pk + name + "_didx"]], g[pk + name + "_dval"], g[pk + name + "_eref"])
            _check(pk + name + " weight sum", [w.sum()], [g[pk + name + "_dsum"]], w.size * float(g[pk + name + "_eref"]))


def test_onpolicy_rows_of_a_ragged_buffer_without_obs_next(g):
    """`_buffer_rows` on sub-buffers of uneven length, one of them wrapped around, and no obs_next store: obs_next is obs at the
    buffer's `next` index, the shaped entries are the valid rows' and every other reward stays bit-identical."""
    from dqn_restatement import RestatedBuffer

    n_env, S, D = 3, 8, 18
    rs = np.random.RandomState(6)
    buf = DeviceVectorReplayBuffer(n_env * S, n_env, 1, D, device=DEV, ignore_obs_next=True)
    assert buf.obs_next_store is None
    RB = RestatedBuffer(n_env, S, 1)
    obs_np, act_np = np.zeros((n_env * S, D), np.float32), np.zeros(n_env * S, np.int64)
    for t in range(11):
        ids = np.array([e for e, n in enumerate((11, 5, 8)) if t < n])
        o, a = rs.standard_normal((len(ids), 1, D)).astype(np.float32), rs.randint(0, 5, (len(ids), 1))
        r, term = rs.standard_normal((len(ids), 1)).astype(np.float32), rs.rand(len(ids)) < 0.2
        buf.add(Batch(obs=o, act=a, rew=r, terminated=term, truncated=np.zeros(len(ids), bool), obs_next=o), buffer_ids=ids)
        for j, e in enumerate(ids):
            cur = RB.add(int(e), r[j, 0], bool(term[j]), False)
            obs_np[cur], act_np[cur] = o[j, 0], a[j, 0]
    ppo = PPO(net=DiscreteActorCritic(D, 5, 64, device=DEV), dispatch="pooled")
    algo = _on_wrapper(g, ppo)
    idx = RB.sample_indices_all()
    assert len(idx) == 8 + 5 + 8 and np.array_equal(idx, buf.sample_indices(0))
    x, act, ids = algo._buffer_rows(buf)
    want = np.stack([obs_np[idx], obs_np[RB.next(idx)]], 1).reshape(-1, D)
    assert np.array_equal(x.cpu().numpy(), want) and np.array_equal(act.cpu().numpy(), act_np[idx])
    store_pos = (idx % S) * n_env + idx // S        # rew_store is [slot, env, agent]
    assert np.array_equal(ids.cpu().numpy(), store_pos)
    before = buf.rew_store.clone()
    mse, _ = algo._icm_forward(x, act, rew_io=buf.rew_store, ids=ids)
    b, a = before.cpu().numpy().reshape(-1), buf.rew_store.cpu().numpy().reshape(-1)
    want_store = b.copy()
    want_store[store_pos] = b[store_pos] + mse.cpu().numpy() * np.float32(float(g["reward_scale"]))
    assert np.array_equal(a, want_store) and (a != b).sum() == len(idx)
    refs = {dt: IcmRestatement(algo.model.flat.double().cpu().numpy(), [18, 32, 16], 5, (32,), dtype=dt).loss_grads(
        obs_np[idx], act_np[idx], obs_np[RB.next(idx)], float(g["w"]), float(g["lr_scale"])) for dt in (torch.float64, torch.float32)}
    _check("ragged mse", mse.cpu().numpy(), refs[torch.float64]["mse"], np.abs(refs[torch.float64]["mse"] - refs[torch.float32]["mse"]).max())


def test_module_needs_the_loss_weights_to_keep_a_gradient(g):
    m = _icm(g, g["md_init"])
    with pytest.raises(ValueError, match="forward_loss_weight"):
        m(g["md_s1"], g["md_act"], g["md_s2"])
    mse, _ = m(g["md_s1"], g["md_act"], g["md_s2"], save=False)
    assert m.head is None and mse.shape == (37,)
    with pytest.raises(RuntimeError, match="before forward"):
        m.backward()


# ---- inside MultiAgentOffPolicyAlgorithm ----------------------------------------------------------------------------------
def test_offpolicy_wrapper_as_an_agents_learner(g):
    from test_host_dqn import _Env
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm

    rs = np.random.RandomState(8)
    N, E, T, D, A = 2, 4, 6, 6, 5
    buf = DeviceVectorReplayBuffer(E * 8, E, n_agent=N, obs_dim=D, device=DEV)
    for t in range(T):
        buf.add(Batch(obs=rs.randn(E, N, D).astype(np.float32), act=rs.randint(0, A, (E, N)), rew=rs.randn(E, N).astype(np.float32),
                      terminated=rs.rand(E) < 0.2, truncated=rs.rand(E) < 0.1, obs_next=rs.randn(E, N, D).astype(np.float32)))
    mk = lambda i: _dqn(np.random.RandomState(30 + i).standard_normal(6 * 16 + 16 + 16 * 5 + 5) * 0.3, [D, 16, A],  # noqa: E731
                        n_step_return_horizon=3, target_update_freq=2)
    alone = [mk(i) for i in range(N)]
    ours = [ICMOffPolicyWrapper(wrapped_algorithm=mk(i), model=_icm(g, g["off_init"]), optim=AdamOptimizerFactory(lr=float(g["lr"])),
                                **_kw(g)) for i in range(N)]
    ma = MultiAgentOffPolicyAlgorithm(algorithms=ours, env=_Env(N))
    ma.is_within_training_step = True
    assert all(o.wrapped_algorithm.is_within_training_step for o in ours)
    rew = buf.rew_store.clone()
    stats = ma.update(buf, 0).get_loss_stats_dict()
    idx = buf.sample_indices(0)
    obs, nxt, act = (buf._gather(s, _d(idx)) for s in (buf.obs_store, buf.obs_next_store, buf.act_store))
    for k in range(N):
        s = alone[k]._update_with_batch(alone[k]._preprocess_batch(Batch(), buf, idx, agent=k))
        assert stats[f"agent_{k}/loss"] == s.loss and np.isfinite(s.loss)
        assert torch.equal(ours[k].wrapped_algorithm.policy.model.flat.data, alone[k].policy.model.flat.data)   # Q63, per agent
        refs = [IcmRestatement(g["off_init"], g["feat_dims"], A, (32,), lr=float(g["lr"]), dtype=dt).update(
            obs[:, k].cpu().numpy(), act[:, k].cpu().numpy(), nxt[:, k].cpu().numpy(), float(g["w"]), float(g["lr_scale"]))
            for dt in (torch.float64, torch.float32)]
        _check(f"agent {k} icm stats", [stats[f"agent_{k}/{n}"] for n in STATS], [refs[0][n] for n in STATS],
               max(abs(refs[0][n] - refs[1][n]) for n in STATS))
        assert ours[k].optim.step_count == 1
    assert stats["agent_0/icm_loss"] != stats["agent_1/icm_loss"] and torch.equal(buf.rew_store, rew)
    ma.update(buf, 9)   # a sampled subset runs too
