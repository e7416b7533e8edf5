"""GPU tests (`-m gpu`) of the Collector's per-step device loop under Box actions (data/collector.py): f32 [E, N, 5] actions from a
Gaussian GenericPPO, MADDPG or SAC behind the parameter-sharing wrapper, stepped through the continuous_actions=True device env
(csrc/mpe.hip) into an act_dim = 5 buffer; eager and as a captured graph."""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
E, N, H, CYCLES = 5, 3, 32, 2
POLICIES = ["ppo-local", "ppo-global", "maddpg", "sac-shared"]

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import GenericPPO, SACPolicy, policy_within_training_step
    from tianshou_marl_amd.algorithm.multiagent.ctde import DecentralizedActor, MADDPGPolicy
    from tianshou_marl_amd.algorithm.multiagent.marl import MultiAgentPolicy
    from tianshou_marl_amd.data import Collector, VectorReplayBuffer
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.utils.net import ContinuousActorProbabilistic, FlatMLP, GaussianActorCritic


def _policy(kind, env):
    D, box = env.obs_dim, env.action_space[0]
    if kind.startswith("ppo"):
        glob = kind == "ppo-global"
        net = GaussianActorCritic(D, 5, (H, H), act="tanh", critic_obs_dim=N * D if glob else None, device=DEV, seed=5)
        return GenericPPO(net=net, critic_input="global" if glob else "local", n_agent=N if glob else 1, dispatch="pooled", seed=11,
                          action_scaling=True, action_bound_method="clip", action_space=box)
    if kind == "maddpg":
        critics = [FlatMLP([N * (D + 5), H, H, 1], device=DEV, seed=50 + i) for i in range(N)]
        return MADDPGPolicy([DecentralizedActor(D, 5, H, device=DEV, seed=i) for i in range(N)], critics, None, box, N, seed=3,
                            noise_std=0.3, clip_actions=True)
    sac = [SACPolicy(actor=ContinuousActorProbabilistic(D, 5, (H, H), device=DEV, seed=4 + i), action_space=box, seed=4 + i) for i in range(N)]
    return MultiAgentPolicy(dict(zip(env.agents, [sac[0]] * N if kind == "sac-shared" else sac)), env.agent_idx)


def _sampling(pol):
    """Within a training step the policies sample: PPO its Gaussian, SAC its squashed normal (MADDPG's noise_std always acts)."""
    return policy_within_training_step(pol) if hasattr(pol, "is_within_training_step") else contextlib.nullcontext()


def _job(kind, use_graph=False, box_env=True, act_dim=5):
    env = DeviceSimpleSpreadVectorEnv(E, N, max_cycles=CYCLES, device=DEV, seed=9, continuous_actions=box_env)
    pol = _policy(kind, DeviceSimpleSpreadVectorEnv(1, N, device=DEV, continuous_actions=True))
    buf = VectorReplayBuffer(E * 16, E, act_dim=act_dim, device=DEV)
    col = Collector(pol, env, buf, use_graph=use_graph)
    col.reset()
    return env, pol, buf, col


@pytest.mark.parametrize("kind", POLICIES)
def test_collected_rows_replay_through_a_fresh_env(kind):
    env, pol, buf, col = _job(kind)
    with _sampling(pol):
        st = col.collect(n_step=3 * E)
    assert not col._can_fuse() and st.n_collected_steps == 3 * E and st.n_collected_episodes == E
    assert buf.act_store.shape == (16, E, N, 5) and buf.act_store.dtype == torch.float32
    act = buf.act_store[:3]
    assert (act != act[:, :1, :1]).any() and not torch.equal(act[0], act[1])   # per row, per step
    twin = DeviceSimpleSpreadVectorEnv(E, N, max_cycles=CYCLES, device=DEV, seed=9, continuous_actions=True)
    obs = twin.reset_device().clone()
    for t in range(3):
        # PPO steps the env with map_action of the stored sample (float64 in, as csrc/gauss.hip evaluates it; one rounding)
        a = torch.from_numpy(pol.map_action(act[t].double()).astype(np.float32)).to(DEV) if kind.startswith("ppo") else act[t]
        obs_next, rew, _, trunc, _ = twin.step_device(a.contiguous())
        for name, want in (("obs", obs), ("obs_next", obs_next), ("rew", rew), ("trunc", trunc)):
            assert torch.equal(getattr(buf, name + "_store")[t], want), (t, name)
        if kind.startswith("ppo"):   # ops.gauss_logp_entropy: "on gauss_sample's act the sample's logp, bit for bit"
            raw = FlatMLP.forward(pol.net.actor, obs.reshape(-1, env.obs_dim), save=False)
            logp = ops.gauss_logp_entropy(raw, act[t].reshape(-1, 5), **pol._gauss_kw())[0]
            assert torch.equal(buf.logp_store[t].reshape(-1), logp) and (logp != 0).all()
        obs = twin.obs_cur.clone()


@pytest.mark.parametrize("kind", POLICIES)
def test_captured_collect_equals_eager(kind):
    outs = []
    for use_graph in (False, True):
        env, pol, buf, col = _job(kind, use_graph)
        with _sampling(pol):
            stats = [col.collect(n_step=3 * E) for _ in range(3)]   # use_graph: eager, capture + replay, replay
        assert any(k[0] == "graph" for k in col._ws if isinstance(k, tuple)) == use_graph
        outs.append([getattr(buf, k + "_store").clone() for k in ("act", "obs", "obs_next", "rew", "trunc", "logp", "vs", "done")] +
                    [buf.index.state.clone(), env.obs_cur.clone(), env.rng_tick.clone(),
                     torch.as_tensor(np.concatenate([np.ravel(s.returns) for s in stats]))])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert not torch.equal(outs[0][0][3:6], outs[0][0][6:9])   # the replays draw new actions


def test_n_episode_mode_and_mismatches():
    for kind in ("ppo-local", "maddpg"):
        env, pol, buf, col = _job(kind)
        st = col.collect(n_episode=7)
        assert st.n_collected_episodes == 7 and (st.lens == CYCLES).all() and buf.act_store[:2 * CYCLES].abs().sum() > 0
    with pytest.raises(ValueError, match=r"Box\(5,\) actions but the VectorReplayBuffer stores discrete"):
        _job("ppo-local", act_dim=None)[3].collect(n_step=E)
    with pytest.raises(ValueError, match="takes discrete .* actions but GenericPPO emits Box"):
        _job("ppo-local", box_env=False, act_dim=None)[3].collect(n_step=E)
    with pytest.raises(NotImplementedError, match="independent or grouped member policies with Box actions"):
        _job("sac-independent")[3].collect(n_step=E)
