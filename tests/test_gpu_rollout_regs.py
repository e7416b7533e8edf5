"""GPU tests (`-m gpu`) of the eight-wave tile form of the persistent rollout (csrc/rollout.hip with csrc/rollout_fwd.h): its forward
keeps a wave's weight fragments in registers for the whole launch and its hidden activations k-fragment-major in LDS, and the
observation rows of a step are stored beside the next step's head.  None of that may change a bit: every store of the launch is compared
with `torch.equal` against the unfused sequence policy_forward -> mpe_step -> vrb_add, at the tile's edges (a full tile, a ragged second
tile, a single env), with episodes ending inside the launch / at its last step / not at all (the bootstrap pass then writes v_next),
through the `<18, 3>` and the generic instantiation, sampling and argmax."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.ppo import PPO, policy_within_training_step
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.utils.net import DiscreteActorCritic

DEV = "cuda"


def _collect(n_env, N, max_cycles, steps, fused, mode, generic, seed=5):
    env = DeviceSimpleSpreadVectorEnv(n_env, N, max_cycles=max_cycles, device=DEV, seed=seed)
    net = DiscreteActorCritic(env.obs_dim, env.n_act, 64, device=DEV, seed=seed)
    algo = PPO(net=net, seed=seed, deterministic_eval=mode == 2)
    buf = DeviceVectorReplayBuffer(n_env * (steps + 1), n_env, N, env.obs_dim, device=DEV)
    col = Collector(algo, env, buf, fused_rollout=fused, use_graph=False)
    col.reset()
    assert col._can_fuse() == fused
    with ops.kernel_override(rollout_form=1, generic_kernels=generic):   # the tile form (eight waves at these sizes)
        if mode == 1:
            with policy_within_training_step(algo):
                st = col.collect(n_step=n_env * steps)
        else:
            st = col.collect(n_step=n_env * steps)   # deterministic_eval outside a training step: dist.mode
    torch.cuda.synchronize()
    out = dict(
        obs=buf.obs_store.clone(), obs_next=buf.obs_next_store.clone(), act=buf.act_store.clone(), rew=buf.rew_store.clone(),
        trunc=buf.trunc_store.clone(), term=buf.term_store.clone(), logp=buf.logp_store.clone(), vs=buf.vs_store.clone(),
        done=buf.done_store.clone(), state=buf.index.state.clone(), apos=env.agent_pos.clone(), avel=env.agent_vel.clone(),
        lpos=env.landmark_pos.clone(), steps=env.steps.clone(), ep=env.episode_ctr.clone(), obs_cur=env.obs_cur.clone(),
        tick=env.rng_tick.clone(), returns=np.asarray(st.returns).copy(), lens=np.asarray(st.lens).copy(),
        n_ep=st.n_collected_episodes)
    return out, buf, net, env


# (n_env, N, max_cycles, steps, generic_kernels)
CASES = [
    (5, 3, 25, 6, 0),    # one full tile (15 of 16 rows); no episode ends: the bootstrap pass writes the last row's v_next
    (7, 3, 25, 5, 0),    # a ragged second tile with 2 envs
    (1, 3, 25, 5, 0),    # a single env
    (7, 3, 3, 7, 0),     # episodes end inside the launch (steps 3 and 6), the launch ends inside an episode
    (7, 3, 3, 6, 0),     # ... and at the launch's last step
    (6, 4, 25, 5, 0),    # N = 4, D = 24: the generic instantiation (W1 stays in LDS), two tiles
    (6, 4, 2, 5, 0),     # ... with episode ends
    (7, 3, 3, 7, 1),     # N = 3 through the generic instantiation
]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n_env,N,max_cycles,steps,generic", CASES)
def test_eight_wave_rollout_stores_the_unfused_bits(n_env, N, max_cycles, steps, generic, mode):
    ref, _, _, _ = _collect(n_env, N, max_cycles, steps, False, mode, generic)
    got, buf, net, env = _collect(n_env, N, max_cycles, steps, True, mode, generic)
    for k in ref:
        if isinstance(ref[k], torch.Tensor):
            assert torch.equal(ref[k], got[k]), k
        elif isinstance(ref[k], np.ndarray):
            assert np.array_equal(ref[k], got[k]), k
        else:
            assert ref[k] == got[k], k
    # v_next of every stored row (next step's forward, terminal-observation forward, bootstrap pass) == a critic pass over obs_next
    want = ops.policy_forward(net.flat.data, buf.obs_next_store[:steps].reshape(-1, env.obs_dim), 5, 64,
                              mode="none")["value"].reshape(steps, n_env, N)
    assert torch.equal(buf.vnext_store[:steps], want)
    # ... and v_s == one over obs
    want_s = ops.policy_forward(net.flat.data, buf.obs_store[:steps].reshape(-1, env.obs_dim), 5, 64,
                                mode="none")["value"].reshape(steps, n_env, N)
    assert torch.equal(buf.vs_store[:steps], want_s)
