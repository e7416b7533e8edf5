"""GPU tests (`-m gpu`) of the on-policy learners' snapshots and checkpoints while they train: a `copy.deepcopy` of a PPO / a
GenericPPO that has updated twice, and a fresh instance that loaded its `state_dict()`, continue bit for bit as the original does
-- parameters, both Adam moments, the step count and the four loss statistics of the next update on the same buffer.  The layout
of the checkpoint itself is pinned on the host (tests/test_host_ppo_checkpoint.py)."""
import copy

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tianshou_marl_amd.algorithm import PPO, GenericPPO, policy_within_training_step
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.utils.net import DiscreteActorCritic, MLPActorCritic

DEV = "cuda"
N_ENV, N, T = 4, 3, 8   # 96 samples: three minibatches of 32 for the pooled learner, one per agent for the per-agent one


def _make(kind, use_graph, seed):
    """`fused`: PPO on the 64-wide kernels; `rows`: GenericPPO on 128 x 128, the narrowest net the row kernels accept."""
    if kind == "fused":
        return PPO(net=DiscreteActorCritic(18, 5, 64, device=DEV, seed=seed), shuffle="device", seed=7, lr=1e-3, use_graph=use_graph)
    return GenericPPO(net=MLPActorCritic(18, 5, (128, 128), device=DEV, seed=seed), shuffle="device", seed=7, lr=1e-3,
                      graph=use_graph)


def _update(algo, buf):
    with policy_within_training_step(algo):
        st = algo.update(buf, 32, 2)
    return st.get_loss_stats_dict()


def _state(algo, losses):
    torch.cuda.synchronize()
    return dict(flat=algo.net.flat.data.clone().view(torch.int32), m=algo.exp_avg.clone().view(torch.int32),
                v=algo.exp_avg_sq.clone().view(torch.int32), opt_step=algo.opt_step, losses=losses)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", ["fused", "rows"])
def test_a_snapshot_and_a_loaded_checkpoint_continue_as_the_original(kind, use_graph):
    algo = _make(kind, use_graph, seed=3)
    env = DeviceSimpleSpreadVectorEnv(N_ENV, N, max_cycles=T, device=DEV, seed=3)
    buf = DeviceVectorReplayBuffer(N_ENV * T, N_ENV, N, env.obs_dim, device=DEV)
    col = Collector(algo, env, buf, use_graph=use_graph)
    col.reset()
    for _ in range(2):
        with policy_within_training_step(algo):
            col.collect(n_step=N_ENV * T)
        _update(algo, buf)
        col.reset_buffer(keep_statistics=True)
    assert algo.opt_step > 0 and bool(algo.exp_avg.any())
    torch.manual_seed(5)
    rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    snap = copy.deepcopy(algo)
    # a snapshot draws nothing from the global generators and seeds neither: the device's too is where it was
    assert torch.equal(torch.get_rng_state(), rng) and torch.equal(torch.cuda.get_rng_state(), dev_rng)
    loaded = _make(kind, use_graph, seed=4)
    loaded.load_state_dict(algo.state_dict())
    for other in (snap, loaded):
        assert type(other) is type(algo) and other.net.flat.data_ptr() != algo.net.flat.data_ptr()
        assert torch.equal(other.net.flat.data, algo.net.flat.data) and other.opt_step == algo.opt_step
        assert torch.equal(other.exp_avg, algo.exp_avg) and torch.equal(other.exp_avg_sq, algo.exp_avg_sq)
        if other.net.image is not None:
            assert torch.equal(other.net.image[other.net.image_map.long()], other.net.flat.data)
    # one more update each, on the same rows
    with policy_within_training_step(algo):
        col.collect(n_step=N_ENV * T)
    want = _state(algo, _update(algo, buf))
    assert want["opt_step"] == 3 * snap.opt_step // 2 and not torch.equal(want["flat"], snap.net.flat.data.view(torch.int32))
    for name, other in (("snapshot", snap), ("loaded", loaded)):
        got = _state(other, _update(other, buf))
        for k, v in want.items():
            assert torch.equal(got[k], v) if isinstance(v, torch.Tensor) else got[k] == v, (name, k)
