"""GPU tests (`-m gpu`) of the rollout launch's ride-along (csrc/rollout.hip, rollout_kernel<.., PERM>): the spare workgroups of
the persistent rollout draw the permutations of the update that follows the collect.  Everything is bit-identity: the permutations
against their own launch (`ops.random_permutations`, `PPO._device_perm`), the rollout's stores against a launch without the
request, a whole `PPO.update` with `rollout_prep` on against off and against the eager update."""
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
SEED = 3


def _job(n_env, N, T, **ppo_kw):
    env = DeviceSimpleSpreadVectorEnv(n_env, N, max_cycles=T, device=DEV, seed=SEED)
    net = DiscreteActorCritic(env.obs_dim, env.n_act, 64, device=DEV, seed=SEED)
    algo = PPO(net=net, seed=SEED, shuffle="device", dispatch="per_agent", **ppo_kw)
    buf = DeviceVectorReplayBuffer(n_env * T, n_env, N, env.obs_dim, device=DEV)
    col = Collector(algo, env, buf, use_graph=False)
    col.reset()
    return env, net, algo, buf, col


def _rollout_state(env, buf):
    """Everything a collect writes, as int32 views (bit patterns)."""
    t = dict(obs=buf.obs_store, obs_next=buf.obs_next_store, act=buf.act_store, rew=buf.rew_store, logp=buf.logp_store,
             vs=buf.vs_store, vnext=buf.vnext_store, apos=env.agent_pos, avel=env.agent_vel, lpos=env.landmark_pos,
             steps=env.steps, obs_cur=env.obs_cur)
    out = {k: v.clone().view(torch.int32) for k, v in t.items()}
    out.update(trunc=buf.trunc_store.clone(), term=buf.term_store.clone(), done=buf.done_store.clone(),
               state=buf.index.state.clone(), ep=env.episode_ctr.clone(), tick=env.rng_tick.clone())
    return out


def _collect_with_request(n, n_perm, n_cu=0, counter=12345, repeat=1):
    """Two collects of a 7 x 3 x 5 job (2 rollout workgroups of 5 envs) whose launches carry a hand-made request; -> what they wrote."""
    N = 3
    env, net, algo, buf, col = _job(7, N, 5)
    col.prep_n_cu = n_cu
    out = torch.full((n_perm, n), -1, dtype=torch.int64, device=DEV)
    ctr = torch.tensor([counter], dtype=torch.int64, device=DEV)
    seen = []
    req = dict(out=out, n=n, n_perm=n_perm, seed=SEED ^ 0x5DEECE66D, counter_dev=ctr, scale=N, group_size=repeat, offset_mul=1)
    algo.rollout_prep_request = lambda b: dict(req, gen=len(seen), key=None)
    algo.rollout_prep_done = lambda r, taken: seen.append(taken)
    with policy_within_training_step(algo):
        col.collect(n_step=7 * 3)
        col.collect(n_step=7 * 2)   # (a second launch: the first left the arrival count of the counter advance at zero)
    torch.cuda.synchronize()
    return algo, out, ctr, seen, _rollout_state(env, buf)


@pytest.fixture(scope="module")
def plain_rollout():
    """The same two collects without any request: the rollout's own launch."""
    env, net, algo, buf, col = _job(7, 3, 5)
    algo.rollout_prep = False
    with policy_within_training_step(algo):
        col.collect(n_step=7 * 3)
        col.collect(n_step=7 * 2)
    torch.cuda.synchronize()
    return _rollout_state(env, buf)


# n * n_perm / 512 spare workgroups are useful: 1 for (75, 1), 8 for (1200, 3), the cap of 64 for (25600, 6); repeat 2 with six
# permutations: three agent groups of two
@pytest.mark.parametrize("n,n_perm,repeat", [(75, 1, 1), (75, 3, 1), (1200, 3, 1), (1200, 6, 2), (25600, 1, 1), (25600, 3, 1),
                                             (25600, 6, 2)])
def test_ride_along_permutations_equal_their_own_launch(n, n_perm, repeat, plain_rollout):
    algo, out, ctr, seen, state = _collect_with_request(n, n_perm, repeat=repeat)
    assert seen == [True, True]
    assert int(ctr.item()) == 12345   # read, never written
    ref = ops.random_permutations(n, n_perm, SEED ^ 0x5DEECE66D, counter_dev=ctr, scale=3, group_size=repeat, offset_mul=1)
    assert torch.equal(out, ref)
    # ... which are the draws of the eager update: draw number perm_base + agent * repeat + step, as lane ids of that agent
    for p in range(n_perm):
        a, r = divmod(p, repeat)
        assert torch.equal(out[p], algo._device_perm(n, 12345, a, repeat, r) * 3 + a)
    for k, v in plain_rollout.items():
        assert torch.equal(v, state[k]), k


def test_no_idle_cu_declines_and_changes_nothing(plain_rollout):
    """A device that (by override) has no more CUs than the rollout has workgroups: the launcher declines, the launch is the
    plain one and the request's buffer is not touched."""
    algo, out, ctr, seen, state = _collect_with_request(1200, 3, n_cu=2)
    assert seen == [False, False]
    assert bool((out == -1).all())
    for k, v in plain_rollout.items():
        assert torch.equal(v, state[k]), k


def _train(n_env, T, minibatch, steps=3, partial_last=False, **ppo_kw):
    """`steps` collect + update rounds -> parameters, moments, the last update's losses, counters, the next rollout's first actions."""
    prep = ppo_kw.pop("rollout_prep", True)
    env, net, algo, buf, col = _job(n_env, 3, T, **ppo_kw)
    algo.rollout_prep = prep
    for i in range(steps):
        with policy_within_training_step(algo):
            col.collect(n_step=n_env * (10 if partial_last and i == steps - 1 else T))
            st = algo.update(buf, minibatch, 1)
        col.reset_buffer(keep_statistics=True)
    with policy_within_training_step(algo):
        col.collect(n_step=n_env)
    torch.cuda.synchronize()
    prepared = sum(1 for g in algo._ws.values() if isinstance(g, dict) and g.get("graph_prep") is not None)
    res = dict(flat=net.flat.data.clone().view(torch.int32), m=algo.exp_avg.clone().view(torch.int32),
               v=algo.exp_avg_sq.clone().view(torch.int32), act=buf.act_store[0].clone(), opt_step=algo.opt_step,
               perm_ctr=int(algo._perm_ctr.item()), losses=st.get_loss_stats_dict())
    step_dev = [int(g["step_dev"].item()) for g in algo._ws.values() if isinstance(g, dict) and "perm_request" in g]
    return res, prepared, step_dev


def _same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k], k


# 1024 x 3 x 25: the headline shape, 205 rollout workgroups; 7 x 3 x 25 with minibatches of 32: ragged last tile, six steps per agent
@pytest.mark.parametrize("n_env,minibatch", [(1024, 4096), (7, 32)])
def test_update_behind_a_preparing_rollout_equals_the_plain_update(n_env, minibatch):
    on, prepared, step_dev = _train(n_env, 25, minibatch, use_graph=True)
    assert prepared == 1 and step_dev == [on["opt_step"]]   # the prepared variant replayed; the draw counter is where Adam left it
    off, prepared_off, _ = _train(n_env, 25, minibatch, use_graph=True, rollout_prep=False)
    assert prepared_off == 0
    _same(on, off)
    eager, _, _ = _train(n_env, 25, minibatch, use_graph=False)
    _same(on, eager)


def test_a_collect_that_does_not_fill_the_buffer_falls_back():
    """The last round collects 10 of 25 steps: its update is another captured sequence, which draws its own permutations."""
    on, _, _ = _train(7, 25, 32, partial_last=True, use_graph=True)
    off, _, _ = _train(7, 25, 32, partial_last=True, use_graph=True, rollout_prep=False)
    _same(on, off)
