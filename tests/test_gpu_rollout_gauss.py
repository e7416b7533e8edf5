"""GPU tests (`-m gpu`) of the Gaussian persistent rollout (`tsm_rollout_spread_gauss`, csrc/rollout_gauss.hip): one launch per collect(n_step) against the
per-step device loop, bit for bit; its first step against float64 (bar: max |hip - ref64| <= 1e-5 max |ref64| per tensor, the GRU
and LayerNorm tests' bar); and the rule that selects it."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
sys.path.insert(0, os.path.dirname(__file__))

if torch.cuda.is_available():
    import gauss_restatement as gr
    from tianshou_marl_amd.algorithm import GenericPPO, policy_within_training_step
    from tianshou_marl_amd.data import Collector, PrioritizedVectorReplayBuffer, VectorReplayBuffer
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.utils.net import GaussianActorCritic

# (act, conditioned_sigma, unbounded, bound, scaling)
HEADS = [("tanh", False, False, "clip", True), ("relu", True, False, "tanh", False), ("tanh", True, True, None, False)]
CASES = ([(3, 7, h, c) for h in HEADS for c in ("local", "global")] +
         [(8, 3, HEADS[0], "local"), (2, 9, HEADS[0], "local")])   # dead tile row + ragged last workgroup; D = 48; D = 12 < 16
STORES = ["act", "obs", "obs_next", "rew", "term", "trunc", "done", "logp"]
ENV_STATE = ["obs_cur", "agent_pos", "agent_vel", "landmark_pos", "steps", "episode_ctr", "rng_tick"]


def _job(N, E, head, critic, fused, hidden=(64, 64), det=False, buffer=None, act_dim=5):
    act, cond, unbounded, bound, scaling = head
    env = DeviceSimpleSpreadVectorEnv(E, N, max_cycles=2, device=DEV, seed=9, continuous_actions=True)
    D, glob = env.obs_dim, critic == "global"
    net = GaussianActorCritic(D, 5, hidden, act=act, max_action=1.5, unbounded=unbounded, conditioned_sigma=cond,
                              critic_obs_dim=N * D if glob else None, device=DEV, seed=5)
    gen = torch.Generator().manual_seed(3)   # biases and sigma_param off their zero initial values
    net.flat.data.add_(0.1 * torch.randn(net.flat.data.numel(), generator=gen).to(DEV))
    pol = GenericPPO(net=net, critic_input=critic, n_agent=N if glob else 1, dispatch="pooled", seed=11, action_scaling=scaling,
                     action_bound_method=bound, action_space=env.action_space[0], deterministic_eval=det)
    buf = (buffer or VectorReplayBuffer)(E * 16, E, act_dim=act_dim, device=DEV)
    col = Collector(pol, env, buf, fused_rollout=fused)
    col.reset()
    return env, pol, buf, col


def _two_collects(N, E, head, critic, fused, det=False):
    env, pol, buf, col = _job(N, E, head, critic, fused, det=det)
    assert col._can_fuse() == fused
    if det:
        stats = [col.collect(n_step=5 * E) for _ in range(2)]
    else:
        with policy_within_training_step(pol):
            stats = [col.collect(n_step=5 * E) for _ in range(2)]
    out = {k: getattr(buf, k + "_store").clone() for k in STORES + (["vs"] if critic == "local" else [])}
    out.update({k: getattr(env, k).clone() for k in ENV_STATE}, index=buf.index.state.clone())
    out["returns"] = torch.as_tensor(np.concatenate([np.ravel(s.returns) for s in stats]))
    out["lens"] = torch.as_tensor(np.concatenate([np.ravel(s.lens) for s in stats]))
    return out, buf, env


@pytest.mark.parametrize("N,E,head,critic", CASES + [(3, 7, HEADS[0], "det")])
def test_fused_collect_equals_the_per_step_loop_bit_for_bit(N, E, head, critic):
    det, critic = critic == "det", "local" if critic == "det" else critic   # det: deterministic_eval outside a training step
    (got, buf, env), (ref, _, _) = _two_collects(N, E, head, critic, True, det), _two_collects(N, E, head, critic, False, det)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    assert not torch.equal(got["act"][:5], got["act"][5:10]) and got["act"][:10].abs().sum() > 0   # the counter advanced
    assert int(env.rng_tick.item()) == 2 * 5 * E * N * 5 and len(got["lens"]) == 5 * E   # episodes end inside and between launches
    if critic == "global":
        assert buf.logp_outputs_version is not None and buf.behaviour_outputs_version is None
    else:
        assert buf.behaviour_outputs_version is not None


@pytest.mark.parametrize("cond", [False, True])
def test_first_step_against_float64(cond):
    """Worst ratios to the bar on an MI355X: act 0.034, logp 0.013, vs 0.031."""
    N, E, head = 3, 7, ("tanh", cond, False, "clip", True)
    env, pol, buf, col = _job(N, E, head, "local", True)
    with policy_within_training_step(pol):
        col.collect(n_step=E)
    actor, obs = pol.net.actor, buf.obs_store[0].reshape(E * N, -1).cpu().double()
    with torch.no_grad():
        raw, vs = gr.mlp(actor)(obs), gr.mlp(pol.net.critic)(obs).reshape(-1)
    sigma_raw = raw[:, 5:] if cond else actor.sigma_param.cpu().double()
    d = gr.dist(raw[:, :5], sigma_raw, cond, False, actor.max_action)
    act = d.base_dist.loc + d.base_dist.scale * torch.as_tensor(gr.normals(E * N, 5, pol.seed, 0, None))   # the first collect: tick 0
    got_act = buf.act_store[0].reshape(E * N, 5).cpu()
    for name, got, ref in (("act", got_act, act), ("logp", buf.logp_store[0].reshape(-1).cpu(), d.log_prob(got_act.double())),
                           ("vs", buf.vs_store[0].reshape(-1).cpu(), vs)):
        ratio = float((got.double() - ref).abs().max() / (1e-5 * ref.abs().max()))
        print(f"PARITY rollout_gauss {name} cond={cond}: {ratio:.3g} of the bar")
        assert ratio <= 1.0, name
    # the env was stepped with map_action of the stored sample: from rest, an agent out of every other's contact range (0.405)
    # leaves the step with velocity = force * dt = (a[2] - a[1], a[4] - a[3]) * accel * dt
    low, high = pol.action_space.low.astype(np.float64), pol.action_space.high.astype(np.float64)
    ea = gr.map_action(got_act.numpy(), "clip", low, high)
    vel = np.stack([ea[:, 2] - ea[:, 1], ea[:, 4] - ea[:, 3]], 1) * 5.0 * 0.1
    free = (obs[:, 4 + 2 * N:4 + 2 * N + 2 * (N - 1)].reshape(E * N, N - 1, 2).norm(dim=2) > 0.41).all(1).numpy()
    got_vel = buf.obs_next_store[0].reshape(E * N, -1)[:, :2].cpu().numpy()
    assert free.sum() > 0 and np.abs(got_vel - vel)[free].max() <= 1e-5 * np.abs(vel).max()


def test_the_selection_rule():
    assert not _job(3, 7, HEADS[0], "local", True, hidden=(32, 32))[3]._can_fuse()
    assert not _job(3, 7, HEADS[0], "local", True, buffer=lambda n, b, **kw: PrioritizedVectorReplayBuffer(n, b, 0.6, 0.4, **kw))[3]._can_fuse()
    assert not _job(3, 7, HEADS[0], "local", False)[3]._can_fuse()
    with pytest.raises(ValueError, match=r"Box\(5,\) actions but the VectorReplayBuffer stores discrete"):
        _job(3, 7, HEADS[0], "local", True, act_dim=None)[3].collect(n_step=7)
