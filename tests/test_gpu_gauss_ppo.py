"""GPU tests (`-m gpu`) of GenericPPO on a GaussianActorCritic: one whole update against tests/gauss_restatement.py's float64
autograd run with the same device-drawn minibatch permutations, clip_grad_norm_ and torch.optim.Adam.  Bar: the one
tests/test_gpu_generic_ppo.py::test_row_minibatches_with_centralized_critic_match_float64_autograd holds the categorical path's
whole update to -- parameters rtol 5e-5 / atol 5e-6, mean loss rel 2e-5 / abs 2e-6 (here on each of the four reported losses)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gauss_restatement as gr  # noqa: E402
import sampling_restatement as sr  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd.algorithm import NPG, GenericPPO, policy_within_training_step
    from tianshou_marl_amd.data import Batch, VectorReplayBuffer
    from tianshou_marl_amd.data.batch import split_bounds
    from tianshou_marl_amd.utils.net import GaussianActorCritic

DEV = "cuda"
E, N, T, D, AD = 4, 2, 8, 6, 3
SEED, LR, GN, BATCH, REPEAT = 11, 1e-3, 0.5, 24, 2


def _setup(glob: bool, cond: bool, graph: bool):
    net = GaussianActorCritic(D, AD, (32, 32), act="tanh", max_action=2.0, conditioned_sigma=cond,
                              critic_obs_dim=N * D if glob else None, device=DEV, seed=5)
    if not cond:
        net.actor.sigma_param.copy_(torch.tensor([-0.5, 0.1, -1.0]))
    algo = GenericPPO(net=net, critic_input="global" if glob else "local", n_agent=N if glob else 1, dispatch="pooled",
                      shuffle="device", seed=SEED, lr=LR, max_grad_norm=GN, value_clip=True, graph=graph)
    assert algo.gaussian and not (algo.fused_actor or algo.fused_critic)
    rng = np.random.default_rng(7)
    buf = VectorReplayBuffer(E * T, E, act_dim=AD, device=DEV)
    for t in range(T):
        buf.add(Batch(obs=rng.standard_normal((E, N, D)).astype(np.float32), act=rng.standard_normal((E, N, AD)).astype(np.float32),
                      rew=rng.standard_normal((E, N)).astype(np.float32), terminated=rng.random((E, N)) < 0.1,
                      truncated=np.full((E, N), t == T - 1), obs_next=rng.standard_normal((E, N, D)).astype(np.float32)))
    return net, algo, buf


@pytest.mark.parametrize("cond", [True, False], ids=["conditioned", "sigma_param"])
@pytest.mark.parametrize("glob", [False, True], ids=["local", "global"])
def test_one_update_matches_float64_autograd(oracle, glob, cond):
    net, algo, buf = _setup(glob, cond, graph=False)
    c = lambda x: x[:T].cpu().numpy()  # noqa: E731
    store = dict(obs=c(buf.obs_store), obs_next=c(buf.obs_next_store), act=c(buf.act_store))
    L = E * N
    gae = lambda v_s, v_n: oracle.gae_lanes(v_s, v_n, c(buf.rew_store).reshape(T, L), c(buf.term_store).reshape(T, L).astype(bool),  # noqa: E731
                                            c(buf.trunc_store).reshape(T, L).astype(bool), 0.99, 0.95)
    n_units = T * E if glob else T * L   # joint rows with the centralized critic (row minibatches), else lanes
    bounds = split_bounds(n_units, BATCH // N if glob else BATCH, True)
    perms = [sr.random_permutations(n_units, 1, SEED ^ 0x5DEECE66D, counter=r)[0][0] for r in range(REPEAT)]
    actor, sigma, critic, losses = gr.update(net, store, gae, bounds, perms, N, glob, LR, GN)
    with policy_within_training_step(algo):
        st = algo.update(buf, BATCH, REPEAT)
    assert st.gradient_steps == len(losses) == REPEAT * len(bounds)
    for got, ref in zip((st.loss.mean, st.actor_loss.mean, st.vf_loss.mean, st.ent_loss.mean), losses.mean(0)):
        assert got == pytest.approx(ref, rel=2e-5, abs=2e-6)
    for f, ref in ((net.actor, actor), (net.critic, critic)):
        for i, lin in enumerate([m for m in ref if isinstance(m, torch.nn.Linear)]):
            np.testing.assert_allclose(f.weight(i).cpu().numpy(), lin.weight.detach().numpy(), rtol=5e-5, atol=5e-6)
            np.testing.assert_allclose(f.bias(i).cpu().numpy(), lin.bias.detach().numpy(), rtol=5e-5, atol=5e-6)
    if not cond:
        np.testing.assert_allclose(net.actor.sigma_param.cpu().numpy(), sigma.detach().numpy(), rtol=5e-5, atol=5e-6)


@pytest.mark.parametrize("cond", [True, False], ids=["conditioned", "sigma_param"])
def test_captured_update_equals_eager_launches(cond):
    def run(graph):
        net, algo, buf = _setup(True, cond, graph)
        with policy_within_training_step(algo):
            algo.update(buf, BATCH, REPEAT)        # the first update of a shape runs eagerly
            st = algo.update(buf, BATCH, REPEAT)   # graph=True: captured and replayed
        return net.flat.data.clone(), st.get_loss_stats_dict(), algo.opt_step

    (p_e, l_e, s_e), (p_g, l_g, s_g) = run(False), run(True)
    assert s_e == s_g and torch.equal(p_e, p_g) and l_e == l_g


def test_acting_returns_the_raw_sample_and_the_env_action():
    net, algo, _ = _setup(False, False, False)
    algo2 = GenericPPO(net=net, dispatch="pooled", action_scaling=True, action_bound_method="tanh", low=[-1.0, 0.0, 2.0], high=3.0,
                       deterministic_eval=True)
    obs = torch.randn(E, N, D, device=DEV)
    res = algo2.act_device(obs)   # outside a training step: the mode
    assert res["act"].shape == (E * N, AD) and res["act"].dtype == torch.float32
    raw = net.actor(obs.reshape(-1, D), save=False)
    assert torch.allclose(res["act"], 2.0 * torch.tanh(raw), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(res["env_act"].cpu().numpy(), algo2.map_action(res["act"]), rtol=1e-5, atol=1e-6)
    with policy_within_training_step(algo2):
        a1, a2 = algo2.act_device(obs)["act"], algo2.act_device(obs)["act"]
    assert not torch.equal(a1, a2) and not torch.equal(a1, res["act"])   # sampled, and the counter advances


def test_what_is_not_built_says_so():
    net = GaussianActorCritic(D, AD, (32, 32), device=DEV, seed=1)
    with pytest.raises(NotImplementedError, match="GaussianActorCritic"):
        NPG(net=net)
