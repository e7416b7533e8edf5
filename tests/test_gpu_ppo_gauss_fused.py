"""GPU tests (`-m gpu`) of the one-launch Gaussian PPO gradient step (csrc/ppo_gauss.hip): `ops.ppo_update_gauss` against float64
autograd (tests/gauss_restatement.py: `mlp` copies of both nets, `head` for the policy terms, the clipped value loss), its refusals,
and `GenericPPO(fused_actor=True)` over 64-64 Gaussian nets through one whole `update`.

Bar: the one tests/test_gpu_gauss_ppo.py holds the non-fused chain to against the same restatement -- gradients rtol 5e-5 / atol
5e-6 (in units of the gradient's largest magnitude), losses rel 2e-5 / abs 2e-6, parameters after an update rtol 5e-5 / atol 5e-6.
Shapes: M = 4113 is the smallest M whose grid (129 workgroup pairs) walks two tiles each, with a ragged last tile of one row; the
two cases of that size use tanh nets, because no seed keeps a million relu pre-activations 1e-4 away from zero."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gauss_restatement as gr  # noqa: E402
import sampling_restatement as sr  # noqa: E402

from tianshou_marl_amd import ops  # noqa: E402
from tianshou_marl_amd.utils.net import GaussianActorCritic  # noqa: E402

DEV = "cuda"
EPS, DUAL, VF, ENT, MAX_ACTION = 0.2, 3.0, 0.5, 0.01, 2.0
CASES = [  # (M, D, Ad, conditioned sigma, activation, seed: one whose float64 reference passes `_reference`'s own assertions)
    (1, 18, 5, False, "relu", 0), (15, 1, 1, True, "tanh", 1), (16, 63, 8, True, "relu", 24), (17, 64, 8, False, "tanh", 3),
    (33, 18, 16, False, "relu", 66), (33, 63, 5, True, "tanh", 5), (17, 1, 1, False, "relu", 83), (4113, 18, 5, False, "tanh", 7),
    (4113, 64, 8, True, "tanh", 8)]


def _inputs(net, actor, critic, M, unbounded, rng, dev):
    """A batch of n > M rows, NaN outside the M rows of a non-identity `perm`; the M rows are drawn around the float64 nets' own
    outputs so that every kink is far by construction: ratios in [0.5, 0.79] | [0.81, 1.19] | [1.21, 2] | [3.2, 4] (dual clip at
    3), |adv| >= 0.1, |v - v_old| in [0.05, 0.15] | [0.25, 0.4] around eps, |ret - v| >= 0.5."""
    D, Ad, cond = net.obs_dim, net.act_dim, net.actor.conditioned_sigma
    n = 2 * M + 3
    perm = rng.permutation(n)[:M]
    x = rng.standard_normal((M, D)).astype(np.float32)
    with torch.no_grad():
        raw, v = actor(torch.as_tensor(x).double()), critic(torch.as_tensor(x).double()).squeeze(-1).numpy()
        sg = raw[:, Ad:] if cond else net.actor.sigma_param.cpu().double()
        d = gr.dist(raw[:, :Ad], sg, cond, unbounded, MAX_ACTION)
        act = (d.base_dist.loc + d.base_dist.scale * torch.as_tensor(rng.standard_normal((M, Ad)))).float()
        logp = d.log_prob(act.double()).numpy()
    lo, hi = np.array([0.5, 0.81, 1.21, 3.2]), np.array([0.79, 1.19, 2.0, 4.0])
    band = rng.integers(0, 4, M)
    sign = lambda: rng.choice([-1.0, 1.0], M)  # noqa: E731
    rows = dict(obs=x, act=act.numpy(), logp_old=logp - np.log(rng.uniform(lo[band], hi[band])),
                adv=sign() * (0.1 + np.abs(rng.standard_normal(M))), ret=v + sign() * (0.5 + 0.5 * np.abs(rng.standard_normal(M))),
                v_old=v + sign() * np.where(rng.random(M) < 0.5, rng.uniform(0.05, 0.15, M), rng.uniform(0.25, 0.4, M)))
    rows = {k: np.asarray(a, np.float32) for k, a in rows.items()}
    full = {}
    for k, a in rows.items():
        full[k] = torch.full((n, *a.shape[1:]), float("nan"))
        full[k][perm] = torch.as_tensor(a)
    return rows, {k: a.to(dev) for k, a in full.items()}, torch.as_tensor(perm).to(dev)


def _reference(net, actor, critic, rows, unbounded, dual, norm, vclip):
    """float64: (flat gradient in the vector's order, [loss, clip, vf, ent]); asserts the case is off every kink."""
    Ad, cond = net.act_dim, net.actor.conditioned_sigma
    for p in [*actor.parameters(), *critic.parameters()]:
        p.grad = None
    x = torch.as_tensor(rows["obs"]).double()
    outs = []
    for seq in (actor, critic):
        h = x
        for m in seq:
            h = m(h)
            if isinstance(m, torch.nn.Linear) and m is not seq[-1] and net.actor.act == "relu":
                assert h.abs().min() >= 1e-4   # no relu unit within 1e-4 of its kink
        outs.append(h)
    raw, v = outs[0], outs[1].squeeze(-1)
    sg = raw[:, Ad:].detach().numpy() if cond else net.actor.sigma_param.cpu().double().numpy()
    hd = gr.head(raw[:, :Ad].detach().numpy(), sg, rows["act"], rows["logp_old"], rows["adv"], cond, unbounded, MAX_ACTION, norm,
                 ENT, eps_clip=EPS, dual_clip=dual)
    if np.isfinite(hd["adv"]).all():   # tests/test_gpu_gauss.py's _assert_off_the_kinks
        r, A = hd["ratio"], hd["adv"]
        assert np.abs(r - (1 - EPS)).min() >= 1e-3 and np.abs(r - (1 + EPS)).min() >= 1e-3
        if dual and (A < 0).any():
            assert np.abs(dual * A - np.minimum(r * A, np.clip(r, 1 - EPS, 1 + EPS) * A))[A < 0].min() >= 1e-3
        assert not cond or (np.abs(sg + 20).min() >= 1e-3 and np.abs(sg - 2).min() >= 1e-3)
    raw.backward(torch.as_tensor(np.concatenate([hd["d_mu"], hd["d_sigma"]], 1) if cond else hd["d_mu"]))
    ret, v_old = torch.as_tensor(rows["ret"]).double(), torch.as_tensor(rows["v_old"]).double()
    vf = (ret - v) ** 2
    if vclip:
        assert ((v.detach() - v_old).abs() - EPS).abs().min() >= 1e-3
        vf = torch.max(vf, (ret - (v_old + (v - v_old).clamp(-EPS, EPS))) ** 2)
    vf = vf.mean()
    (VF * vf).backward()
    grads = [p.grad.reshape(-1) for p in actor.parameters()] + ([] if cond else [torch.as_tensor(hd["d_sigma"]).reshape(-1)]) + \
        [p.grad.reshape(-1) for p in critic.parameters()]
    vf = float(vf.detach())
    return torch.cat(grads).numpy(), np.array([hd["clip_loss"] + VF * vf - ENT * hd["ent_loss"], hd["clip_loss"], vf, hd["ent_loss"]])


def _net(D, Ad, cond, act, seed, dev):
    net = GaussianActorCritic(D, Ad, (64, 64), act=act, max_action=MAX_ACTION, conditioned_sigma=cond, device=dev, seed=seed)
    g = torch.Generator().manual_seed(seed)
    for f in (net.actor, net.critic):   # (the init's biases are zero: a bias read at a wrong offset would not show)
        for i in range(3):
            f.bias(i).copy_(torch.empty(f.dims[i + 1]).uniform_(-0.2, 0.2, generator=g))
    if cond:   # sigma_raw near 0, but column 0 at 3: past the clamp at 2, where d loss / d sigma_raw is zero
        net.actor.weight(2)[Ad:].mul_(0.3)
        net.actor.bias(2)[Ad] = 3.0
    else:
        net.actor.sigma_param.copy_(torch.linspace(-1.0, 0.2, Ad))
    return net


@pytest.mark.parametrize("M,D,Ad,cond,act,seed", CASES)
def test_kernel_matches_float64_autograd(M, D, Ad, cond, act, seed, dev=DEV):
    net = _net(D, Ad, cond, act, seed, dev)
    actor, critic = gr.mlp(net.actor), gr.mlp(net.critic)
    P, rng = net.flat.numel(), np.random.default_rng(seed)
    nb = ops.ppo_update_gauss_grid(M)
    assert M < 4113 or (nb >= 2 and -(-M // 16) >= 2 * nb)
    batches = [_inputs(net, actor, critic, M, unb, rng, dev) for unb in (False, True)]   # (actions and logp_old follow mu)
    for flags in range(16):
        unbounded, dual, norm, vclip = bool(flags & 1), DUAL if flags & 2 else None, bool(flags & 4), bool(flags & 8)
        rows, full, perm = batches[unbounded]
        grad, losses = _reference(net, actor, critic, rows, unbounded, dual, norm, vclip)
        if dev != DEV:   # (the reference's own conditions, checked without a device when the seeds were chosen)
            continue
        cfg = ops.make_ppo_cfg(EPS, dual, vclip, norm, VF, ENT)
        stats = ops.ppo_adv_stats(full["adv"], torch.tensor([0, M], device=dev), perm=perm)[0] if norm else None

        def run():
            slabs = torch.full((nb, P + 3), float("nan"), device=dev)
            step = torch.zeros(1, dtype=torch.int64, device=dev)
            _, partial = ops.ppo_update_gauss(
                net.flat.data, full["obs"], full["act"], full["logp_old"], full["adv"], full["ret"], cfg, act_fn=act,
                conditioned_sigma=cond, max_action=MAX_ACTION, unbounded=unbounded, adv_stats=stats, v_s_old=full["v_old"],
                perm=perm, slabs=slabs, slab_stride=P + 3, opt_step_dev=step)
            assert step.item() == 1
            return slabs, partial

        (slabs, partial), (slabs2, partial2) = run(), run()
        bits = lambda s: s[:, :P].contiguous().view(torch.int32)  # noqa: E731  (bits: the NaN case compares too)
        assert torch.equal(bits(slabs), bits(slabs2)) and torch.equal(partial.view(torch.int64), partial2.view(torch.int64))
        assert torch.isnan(slabs[:, P:]).all()   # the pad past the parameters belongs to no workgroup
        scal = torch.empty(1, 4, device=dev)
        ops.ppo_finalize_many(partial, 2 * nb * 4, torch.tensor([2 * nb], dtype=torch.int32, device=dev),
                              torch.tensor([M], device=dev), cfg, scal)
        got, got_l = slabs[:, :P].double().sum(0).cpu().numpy(), scal[0].cpu().numpy()
        name = f"unbounded={unbounded} dual={dual} norm={norm} vclip={vclip}"
        if M == 1 and norm:   # torch.std of one row is NaN (ppo.py:185): the reference has no finite gradient to hold to
            b3 = slice(net.actor.n_mlp_params - net.actor.dims[-1], net.actor.n_mlp_params)   # the row's d loss / d raw itself
            assert not np.isfinite(grad[b3]).any() and not np.isfinite(got[b3]).any()
            continue
        scale = np.abs(grad).max()
        print(f"{name}: grad err / max {np.abs(got - grad).max() / scale:.2e}, loss err {np.abs(got_l - losses).max():.2e}")
        np.testing.assert_allclose(got / scale, grad / scale, rtol=5e-5, atol=5e-6, err_msg=name)
        np.testing.assert_allclose(got_l, losses, rtol=2e-5, atol=2e-6, err_msg=name)


@pytest.mark.parametrize("D,hidden,Ad,cond,act,match", [
    (18, (32, 32), 5, False, "relu", "64"), (18, (128, 128), 5, False, "relu", "64"), (18, (64, 32), 5, False, "relu", "64"),
    (65, (64, 64), 5, False, "relu", r"\[1, 64\]"), (18, (64, 64), 9, True, "tanh", r"\[1, 16\]"),
    (18, (64, 64), 5, False, "sigmoid", "relu")])
def test_refusals_name_the_limit(D, hidden, Ad, cond, act, match):
    with pytest.raises(ValueError, match=match):
        ops.ppo_update_gauss_check(D, hidden, Ad, cond, act)


E, N, T, BATCH, REPEAT, SEED = 4, 2, 8, 24, 2, 11


def _algo(D, Ad, cond, graph, **kw):
    from tianshou_marl_amd.algorithm import GenericPPO
    from tianshou_marl_amd.data import Batch, VectorReplayBuffer

    net = GaussianActorCritic(D, Ad, (64, 64), act="tanh", max_action=MAX_ACTION, conditioned_sigma=cond,
                              critic_obs_dim=N * D if kw.get("critic_input") == "global" else None, device=DEV, seed=5)
    if not cond:
        net.actor.sigma_param.copy_(torch.linspace(-1.0, 0.2, Ad))
    algo = GenericPPO(net=net, dispatch="pooled", shuffle="device", seed=SEED, lr=1e-3, max_grad_norm=0.5, value_clip=True,
                      graph=graph, **kw)
    rng = np.random.default_rng(7)
    buf = VectorReplayBuffer(E * T, E, act_dim=Ad, device=DEV)
    for t in range(T):
        buf.add(Batch(obs=rng.standard_normal((E, N, D)).astype(np.float32), act=rng.standard_normal((E, N, Ad)).astype(np.float32),
                      rew=rng.standard_normal((E, N)).astype(np.float32), terminated=rng.random((E, N)) < 0.1,
                      truncated=np.full((E, N), t == T - 1), obs_next=rng.standard_normal((E, N, D)).astype(np.float32)))
    return net, algo, buf


@pytest.mark.parametrize("cond", [True, False], ids=["conditioned", "sigma_param"])
def test_update_matches_float64_autograd_and_its_capture(oracle, cond):
    from tianshou_marl_amd.algorithm import policy_within_training_step
    from tianshou_marl_amd.data.batch import split_bounds

    net, algo, buf = _algo(18, 5, cond, False)
    assert algo.gaussian and algo.fused_gauss and not (algo.fused_actor or algo.fused_critic)
    c = lambda x: x[:T].cpu().numpy()  # noqa: E731
    L = E * N
    gae = lambda v_s, v_n: oracle.gae_lanes(v_s, v_n, c(buf.rew_store).reshape(T, L), c(buf.term_store).reshape(T, L).astype(bool),  # noqa: E731
                                            c(buf.trunc_store).reshape(T, L).astype(bool), 0.99, 0.95)
    bounds = split_bounds(T * L, BATCH, True)
    perms = [sr.random_permutations(T * L, 1, SEED ^ 0x5DEECE66D, counter=r)[0][0] for r in range(REPEAT)]
    actor, sigma, critic, losses = gr.update(net, dict(obs=c(buf.obs_store), obs_next=c(buf.obs_next_store), act=c(buf.act_store)),
                                             gae, bounds, perms, N, False, 1e-3, 0.5)
    with policy_within_training_step(algo):
        st = algo.update(buf, BATCH, REPEAT)
    for got, ref in zip((st.loss.mean, st.actor_loss.mean, st.vf_loss.mean, st.ent_loss.mean), losses.mean(0)):
        assert got == pytest.approx(ref, rel=2e-5, abs=2e-6)
    ref_flat = torch.cat([p.detach().reshape(-1) for p in [*actor.parameters(), *([] if cond else [sigma]), *critic.parameters()]])
    np.testing.assert_allclose(net.flat.data.cpu().numpy(), ref_flat.numpy(), rtol=5e-5, atol=5e-6)

    def second(graph):   # the first update of a shape runs eagerly; graph=True captures and replays the second
        net, algo, buf = _algo(18, 5, cond, graph)
        with policy_within_training_step(algo):
            algo.update(buf, BATCH, REPEAT)
            st = algo.update(buf, BATCH, REPEAT)
        return net.flat.data.clone(), st.get_loss_stats_dict(), algo.opt_step

    (p_e, l_e, s_e), (p_g, l_g, s_g) = second(False), second(True)
    assert s_e == s_g == 2 * REPEAT * len(bounds) and torch.equal(p_e, p_g) and l_e == l_g


@pytest.mark.parametrize("kw", [dict(fused_actor=False), dict(critic_input="global", n_agent=N)], ids=["fused_actor=False", "global"])
def test_the_chain_still_serves_what_the_fused_step_does_not(kw):
    from tianshou_marl_amd.algorithm import policy_within_training_step

    net, algo, buf = _algo(6, 3, False, False, **kw)
    before = net.flat.data.clone()
    assert algo.gaussian and not algo.fused_gauss
    with policy_within_training_step(algo):
        st = algo.update(buf, BATCH, REPEAT)
    assert np.isfinite(st.loss.mean) and not torch.equal(before, net.flat.data)
