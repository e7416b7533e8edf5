"""GPU tests (`-m gpu`) of the learned global states end to end, against the reference's own float64 run
(tests/golden/gstate.npz): `GlobalStateConstructor("attention" | "graph")` -- `build`, `build_joint` and `backward` (forward and
every parameter gradient, summed over the slabs) -- and one `CTDEPolicy(state_constructor=...).learn` step (both losses, the
post-step weights of critic, actor and constructor); a checkpoint round trip and a lagged twin; and `learn` without a constructor
against the lines it had before the constructor branch existed.  The bar is the project's: max |hip - ref64| <= 1e-5 max |ref64|
per array -- a reference parameter for gradients, a net's flat vector for post-step weights (Adam's step is relative to each
entry's own gradient; the fixture's note on its eps says what that does to an entry whose gradient is zero)."""
import hashlib
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.multiagent.ctde import CentralizedCritic, CTDEPolicy, DecentralizedActor, GlobalStateConstructor
    from tianshou_marl_amd.data.batch import Batch
    from tianshou_marl_amd.utils.net import FlatAdam, FlatMLP, lagged_copy

G = np.load(os.path.join(HERE, "golden", "gstate.npz"))
CASES = [f"at{i}_" for i in range(len(G["att_cases"]))] + [f"gr{i}_" for i in range(len(G["graph_cases"]))]


def _bar(name, got, ref, tol=1e-5):
    got = got.double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"PARITY {name}: err {err:.3g} of max |ref| {scale:.3g}")
    assert np.isfinite(got).all() and err <= tol * scale, (name, err, scale)


def _constructor(p, sub="w_", seed=0):
    mode = "attention" if p.startswith(("at", "la")) else "graph"
    N, D, H = (int(x) for x in G[p + "dims"][:3])
    adj = torch.as_tensor(G[p + "adjacency"]) if p + "adjacency" in G else None
    gsc = GlobalStateConstructor(mode, obs_dim=D, n_agents=N, hidden_dim=H, adjacency_matrix=adj, device=DEV, seed=seed)
    gsc.load_state_dict({k: G[f"{p}{sub}{k}"] for k, _ in gsc.net.reference_named_views()})
    return gsc


@pytest.mark.parametrize("p", CASES)
def test_build_and_backward_match_the_reference(p):
    gsc = _constructor(p)
    obs = torch.as_tensor(G[p + "obs"]).to(DEV)                      # [B, N, D]
    B, N, _ = obs.shape
    state = gsc.build({f"agent_{n}": obs[:, n].cpu() for n in range(N)})
    _bar(p + "build", state, G[p + "state"])
    assert tuple(state.shape) == (B, gsc.net.hidden_dim)
    joint = gsc.build_joint(obs, save=True)
    assert torch.equal(joint, state) and torch.equal(gsc.build_joint(obs), state)
    d_state = torch.as_tensor(G[p + "d_state"]).to(DEV)
    for n_split in (0, 3):
        slabs = gsc.backward(d_state, n_split=n_split)
        assert slabs.shape == (n_split or ops.mlp_n_split(B), gsc.net.flat.numel())
        grad = slabs.double().sum(0)
        for k, v in gsc.net.reference_named_views(grad):
            _bar(f"{p}grad {k} n_split={n_split}", v, G[f"{p}g_{k}"])
    assert torch.equal(gsc.backward(d_state, n_split=3), slabs)    # a second run: the same bits


def _learn_policy(p):
    N, D, H, B, A, hid = (int(x) for x in G[p + "dims"])
    lr, eps, gamma = (float(x) for x in G[p + "hyper"])
    gsc = _constructor(p, "gsc_w_")
    actor, critic = DecentralizedActor(D, A, hidden_dim=hid, device=DEV, seed=0), CentralizedCritic(H, N, hidden_dim=hid, device=DEV, seed=0)
    for name, net in (("actor", actor), ("critic", critic)):
        net.load_reference_state_dict({k: G[f"{p}{name}_w_{k}"] for k, _ in net.reference_named_views()})
    adam = lambda net: FlatAdam(net, lr=lr, eps=eps)  # noqa: E731
    pol = CTDEPolicy(actor=actor, critic=critic, optim_actor=adam(actor), optim_critic=adam(critic), state_constructor=gsc,
                     optim_state=adam(gsc.net), discount_factor=gamma)
    batch = Batch(obs=G[p + "obs"][:, 0], act=G[p + "act"], rew=G[p + "rew"], obs_next=G[p + "obs_next"][:, 0],
                  terminated=G[p + "terminated"], global_obs=G[p + "obs"].reshape(B, N * D),
                  global_obs_next=G[p + "obs_next"].reshape(B, N * D))
    return pol, batch


@pytest.mark.parametrize("p", ["la_", "lg_"])
def test_learn_step_matches_the_reference(p):
    pol, batch = _learn_policy(p)
    gsc, before = pol.state_constructor, pol.state_constructor.net.flat.data.clone()
    losses = pol.learn(batch)
    for i, k in enumerate(("actor_loss", "critic_loss")):
        _bar(p + k, np.array([losses[k]]), G[p + "losses"][i:i + 1])
    assert not torch.equal(before, gsc.net.flat.data)
    for name, net in (("gsc", gsc.net), ("actor", pol.actor), ("critic", pol.critic)):
        ref = np.concatenate([G[f"{p}{name}_after_{k}"].reshape(-1) for k, _ in net.reference_named_views()])
        _bar(f"{p}{name} post-step vector", net.flat.data, ref)
    assert list(pol.state_dict()) == [f"{n}.fc{i}.{w}" for n in ("actor", "critic") for i in (1, 2, 3) for w in ("weight", "bias")]
    assert pol.optim_state.step_count == pol.optim_critic.step_count == 1
    # a second policy from the same fixture takes the same step, bit for bit
    pol2, _ = _learn_policy(p)
    pol2.learn(batch)
    assert all(torch.equal(a.flat.data, b.flat.data) for a, b in ((pol.actor, pol2.actor), (pol.critic, pol2.critic),
                                                                   (gsc.net, pol2.state_constructor.net)))


@pytest.mark.parametrize("p", ["at0_", "gr1_"])
def test_checkpoint_round_trip_and_lagged_twin(p):
    gsc = _constructor(p)
    obs = torch.as_tensor(G[p + "obs"]).to(DEV)
    want = gsc.build_joint(obs)
    sd = gsc.state_dict()
    assert list(sd) == [str(k) for k in G[p + "keys"]] and all(not v.is_cuda for v in sd.values())
    other = _constructor(p, seed=9)
    other.net.flat.data.normal_()
    other.load_state_dict(sd)
    assert torch.equal(other.net.flat.data, gsc.net.flat.data) and torch.equal(other.build_joint(obs), want)
    twin = lagged_copy(gsc.net)
    assert type(twin) is type(gsc.net) and twin.flat.data_ptr() != gsc.net.flat.data_ptr()
    assert torch.equal(twin.forward(obs, save=False), want)
    gsc.net.flat.data.mul_(0.5)                                      # the twin lags
    assert torch.equal(twin.forward(obs, save=False), want) and not torch.equal(gsc.build_joint(obs), want)
    # the optimizer's checkpoint lists the reference's parameters
    opt = FlatAdam(gsc.net)
    gsc.build_joint(obs, save=True)
    opt.step(gsc.backward(torch.ones_like(want)))
    assert [tuple(s["exp_avg"].shape) for s in opt.state_dict()["state"].values()] == [tuple(v.shape) for v in sd.values()]


def _parent_learn(pol, batch):
    """`CTDEPolicy.learn`'s eager lines as they stood before the constructor branch (no store, no chain)."""
    t = pol._t
    obs, act, rew = t(batch.obs, torch.float32), t(batch.act, torch.int64).reshape(-1), t(batch.rew, torch.float32).reshape(-1)
    terminated = t(batch.terminated, torch.uint8).reshape(-1)
    B = obs.shape[0]
    critic_in, critic_in_next = t(batch.global_obs, torch.float32), t(batch.global_obs_next, torch.float32)
    q = pol.critic(critic_in, save=True).reshape(B, -1)
    q_next = pol.critic(critic_in_next, save=False).reshape(B, -1)
    logits = FlatMLP.forward(pol.actor, obs, save=True)
    dq, dlogits, scalars = ops.ctde_td_head(q, q_next, rew, terminated, pol.discount_factor, logits, act)
    pol.optim_critic.zero_grad()
    pol.optim_critic.step(pol.critic.backward(dq))
    pol.optim_actor.zero_grad()
    pol.optim_actor.step(pol.actor.backward(dlogits))
    s = scalars.cpu().numpy()
    return {"actor_loss": float(s[0]), "critic_loss": float(s[1])}


def test_learn_without_a_constructor_is_what_it_was():
    p = "la_"
    N, D, H, B, A, hid = (int(x) for x in G[p + "dims"])

    def run(step):
        actor, critic = DecentralizedActor(D, A, hid, device=DEV, seed=3), CentralizedCritic(N * D, N, hid, device=DEV, seed=4)
        pol = CTDEPolicy(actor=actor, critic=critic)
        assert pol.state_constructor is None and pol.optim_state is None
        batch = Batch(obs=G[p + "obs"][:, 0], act=G[p + "act"], rew=G[p + "rew"], obs_next=G[p + "obs_next"][:, 0],
                      terminated=G[p + "terminated"], global_obs=G[p + "obs"].reshape(B, N * D),
                      global_obs_next=G[p + "obs_next"].reshape(B, N * D))
        out = [step(pol, batch) for _ in range(3)]
        h = hashlib.sha256()
        for net in (actor, critic):
            h.update(net.flat.data.cpu().numpy().tobytes())
        h.update(np.array([[o["actor_loss"], o["critic_loss"]] for o in out]).tobytes())
        return h.hexdigest()

    assert run(lambda pol, b: pol.learn(b)) == run(_parent_learn)


def test_learn_with_a_constructor_needs_the_joint_observation():
    pol, batch = _learn_policy("la_")
    local = Batch(obs=batch.obs, act=batch.act, rew=batch.rew, obs_next=batch.obs_next, terminated=batch.terminated)
    with pytest.raises(ValueError, match="global_obs"):
        pol.learn(local)
    local.global_obs, local.global_obs_next = batch.global_obs[:, :8], batch.global_obs_next
    with pytest.raises(ValueError, match="concatenated joint observation"):
        pol.learn(local)
