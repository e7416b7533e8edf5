"""CPU tests of the Rainbow port: the import surface, the refusals of `ops.rainbow_check`, the entry points and the constructors
(all of which fail before touching a device), the flat layout and init of `RainbowNet`, the recorded reference signatures, the
reference-layout checkpoint keys, and the float64 restatement (tests/rainbow_restatement.py) against the reference's own runs
(tests/golden/rainbow.npz) to 1e-10 relative."""
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "rainbow.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")

from dqn_restatement import nstep_walk  # noqa: E402
from rainbow_restatement import (RainbowNetRestatement, RainbowRestatement, compose, dueling_combine,  # noqa: E402
                                 dueling_combine_backward, noise_of, noisy_grad, philox_normals, split_flat)
from test_host_dqn import _Discrete, _Env, check_digest, up_inputs  # noqa: E402

REL = 1e-10


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def net_case(g, tag):
    """(restatement, RainbowNet keyword arguments) of the `nl` / `du` section."""
    d = [int(x) for x in g[f"{tag}_dims"]]
    obs_dim, A, N, B, dueling, nh, nq, nv = d[:8]
    hidden, qh, vh = tuple(d[8:8 + nh]), tuple(d[8 + nh:8 + nh + nq]), tuple(d[8 + nh + nq:])
    R = RainbowNetRestatement(obs_dim, hidden, A, N, qh, vh, bool(dueling), True)
    return R, dict(obs_dim=obs_dim, hidden_sizes=hidden, n_act=A, num_atoms=N, q_hidden=qh, v_hidden=vh, dueling=bool(dueling))


def up_case(g):
    obs_dim, A, N, h, qh, vh = (int(x) for x in g["up_dims"])
    R = RainbowNetRestatement(obs_dim, (h,), A, N, (qh,), (vh,), True, True)
    return R, dict(obs_dim=obs_dim, hidden_sizes=(h,), n_act=A, num_atoms=N, q_hidden=(qh,), v_hidden=(vh,))


def _rainbow(device="cpu", net_kw=None, policy_kw=None, optim=None, **kw):
    from tianshou_marl_amd.algorithm import RainbowDQN, RainbowPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import RainbowNet

    nk = dict(obs_dim=6, hidden_sizes=(32,), n_act=5, num_atoms=51, q_hidden=(32,), v_hidden=(32,), seed=0)
    nk.update(net_kw or {})
    net = RainbowNet(device=device, **nk)
    pol = RainbowPolicy(model=net, action_space=_Discrete(nk["n_act"]), num_atoms=nk["num_atoms"], **(policy_kw or {}))
    return RainbowDQN(policy=pol, optim=optim or AdamOptimizerFactory(), **kw)


def test_importable_beside_the_siblings():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import C51, C51Policy, RainbowDQN, RainbowPolicy
    from tianshou_marl_amd.algorithm.rainbow import RainbowDQN as R2
    from tianshou_marl_amd.utils.net import RainbowNet

    assert RainbowDQN is R2 and issubclass(RainbowDQN, C51) and issubclass(RainbowPolicy, C51Policy)
    assert RainbowPolicy._model_cls is RainbowNet
    for name in ("rainbow_check", "noisy_net_table", "noisy_sample", "noisy_compose", "noisy_grad", "dueling_combine",
                 "dueling_combine_backward", "dueling_features", "dueling_features_backward"):
        assert callable(getattr(ops, name)), name


def test_rainbow_check_names_the_limit_without_a_device():
    from tianshou_marl_amd import _abi, ops

    t = ops.noisy_net_table([(6, 32, 1), (32, 255, 1), (32, 51, 0)])
    ops.rainbow_check(t)
    assert (t.P, t.P_eff, t.n_slots) == (2 * 6 * 32 + 3 * 32 + 6 + 2 * 32 * 255 + 3 * 255 + 32 + 32 * 51 + 51,
                                          6 * 32 + 32 + 32 * 255 + 255 + 32 * 51 + 51, 6 + 32 + 32 + 255)
    assert (t.layer[2].off, t.layer[2].eff_off, t.layer[2].slot_off) == (t.P - 32 * 51 - 51, t.P_eff - 32 * 51 - 51, t.n_slots)
    ops.rainbow_check(ops.noisy_net_table([(1, 1, 1)]))
    with pytest.raises(ValueError, match=r"25 layers outside \[1, 24\]"):
        ops.noisy_net_table([(2, 2, 1)] * 25)
    bad = ops.noisy_net_table([(6, 32, 1), (32, 5, 1)])
    bad.n_layers = 25
    with pytest.raises(ValueError, match=r"n_layers = 25 outside \[1, 24\]"):
        ops.rainbow_check(bad)
    for field, value, msg in (("off", 7, "layer 1 starts at"), ("eff_off", 0, "layer 1 starts at"), ("slot_off", 1, "layer 1 starts at"),
                              ("n_in", 0, "widths must lie in"), ("n_out", 65537, "widths must lie in"), ("noisy", 2, "neither 0 nor 1")):
        bad = ops.noisy_net_table([(6, 32, 1), (32, 5, 1)])
        setattr(bad.layer[1], field, value)
        with pytest.raises(ValueError, match=msg):
            ops.rainbow_check(bad)
    for field in ("P", "P_eff", "n_slots"):
        bad = ops.noisy_net_table([(6, 32, 1), (32, 5, 1)])
        setattr(bad, field, getattr(bad, field) + 1)
        with pytest.raises(ValueError, match="its layers add up to"):
            ops.rainbow_check(bad)
    with pytest.raises(ValueError, match="null layer table"):
        _abi.call("tsm_rainbow_check", None)


def test_entry_points_reject_bad_arguments_without_a_device():
    import ctypes as C

    from tianshou_marl_amd import _abi, ops

    t = ops.noisy_net_table([(6, 32, 1), (32, 5, 0)])
    ref = C.byref(t)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_noisy_sample", ref, None, 1, 0, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_noisy_compose", ref, None, 1, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_noisy_grad", ref, None, None, 1, 1, None, None)
    with pytest.raises(ValueError, match=r"n_split = 0 outside"):
        _abi.call("tsm_noisy_grad", ref, 8, 8, 0, 1, 8, None)
    plain = ops.noisy_net_table([(6, 32, 0)])
    _abi.call("tsm_noisy_sample", C.byref(plain), None, 1, 0, None, None)      # no slot: nothing to do, no pointer is read
    bad = ops.noisy_net_table([(6, 32, 1)])
    bad.P += 1
    for entry, args in (("tsm_noisy_sample", (8, 1, 0, None, None)), ("tsm_noisy_compose", (8, 1, 8, None)),
                        ("tsm_noisy_grad", (8, 8, 1, 1, 8, None))):
        with pytest.raises(ValueError, match="its layers add up to"):
            _abi.call(entry, C.byref(bad), *args)
    for entry, args in (("tsm_dueling_combine", lambda R, A, N: (None, None, R, A, N, None, None)),
                        ("tsm_dueling_combine_backward", lambda R, A, N: (None, R, A, N, None, None, None))):
        with pytest.raises(ValueError, match=r"n_atoms = 257 outside \[2, 256\]"):
            _abi.call(entry, *args(4, 5, 257))
        with pytest.raises(ValueError, match=r"n_act = 65 outside \[1, 64\]"):
            _abi.call(entry, *args(4, 65, 51))
        with pytest.raises(ValueError, match="out of range"):
            _abi.call(entry, *args(-1, 5, 51))
        with pytest.raises(ValueError, match="null pointer"):
            _abi.call(entry, *args(4, 5, 51))
        _abi.call(entry, *args(0, 5, 51))
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_dueling_features", None, 4, None, None)
    with pytest.raises(ValueError, match="out of range"):
        _abi.call("tsm_dueling_features", None, -1, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_dueling_features_backward", None, None, None, 4, None, None)
    _abi.call("tsm_dueling_features_backward", None, None, None, 0, None, None)


def test_ops_refuse_cpu_tensors_and_check_shapes_first():
    from tianshou_marl_amd import ops

    t = ops.noisy_net_table([(6, 32, 1), (32, 10, 1)])
    flat, q, v = torch.zeros(t.P), torch.zeros(4, 10), torch.zeros(4, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.noisy_sample(t, flat, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.noisy_compose(t, flat, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.noisy_grad(t, flat, torch.zeros(2, t.P_eff), True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dueling_combine(q, v, 5, 2)
    with pytest.raises(ValueError, match=r"v must be \[4, 2\]"):
        ops.dueling_combine(q, torch.zeros(4, 3), 5, 2)
    with pytest.raises(ValueError, match=r"\[R, 5 \* 3\]"):
        ops.dueling_combine_backward(q, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dueling_combine_backward(q, 5, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dueling_features(q)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dueling_features_backward(q, q, q)


def test_net_is_one_flat_vector_with_the_reference_init(g):
    from tianshou_marl_amd.utils.net import RainbowNet

    R, kw = up_case(g)
    net = RainbowNet(device="cpu", seed=3, **kw)
    assert net.flat.numel() == R.P == g["up_init"].size and net.n_slots == R.n_slots and net.dims == [6, 255]
    assert [(int(i), int(o), bool(z)) for i, o, z in net._layers] == R.layers
    for (i, o, z), v in zip(R.layers, net.layer_views()):
        b = 1.0 / np.sqrt(i)
        assert list(v) == ["mu_W", "sigma_W", "mu_bias", "sigma_bias", "eps_p", "eps_q"]
        assert float(v["mu_W"].abs().max()) <= b and float(v["mu_bias"].abs().max()) <= b and float(v["mu_W"].abs().max()) > b / 2
        assert torch.equal(v["sigma_W"], torch.full((o, i), np.float32(0.5 / np.sqrt(i)))) and torch.equal(
            v["sigma_bias"], torch.full((o,), np.float32(0.5 / np.sqrt(i))))
        assert v["eps_p"].shape == (i,) and v["eps_q"].shape == (o,) and bool(v["eps_p"].any())
    same, other = RainbowNet(device="cpu", seed=3, **kw), RainbowNet(device="cpu", seed=4, **kw)
    assert torch.equal(same.flat.data, net.flat.data) and not torch.equal(other.flat.data, net.flat.data)
    eps = np.arange(net.n_slots, dtype=np.float32)
    net.set_noise(eps)
    assert np.array_equal(net.noise().numpy(), eps) and np.array_equal(noise_of(net.flat.data.double().numpy(), R.layers), eps)
    with pytest.raises(ValueError, match="noise slots"):
        net.set_noise(eps[:-1])
    twin = net.clone_over(torch.zeros(R.P))
    assert twin.flat.numel() == R.P and twin.table.P_eff == net.table.P_eff
    plain = RainbowNet(6, (32,), 5, 51, dueling=False, noisy_std=None, device="cpu", seed=1)
    assert plain.n_slots == 0 and plain.flat.numel() == 6 * 32 + 32 + 32 * 255 + 255 and list(plain.layer_views()[0]) == ["weight", "bias"]
    with pytest.raises(RuntimeError, match="before forward"):
        net.backward(torch.zeros(1, 255))


def test_constructors_validate():
    from tianshou_marl_amd.algorithm import C51Policy, RainbowDQN, RainbowPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import FlatMLP, RainbowNet

    with pytest.raises(ValueError, match="n_atoms = 257"):
        RainbowNet(6, (32,), 5, 257, device="cpu")
    with pytest.raises(ValueError, match="n_act = 65"):
        RainbowNet(6, (32,), 65, 51, device="cpu")
    with pytest.raises(ValueError, match="need a trunk"):
        RainbowNet(6, (), 5, 51, device="cpu")
    with pytest.raises(ValueError, match="dueling=False"):
        RainbowNet(6, (32,), 5, 51, q_hidden=(8,), dueling=False, device="cpu")
    with pytest.raises(ValueError, match="storage must be"):
        RainbowNet(6, (32,), 5, 51, device="cpu", storage=torch.zeros(7))
    mlp = FlatMLP([6, 32, 255], device="cpu", seed=0)
    with pytest.raises(TypeError, match="RainbowNet"):
        RainbowPolicy(model=mlp, action_space=_Discrete(5))
    net = RainbowNet(6, (32,), 5, 51, device="cpu", seed=0)
    with pytest.raises(ValueError, match="emits 51 atoms"):
        RainbowPolicy(model=net, action_space=_Discrete(5), num_atoms=21)
    with pytest.raises(ValueError, match="255 outputs"):
        RainbowPolicy(model=net, action_space=_Discrete(4))
    with pytest.raises(TypeError, match="needs a RainbowPolicy"):
        RainbowDQN(policy=C51Policy(model=mlp, action_space=_Discrete(5)), optim=AdamOptimizerFactory())
    pol = RainbowPolicy(model=net, action_space=_Discrete(5))
    with pytest.raises(ValueError, match="weight_decay != 0 on a noisy net"):
        RainbowDQN(policy=pol, optim=AdamOptimizerFactory(weight_decay=1e-4))
    with pytest.raises(AssertionError, match="n_step_return_horizon"):
        RainbowDQN(policy=pol, optim=AdamOptimizerFactory(), n_step_return_horizon=0)
    plain = RainbowNet(6, (32,), 5, 51, noisy_std=None, device="cpu", seed=0)       # no noise slot to decay: legal
    RainbowDQN(policy=RainbowPolicy(model=plain, action_space=_Discrete(5)), optim=AdamOptimizerFactory(weight_decay=1e-4))
    algo = RainbowDQN(policy=pol, optim=AdamOptimizerFactory(lr=3e-4), target_update_freq=2)
    assert algo.use_target_network and algo.optim.lr == 3e-4 and torch.equal(algo.model_old.flat.data, net.flat.data)
    assert isinstance(algo.model_old, RainbowNet) and algo.model_old.flat.data_ptr() != net.flat.data_ptr()
    algo.eval()                                   # the lagged net follows the algorithm's mode
    assert not net.training and not algo.model_old.training
    algo.train()
    assert net.training and algo.model_old.training
    with pytest.raises(RuntimeError, match="outside of a training step"):
        algo.update(None, 8)


def test_member_of_a_multiagent_algorithm_and_checkpoint_round_trip(g):
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm

    ma = MultiAgentOffPolicyAlgorithm(algorithms=[_rainbow(), _rainbow()], env=_Env(2))
    assert set(ma.state_dict()) == {"agent_0", "agent_1"}
    ma.is_within_training_step = True
    assert ma.get_algorithm("agent_1").is_within_training_step
    algo = _rainbow(target_update_freq=2)
    sd = algo.to_reference_state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g["sd_shapes"]]
    assert any(k.endswith("eps_p") for k in sd) and any(k.startswith("model_old.model.") for k in sd)     # the noise is in it
    other = _rainbow(target_update_freq=2, net_kw=dict(seed=5))
    other.load_reference_state_dict(sd)
    assert torch.equal(other.policy.model.flat.data, algo.policy.model.flat.data)
    assert torch.equal(other.target_flat, algo.target_flat)
    algo._iter, algo._noise_ctr = 5, 10
    other.policy.model.flat.data.zero_()
    other.load_state_dict(algo.state_dict())
    assert other._iter == 5 and other._noise_ctr == 10 and torch.equal(other.policy.model.flat.data, algo.policy.model.flat.data)


def test_recorded_signatures_are_accepted(g):
    """Every parameter of the reference's constructors exists here under its name with its default (ours may add more)."""
    from tianshou_marl_amd.algorithm import RainbowDQN, RainbowPolicy

    for cls, key in ((RainbowPolicy, "sig_C51Policy"), (RainbowDQN, "sig_RainbowDQN")):
        mine = inspect.signature(cls.__init__).parameters
        for item in g[key]:
            name, default = str(item).split("=", 1)
            assert name in mine, (cls.__name__, name)
            ours = "<required>" if mine[name].default is inspect.Parameter.empty else repr(mine[name].default)
            assert ours == default, (cls.__name__, name, ours, default)


# ---- the restatement against the reference's runs --------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nl", "du"])
def test_restatement_reproduces_the_net(g, tag):
    R, _ = net_case(g, tag)
    init, x, d = g[f"{tag}_init"], g[f"{tag}_x"], g[f"{tag}_d"]
    for mode, training in (("train", True), ("eval", False)):
        y, cache = R.forward(init, x, training)
        assert R.min_relu_gap(cache) > float(g["delta"])
        grad = R.backward(cache, d)
        check_digest(g, f"{tag}_{mode}_out", y.reshape(-1))
        check_digest(g, f"{tag}_{mode}_grad", grad)
        for v in split_flat(grad, R.layers):
            assert not v["eps_p"].any() and not v["eps_q"].any()
            assert training or not (v["sigma_W"].any() or v["sigma_bias"].any())


def test_restatement_pieces_agree_with_each_other(g):
    R, _ = net_case(g, "du")
    init = g["du_init"].astype(np.float64)
    mu = compose(init, R.layers, False)
    flat0 = init.copy()
    for v in split_flat(flat0, R.layers):
        v["eps_p"][...], v["eps_q"][...] = 0.0, 0.0
    assert np.array_equal(compose(flat0, R.layers, True), mu) and not np.array_equal(compose(init, R.layers, True), mu)
    eg = np.random.RandomState(0).standard_normal(mu.size)
    back = noisy_grad(flat0, R.layers, eg, True)
    assert np.array_equal(compose(back, R.layers, False), eg)              # the mu blocks are the effective gradient
    rs = np.random.RandomState(1)
    q, v, d = rs.standard_normal((4, 15)), rs.standard_normal((4, 5)), rs.standard_normal((4, 15))
    out = dueling_combine(q, v, 3, 5)
    np.testing.assert_allclose(out.reshape(4, 3, 5).mean(1), v, atol=1e-15)
    d_q, d_v = dueling_combine_backward(d, 3, 5)
    np.testing.assert_allclose((out * d).sum(), (q * d_q).sum() + (v * d_v).sum(), rtol=1e-12)   # the adjoint of a linear map
    z64, z32 = philox_normals(7, 3, 4096), philox_normals(7, 3, 4096, np.float32)
    assert z32.dtype == np.float32 and np.abs(z64 - z32).max() < 1e-4 and abs(z64.mean()) < 0.1 and abs(z64.var() - 1) < 0.1
    assert np.array_equal(philox_normals(7, 3, 10), z64[:10]) and not np.array_equal(philox_normals(7, 4, 10), z64[:10])


def test_restatement_reproduces_the_updates(g):
    gd = np.load(DQN_GOLD)
    _, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    R, _ = up_case(g)
    assert (R.A, R.N, B, n_step, freq, steps) == (5, 51, 37, 3, 2, 3)
    RS = RainbowRestatement(g["up_init"], R, target_update_freq=freq)
    eps = g["up_eps"]
    for k in range(steps):
        pk = f"up_s{k}_"
        idx = g[pk + "indices"]
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        assert not np.array_equal(idx, idx_n)
        r = RS.update(obs[idx], act[idx], obs_next[idx], None, mc, gpow, vmask, eps_online=eps[k, 0], eps_target=eps[k, 1])
        assert r["relu_gap"] > float(g["delta"])
        assert r["loss"] == pytest.approx(float(g[pk + "loss"][0]), rel=REL, abs=0)
        check_digest(g, pk + "returns", r["returns"].reshape(-1))
        check_digest(g, pk + "grad", r["grads"])
        check_digest(g, pk + "weights", RS.weights())
        check_digest(g, pk + "targets", RS.targets())
        # quirk Q40: a copy call leaves the lagged net with the online net's noise
        lag = noise_of(RS.targets(), R.layers)
        assert np.array_equal(lag, eps[k, 0 if k % freq == 0 else 1].astype(np.float64))
        assert np.array_equal(noise_of(RS.weights(), R.layers), eps[k, 0].astype(np.float64))
