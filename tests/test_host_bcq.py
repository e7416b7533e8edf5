"""CPU tests of BCQ: the float64 restatement (tests/bcq_restatement.py) against the reference's own float64 run in
tests/golden/bcq.npz at 1e-10, central differences of the closed-form VAE and perturbation gradients, constructor signatures
against the reference's, the checkpoint's key names and shapes against the reference's state_dict, the host-side refusals of
the new wrappers and of `tsm_bcq_check`.  Nothing is launched."""
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "bcq.npz")

import bcq_restatement as R  # noqa: E402
from cac_restatement import det_actor_head  # noqa: E402
from test_host_cql import buffer_rows, flat_rows  # noqa: E402

from tianshou_marl_amd import _abi, _build, ops  # noqa: E402

N_CASES = 6
NETS = ["pert", "critic", "critic2", "vae", "pert_old", "critic_old", "critic2_old"]
STAT_KEYS = ("actor_loss", "critic1_loss", "critic2_loss", "vae_loss")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def cases(g):
    out = []
    for i, c in enumerate(g["cases"]):
        no_c2, lmbda, phi, ls_bias, M = str(c).split("|")
        out.append(dict(i=i, no_c2=bool(int(no_c2)), lmbda=float(lmbda), phi=float(phi), ls_bias=float(ls_bias), max_action=float(M)))
    return out


def dims_of(g) -> dict:
    D, Ad, h1, h2, B, n_env, S, T, K, L, S_act, n_act, v1, v2 = (int(x) for x in g["dims"])
    return dict(D=D, Ad=Ad, hid=(h1, h2), B=B, T=T, K=K, L=L, S=S_act, n_act=n_act, vhid=(v1, v2))


def restatement_of(g, c):
    d = dims_of(g)
    D, Ad, L, hid, vhid = d["D"], d["Ad"], d["L"], d["hid"], d["vhid"]
    pk = f"c{c['i']}_"
    init = {n: g[pk + "init_" + n] for n in ("pert", "critic", "critic2", "vae") if pk + "init_" + n in g}
    return R.BcqRestatement(init, D, Ad, L, [D + Ad, *hid, Ad], [D + Ad, *hid, 1], [D + Ad, *vhid, 2 * L], [D + L, *vhid, Ad],
                            float(g["tau"]), float(g["gamma"]), lr=float(g["lr"]), max_action=c["max_action"], phi=c["phi"],
                            lmbda=c["lmbda"], num_sampled_action=d["K"], forward_sampled_times=d["S"])


@pytest.mark.parametrize("ci", range(N_CASES))
def test_restatement_follows_the_reference_float64_run(g, ci):
    c = cases(g)[ci]
    assert len(cases(g)) == N_CASES
    pk = f"c{ci}_"
    rows, _ = buffer_rows(g, int(g[pk + "seed"]), dims_of(g)["T"])
    fr = flat_rows(g, rows)
    Rst = restatement_of(g, c)
    for k in range(2):
        sk = f"{pk}s{k}_"
        idx = g[sk + "indices"]
        r = Rst.update(fr["obs"][idx], fr["act"][idx], fr["rew"][idx], fr["done"][idx], fr["obs_next"][idx], g[sk + "z_vae"],
                       g[sk + "z_next"], g[sk + "z_obs"])
        assert np.allclose([r[q] for q in STAT_KEYS], g[sk + "stats"], rtol=1e-10, atol=1e-13)
        assert np.allclose(r["target"], g[sk + "target"], rtol=1e-12, atol=0)
        for n, gv in r["grads"].items():
            assert np.allclose(gv, g[f"{sk}grad_{n}"], rtol=1e-10, atol=1e-15), (k, n)
        assert (Rst.clipped, Rst.below) == (float(g[sk + "clipped"]), float(g[sk + "below"]))
        assert (Rst.clipped > 0) == (c["phi"] > 0.1) and (Rst.below > 0) == (c["ls_bias"] < 0)   # what each case is there for
    for n in NETS:
        assert np.allclose(Rst.weights(n), g[f"{pk}s1_w_{n}"], rtol=1e-10, atol=1e-13), n
    a = Rst.act(g[pk + "act_obs"], g[pk + "act_z"])
    assert np.allclose(a["act"], g[pk + "act"], rtol=1e-10, atol=1e-13) and np.array_equal(a["index"], g[pk + "act_index"])
    assert Rst.kink > float(g["delta"])
    if c["no_c2"]:
        assert np.array_equal(Rst.weights("critic"), Rst.weights("critic2"))


def test_closed_form_vae_gradients_match_a_central_difference():
    """A check of the YARDSTICK alone (tests/bcq_restatement.py; no product code runs): vae_loss as a function of the encoder's
    output and of the decoder's raw output, through a linear decoder."""
    rs = np.random.RandomState(3)
    B, D, Ad, L, M = 4, 2, 3, 5, 1.5
    obs, act, eps = rs.standard_normal((B, D)), rs.uniform(-1, 1, (B, Ad)), rs.standard_normal((B, L))
    head = rs.standard_normal((B, 2 * L))
    head[0, L] = -4.5      # below the clamp: no gradient to that raw log_std
    W, b = rs.standard_normal((Ad, D + L)), rs.standard_normal(Ad)
    above = head.copy()
    above[1, L + 1] = 15.5  # above it (std^2 = exp(30) swamps a difference quotient: the zero alone is checked)
    x_above, std_above = R.latent(above, eps, obs)
    g_above = R.latent_grad((R.vae_head(x_above @ W.T + b, act, above, M)["d_raw"] @ W)[:, D:], above, eps)
    assert std_above[1, 1] == np.exp(15.0) and g_above[1, L + 1] == 0.0 and g_above[1, L] != 0.0

    def loss(hd):
        x_dec, _ = R.latent(hd, eps, obs)
        return R.vae_head(x_dec @ W.T + b, act, hd, M)["vae_loss"]

    x_dec, std = R.latent(head, eps, obs)
    assert std[0, 0] == np.exp(-4.0)
    vh = R.vae_head(x_dec @ W.T + b, act, head, M)
    d_head = R.latent_grad((vh["d_raw"] @ W)[:, D:], head, eps)
    assert d_head[0, L] == 0.0
    h = 1e-6
    for i in range(B):
        for j in range(2 * L):
            up, dn = head.copy(), head.copy()
            up[i, j] += h
            dn[i, j] -= h
            assert abs((loss(up) - loss(dn)) / (2 * h) - d_head[i, j]) < 1e-6 * max(1.0, abs(d_head[i, j])), (i, j)


def test_perturbation_factor_matches_a_central_difference_and_vanishes_past_the_clamp():
    """A check of the YARDSTICK alone (no product code runs): the restated factor with the restated actor head."""
    rs = np.random.RandomState(4)
    n, D, Ad, phi, M = 5, 2, 3, 0.5, 1.5
    x_in = np.concatenate([rs.standard_normal((n, D)), rs.uniform(-0.5, 0.5, (n, Ad))], 1)   # |u| < 0.5 + phi M < M
    x_in[0, D] = M - 0.01   # but this one: with raw_p = 2 it leaves the bounds
    raw_p = rs.standard_normal((n, Ad))
    raw_p[0, 0] = 2.0
    c, b0 = rs.standard_normal((n, Ad)), rs.standard_normal(n)
    q_of = lambda rp: (c * R.perturb(rp, x_in, D, phi, M)[0][:, D:]).sum(1) + b0   # noqa: E731  (a linear critic)
    x_out, factor, u = R.perturb(raw_p, x_in, D, phi, M)
    assert u[0, 0] > M and x_out[0, D] == M and factor[0, 0] == 0.0 and (factor[1:] > 0).all()
    ah = det_actor_head(c, factor, q_of(raw_p), M)
    h = 1e-6
    for i in range(n):
        for k in range(Ad):
            up, dn = raw_p.copy(), raw_p.copy()
            up[i, k] += h
            dn[i, k] -= h
            assert abs((-q_of(up).mean() + q_of(dn).mean()) / (2 * h) - ah["d_raw"][i, k]) < 1e-7


def test_kernel_restatements_at_their_edges():
    """A check of the YARDSTICK alone (no product code runs): hand-computed values of the restated kernels."""
    z = np.array([[0.5, -0.5, 0.7, -0.7, 0.1]])
    assert np.array_equal(R.decode_rows(np.zeros((1, 2)), 1, None, z)[:, 2:], [[0.5, -0.5, 0.5, -0.5, 0.1]])
    rows = R.decode_rows(np.arange(4.0).reshape(2, 2), 3, np.full((1, 2), 9.0), np.zeros((7, 1)))
    assert np.array_equal(rows[:, 0], [0, 0, 0, 2, 2, 2, 9])
    q = np.array([1.0, 3.0, 3.0, 2.0, 5.0, 5.0])
    act, index = R.select(q, np.arange(12.0).reshape(6, 2), 3, 1, 1)
    assert np.array_equal(index, [1, 1]) and np.array_equal(act, [[3.0], [9.0]])   # the first of the tied maxima
    t = R.target([1.0, 4.0, 2.0, 0.0], [3.0, 2.0, 2.0, 1.0], [10.0, 20.0], [True, False], 2, 0.5, 0.75)
    assert np.array_equal(t, [10.0 + 0.5 * max(0.75 * 1 + 0.25 * 3, 0.75 * 2 + 0.25 * 4), 20.0])


def test_signatures_and_defaults_are_the_reference_ones(g):
    from tianshou_marl_amd.algorithm import BCQ, BCQPolicy

    for cls in (BCQ, BCQPolicy):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        mine = [f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}" for q in ps]
        ref = [str(x) for x in g[f"sig_{cls.__name__}"]]
        assert mine[:len(ref)] == ref, (cls.__name__, mine, ref)
        assert all(q.default is not inspect.Parameter.empty for q in ps[len(ref):])
        assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for q in ps)


def test_net_views_carry_the_reference_keys_and_cover_the_vector(g):
    from tianshou_marl_amd.utils.net import VAE, ContinuousCritic, Perturbation

    d = dims_of(g)
    D, Ad, L = d["D"], d["Ad"], d["L"]
    nets = {"policy.actor_perturbation.": Perturbation(obs_dim=D, act_dim=Ad, hidden_sizes=d["hid"], device="cpu", seed=1),
            "policy.critic.": ContinuousCritic(D, Ad, d["hid"], device="cpu", seed=2),
            "policy.vae.": VAE(encoder_hidden_sizes=d["vhid"], decoder_hidden_sizes=d["vhid"], obs_dim=D, act_dim=Ad, latent_dim=L,
                               device="cpu", seed=3)}
    ref = dict(zip((str(k) for k in g["sd_keys"]), (str(s) for s in g["sd_shapes"])))
    for prefix, net in nets.items():
        views = net.reference_named_views()
        want = [k for k in ref if k.startswith(prefix)]
        assert [prefix + k for k, _ in views] == want   # the reference module's state_dict order
        for k, v in views:
            assert "x".join(str(s) for s in v.shape) == ref[prefix + k], k
        assert sum(v.numel() for _, v in views) == net.flat.numel() == sum(v.numel() for v in net.param_views())
        ptrs = sorted((v.data_ptr(), v.numel()) for v in net.param_views())   # the optimizer's split tiles the vector in order
        assert [p for p, _ in ptrs] == [v.data_ptr() for v in net.param_views()]
    vae = nets["policy.vae."]
    views = dict(vae.reference_named_views())
    W, b = vae.encoder.weight(vae.encoder.n_layers - 1), vae.encoder.bias(vae.encoder.n_layers - 1)
    assert torch.equal(views["mean.weight"], W[:L]) and torch.equal(views["log_std.weight"], W[L:])
    assert torch.equal(views["mean.bias"], b[:L]) and torch.equal(views["log_std.bias"], b[L:])
    sd = vae.to_reference_state_dict()
    twin = vae.clone_over(torch.zeros_like(vae.flat.data))
    twin.load_reference_state_dict(sd)
    assert torch.equal(twin.flat.data, vae.flat.data) and twin.decoder.flat.data_ptr() != vae.decoder.flat.data_ptr()
    assert (vae.max_action, vae.latent_dim) == (twin.max_action, twin.latent_dim)
    prefixes = {k.split("preprocess")[0].split("encoder")[0].split("mean")[0].split("log_std")[0].split("decoder")[0].split("last")[0]
                for k in ref}
    assert prefixes == {"policy.actor_perturbation.", "policy.critic.", "policy.vae.", "actor_perturbation_target.module.",
                        "critic_target.module.", "critic2.", "critic2_target.module."}


def test_checkpoint_in_the_reference_layout_has_exactly_the_reference_module_keys(g):
    from tianshou_marl_amd.algorithm import BCQ, BCQPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import VAE, ContinuousCritic, Perturbation

    class Box:
        def __init__(self, n):
            self.shape, self.low, self.high = (n,), np.full(n, -1.0, np.float32), np.full(n, 1.0, np.float32)

    d = dims_of(g)
    D, Ad, L = d["D"], d["Ad"], d["L"]
    opt = lambda: AdamOptimizerFactory(lr=1e-3)  # noqa: E731

    def make(seed, critic2):
        policy = BCQPolicy(actor_perturbation=Perturbation(obs_dim=D, act_dim=Ad, hidden_sizes=d["hid"], device="cpu", seed=seed),
                           action_space=Box(Ad), critic=ContinuousCritic(D, Ad, d["hid"], device="cpu", seed=seed + 1),
                           vae=VAE(encoder_hidden_sizes=d["vhid"], decoder_hidden_sizes=d["vhid"], obs_dim=D, act_dim=Ad,
                                   latent_dim=L, device="cpu", seed=seed + 2), forward_sampled_times=d["S"])
        c2 = ContinuousCritic(D, Ad, d["hid"], device="cpu", seed=seed + 3) if critic2 else None
        return BCQ(policy=policy, actor_perturbation_optim=opt(), critic_optim=opt(), vae_optim=opt(), critic2=c2)

    a = make(1, True)
    sd = a.to_reference_state_dict()
    ref = dict(zip((str(k) for k in g["sd_keys"]), (str(s) for s in g["sd_shapes"])))
    assert [k for k in sd if k != "sample_ctr"] == list(ref)   # the module keys, in the reference's order; then the counter
    for k, shape in ref.items():
        assert "x".join(str(n) for n in sd[k].shape) == shape, k
    b = make(11, False)
    assert torch.equal(b.critic2.flat.data, b.critic.flat.data) and b.critic2 is not b.critic   # critic2=None: a copy
    b.policy._sample_ctr = 5
    b.load_reference_state_dict(sd)
    assert b.policy._sample_ctr == 0
    for (pa, na), (_, nb) in zip(a._nets(), b._nets()):
        assert torch.equal(na.flat.data, nb.flat.data), pa
    native = a.state_dict()
    assert {"actor_perturbation_optim", "critic_optim", "critic2_optim", "vae_optim", "sample_ctr"} <= set(native)
    b2 = make(21, True)
    b2.load_state_dict(native)
    assert torch.equal(b2.actor_perturbation_target.flat.data, a.actor_perturbation_target.flat.data)


def test_wrappers_refuse_cpu_tensors():
    z, q = torch.zeros(4, 3), torch.zeros(4)
    x = torch.zeros(4, 5)
    calls = [lambda: ops.bcq_latent(torch.zeros(4, 6), z, x), lambda: ops.bcq_decode_rows(x, 1, None, z),
             lambda: ops.bcq_action_rows(z, torch.zeros(4, 8), 5), lambda: ops.bcq_target(q, q, q, q.bool(), 1, 0.99, 0.75),
             lambda: ops.bcq_vae_head(z, z, torch.zeros(4, 6)), lambda: ops.bcq_latent_grad(z, torch.zeros(4, 6), z),
             lambda: ops.bcq_perturb(z, torch.zeros(4, 8), 0.05), lambda: ops.bcq_select(q, torch.zeros(4, 8), 2, 5, 3)]
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


def test_bcq_check_bounds_through_the_abi():
    _build.build()
    _abi.load()
    _abi.call("tsm_bcq_check", 1, 1, 1)
    _abi.call("tsm_bcq_check", _abi.CAC_MAX_ACT_DIM, 2 * _abi.CAC_MAX_ACT_DIM, 100)
    with pytest.raises(ValueError, match=r"act_dim = 65 outside \[1, 64\]"):
        _abi.call("tsm_bcq_check", _abi.CAC_MAX_ACT_DIM + 1, 1, 1)
    with pytest.raises(ValueError, match=r"latent_dim = 129 outside \[1, 128\]"):
        _abi.call("tsm_bcq_check", 1, 2 * _abi.CAC_MAX_ACT_DIM + 1, 1)
    with pytest.raises(ValueError, match=r"latent_dim = 0 outside"):
        ops.bcq_check(3, 0)
    with pytest.raises(ValueError, match="at least 1 but got: 0"):
        ops.bcq_check(3, 2, 0)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_bcq_latent", None, None, None, 4, 2, 3, None, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_bcq_decode_rows", 1, 2, 1, None, 1, 1, 2, 3, 1, None)   # n_b = 1 without src_b
    with pytest.raises(ValueError, match="must not be x_in"):
        _abi.call("tsm_bcq_perturb", 1, 8, 4, 2, 3, 0.05, 1.0, 8, None, None)
    with pytest.raises(ValueError, match=r"columns \[6, 9\) leave the row of 8"):
        _abi.call("tsm_bcq_select", 1, 1, 8, 6, 4, 2, 3, 1, 1, None)
    for name in ("tsm_bcq_action_rows", "tsm_bcq_target", "tsm_bcq_vae_head", "tsm_bcq_latent_grad"):
        assert name in _abi.SIGNATURES
