"""CPU tests of REDQ: the float64 restatement (tests/redq_restatement.py) against the reference's own float64 run in
tests/golden/redq.npz at 1e-10, the constructor's refusals, statistics fields, constructor signatures and checkpoint keys
against the reference's, the default subset draw against np.random.choice, the u64 subset mask, the `EnsembleCritic`'s flat
layout and init, and the host-side refusals of the new wrappers and entry points.  Nothing is launched."""
import dataclasses
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "redq.npz")

import redq_restatement as R  # noqa: E402
from dqn_restatement import nstep_walk  # noqa: E402
from test_host_cac import _Box, buffer_rows, flat_rows  # noqa: E402

from tianshou_marl_amd import _abi, _build, ops  # noqa: E402

N_CASES = 4
NETS = ("actor", "critic", "critic_old")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def cases(g):
    out = []
    for i, c in enumerate(g["cases"]):
        E, M, mode, n_step, prio, alpha = str(c).split("|")
        out.append(dict(i=i, E=int(E), M=int(M), mode=mode, n_step=int(n_step), prio=bool(int(prio)), alpha=alpha))
    return out


def dims_of(g):
    D, Ad, h1, h2 = (int(x) for x in g["dims"][:4])
    return [D, h1, h2, 2 * Ad], [D + Ad, h1, h2, 1]


def restatement_of(g, c):
    a_dims, c_dims = dims_of(g)
    pk = f"c{c['i']}_"
    fixed, la, te = g["sac"]
    alpha = R.alpha_state(float(la)) if c["alpha"] == "auto" else float(fixed)
    return R.RedqRestatement({n: g[pk + "init_" + n] for n in ("actor", "critic")}, a_dims, c_dims, c["E"], c["M"], c["mode"],
                             float(g["tau"]), lr=float(g["lr"]), actor_delay=int(g["actor_delay"]),
                             max_action=float(g["max_action"]), alpha=alpha, target_entropy=float(te), alpha_lr=float(g["lr"]))


def mine_stats(r):
    return np.array([r["actor_loss"], r["critic_loss"], r["alpha"], np.nan if r["alpha_loss"] is None else r["alpha_loss"]])


@pytest.mark.parametrize("ci", range(N_CASES))
def test_restatement_follows_the_reference_float64_run(g, ci):
    c = cases(g)[ci]
    assert len(cases(g)) == N_CASES and [str(k) for k in g["stat_keys"]] == ["actor_loss", "critic_loss", "alpha", "alpha_loss"]
    pk = f"c{ci}_"
    rows, RB = buffer_rows(g, int(g[pk + "seed"]))
    fr = flat_rows(g, rows)
    Rs = restatement_of(g, c)
    stepped = []
    for k in range(int(g["n_calls"])):
        sk = f"{pk}s{k}_"
        idx = g[sk + "indices"]
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, c["n_step"], float(g["gamma"]), 0)
        r = Rs.update(fr["obs"][idx], fr["act"][idx], fr["obs_next"][idx_n], mc, gpow, vmask, g[sk + "subset"],
                      weight=g.get(sk + "weight_in"), z_target=g[sk + "z_target"], z_actor=g.get(sk + "z_actor"))
        assert np.allclose(mine_stats(r), g[sk + "stats"], rtol=1e-10, atol=0, equal_nan=True)
        assert np.allclose(r["returns"], g[sk + "returns"], rtol=1e-10, atol=1e-13)
        assert np.allclose(r["prio"], g[sk + "prio"], rtol=1e-10, atol=1e-13)
        assert ("actor" in r["grads"]) == bool(g[sk + "actor_stepped"])
        stepped.append(bool(g[sk + "actor_stepped"]))
        for n, gv in r["grads"].items():
            assert np.allclose(gv, g[f"{sk}grad_{n}"], rtol=1e-10, atol=1e-15), (k, n)
        if c["alpha"] == "auto":
            assert np.isclose(Rs.alpha["log_alpha"], g[sk + "log_alpha"][0], rtol=1e-10)
    assert stepped == [False, True, False]   # call `actor_delay` is the first stepping one, not call 0
    assert g[pk + "s0_stats"][0] == 0.0 and np.isnan(g[pk + "s0_stats"][3]) and g[pk + "s2_stats"][0] == g[pk + "s1_stats"][0]
    for n in NETS:
        assert np.allclose(Rs.weights(n), g[f"{pk}s2_w_{n}"], rtol=1e-10, atol=1e-13), n
    assert Rs.kink > float(g["delta"])


def test_restated_ensemble_forward_is_the_per_member_mlp():
    rs = np.random.RandomState(0)
    dims, E, B = [5, 7, 3, 1], 3, 4
    P = sum(E * (dims[i] * dims[i + 1] + dims[i + 1]) for i in range(3))
    flat, x = rs.standard_normal(P), rs.standard_normal((B, dims[0]))
    out = R.ens_forward(flat, dims, E, x)[-1]
    layers = R.ens_layers(flat, dims, E)
    for e in range(E):
        h = x
        for i, (W, b) in enumerate(layers):
            h = h @ W[e] + b[e]
            if i < 2:
                h = np.maximum(h, 0)
        assert np.allclose(out[e], h, rtol=1e-13)


def cpu_learner(g, E=4, M=2, alpha="auto", critic=None, **kw):
    from tianshou_marl_amd.algorithm import REDQ, AutoAlpha, REDQPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import ContinuousActorProbabilistic, EnsembleCritic

    D, Ad, h1, h2 = (int(x) for x in g["dims"][:4])
    opt = lambda: AdamOptimizerFactory(lr=1e-3)  # noqa: E731
    actor = ContinuousActorProbabilistic(D, Ad, (h1, h2), conditioned_sigma=True, device="cpu", seed=0)
    critic = EnsembleCritic(D, Ad, E, (h1, h2), device="cpu", seed=1) if critic is None else critic
    a = AutoAlpha(-float(Ad), -1.0, opt()) if alpha == "auto" else 0.2
    return REDQ(policy=REDQPolicy(actor=actor, action_space=_Box(Ad)), policy_optim=opt(), critic=critic, critic_optim=opt(),
                ensemble_size=E, subset_size=M, alpha=a, **kw)


def test_constructor_refusals_are_the_reference_ones(g):
    from tianshou_marl_amd.utils.net import ContinuousCritic, EnsembleCritic

    with pytest.raises(ValueError, match="Unsupported target_mode: max"):
        cpu_learner(g, target_mode="max")
    for E, M in ((4, 0), (4, 5), (2, 3)):
        with pytest.raises(ValueError, match=r"Should be 0 < subset_size=\d <= ensemble_size=\d"):
            cpu_learner(g, E=E, M=M, critic=EnsembleCritic(6, 3, 4, (16, 16), device="cpu"))
    with pytest.raises(ValueError, match="holds 3 members, ensemble_size = 4"):
        cpu_learner(g, E=4, critic=EnsembleCritic(6, 3, 3, (16, 16), device="cpu"))
    with pytest.raises(TypeError, match="must be an EnsembleCritic"):
        cpu_learner(g, critic=ContinuousCritic(6, 3, (16, 16), device="cpu"))
    with pytest.raises(ValueError, match=r"must map 6 \+ 3 -> 1"):
        cpu_learner(g, critic=EnsembleCritic(5, 3, 4, (16, 16), device="cpu"))
    algo = cpu_learner(g)
    assert algo.critic_gradient_step == 0 and algo._last_actor_loss == 0.0 and algo.subset_source is None and algo.noise_source is None
    assert algo.policy.action_bound_method == "clip" and not hasattr(algo, "actor_old")


def test_signatures_statistics_and_checkpoint_keys_are_the_reference_ones(g):
    from tianshou_marl_amd.algorithm import REDQ, REDQPolicy, REDQTrainingStats

    for cls in (REDQPolicy, REDQ):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        mine = [f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}" for q in ps]
        ref = [str(x) for x in g[f"sig_{cls.__name__}"]]
        assert mine[:len(ref)] == ref, (cls.__name__, mine, ref)
        assert all(q.default is not inspect.Parameter.empty for q in ps[len(ref):])   # extras (seed) have defaults
        assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for q in ps)
    mine = [f.name for f in dataclasses.fields(REDQTrainingStats)]
    assert [f for f in mine if f in set(str(x) for x in g["stats_fields"])] == [str(x) for x in g["stats_fields"]]
    algo = cpu_learner(g, E=int(g["sd_ensemble_size"]))
    sd = algo.to_reference_state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_redq_keys"]]
    assert [",".join(str(n) for n in v.shape) for v in sd.values()] == [str(x) for x in g["sd_redq_shapes"]]
    other = cpu_learner(g, E=int(g["sd_ensemble_size"]))
    for _, net in other._nets():
        net.flat.data.add_(1.0)
    other.load_reference_state_dict(sd)
    for (_, a), (_, b) in zip(algo._nets(), other._nets()):
        assert torch.equal(a.flat.data, b.flat.data)


def test_native_state_dict_round_trips_counters_and_alpha(g):
    algo = cpu_learner(g)
    algo.critic_gradient_step, algo._last_actor_loss, algo.policy._sample_ctr = 7, -0.25, 123
    algo.alpha.set_log_alpha(-0.5)
    sd = algo.state_dict()
    assert {"critic_gradient_step", "_last_actor_loss", "alpha", "sample_ctr", "critic", "critic_old.module", "policy.actor",
            "policy_optim", "critic_optim"} <= set(sd)
    other = cpu_learner(g)
    other.load_state_dict(sd)
    assert (other.critic_gradient_step, other._last_actor_loss, other.policy._sample_ctr) == (7, -0.25, 123)
    assert float(other.alpha._log_alpha) == -0.5
    shapes = algo.critic_optim._shapes()   # the Adam state splits by the reference's parameter shapes
    assert shapes[0] == (4, 9, 16) and shapes[1] == (4, 1, 16) and sum(int(np.prod(s)) for s in shapes) == algo.critic.flat.numel()
    assert "alpha" not in cpu_learner(g, alpha="fix").state_dict()


def test_default_subset_is_numpys_global_choice_and_the_hook_replaces_it(g):
    algo = cpu_learner(g, E=10, M=2)
    for s in (0, 1, 12345):
        np.random.seed(s)
        want = np.random.choice(10, 2, replace=False)
        after = np.random.get_state()[1].copy()
        np.random.seed(s)
        got = algo._subset()
        assert np.array_equal(got, want) and np.array_equal(np.random.get_state()[1], after)   # one draw, no more
    algo.subset_source = lambda E, M: [7, 3][:M]
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    assert algo._subset().tolist() == [7, 3] and np.array_equal(np.random.get_state()[1], before)


def test_subset_mask_has_one_bit_per_member():
    assert ops.redq_subset_mask([0], 1) == 1 and ops.redq_subset_mask(np.array([3, 1]), 4) == 0b1010
    assert ops.redq_subset_mask(range(64), 64) == 2**64 - 1 and ops.redq_subset_mask([63], 64) == 1 << 63
    for idx, E in (([3, 1], 4), ([0, 9, 5], 10)):
        assert ops.redq_subset_mask(idx, E) == R.subset_mask(idx, E)
    for idx, E in (([], 4), ([1, 1], 4), ([4], 4), ([-1], 4), ([0], 65)):
        with pytest.raises(ValueError, match="not a set of distinct members"):
            ops.redq_subset_mask(idx, E)


def test_ensemble_critic_layout_init_and_lagged_copy():
    from tianshou_marl_amd.utils.net import EnsembleCritic, lagged_copy

    net = EnsembleCritic(6, 3, 4, (16, 8), device="cpu", seed=3)
    assert net.dims == [9, 16, 8, 1] and net.flat.numel() == 4 * (9 * 16 + 16 + 16 * 8 + 8 + 8 + 1) == ops.ens_mlp_param_count(net.desc, 4)
    assert net.param_shapes() == [(4, 9, 16), (4, 1, 16), (4, 16, 8), (4, 1, 8), (4, 8, 1), (4, 1, 1)]
    # views of the flat vector, in the reference's parameters() order: no transpose
    assert net.weight(0).data_ptr() == net.flat.data.data_ptr() and net.bias(0).data_ptr() == net.flat.data[4 * 9 * 16:].data_ptr()
    assert net.weight(1).data_ptr() == net.flat.data[4 * (9 * 16 + 16):].data_ptr()
    for i, k in enumerate((9, 16, 8)):   # EnsembleLinear's init: uniform +-sqrt(1 / in) for weight and bias
        bound = np.sqrt(1.0 / k)
        for v in (net.weight(i), net.bias(i)):
            assert float(v.abs().max()) <= bound and (v.numel() < 64 or float(v.abs().max()) > 0.8 * bound)
    assert torch.equal(EnsembleCritic(6, 3, 4, (16, 8), device="cpu", seed=3).flat.data, net.flat.data)
    state = torch.random.get_rng_state()
    twin = lagged_copy(net)
    assert torch.equal(torch.random.get_rng_state(), state)   # the global RNG is not drawn from
    assert torch.equal(twin.flat.data, net.flat.data) and twin.flat.data_ptr() != net.flat.data_ptr()
    assert twin.ensemble_size == 4 and twin.dims == net.dims
    sd = net.to_reference_state_dict("critic.")
    assert list(sd)[:2] == ["critic.preprocess.model.model.0.weight", "critic.preprocess.model.model.0.bias_weights"]
    assert list(sd)[-2:] == ["critic.last.model.0.weight", "critic.last.model.0.bias_weights"]


def test_wrappers_refuse_cpu_tensors_and_entries_check_bounds_without_a_device():
    _build.build()
    _abi.load()
    assert _abi.ENS_MAX_MEMBERS == 64 and _abi.REDQ_ROWS_PER_BLOCK == 256
    q, u = torch.zeros(3, 4), torch.zeros(4, dtype=torch.uint8)
    desc = ops.mlp_desc([9, 16, 1])
    P = ops.ens_mlp_param_count(desc, 3)
    assert P == 3 * (9 * 16 + 16 + 16 + 1) and _abi.call("tsm_ens_mlp_act_elems", desc, 3, 5) == 3 * 5 * 17
    for f in (lambda: ops.redq_target(q, 1, "min", q[0], q[0], u), lambda: ops.redq_critic_head(q, q[0]), lambda: ops.redq_mean_q(q),
              lambda: ops.ens_mlp_forward(desc, 3, torch.zeros(P), torch.zeros(4, 9))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()
    with pytest.raises(ValueError, match=r"ensemble size 65 outside \[1, 64\]"):
        ops.ens_mlp_param_count(desc, 65)
    assert _abi.call("tsm_ens_mlp_param_count", desc, 0) == -1 and _abi.call("tsm_ens_mlp_act_elems", desc, 65, 4) == -1
    # E = 65, a mismatched pointer set, a bad window, too many slabs: TSM_ERR_INVALID before any launch
    with pytest.raises(ValueError, match="ensemble size 65"):
        _abi.call("tsm_ens_mlp_forward", desc, 65, 1, 1, 4, 1, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_ens_mlp_forward", desc, 3, 1, None, 4, 1, None)
    with pytest.raises(ValueError, match="d_acts workspace required"):
        _abi.call("tsm_ens_mlp_backward", desc, 3, 1, 1, 4, 1, 1, None, 1, 1, 0, None)
    with pytest.raises(ValueError, match=r"x n_split 22000 outside \[1, 65535\]"):
        _abi.call("tsm_ens_mlp_backward", desc, 3, 1, 1, 4, 1, 1, 1, 22000, 1, 0, None)
    with pytest.raises(ValueError, match="slab_stride smaller"):
        _abi.call("tsm_ens_mlp_backward", desc, 3, 1, 1, 4, 1, 1, 1, 2, 1, P - 1, None)
    with pytest.raises(ValueError, match="leave the input width 9"):
        _abi.call("tsm_ens_mlp_input_grad", desc, 3, 1, 1, 4, 1, 1, 1, 7, 3, 1, 3, None)
    with pytest.raises(ValueError, match="ldx = 2 smaller"):
        _abi.call("tsm_ens_mlp_input_grad", desc, 3, 1, 1, 4, 1, 1, 1, 5, 3, 1, 2, None)
    with pytest.raises(ValueError, match="neither min"):
        _abi.call("tsm_redq_target", 1, 4, 3, 2, None, None, 1, 1, 1, 4, 1, None)
    for mask in (0, 1 << 4):
        with pytest.raises(ValueError, match="at least one of the 4 members and no other"):
            _abi.call("tsm_redq_target", 1, 4, mask, 0, None, None, 1, 1, 1, 4, 1, None)
    with pytest.raises(ValueError, match="comes with alpha_dev"):
        _abi.call("tsm_redq_target", 1, 4, 3, 0, 1, None, 1, 1, 1, 4, 1, None)
    with pytest.raises(ValueError, match="ensemble size 0"):
        _abi.call("tsm_redq_critic_head", 1, 0, 1, None, 4, 1, 1, 1, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_redq_mean_q", 1, 4, 4, None, None)
