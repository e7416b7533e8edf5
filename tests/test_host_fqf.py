"""CPU tests of the FQF port: the import surface, the constructors' refusals, tsm_fqf_check and the argument checks of
tsm_fqf_propose / tsm_fqf_propose_backward / tsm_fqf_values / tsm_fqf_head (which fail before touching a device), the recorded
reference signatures and statistics fields, the reference-layout checkpoint keys, and the float64 restatement
(tests/fqf_restatement.py) against the reference's own runs (tests/golden/fqf.npz) to 1e-10 relative."""
import dataclasses
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "fqf.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")

from dqn_restatement import nstep_walk  # noqa: E402
from fqf_restatement import FqfRestatement, fqf_head, fqf_values, fractions_of, propose  # noqa: E402
from test_host_dqn import _Discrete, _Env, check_digest, up_inputs  # noqa: E402

# (R, H, N, the preprocess net ends in its ReLU): rows no multiple of the workgroup's 16; H a multiple of 16 but not of 64 with
# the smallest N; both maxima
PP_CASES = [(37, 32, 8, 1), (37, 48, 3, 0), (17, 512, 64, 1)]
# (A, N): the update's shape, both minima, the largest N, the largest A
GRID = [(5, 8), (1, 3), (3, 64), (64, 4)]
ENT_COEFS = (0.0, 0.01)
STAT_KEYS = ("loss", "quantile_loss", "fraction_loss", "entropy_loss")
REL = 1e-10


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def pp_inputs(case):
    """Features, the fraction layer and the upstream gradient of one case, from a seeded stream."""
    R, H, N, _ = case
    rs = np.random.RandomState(9000 + 131 * R + 17 * N + H)
    bound = 1.0 / np.sqrt(H)
    return dict(f=rs.standard_normal((R, H)).astype(np.float32), Wf=rs.uniform(-bound, bound, (N, H)).astype(np.float32),
                bf=rs.uniform(-bound, bound, N).astype(np.float32), d_logits=rs.standard_normal((R, N)).astype(np.float32))


def head_inputs(g, A, N):
    """The shared head inputs of one (A, N): the i8 lattices back as float32 values, the rest as stored; the fractions of both
    proposals in float64."""
    p = f"hd_A{A}_N{N}_"
    d = {k: g[p + k] for k in ("xf", "xf_next", "act", "mc", "gpow", "vmask", "weight", "mask")}
    d.update({k: (g[p + k].astype(np.float32) / np.float32(8.0)) for k in ("out", "on", "tg")})
    d["out_tau"] = g[p + "out_tau"].astype(np.float32) / np.float32(16.0)
    d["fr"], d["fr_next"] = fractions_of(d["xf"]), fractions_of(d["xf_next"])
    return d


def case_flags(case):
    """'t1w0m1e1' -> (target net, weight, mask, index into ENT_COEFS)."""
    case = str(case)
    return case[1] == "1", case[3] == "1", case[5] == "1", int(case[7])


def ref_head(d, case):
    tgt, wgt, msk, e = case_flags(case)
    return fqf_head(d["out"], d["out_tau"], d["xf"], d["on"], d["fr_next"]["taus"], d["tg"] if tgt else None,
                    d["mask"] if msk else None, d["act"], d["mc"], d["gpow"], d["vmask"], d["weight"] if wgt else None, ENT_COEFS[e])


def up_net_dims(g):
    d = [int(x) for x in g["up_dims"]]
    return dict(pre=d[:2], hidden=d[2:3], A=d[3], C=d[4], N=d[5])


def up_restatement(g, freq):
    u = up_net_dims(g)
    return FqfRestatement(g["up_init"], g["up_frac_init"], u["pre"], [u["pre"][-1], *u["hidden"], u["A"]], u["C"], u["N"],
                          feature_act=True, target_update_freq=freq, ent_coef=float(g["up_ent_coef"]))


def _fqf(pre=(6, 32), A=5, hidden=(32,), C=8, N=8, policy_kw=None, **kw):
    from tianshou_marl_amd.algorithm import FQF, FQFPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import FractionProposalNet, FullQuantileNet

    net = FullQuantileNet(list(pre), A, hidden, num_cosines=C, device="cpu", seed=0)
    frac = FractionProposalNet(N, pre[-1], device="cpu", seed=1)
    pol = FQFPolicy(model=net, fraction_model=frac, action_space=_Discrete(A), **(policy_kw or {}))
    return FQF(policy=pol, optim=AdamOptimizerFactory(), fraction_optim=AdamOptimizerFactory(lr=2e-4), **kw)


def test_importable_from_algorithm():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import FQF, QRDQN, FQFPolicy, FQFTrainingStats, QRDQNPolicy
    from tianshou_marl_amd.algorithm.fqf import FQF as F2
    from tianshou_marl_amd.utils.net import FractionProposalNet, FullQuantileNet, ImplicitQuantileNet

    assert FQF is F2 and issubclass(FQFPolicy, QRDQNPolicy) and issubclass(FQF, QRDQN) and FQFTrainingStats is not None
    assert issubclass(FullQuantileNet, ImplicitQuantileNet) and FractionProposalNet is not None
    for name in ("fqf_check", "fqf_propose", "fqf_propose_backward", "fqf_values", "fqf_head"):
        assert callable(getattr(ops, name)), name


def test_fqf_check_names_the_limit_without_a_device():
    from tianshou_marl_amd import _abi, ops

    for N, H, A in ((3, 16, 1), (64, 512, 64), (3, 512, 64), (64, 16, 1)):
        ops.fqf_check(N, H, A)
    for args, msg in (((2, 32, 5), r"num_fractions = 2 outside \[3, 64\]"), ((65, 32, 5), r"num_fractions = 65 outside \[3, 64\]"),
                      ((8, 8, 5), r"embedding_dim = 8 is not a multiple of 16 in \[16, 512\]"),
                      ((8, 24, 5), "embedding_dim = 24 is not a multiple of 16"), ((8, 528, 5), r"embedding_dim = 528 .* \[16, 512\]"),
                      ((8, 32, 0), r"n_act = 0 outside \[1, 64\]"), ((8, 32, 65), r"n_act = 65 outside \[1, 64\]")):
        with pytest.raises(ValueError, match=msg):
            ops.fqf_check(*args)
    _abi.call("tsm_fqf_check", 8, 32, 5)


def test_entry_points_reject_bad_arguments_without_a_device():
    from tianshou_marl_amd import _abi

    fwd = lambda R=37, N=8, H=32: _abi.call("tsm_fqf_propose", None, None, None, R, N, H, 1, None, None, None, None, None)  # noqa: E731
    bwd = lambda R=37, N=8, H=32, ns=1, stride=10000, wo=0, bo=256: _abi.call(  # noqa: E731
        "tsm_fqf_propose_backward", None, None, R, N, H, 1, ns, None, stride, wo, bo, None)
    for fn in (fwd, bwd):
        with pytest.raises(ValueError, match="num_fractions = 2 "):
            fn(N=2)
        with pytest.raises(ValueError, match="embedding_dim = 40"):
            fn(H=40)
        with pytest.raises(ValueError, match="R = 0 out of range"):
            fn(R=0)
        with pytest.raises(ValueError, match="null pointer"):
            fn()
    with pytest.raises(ValueError, match="n_split = 0"):
        bwd(ns=0)
    for kw in (dict(bo=100), dict(stride=260), dict(wo=-1)):   # bias inside the weight block; past the slab's end; before it
        with pytest.raises(ValueError, match="must lie apart inside a slab"):
            bwd(**kw)
    vals = lambda R=4, N=8, A=5: _abi.call("tsm_fqf_values", None, None, R, N, A, None, None)  # noqa: E731
    with pytest.raises(ValueError, match="n_act = 65"):
        vals(A=65)
    with pytest.raises(ValueError, match="num_fractions = 65"):
        vals(N=65)
    with pytest.raises(ValueError, match="null pointer"):
        vals()
    vals(R=0)   # nothing to do: no pointer is read
    head = lambda B=37, A=5, N=8: _abi.call("tsm_fqf_head", *([None] * 14), 0.01, B, A, N, *([None] * 7))  # noqa: E731
    with pytest.raises(ValueError, match="n_act = 0"):
        head(A=0)
    with pytest.raises(ValueError, match="num_fractions = 2 "):
        head(N=2)
    with pytest.raises(ValueError, match="B = 0"):
        head(B=0)
    with pytest.raises(ValueError, match="null pointer"):
        head()


def test_ops_refuse_cpu_tensors_and_check_shapes_first():
    from tianshou_marl_amd import ops

    f, Wf, bf, v = torch.zeros(4, 16), torch.zeros(3, 16), torch.zeros(3), torch.zeros(4)
    out, taus, hats = torch.zeros(4, 3, 5), torch.zeros(4, 4), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fqf_propose(f, Wf, bf)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fqf_propose_backward(hats, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fqf_values(out, taus, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fqf_head(out, torch.zeros(4, 2, 5), torch.zeros(4, 5), out, taus, hats, hats, v, v.long(), v, v, v.to(torch.uint8))


def test_nets_are_flat_vectors_with_the_reference_init():
    from tianshou_marl_amd.utils.net import FractionProposalNet, FullQuantileNet

    frac = FractionProposalNet(8, 32, device="cpu", seed=3)
    assert frac.flat.numel() == 8 * 32 + 8 and frac.Wf.shape == (8, 32) and frac.bf.shape == (8,)
    assert frac.Wf.data_ptr() == frac.flat.data_ptr() and frac.bf.data_ptr() == frac.flat.data_ptr() + 4 * 256
    bound = 0.01 * np.sqrt(6.0 / (32 + 8))          # xavier_uniform_(gain=0.01), zero bias (discrete.py:235-236)
    assert 0.5 * bound < float(frac.Wf.abs().max()) <= bound and not frac.bf.any()
    assert [k for k, _ in frac.reference_named_views()] == ["net.weight", "net.bias"]
    twin = frac.clone_over(torch.zeros_like(frac.flat.data))
    assert (twin.num_fractions, twin.embedding_dim, twin.feature_act) == (8, 32, True)
    with pytest.raises(ValueError, match="storage must be"):
        frac.clone_over(torch.zeros(7))
    with pytest.raises(ValueError, match="num_fractions = 2 "):
        FractionProposalNet(2, 32, device="cpu")
    with pytest.raises(ValueError, match="embedding_dim = 24"):
        FractionProposalNet(8, 24, device="cpu")
    with pytest.raises(RuntimeError, match="before forward"):
        frac.backward(torch.zeros(4, 8))
    net = FullQuantileNet([6, 32], 5, (32,), num_cosines=8, device="cpu", seed=0)
    assert type(net.clone_over(torch.zeros_like(net.flat.data))) is FullQuantileNet


def test_constructors_validate():
    from tianshou_marl_amd.algorithm import FQF, FQFPolicy, IQNPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import FlatAdam, FractionProposalNet, FullQuantileNet, ImplicitQuantileNet

    net = FullQuantileNet([6, 32], 5, (32,), num_cosines=8, device="cpu", seed=0)
    frac = FractionProposalNet(8, 32, device="cpu", seed=1)
    with pytest.raises(TypeError, match="FullQuantileNet"):
        FQFPolicy(model=ImplicitQuantileNet([6, 32], 5, device="cpu"), fraction_model=frac, action_space=_Discrete(5))
    with pytest.raises(TypeError, match="FractionProposalNet"):
        FQFPolicy(model=net, fraction_model=torch.nn.Linear(32, 8), action_space=_Discrete(5))
    with pytest.raises(ValueError, match="features of width 16"):
        FQFPolicy(model=net, fraction_model=FractionProposalNet(8, 16, device="cpu"), action_space=_Discrete(5))
    with pytest.raises(ValueError, match="5 outputs"):
        FQFPolicy(model=net, fraction_model=frac, action_space=_Discrete(4))
    pol = FQFPolicy(model=net, fraction_model=frac, action_space=_Discrete(5), eps_training=0.25)
    assert pol.n_act == 5 and pol.fraction_model is frac and not isinstance(pol, IQNPolicy)
    with pytest.raises(ValueError, match="pass `fractions`"):
        pol.compute_q_value(torch.zeros(4, 5, 8), None)
    with pytest.raises(TypeError, match="needs a FQFPolicy"):
        FQF(policy=torch.nn.Linear(2, 2), optim=AdamOptimizerFactory(), fraction_optim=AdamOptimizerFactory())
    with pytest.raises(TypeError, match="fraction_optim"):
        FQF(policy=pol, optim=AdamOptimizerFactory(), fraction_optim=None)
    with pytest.raises(ValueError, match="own flat parameter vector"):
        FQF(policy=pol, optim=AdamOptimizerFactory(), fraction_optim=FlatAdam(net))
    algo = FQF(policy=pol, optim=AdamOptimizerFactory(lr=3e-4), fraction_optim=AdamOptimizerFactory(lr=2e-5), num_fractions=13,
               ent_coef=0.01, target_update_freq=2)
    tau = torch.linspace(0, 1, 14)                       # `num_fractions` sizes tau_hat and nothing else
    assert algo.tau_hat.shape == (1, 13, 1) and torch.equal(algo.tau_hat.view(-1), (tau[:-1] + tau[1:]) / 2)
    assert algo.optim.lr == 3e-4 and algo.fraction_optim.lr == 2e-5 and algo.ent_coef == 0.01
    assert algo.optim.param.data_ptr() == net.flat.data_ptr() and algo.optim.param.numel() == net.flat.numel()
    assert algo.fraction_optim.param.data_ptr() == frac.flat.data_ptr()
    assert isinstance(algo.model_old, FullQuantileNet) and torch.equal(algo.model_old.flat.data, net.flat.data)
    assert not hasattr(algo, "fraction_model_old")       # there is no lagged fraction model
    with pytest.raises(RuntimeError, match="outside of a training step"):
        algo.update(None, 8)


def test_member_of_a_multiagent_algorithm_and_checkpoint_round_trip():
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm

    algo, other = _fqf(target_update_freq=2), _fqf(target_update_freq=2)
    ma = MultiAgentOffPolicyAlgorithm(algorithms=[algo, _fqf()], env=_Env(2))
    assert set(ma.state_dict()) == {"agent_0", "agent_1"}
    algo.policy.fraction_model.flat.data.add_(0.5)
    algo.policy.model.flat.data.mul_(0.5)
    algo._iter, algo.fraction_optim.step_count, algo.optim.step_count = 5, 3, 3
    algo.fraction_optim.exp_avg.fill_(0.25)
    other.load_state_dict(algo.state_dict())
    assert other._iter == 5 and other.fraction_optim.step_count == 3 and other.optim.step_count == 3
    assert torch.equal(other.policy.fraction_model.flat.data, algo.policy.fraction_model.flat.data)
    assert torch.equal(other.policy.model.flat.data, algo.policy.model.flat.data)
    assert torch.equal(other.fraction_optim.exp_avg, algo.fraction_optim.exp_avg) and other.fraction_optim.lr == 2e-4


def test_recorded_signatures_and_stats_fields_are_accepted(g):
    """Every parameter of the reference's constructors exists here under its name, at its position, with its default (ours
    may add more, with defaults); FQFTrainingStats has the reference's fields."""
    from tianshou_marl_amd.algorithm import FQF, FQFPolicy, FQFTrainingStats

    for cls in (FQFPolicy, FQF):
        mine = inspect.signature(cls.__init__).parameters
        names = [n for n in mine if n != "self"]
        for pos, item in enumerate(g[f"sig_{cls.__name__}"]):
            name, default = str(item).split("=", 1)
            assert names[pos] == name, (cls.__name__, pos, name, names)
            ours = "<required>" if mine[name].default is inspect.Parameter.empty else repr(mine[name].default)
            assert ours == default, (cls.__name__, name, ours, default)
        for n in names[len(g[f"sig_{cls.__name__}"]):]:
            assert mine[n].default is not inspect.Parameter.empty, (cls.__name__, n)
    mine = [f.name for f in dataclasses.fields(FQFTrainingStats)]
    for name in g["sig_FQFTrainingStats"]:
        assert str(name) in mine, name
    assert set(STAT_KEYS) <= set(mine)
    s = FQFTrainingStats(loss=1.0, quantile_loss=0.5, fraction_loss=0.25, entropy_loss=2.0)
    assert s.get_loss_stats_dict()["quantile_loss"] == 0.5


def test_reference_checkpoint_layout(g):
    u = up_net_dims(g)
    mk = lambda: _fqf(u["pre"], u["A"], u["hidden"], u["C"], u["N"], target_update_freq=2)  # noqa: E731
    algo = mk()
    sd = algo.to_reference_state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g["sd_shapes"]]
    keys = list(sd.keys())
    first = lambda p: min(i for i, k in enumerate(keys) if k.startswith(p))  # noqa: E731
    assert keys[0] == "tau_hat" and first("policy.model.") < first("policy.fraction_model.net.") < first("model_old.module.")
    assert algo.policy.model.flat.numel() == len(g["up_init"]) and algo.policy.fraction_model.flat.numel() == len(g["up_frac_init"])
    other = mk()
    for t in (other.policy.model.flat.data, other.target_flat, other.policy.fraction_model.flat.data):
        t.zero_()
    other.load_reference_state_dict(sd)
    assert torch.equal(other.policy.model.flat.data, algo.policy.model.flat.data) and torch.equal(other.target_flat, algo.target_flat)
    assert torch.equal(other.policy.fraction_model.flat.data, algo.policy.fraction_model.flat.data)


# ---- the restatement against the reference's runs --------------------------------------------------------------------
@pytest.mark.parametrize("case", PP_CASES)
def test_restatement_reproduces_the_proposal(g, case):
    p = "pp_R%d_H%d_N%d_" % case[:3]
    d = pp_inputs(case)
    r = propose(d["f"], d["Wf"], d["bf"], bool(case[3]), d["d_logits"])
    assert not case[3] or np.abs(d["f"]).min() > float(g["delta"])
    assert (r["taus"][:, 0] == 0).all() and (np.diff(r["taus"], axis=1) > 0).all() and np.abs(r["taus"][:, -1] - 1).max() < 1e-12
    for k in ("taus", "tau_hats", "entropies", "dWf", "dbf"):
        check_digest(g, p + k, r[k].reshape(-1))


@pytest.mark.parametrize("A,N", GRID)
def test_fixture_rows_cover_the_cases_asked_for_and_values_match(g, A, N):
    d = head_inputs(g, A, N)
    p = f"dv_A{A}_N{N}_"
    assert d["out"].shape == (37, N, A) and d["out_tau"].shape == (37, N - 1, A) and d["xf"].shape == (37, N) and not d["vmask"][5]
    q = g[p + "q"]
    if A > 1:
        assert np.array_equal(d["on"][3, :, 0], d["on"][3, :, 1]) and q[3, 0] == q[3, 1] == q[3].max() and g[p + "act"][3] == 0
    r0, r1 = fqf_values(d["on"], d["fr_next"]["taus"]), fqf_values(d["on"], d["fr_next"]["taus"], d["mask"])
    np.testing.assert_allclose(r0["q"], q, rtol=REL, atol=REL * np.abs(q).max())
    assert np.array_equal(r0["act"], g[p + "act"]) and np.array_equal(r1["act"], g[p + "act_masked"])
    assert d["mask"][np.arange(37), r1["act"]].all()
    assert len(g["cases"]) == 16 and tuple(g["ent_coefs"]) == ENT_COEFS


@pytest.mark.parametrize("A,N", GRID)
def test_restatement_reproduces_the_head(g, A, N):
    d = head_inputs(g, A, N)
    p = f"hq_A{A}_N{N}_"
    for c, case in enumerate(g["cases"]):
        h = ref_head(d, case)
        assert h["returns"].shape == (37, N) and h["cmp_gap"] > float(g["delta"])
        for i, k in enumerate(STAT_KEYS):
            assert h[k] == pytest.approx(float(g[p + "stats"][c, 0, i]), rel=REL, abs=1e-13), (case, k)
        np.testing.assert_allclose(h["prio"], g[p + "prio"][c], rtol=REL, atol=REL * np.abs(g[p + "prio"][c]).max(), err_msg=case)
        assert np.array_equal(h["a_star"], g[p + "astar"][c]), case
        check_digest(g, f"{p}c{c}_dout", h["d_out"].reshape(-1))
        check_digest(g, f"{p}c{c}_dlog", h["d_logits"].reshape(-1))
        check_digest(g, f"{p}c{c}_ret", h["returns"].reshape(-1))
        assert (np.abs(h["u"]) > 1.0).any() and (np.abs(h["u"]) < 1.0).any()


def test_restatement_reproduces_the_updates(g):
    gd = np.load(DQN_GOLD)
    _, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    u = up_net_dims(g)
    assert (u["pre"], u["hidden"], u["A"], u["C"], u["N"], B, n_step, freq, steps) == ([6, 32], [32], 5, 8, 8, 37, 3, 2, 3)
    assert float(g["up_ent_coef"]) == 0.01
    R = up_restatement(g, freq)
    for k in range(steps):
        pk = f"up_s{k}_"
        idx = g[pk + "indices"]
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        r = R.update(obs[idx], act[idx], obs_next[idx_n], None, mc, gpow, vmask)
        assert r["head_gap"] > float(g["delta"]) and r["relu_gap"] > float(g["relu_delta"])
        for i, key in enumerate(STAT_KEYS):
            assert r[key] == pytest.approx(float(g[pk + "stats"][0, i]), rel=REL, abs=1e-13), key
        check_digest(g, pk + "returns", r["returns"].reshape(-1))
        check_digest(g, pk + "weights", R.weights())
        check_digest(g, pk + "targets", R.targets())
        check_digest(g, pk + "frac_weights", R.frac_weights())
