"""GPU tests (`-m gpu`) of FQF: tsm_fqf_propose / _propose_backward, tsm_fqf_values and tsm_fqf_head (csrc/fqf.hip),
`FractionProposalNet` and `FullQuantileNet`, updates of the learner on a device buffer, in front of a prioritized buffer and as
a member of MultiAgentOffPolicyAlgorithm, and the acting path.

References: tests/golden/fqf.npz (the reference's own float64 and float32 runs) and the float64 restatement
(tests/fqf_restatement.py, pinned to those runs to 1e-10 by tests/test_host_fqf.py; it supplies the full arrays of which the
fixture keeps digests).  Bars, those of test_gpu_iqn.py:
  * a*, actions, zeros of the gradients: exact;
  * everything else the kernels produce: max |hip - ref64| <= 1e-5 max |ref64| + e_ref per array (`_bar`), e_ref = max |ref32 -
    ref64| of the reference's own two runs, or of the restatement's float32 and float64 runs where the reference returns no
    such array (logp, the saturated proposal); for the composite nets' backward 64 ulp of the array's scale, as test_gpu_iqn.py;
  * losses, returns, gradients and weights of full updates, IS weights and tree leaves: test_gpu_dqn.py's `_check`.
Every comparison prints `PARITY name: ...` with the ratio to its bar."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "fqf.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")
DEV = "cuda"

from dqn_restatement import nstep_walk  # noqa: E402
from fqf_restatement import FqfRestatement, fqf_values, propose  # noqa: E402
from test_gpu_distq import _bar, _up_buffer  # noqa: E402
from test_gpu_dqn import _check, _d, _ulp_floor  # noqa: E402
from test_host_dqn import _Discrete, _Env, up_inputs  # noqa: E402
from test_host_fqf import (ENT_COEFS, GRID, PP_CASES, STAT_KEYS, case_flags, head_inputs, pp_inputs, ref_head,  # noqa: E402
                           up_net_dims, up_restatement)

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import FQF, FQFPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch, PrioritizedVectorReplayBuffer
    from tianshou_marl_amd.data.buffer import DeviceAECReplayBuffer, DeviceVectorReplayBuffer
    from tianshou_marl_amd.utils.net import FlatAdam, FractionProposalNet, FullQuantileNet

ULP64 = 64 * np.finfo(np.float32).eps


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def gd():
    return dict(np.load(DQN_GOLD))


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _n(t):
    return t.cpu().numpy()


# ---- the proposal -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PP_CASES)
def test_proposal_forward_and_backward_match_reference(g, case):
    R, H, N, act_f = case
    p = "pp_R%d_H%d_N%d_" % case[:3]
    d = pp_inputs(case)
    r = propose(d["f"], d["Wf"], d["bf"], bool(act_f), d["d_logits"])
    f, Wf, bf, d_logits = (_d(d[k]) for k in ("f", "Wf", "bf", "d_logits"))
    taus, tau_hats, logp, ent = ops.fqf_propose(f, Wf, bf, relu_f=bool(act_f))
    assert taus.shape == (R, N + 1) and tau_hats.shape == (R, N) and logp.shape == (R, N) and ent.shape == (R,)
    assert not taus[:, 0].any() and (taus[:, 1:] > taus[:, :-1]).all()
    _bar(p + "taus", _n(taus), r["taus"], g[p + "taus_eref"])
    _bar(p + "tau_hats", _n(tau_hats), r["tau_hats"], g[p + "tau_hats_eref"])
    _bar(p + "entropies", _n(ent), r["entropies"], g[p + "entropies_eref"])
    r32 = propose(d["f"], d["Wf"], d["bf"], bool(act_f), dtype=torch.float32)       # the reference does not return logp
    _bar(p + "logp", _n(logp), r["logp"], np.abs(r32["logp"] - r["logp"]).max())
    # three slabs over the rows (uneven), inside a wider joint layout whose other slots must stay
    n_split, P, w_off = 3, N * H + N + 24, 16
    slabs = torch.full((n_split, P), 7.0, device=DEV)
    ops.fqf_propose_backward(d_logits, f, n_split, slabs=slabs, slab_stride=P, w_off=w_off, relu_f=bool(act_f))
    total = _n(slabs.double().sum(0))
    _bar(p + "dWf", total[w_off:w_off + N * H].reshape(N, H), r["dWf"], g[p + "dWf_eref"])
    _bar(p + "dbf", total[w_off + N * H:w_off + N * H + N], r["dbf"], g[p + "dbf_eref"])
    assert (slabs[:, :w_off] == 7.0).all() and (slabs[:, w_off + N * H + N:] == 7.0).all()
    # more slabs than rows: the empty ones are written as zeros; the same call twice gives the same bits
    a = ops.fqf_propose_backward(d_logits, f, R + 2, relu_f=bool(act_f))
    b = ops.fqf_propose_backward(d_logits, f, R + 2, relu_f=bool(act_f))
    assert a.shape == (R + 2, N * H + N) and not a[R:].any() and torch.equal(_bits(a), _bits(b))
    _bar(p + "dWf (R + 2 slabs)", _n(a.double().sum(0))[:N * H].reshape(N, H), r["dWf"], g[p + "dWf_eref"])
    again = ops.fqf_propose(f, Wf, bf, relu_f=bool(act_f))
    for x, y in zip((taus, tau_hats, logp, ent), again):
        assert torch.equal(_bits(x), _bits(y))


def test_proposal_survives_saturated_probabilities():
    case = PP_CASES[0]
    R, H, N, _ = case
    d = pp_inputs(case)
    Wf = d["Wf"] * np.float32(400.0)
    r = propose(d["f"], Wf, d["bf"], True)
    gap = r["logits"].max(1) - r["logits"].min(1)
    assert gap.max() > 30.0
    taus, tau_hats, logp, ent = (_n(x) for x in ops.fqf_propose(_d(d["f"]), _d(Wf), _d(d["bf"]), relu_f=True))
    assert np.isfinite(logp).all() and np.isfinite(ent).all() and (ent >= 0).all()
    assert (np.diff(taus, axis=1) >= 0).all() and taus.min() == 0.0 and taus.max() <= 1.0 + 1e-6
    r32 = propose(d["f"], Wf, d["bf"], True, dtype=torch.float32)
    for name, got in (("taus", taus), ("logp", logp), ("entropies", ent)):
        _bar("saturated " + name, got, r[name], np.abs(r32[name] - r[name]).max())


# ---- values and the head ------------------------------------------------------------------------------------------------
def _head(d, q_next, case, act=None):
    tgt, wgt, msk, e = case_flags(case)
    fr = d["fr"]
    return ops.fqf_head(_d(d["out"]), _d(d["out_tau"]), q_next, _d(d["tg"] if tgt else d["on"]), _d(fr["taus"], torch.float32),
                        _d(fr["tau_hats"], torch.float32),
                        _d(fr["logp"], torch.float32), _d(fr["entropies"], torch.float32), _d(d["act"]) if act is None else act,
                        _d(d["mc"], torch.float32), _d(d["gpow"], torch.float32), _d(d["vmask"]),
                        mask_next=_d(d["mask"]) if msk else None, weight=_d(d["weight"]) if wgt else None, ent_coef=ENT_COEFS[e])


@pytest.mark.parametrize("A,N", GRID)
def test_values_and_head_match_reference(g, A, N):
    d = head_inputs(g, A, N)
    B = 37
    eps0, slot = torch.zeros(1, device=DEV), torch.zeros(4, device=DEV)
    q_next = ops.fqf_values(_d(d["on"]), _d(d["fr_next"]["taus"], torch.float32), A)
    pv = f"dv_A{A}_N{N}_"
    _bar(pv + "q", _n(q_next), g[pv + "q"], g[pv + "q_eref"])
    assert np.array_equal(_n(ops.dqn_egreedy(q_next, eps0, 0)), g[pv + "act"])      # row 3: the first of the tie
    assert np.array_equal(_n(ops.dqn_egreedy(q_next, eps0, 0, mask=_d(d["mask"]))), g[pv + "act_masked"])
    p = f"hq_A{A}_N{N}_"
    worst = {}
    for c, case in enumerate(g["cases"]):
        r = ref_head(d, case)
        assert np.array_equal(r["a_star"], g[p + "astar"][c])
        h = _head(d, q_next, case)
        ops.qmix_finalize(h["partial"], B, slot[:2])
        ops.qmix_finalize(h["partial_frac"], B, slot[2:])
        dout = _n(h["d_out"])
        assert dout.shape == (B, N, A) and h["returns"].shape == (B, N) and h["d_logits"].shape == (B, N)
        off = dout.copy()
        off[np.arange(B), :, d["act"]] = 0.0
        assert not off.any(), case   # exactly zero off the taken action
        s64, s32 = g[p + "stats"][c]
        got = _n(slot).astype(np.float64)
        stats = {"quantile_loss": got[0], "fraction_loss": got[2], "entropy_loss": got[3],
                 "loss": got[0] + (got[2] - ENT_COEFS[case_flags(case)[3]] * got[3])}
        rows = [("returns", _n(h["returns"]), r["returns"], g[p + "ret_eref"][c]),
                ("prio", _n(h["prio"]), g[p + "prio"][c], g[p + "prio_eref"][c]),
                ("d_out", dout, r["d_out"], g[p + "dout_eref"][c]),
                ("d_logits", _n(h["d_logits"]), r["d_logits"], g[p + "dlog_eref"][c])]
        rows += [(k, [stats[k]], [s64[i]], abs(s32[i] - s64[i])) for i, k in enumerate(STAT_KEYS)]
        for key, got_, ref, e in rows:
            worst[key] = max(worst.get(key, 0.0), _bar(f"{p}{case} {key}", got_, ref, e))
        assert abs(got[1] - r["q_taken"].mean()) <= 1e-5 * np.abs(r["q_taken"]).max(), case
    print(f"PARITY {p} worst of {len(g['cases'])} cases:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_head_poisons_an_action_outside_the_range_and_repeats_bit_for_bit(g):
    A, N = 5, 8
    d = head_inputs(g, A, N)
    q_next = ops.fqf_values(_d(d["on"]), _d(d["fr_next"]["taus"], torch.float32), A)
    case = "t1w1m1e1"
    good = _head(d, q_next, case)
    act = _d(d["act"]).clone()       # a copy of the inputs: rows 4 and 9 stand in place of valid rows
    act[4], act[9] = A, -1
    h = _head(d, q_next, case, act=act)
    bad = torch.zeros(37, dtype=torch.bool, device=DEV)
    bad[4] = bad[9] = True
    assert torch.isnan(h["prio"][bad]).all() and not torch.isnan(h["prio"][~bad]).any()
    assert not h["d_out"][bad].any() and h["d_out"][~bad].any() and not h["d_logits"][bad].any() and h["d_logits"][~bad].any()
    assert torch.isnan(h["partial"][0]) and torch.isnan(h["partial"][1])          # loss and q of the first workgroup
    assert torch.isnan(h["partial_frac"][0])                                       # its fraction loss; the entropy stays
    assert torch.equal(_bits(h["partial_frac"][1:]), _bits(good["partial_frac"][1:]))
    assert not torch.isnan(h["partial"][2:]).any() and torch.equal(_bits(h["partial"][2:]), _bits(good["partial"][2:]))
    for key in ("d_out", "d_logits"):
        assert torch.equal(_bits(h[key][~bad]), _bits(good[key][~bad])), key
    assert torch.equal(_bits(h["returns"]), _bits(good["returns"]))
    again = _head(d, q_next, case)
    for key in ("returns", "prio", "d_out", "d_logits", "partial", "partial_frac"):
        assert torch.equal(_bits(good[key]), _bits(again[key])), key


# ---- the nets -----------------------------------------------------------------------------------------------------------
def test_net_backwards_fill_their_slabs_and_adam_steps_them():
    """`FullQuantileNet.backward` and `FractionProposalNet.backward` against the restatement's autograd; the interior pass
    leaves what the first pass saved alone; FlatAdam on the slabs."""
    rs = np.random.RandomState(3)
    R, N, A, pre, hid, C = 21, 5, 3, [4, 24, 32], (16,), 12
    net = FullQuantileNet(pre, A, hid, num_cosines=C, device=DEV, seed=5)
    frac = FractionProposalNet(N, 32, device=DEV, seed=6)
    frac.flat.data.mul_(50.0)        # fractions visibly away from uniform
    x = rs.standard_normal((R, 4)).astype(np.float32)
    d_out, d_logits = rs.standard_normal((R * N, A)).astype(np.float32), rs.standard_normal((R, N)).astype(np.float32)
    out, fr, out_tau = net.forward(_d(x), frac, training=True)
    assert out.shape == (R * N, A) and out_tau.shape == (R * (N - 1), A) and fr.taus.shape == (R, N + 1)
    saved = [t.clone() for t in net._saved]
    plain, fr2, none = net.forward(_d(x), frac, fractions=fr, save=False)
    assert none is None and fr2 is fr and torch.equal(_bits(plain), _bits(out))
    assert all(torch.equal(a, b) for a, b in zip(saved, net._saved))
    slabs, fslabs = net.backward(_d(d_out), 2), frac.backward(_d(d_logits), 2)
    Rs = FqfRestatement(_n(net.flat.data), _n(frac.flat.data), pre, [32, *hid, A], C, N, feature_act=True)
    f = Rs.features(Rs.params, x)
    xf = Rs.frac_logits(f)
    ref_fr = propose(_n(f.detach()), _n(frac.Wf), _n(frac.bf), True)
    ref = Rs.quantiles(Rs.params, f, torch.as_tensor(ref_fr["tau_hats"]))
    ref_tau = Rs.quantiles(Rs.params, f, torch.as_tensor(ref_fr["taus"][:, 1:-1])).detach().numpy()
    ref.backward(torch.as_tensor(d_out).double().view(R, N, A))
    xf.backward(torch.as_tensor(d_logits).double())
    # no reference float32 run stands behind these: 64 ulp of the array's scale stand in for what float32 costs
    for name, got, want in (("taus", _n(fr.taus), ref_fr["taus"]), ("out", _n(out), ref.detach().numpy().reshape(R * N, A)),
                            ("out_tau", _n(out_tau), ref_tau.reshape(R * (N - 1), A)),
                            ("grads", _n(slabs.double().sum(0)), Rs.flat_of([q.grad for q in Rs.params])),
                            ("frac grads", _n(fslabs.double().sum(0)), Rs.flat_of([q.grad for q in Rs.frac]))):
        _bar("nets " + name, got, want, ULP64 * np.abs(want).max())
    for m, s in ((net, slabs), (frac, fslabs)):
        before = m.flat.data.clone()
        FlatAdam(m, lr=1e-3).step(s)
        step = (m.flat.data - before).abs()
        big = s.double().sum(0).abs() > 1e-6
        assert float(step.max()) <= 1.001e-3 and big.any() and float(step[big].min()) > 0.9e-3


# ---- the learner --------------------------------------------------------------------------------------------------------
def _algo(init, frac_init, pre, A, hidden, C, N, seed=0, ent_coef=0.01, **kw):
    net = FullQuantileNet(list(pre), A, tuple(hidden), num_cosines=C, device=DEV, seed=seed)
    frac = FractionProposalNet(N, pre[-1], device=DEV, seed=seed + 1)
    if init is not None:
        net.flat.data.copy_(_d(np.asarray(init, np.float32)))
        frac.flat.data.copy_(_d(np.asarray(frac_init, np.float32)))
    pol = FQFPolicy(model=net, fraction_model=frac, action_space=_Discrete(A), seed=seed)
    return FQF(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), fraction_optim=AdamOptimizerFactory(lr=1e-3), ent_coef=ent_coef, **kw)


def _up_algo(g, gd, **over):
    _, B, n_env, S, n_step, freq, *_ = up_inputs(gd)
    u = up_net_dims(g)
    kw = dict(gamma=float(g["gamma"]), n_step_return_horizon=n_step, target_update_freq=freq, ent_coef=float(g["up_ent_coef"]))
    kw.update(over)
    return _algo(g["up_init"], g["up_frac_init"], u["pre"], u["A"], u["hidden"], u["C"], u["N"], **kw)


def _stats_check(name, stats, ref):
    s64, s32 = ref
    d = stats.get_loss_stats_dict()
    for i, k in enumerate(STAT_KEYS):
        _check(f"{name}{k}", [d[k]], [s64[i]], abs(s32[i] - s64[i]))


def test_three_updates_match_reference(g, gd):
    """Three updates against the fixture; the four statistics, returns, both gradients and both weight vectors under `_check`.
    `fraction_loss` (0.010, a cancelling sum of second differences of quantile values of size 0.3) is the tightest of them."""
    _, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    algo = _up_algo(g, gd)
    model, frac = algo.policy.model, algo.policy.fraction_model
    N = up_net_dims(g)["N"]
    R = up_restatement(g, freq)
    lr = 1e-3
    cond, tol = {"": np.zeros(model.flat.numel()), "frac_": np.zeros(frac.flat.numel())}, {}
    for k in range(steps):
        pk = f"up_s{k}_"
        idx = g[pk + "indices"]
        batch = algo._preprocess_batch(Batch(), buf, idx)
        w_before = model.flat.data.clone()
        stats = algo._update_with_batch(batch)
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        assert np.array_equal(_n(batch.idx_n), idx_n)
        r = R.update(obs[idx], act[idx], obs_next[idx_n], None, mc, gpow, vmask)
        cond[""] += R.adam_cond()
        cond["frac_"] += R.frac_adam_cond()
        _stats_check(pk, stats, g[pk + "stats"])
        _check(f"{pk}returns", _n(batch.returns).reshape(-1), r["returns"].reshape(-1), float(g[pk + "returns_eref"]))
        didx = g[pk + "returns_didx"]
        _check(f"{pk}returns (reference entries)", _n(batch.returns).reshape(-1)[didx], g[pk + "returns_dval"],
               float(g[pk + "returns_eref"]))
        assert batch.returns.shape == (B, N) and batch.weight.shape == (B,) and batch.weight.is_cuda
        for pre, m, slabs, ref_g, ref_w in (("", model, "slabs", r["grads"], R.weights()),
                                            ("frac_", frac, "frac_slabs", r["frac_grads"], R.frac_weights())):
            grad = _n(algo._ws[B][slabs].double().sum(0))
            e = float(g[pk + pre + "grad_eref"])
            _check(f"{pk}{pre}grad", grad, ref_g, e)
            tol.setdefault(pre, 4.0 * max(e, _ulp_floor(ref_g)))
            extra = np.minimum(cond[pre] * tol[pre], 2 * lr * (k + 1))
            w_hip = _n(m.flat.double())
            _check(f"{pk}{pre}weights", w_hip, ref_w, float(g[pk + pre + "weights_eref"]), extra)
            didx = g[pk + pre + "weights_didx"]
            _check(f"{pk}{pre}weights (reference entries)", w_hip[didx], g[pk + pre + "weights_dval"],
                   float(g[pk + pre + "weights_eref"]), extra[didx])
            if pre == "":
                if k % freq == 0:   # the lagged copy: the weights BEFORE the step of calls 0, 2, ...
                    assert torch.equal(algo.target_flat, w_before), k
                tidx = g[pk + "targets_didx"]
                _check(f"{pk}targets (reference entries)", _n(algo.target_flat.double())[tidx], g[pk + "targets_dval"],
                       float(g[pk + "weights_eref"]), extra[tidx])
    assert algo._iter == steps and algo.fraction_optim.step_count == steps and algo.optim.step_count == steps


def test_update_through_a_prioritized_buffer_matches_reference(g, gd):
    _, B, n_env, S, *_ = up_inputs(gd)
    buf = _up_buffer(gd, PrioritizedVectorReplayBuffer, alpha=float(g["pr_alpha"]), beta=float(g["pr_beta"]))
    algo = _up_algo(g, gd)
    for k in range(2):
        pk = f"pr_s{k}_"
        idx = _d(g[pk + "indices"])
        batch = algo._sampled_batch(buf, idx)
        w_in = batch.weight.clone()
        batch = algo._preprocess_batch(batch, buf, idx)
        stats = algo._update_with_batch(batch)
        assert batch.weight.is_cuda and batch.weight.shape == (B,) and (batch.weight >= 0).all()
        algo._postprocess_batch(batch, buf, idx)
        _check(f"{pk}IS weights", _n(w_in), g[pk + "weight"], float(g[pk + "weight_eref"]))
        _stats_check(pk, stats, g[pk + "stats"])
        _check(f"{pk}leaves", _n(buf.weight[np.arange(n_env * S)]), g[pk + "leaves"], float(g[pk + "leaves_eref"]))
        _check(f"{pk}max/min prio", _n(buf.prio), g[pk + "prio"], float(g[pk + "prio_eref"]))
    buf.weight.check()
    algo.is_within_training_step = True
    assert np.isfinite(algo.update(buf, 16).get_loss_stats_dict()["loss"])    # sampled on the device, end to end


def test_multiagent_update_aec_matches_reference(g, gd):
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    d = [int(x) for x in g["ma_dims"]]
    pre, C, NF = d[:2], d[3], d[4]
    assert d[2] == A and pre[0] == D
    env = _Env(N_AG)
    buf = DeviceAECReplayBuffer(n_env * S, n_env, env.agents, obs_dim=D, n_act=A, device=DEV)
    for t in range(T):
        ids = np.array([env.agents[a] for a in gd["ma_turn"][t]], dtype=object)
        nxt = np.array([env.agents[(a + 1) % N_AG] for a in gd["ma_turn"][t]], dtype=object)
        buf.add(Batch(obs=Batch(agent_id=ids, obs=gd["ma_obs"][t], mask=gd["ma_mask"][t]), act=gd["ma_act"][t], rew=gd["ma_rew"][t],
                      terminated=gd["ma_term"][t], truncated=gd["ma_trunc"][t],
                      obs_next=Batch(agent_id=nxt, obs=gd["ma_obs_next"][t])), buffer_ids=np.arange(n_env))
    kw = dict(gamma=float(g["gamma"]), n_step_return_horizon=n_step, target_update_freq=3, ent_coef=float(g["ma_ent_coef"]))
    mk = lambda: [_algo(g["ma_init"][i], g["ma_frac_init"][i], pre, A, (), C, NF, seed=20 + i, **kw) for i in range(N_AG)]  # noqa: E731
    ours, alone = mk(), mk()
    idx = buf.sample_indices(0)
    who = buf[idx].obs.agent_id
    rows = [idx[np.nonzero(who == agent)[0]] for agent in env.agents]
    ma = MultiAgentOffPolicyAlgorithm(algorithms=ours, env=env)
    ma.is_within_training_step = True
    stats = ma.update(buf, 0).get_loss_stats_dict()
    for k, agent in enumerate(env.agents):
        s = alone[k]._update_with_batch(alone[k]._preprocess_batch(Batch(), buf, rows[k], agent=k))
        for key in STAT_KEYS:
            assert stats[f"{agent}/{key}"] == s.get_loss_stats_dict()[key], (agent, key)
        _stats_check(f"ma {agent} ", s, g["ma_stats"][:, k])
        assert torch.equal(ours[k].policy.model.flat.data, alone[k].policy.model.flat.data)
        assert torch.equal(ours[k].policy.fraction_model.flat.data, alone[k].policy.fraction_model.flat.data)


def test_updates_are_deterministic_need_no_target_network_and_refuse_eval_mode(g, gd):
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    idx = g["up_s0_indices"]
    runs = []
    for _ in range(2):
        algo = _up_algo(g, gd)
        for _ in range(2):
            algo._update_with_batch(algo._preprocess_batch(Batch(), buf, idx))
        runs.append([t.clone() for t in (algo.policy.model.flat.data, algo.policy.fraction_model.flat.data, algo.target_flat)])
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(runs[0][0], _d(g["up_init"])) and not torch.equal(runs[0][1], _d(g["up_frac_init"]))
    # without a lagged net the online forward that chose a* is the next distribution
    solo = _up_algo(g, gd, target_update_freq=0)
    assert solo.model_old is None
    batch = solo._preprocess_batch(Batch(), buf, idx)
    pol = solo.policy
    out_on, fr, none = pol.net_forward(batch.rows_next)
    assert none is None and torch.equal(_bits(batch.out_next.reshape(-1)), _bits(out_on.reshape(-1)))
    assert torch.equal(_bits(batch.q_next_online), _bits(ops.fqf_values(out_on, fr.taus, pol.n_act)))
    assert np.isfinite(solo._update_with_batch(batch).get_loss_stats_dict()["loss"]) and batch.returns.shape == (len(idx), 8)
    # quantiles_tau exists only in torch training mode
    algo = _up_algo(g, gd)
    batch = algo._preprocess_batch(Batch(), buf, idx)
    algo.eval()
    algo.policy.model.flat.data.add_(0.125)          # a lagged copy would show
    before, lagged, it = algo.policy.model.flat.data.clone(), algo.target_flat.clone(), algo._iter
    batch.weight = 2.0
    with pytest.raises(RuntimeError, match="training mode"):
        algo._update_with_batch(batch)
    assert torch.equal(before, algo.policy.model.flat.data) and torch.equal(lagged, algo.target_flat)   # nothing was touched
    assert algo._iter == it and batch.weight == 2.0 and algo.optim.step_count == 0 and algo.fraction_optim.step_count == 0
    algo.train()
    assert np.isfinite(algo._update_with_batch(algo._preprocess_batch(Batch(), buf, idx)).get_loss_stats_dict()["loss"])


# ---- acting -------------------------------------------------------------------------------------------------------------
def test_policy_forward_and_act_device_follow_the_mode_and_the_mask():
    rs = np.random.RandomState(4)
    R, A, N = 130, 5, 6
    mask = np.zeros((R, A), bool)
    for r in range(R):
        mask[r, rs.choice(A, 1 + r % 4, replace=False)] = True
    net = FullQuantileNet([4, 32], A, (16,), num_cosines=8, device=DEV, seed=3)
    frac = FractionProposalNet(N, 32, device=DEV, seed=4)
    frac.flat.data.mul_(50.0)
    pol = FQFPolicy(model=net, fraction_model=frac, action_space=_Discrete(A), eps_training=1.0, eps_inference=0.0, seed=11)
    obs = rs.standard_normal((R, 4)).astype(np.float32)
    for mode in (pol.train, pol.eval):
        mode()
        out = pol(Batch(obs=Batch(obs=obs, mask=mask), info=Batch()))
        assert out.logits.shape == (R, A, N) and out.fractions.taus.shape == (R, N + 1) and out.act.dtype == np.int64
        assert out.fractions.tau_hats.shape == (R, N) and out.fractions.entropies.shape == (R,)
        if pol.training:
            assert out.quantiles_tau.shape == (R, A, N - 1)
        else:
            assert out.quantiles_tau is None
        q = fqf_values(_n(out.logits.transpose(1, 2)), _n(out.fractions.taus))["q"]
        top = np.sort(np.where(mask, q, -np.inf), 1)
        clear = ~(top[:, -1] - top[:, -2] < 1e-6)          # rows whose float32 sum could order two actions otherwise
        assert clear.sum() > R // 2 and np.array_equal(out.act[clear], np.where(mask, q, -np.inf).argmax(1)[clear])
        assert np.array_equal(out.act, _n(pol.compute_q_value(out.logits, mask, out.fractions).argmax(1)))
        # given fractions are used as they are (the lagged net's call)
        again = pol(Batch(obs=obs, info=Batch()), model=net, fractions=out.fractions)
        assert torch.equal(again.logits, out.logits) and again.quantiles_tau is None and again.fractions is out.fractions
        res = pol.act_device(_d(obs), mask=_d(mask))                                      # epsilon 0: greedy
        o, fr, none = net.forward(_d(obs), frac, save=False)
        q_dev = ops.fqf_values(o, fr.taus, A)
        assert none is None and torch.equal(_bits(q_dev), _bits(res["q"]))
        assert np.array_equal(_n(res["act"]), _n(ops.dqn_egreedy(q_dev, pol._zero_dev, 0, mask=_d(mask))))
        masked = torch.where(_d(mask), q_dev, torch.full_like(q_dev, -np.inf))
        assert np.array_equal(_n(res["act"]), _n(masked.argmax(1)))                       # the first argmax of the masked value
    pol.is_within_training_step = True                                                     # epsilon 1: legal random actions
    a1 = _n(pol.act_device(_d(obs), mask=_d(mask))["act"])
    assert mask[np.arange(R), a1].all() and not np.array_equal(a1, _n(res["act"]))
