"""GPU tests (`-m gpu`) of IQN: tsm_iqn_taus, tsm_iqn_embed_forward / _backward, tsm_iqn_values and tsm_iqn_head
(csrc/iqn.hip), `ImplicitQuantileNet`, updates of the learner on a device buffer, in front of a prioritized buffer and as a
member of MultiAgentOffPolicyAlgorithm, and the acting path.

References: tests/golden/iqn.npz (the reference's own float64 and float32 runs, under recorded fractions) and the float64
restatement (tests/iqn_restatement.py, pinned to those runs to 1e-10 by tests/test_host_iqn.py; it supplies the full arrays of
which the fixture keeps digests).  Bars, those of test_gpu_distq.py:
  * a*, actions, zeros of the gradient off the taken action: exact;
  * everything else the kernels produce: max |hip - ref64| <= 1e-5 max |ref64| + e_ref per array, e_ref = max |ref32 - ref64|
    of the reference's own two runs;
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
GOLD = os.path.join(HERE, "golden", "iqn.npz")
DQN_GOLD = os.path.join(HERE, "golden", "dqn.npz")
DEV = "cuda"

from dqn_restatement import nstep_walk  # noqa: E402
from iqn_restatement import embed, iqn_head, iqn_values  # noqa: E402
from test_gpu_distq import _bar, _up_buffer  # noqa: E402
from test_gpu_dqn import _check, _d, _ulp_floor  # noqa: E402
from test_host_dqn import _Discrete, _Env, up_inputs  # noqa: E402
from test_host_iqn import EM_CASES, GRID, em_inputs, head_inputs, up_net_dims, up_restatement  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import IQN, IQNPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch, PrioritizedVectorReplayBuffer
    from tianshou_marl_amd.data.buffer import DeviceAECReplayBuffer, DeviceVectorReplayBuffer
    from tianshou_marl_amd.utils.net import ImplicitQuantileNet


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def gd():
    return dict(np.load(DQN_GOLD))


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---- the embedding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EM_CASES)
def test_embedding_forward_and_backward_match_reference(g, case):
    B, S, C, H, act_f = case
    p = "em_B%d_S%d_C%d_H%d_" % case[:4]
    d = em_inputs(case)
    taus = g[p + "taus"]
    r = embed(d["f"], taus, d["We"], d["be"], bool(act_f), d["d_e"])
    f, t, We, be, d_e = (_d(x) for x in (d["f"], taus, d["We"], d["be"], d["d_e"]))
    e, phi = ops.iqn_embed_forward(f, t, We, be, relu_f=bool(act_f))
    assert e.shape == (B * S, H) and phi.shape == (B * S, H)
    _bar(p + "e", e.cpu().numpy(), r["e"], g[p + "e_eref"])
    assert np.array_equal(phi.cpu().numpy() > 0, r["pre"] > 0)       # the ReLU's mask: nothing sits within DELTA of zero
    # three slabs over the batch rows (uneven: 37 = 13 + 13 + 11), inside a wider joint layout whose other slots must stay
    n_split, P, w_off = 3, H * C + H + 24, 16
    slabs = torch.full((n_split, P), 7.0, device=DEV)
    d_f, _ = ops.iqn_embed_backward(d_e, f, phi, t, We, be, n_split, slabs=slabs, slab_stride=P, w_off=w_off, relu_f=bool(act_f))
    _bar(p + "d_f", d_f.cpu().numpy(), r["d_f"], g[p + "d_f_eref"])
    total = slabs.double().sum(0).cpu().numpy()
    _bar(p + "dWe", total[w_off:w_off + H * C].reshape(H, C), r["dWe"], g[p + "dWe_eref"])
    _bar(p + "dbe", total[w_off + H * C:w_off + H * C + H], r["dbe"], g[p + "dbe_eref"])
    assert (slabs[:, :w_off] == 7.0).all() and (slabs[:, w_off + H * C + H:] == 7.0).all()
    # more slabs than batch rows: the empty ones are written as zeros; the same call twice gives the same bits
    a = ops.iqn_embed_backward(d_e, f, phi, t, We, be, B + 2, relu_f=bool(act_f))
    b = ops.iqn_embed_backward(d_e, f, phi, t, We, be, B + 2, relu_f=bool(act_f))
    assert not a[1][B:].any() and torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    _bar(p + "dWe (B + 2 slabs)", a[1].double().sum(0).cpu().numpy()[:H * C].reshape(H, C), r["dWe"], g[p + "dWe_eref"])


def test_net_backward_fills_the_joint_slabs():
    """`ImplicitQuantileNet.backward` against the restatement's autograd through the whole composite net, and FlatAdam on the
    slabs it leaves."""
    from iqn_restatement import IqnRestatement
    from tianshou_marl_amd.utils.net import FlatAdam

    rs = np.random.RandomState(3)
    R, S, A = 21, 5, 3
    net = ImplicitQuantileNet([4, 24, 32], A, (16,), num_cosines=12, device=DEV, seed=5)
    x, taus = rs.standard_normal((R, 4)).astype(np.float32), rs.rand(R, S).astype(np.float32)
    d_out = rs.standard_normal((R * S, A)).astype(np.float32)
    out, t = net.forward(_d(x), S, taus=_d(taus))
    assert out.shape == (R * S, A) and torch.equal(t, _d(taus))
    slabs = net.backward(_d(d_out), 2)
    Rs = IqnRestatement(net.flat.data.cpu().numpy(), [4, 24, 32], [32, 16, A], 12, feature_act=True)
    ref = Rs.net(Rs.params, x, taus)
    ref.backward(torch.as_tensor(d_out).double().view(R, S, A))
    # no reference float32 run stands behind this one: 64 ulp of the array's scale stand in for what float32 costs
    ref_out = ref.detach().numpy().reshape(R * S, A)
    _bar("net out", out.cpu().numpy(), ref_out, 64 * np.finfo(np.float32).eps * np.abs(ref_out).max())
    grads = Rs.flat_of([q.grad for q in Rs.params])
    _bar("net grads", slabs.double().sum(0).cpu().numpy(), grads, 64 * np.finfo(np.float32).eps * np.abs(grads).max())
    before = net.flat.data.clone()
    FlatAdam(net, lr=1e-3).step(slabs)
    step = (net.flat.data - before).abs()
    assert float(step.max()) <= 1.001e-3 and float(step[_d(np.abs(grads) > 1e-6)].min()) > 0.9e-3


# ---- values and the head ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N,Np", GRID)
def test_values_and_head_match_reference(g, A, N, Np):
    d = head_inputs(g, A, N, Np)
    B = 37
    eps0, slot = torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
    q_next = ops.iqn_values(_d(d["on"]), N, A)
    pv = f"dv_A{A}_N{N}_M{Np}_"
    _bar(pv + "q", q_next.cpu().numpy(), g[pv + "q"], g[pv + "q_eref"])
    assert np.array_equal(ops.dqn_egreedy(q_next, eps0, 0).cpu().numpy(), g[pv + "act"])      # row 3: the first of the tie
    assert np.array_equal(ops.dqn_egreedy(q_next, eps0, 0, mask=_d(d["mask"])).cpu().numpy(), g[pv + "act_masked"])
    p = f"hq_A{A}_N{N}_M{Np}_"
    worst = {}
    for c, case in enumerate(g["cases"]):
        tgt, wgt, msk = (case[i] == "1" for i in (1, 3, 5))
        r = iqn_head(d["out"], d["on"], d["tg"] if tgt else None, d["mask"] if msk else None, d["taus"], d["act"], d["mc"],
                     d["gpow"], d["vmask"], d["weight"] if wgt else None)
        assert np.array_equal(r["a_star"], g[p + "astar"][c])
        h = ops.iqn_head(_d(d["out"]), q_next, _d(d["tg"] if tgt else d["on"]), _d(d["taus"]), _d(d["act"]),
                         _d(d["mc"], torch.float32), _d(d["gpow"], torch.float32), _d(d["vmask"]),
                         mask_next=_d(d["mask"]) if msk else None, weight=_d(d["weight"]) if wgt else None)
        ops.qmix_finalize(h["partial"], B, slot)
        dout = h["d_out"].cpu().numpy()
        assert dout.shape == (B, N, A) and h["returns"].shape == (B, Np if tgt else N)
        off = dout.copy()
        off[np.arange(B), :, d["act"]] = 0.0
        assert not off.any(), case   # exactly zero off the taken action
        for key, got, ref, e in (("returns", h["returns"].cpu().numpy(), r["returns"], g[p + "ret_eref"][c]),
                                 ("prio", h["prio"].cpu().numpy(), g[p + "prio"][c], g[p + "prio_eref"][c]),
                                 ("d_out", dout, r["d_out"], g[p + "dout_eref"][c]),
                                 ("loss", [float(slot[0])], [g[p + "loss"][c, 0]], abs(g[p + "loss"][c, 1] - g[p + "loss"][c, 0]))):
            worst[key] = max(worst.get(key, 0.0), _bar(f"{p}{case} {key}", got, ref, e))
        assert abs(float(slot[1]) - r["q_taken"].mean()) <= 1e-5 * np.abs(r["q_taken"]).max(), case
    print(f"PARITY {p} worst of {len(g['cases'])} cases:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_head_poisons_an_action_outside_the_range_and_repeats_bit_for_bit(g):
    A, N, Np = 5, 8, 32
    d = head_inputs(g, A, N, Np)
    q_next = ops.iqn_values(_d(d["on"]), N, A)

    def head(act):
        return ops.iqn_head(_d(d["out"]), q_next, _d(d["tg"]), _d(d["taus"]), act, _d(d["mc"], torch.float32),
                            _d(d["gpow"], torch.float32), _d(d["vmask"]), mask_next=_d(d["mask"]), weight=_d(d["weight"]))

    good = head(_d(d["act"]))
    act = _d(d["act"]).clone()       # a copy of the inputs: rows 4 and 9 stand in place of valid rows
    act[4], act[9] = A, -1
    h = head(act)
    bad = torch.zeros(37, dtype=torch.bool, device=DEV)
    bad[4] = bad[9] = True
    assert torch.isnan(h["prio"][bad]).all() and not torch.isnan(h["prio"][~bad]).any()
    assert not h["d_out"][bad].any() and h["d_out"][~bad].any()
    assert torch.isnan(h["partial"][0]) and torch.isnan(h["partial"][1])          # loss and q of the first workgroup
    assert not torch.isnan(h["partial"][2:]).any() and torch.equal(_bits(h["partial"][2:]), _bits(good["partial"][2:]))
    assert torch.equal(_bits(h["d_out"][~bad]), _bits(good["d_out"][~bad])) and torch.equal(_bits(h["returns"]), _bits(good["returns"]))
    again = head(_d(d["act"]))
    for key in ("returns", "prio", "d_out", "partial"):
        assert torch.equal(_bits(good[key]), _bits(again[key])), key


# ---- the device draw ----------------------------------------------------------------------------------------------------
def test_device_draw_is_uniform_keyed_and_counted():
    a = ops.iqn_taus(512, 8, 11, DEV, offset=100)
    assert a.shape == (512, 8) and a.dtype == torch.float32 and float(a.min()) >= 0.0 and float(a.max()) < 1.0
    assert abs(float(a.double().mean()) - 0.5) <= 0.05          # 4096 draws: about 11 standard errors
    assert torch.equal(_bits(a), _bits(ops.iqn_taus(512, 8, 11, DEV, offset=100)))
    assert not torch.equal(a, ops.iqn_taus(512, 8, 11, DEV, offset=101)) and not torch.equal(a, ops.iqn_taus(512, 8, 12, DEV, offset=100))
    # the counter is per row, host offset plus device counter: row r of one call is row 0 of the call at counter + r
    ctr = torch.tensor([60], dtype=torch.int64, device=DEV)
    assert torch.equal(_bits(ops.iqn_taus(512, 8, 11, DEV, offset=40, offset_dev=ctr)), _bits(a))
    assert torch.equal(_bits(ops.iqn_taus(4, 8, 11, DEV, offset=103)), _bits(a[3:7]))
    odd = ops.iqn_taus(9, 5, 11, DEV, offset=100)                # a count that is no multiple of four
    assert torch.equal(_bits(odd), _bits(a[:9, :5])) and len(torch.unique(a)) > 4000
    # a stream of its own: the epsilon draws of the same seed and counter are other numbers
    q = torch.zeros(512, 8, device=DEV)
    one = torch.ones(1, device=DEV)
    assert ops.dqn_egreedy(q, one, 11, offset=100).shape == (512,)


# ---- the learner --------------------------------------------------------------------------------------------------------
def _algo(init, pre, A, hidden, C, S, seed=0, **kw):
    net = ImplicitQuantileNet(list(pre), A, tuple(hidden), num_cosines=C, device=DEV, seed=seed)
    if init is not None:
        net.flat.data.copy_(_d(np.asarray(init, np.float32)))
    pol = IQNPolicy(model=net, action_space=_Discrete(A), sample_size=S, online_sample_size=S, target_sample_size=S, seed=seed)
    return IQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), **kw)


def _up_algo(g, gd, seed=0):
    _, B, n_env, S, n_step, freq, *_ = up_inputs(gd)
    u = up_net_dims(g)
    return _algo(g["up_init"], u["pre"], u["A"], u["hidden"], u["C"], u["S"], seed=seed, gamma=float(g["gamma"]),
                 n_step_return_horizon=n_step, target_update_freq=freq)


def test_three_updates_match_reference(g, gd):
    _, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(gd)
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    algo = _up_algo(g, gd)
    N = up_net_dims(g)["S"]
    R = up_restatement(g, freq)
    lr, cond, grad_tol = 1e-3, np.zeros(algo.policy.model.flat.numel()), None
    for k in range(steps):
        pk = f"up_s{k}_"
        idx = g[pk + "indices"]
        algo.policy.tau_feed = list(g[pk + "taus"])
        batch = algo._preprocess_batch(Batch(), buf, idx)
        assert len(algo.policy.tau_feed) == 1           # two forwards on the successor rows came first
        w_before = algo.policy.model.flat.data.clone()
        stats = algo._update_with_batch(batch)
        assert not algo.policy.tau_feed and np.array_equal(batch.taus.cpu().numpy(), g[pk + "taus"][2])
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        assert np.array_equal(batch.idx_n.cpu().numpy(), idx_n)
        r = R.update(obs[idx], act[idx], obs_next[idx_n], None, mc, gpow, vmask, g[pk + "taus"])
        cond += R.adam_cond()
        ref64, ref32 = (float(x) for x in g[pk + "loss"])
        _check(f"{pk}loss", [stats.get_loss_stats_dict()["loss"]], [ref64], abs(ref32 - ref64))
        _check(f"{pk}returns", batch.returns.cpu().numpy().reshape(-1), r["returns"].reshape(-1), float(g[pk + "returns_eref"]))
        didx = g[pk + "returns_didx"]
        _check(f"{pk}returns (reference entries)", batch.returns.cpu().numpy().reshape(-1)[didx], g[pk + "returns_dval"],
               float(g[pk + "returns_eref"]))
        assert batch.returns.shape == (B, N) and batch.weight.shape == (B,) and batch.weight.is_cuda
        grad = algo._ws[B]["slabs"].double().sum(0).cpu().numpy()
        e = float(g[pk + "grad_eref"])
        _check(f"{pk}grad", grad, r["grads"], e)
        if grad_tol is None:
            grad_tol = 4.0 * max(e, _ulp_floor(r["grads"]))
        extra = np.minimum(cond * grad_tol, 2 * lr * (k + 1))
        w_hip = algo.policy.model.flat.double().cpu().numpy()
        _check(f"{pk}weights", w_hip, R.weights(), float(g[pk + "weights_eref"]), extra)
        didx = g[pk + "weights_didx"]
        _check(f"{pk}weights (reference entries)", w_hip[didx], g[pk + "weights_dval"], float(g[pk + "weights_eref"]), extra[didx])
        if k % freq == 0:   # the lagged copy: the weights BEFORE the step of calls 0, 2, ...
            assert torch.equal(algo.target_flat, w_before), k
        tidx = g[pk + "targets_didx"]
        _check(f"{pk}targets (reference entries)", algo.target_flat.double().cpu().numpy()[tidx], g[pk + "targets_dval"],
               float(g[pk + "weights_eref"]), extra[tidx])
    assert algo._iter == steps


def test_update_through_a_prioritized_buffer_matches_reference(g, gd):
    _, B, n_env, S, *_ = up_inputs(gd)
    buf = _up_buffer(gd, PrioritizedVectorReplayBuffer, alpha=float(g["pr_alpha"]), beta=float(g["pr_beta"]))
    algo = _up_algo(g, gd)
    for k in range(2):
        pk = f"pr_s{k}_"
        idx = _d(g[pk + "indices"])
        batch = algo._sampled_batch(buf, idx)
        w_in = batch.weight.clone()
        assert w_in.dtype == torch.float32 and w_in.is_cuda
        algo.policy.tau_feed = list(g[pk + "taus"])
        batch = algo._preprocess_batch(batch, buf, idx)
        stats = algo._update_with_batch(batch)
        assert batch.weight.is_cuda and batch.weight.shape == (B,) and (batch.weight >= 0).all()
        algo._postprocess_batch(batch, buf, idx)
        ref64, ref32 = (float(x) for x in g[pk + "loss"])
        _check(f"{pk}IS weights", w_in.cpu().numpy(), g[pk + "weight"], float(g[pk + "weight_eref"]))
        _check(f"{pk}loss", [stats.get_loss_stats_dict()["loss"]], [ref64], abs(ref32 - ref64))
        _check(f"{pk}leaves", buf.weight[np.arange(n_env * S)].cpu().numpy(), g[pk + "leaves"], float(g[pk + "leaves_eref"]))
        _check(f"{pk}max/min prio", buf.prio.cpu().numpy(), g[pk + "prio"], float(g[pk + "prio_eref"]))
    buf.weight.check()
    algo.is_within_training_step = True
    assert np.isfinite(algo.update(buf, 16).get_loss_stats_dict()["loss"])    # sampled and drawn on the device, end to end


def test_multiagent_update_aec_matches_reference(g, gd):
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    d = [int(x) for x in g["ma_dims"]]
    pre, C, NS = d[:2], d[3], d[4]
    assert d[2] == A and pre[0] == D
    env = _Env(N_AG)
    buf = DeviceAECReplayBuffer(n_env * S, n_env, env.agents, obs_dim=D, n_act=A, device=DEV)
    for t in range(T):
        ids = np.array([env.agents[a] for a in gd["ma_turn"][t]], dtype=object)
        nxt = np.array([env.agents[(a + 1) % N_AG] for a in gd["ma_turn"][t]], dtype=object)
        buf.add(Batch(obs=Batch(agent_id=ids, obs=gd["ma_obs"][t], mask=gd["ma_mask"][t]), act=gd["ma_act"][t], rew=gd["ma_rew"][t],
                      terminated=gd["ma_term"][t], truncated=gd["ma_trunc"][t],
                      obs_next=Batch(agent_id=nxt, obs=gd["ma_obs_next"][t])), buffer_ids=np.arange(n_env))
    kw = dict(gamma=float(g["gamma"]), n_step_return_horizon=n_step, target_update_freq=3)
    mk = lambda: [_algo(g["ma_init"][i], pre, A, (), C, NS, seed=20 + i, **kw) for i in range(N_AG)]  # noqa: E731
    ours, alone = mk(), mk()
    idx = buf.sample_indices(0)
    who = buf[idx].obs.agent_id
    rows = [idx[np.nonzero(who == agent)[0]] for agent in env.agents]
    for group in (ours, alone):     # every forward over R rows takes the first R rows of the stored fractions
        for k, a in enumerate(group):
            a.policy.tau_feed = [g["ma_taus"][:len(rows[k])]] * 3
    ma = MultiAgentOffPolicyAlgorithm(algorithms=ours, env=env)
    ma.is_within_training_step = True
    stats = ma.update(buf, 0).get_loss_stats_dict()
    for k, agent in enumerate(env.agents):
        s = alone[k]._update_with_batch(alone[k]._preprocess_batch(Batch(), buf, rows[k], agent=k)).get_loss_stats_dict()["loss"]
        assert stats[f"{agent}/loss"] == s and not ours[k].policy.tau_feed
        ref64, ref32 = float(g["ma_loss"][0, k]), float(g["ma_loss"][1, k])
        _check(f"ma {agent} loss", [s], [ref64], abs(ref32 - ref64))
        assert torch.equal(ours[k].policy.model.flat.data, alone[k].policy.model.flat.data)


def test_update_with_device_draws_is_deterministic_and_draws_afresh(g, gd):
    buf = _up_buffer(gd, DeviceVectorReplayBuffer)
    idx = g["up_s0_indices"]
    runs = []
    for _ in range(2):
        algo = _up_algo(g, gd, seed=5)
        seen = []
        for _ in range(2):
            batch = algo._preprocess_batch(Batch(), buf, idx)
            algo._update_with_batch(batch)
            seen.append(batch.taus.clone())
        assert algo.policy._tau_ctr == 2 * 3 * len(idx) and not torch.equal(seen[0], seen[1])   # three draws per update
        assert float(seen[0].min()) >= 0.0 and float(seen[0].max()) < 1.0
        runs.append((algo.policy.model.flat.data.clone(), algo.target_flat.clone(), seen))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    assert torch.equal(runs[0][2][1], runs[1][2][1])
    other = _up_algo(g, gd, seed=6)
    other._update_with_batch(other._preprocess_batch(Batch(), buf, idx))
    assert not torch.equal(other.policy.model.flat.data, runs[0][0])
    # without a lagged net the next distribution is the online forward that chose a*: two draws, N' = that forward's count
    u = up_net_dims(g)
    solo = _algo(g["up_init"], u["pre"], u["A"], u["hidden"], u["C"], 6, n_step_return_horizon=3)
    solo.policy.target_sample_size = 13
    batch = solo._preprocess_batch(Batch(), buf, idx)
    solo._update_with_batch(batch)
    assert solo.policy._tau_ctr == 2 * len(idx) and batch.returns.shape == (len(idx), 6)


# ---- acting -------------------------------------------------------------------------------------------------------------
def test_policy_forward_and_act_device_follow_the_mode_and_the_mask():
    rs = np.random.RandomState(4)
    R, A = 130, 5
    mask = np.zeros((R, A), bool)
    for r in range(R):
        mask[r, rs.choice(A, 1 + r % 4, replace=False)] = True
    net = ImplicitQuantileNet([4, 32], A, (16,), num_cosines=8, device=DEV, seed=3)
    pol = IQNPolicy(model=net, action_space=_Discrete(A), sample_size=12, online_sample_size=6, target_sample_size=4,
                    eps_training=1.0, eps_inference=0.0, seed=11)
    obs = rs.standard_normal((R, 4)).astype(np.float32)
    for mode, S in ((pol.train, 6), (pol.eval, 12)):
        mode()
        out = pol(Batch(obs=Batch(obs=obs, mask=mask), info=Batch()))
        assert out.logits.shape == (R, A, S) and out.taus.shape == (R, S) and out.act.dtype == np.int64
        q = out.logits.double().cpu().numpy().mean(2)
        top = np.sort(np.where(mask, q, -np.inf), 1)
        clear = ~(top[:, -1] - top[:, -2] < 1e-6)          # rows whose float32 mean could order two actions otherwise
        assert clear.sum() > R // 2 and np.array_equal(out.act[clear], np.where(mask, q, -np.inf).argmax(1)[clear])
        assert np.array_equal(out.act, pol.compute_q_value(out.logits, mask).argmax(1).cpu().numpy())
        # the same fractions again: the net's forward is a function of (obs, taus)
        o2, _ = net.forward(_d(obs), S, taus=out.taus, save=False)
        assert torch.equal(o2.view(R, S, A).transpose(1, 2), out.logits)
    assert pol(Batch(obs=obs, info=Batch()), model=net).logits.shape == (R, A, 4)      # a lagged model: target_sample_size
    for mode, S in ((pol.eval, 12), (pol.train, 6)):
        mode()
        ctr = pol._sample_ctr
        res = pol.act_device(_d(obs), mask=_d(mask))                                   # epsilon 0: greedy
        assert pol._sample_ctr == ctr + R
        taus = ops.iqn_taus(R, S, pol.seed, DEV, offset=ctr)                           # the fractions that call drew
        o, _ = net.forward(_d(obs), S, taus=taus, save=False)
        q = ops.iqn_values(o, S, A)
        assert torch.equal(_bits(q), _bits(res["q"]))                                   # S fractions, those of the counter
        assert np.array_equal(res["act"].cpu().numpy(), ops.dqn_egreedy(q, pol._zero_dev, 0, mask=_d(mask)).cpu().numpy())
        masked = torch.where(_d(mask), q, torch.full_like(q, -np.inf))
        assert np.array_equal(res["act"].cpu().numpy(), masked.argmax(1).cpu().numpy())   # the first argmax of the masked mean
    pol.is_within_training_step = True                                                  # epsilon 1: legal random actions
    a1 = pol.act_device(_d(obs), mask=_d(mask))["act"].cpu().numpy()
    assert mask[np.arange(R), a1].all() and not np.array_equal(a1, res["act"].cpu().numpy())
