"""GPU tests (`-m gpu`) of DQN: the n-step walk (csrc/nstep.hip), the TD head and masked epsilon-greedy acting
(csrc/dqn.hip), DQN updates on a device buffer and MultiAgentOffPolicyAlgorithm on joint-lane and AEC buffers.

References: tests/golden/dqn.npz (the reference's own float64 and float32 runs) and the float64 restatement
(tests/dqn_restatement.py, pinned to the reference by tests/test_host_dqn.py).  Bars:
  * idx_n, vmask, d_q off the taken action, actions: exact;
  * mc, gamma^m, returns, td_error, d_q, head losses: max |hip - ref64| <= 1e-5 max |ref64| per array (the project's
    1e-5 relative bar, DESIGN.md section 6, on the array's scale: a td_error is a difference of two values of that scale);
  * losses, gradients and weights of full updates: test_gpu_qmix.py's  |hip - ref64| <= 4 max(e_ref, 8 ulp(max |ref64|))
    with e_ref = the reference's own float32 error, weights after Adam steps with its `adamcond` allowance.
Every comparison prints `PARITY name: ...` with the worst ratio to its bar."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "dqn.npz")
DEV = "cuda"

from dqn_restatement import DqnRestatement, nstep_walk, td_head  # noqa: E402
from test_host_dqn import _Discrete, _Env, up_inputs  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.dqn import DQN, DiscreteQLearningPolicy
    from tianshou_marl_amd.algorithm.multiagent import MultiAgentOffPolicyAlgorithm
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch
    from tianshou_marl_amd.data.buffer import DeviceAECReplayBuffer, DeviceVectorReplayBuffer
    from tianshou_marl_amd.utils.net import FlatMLP


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _d(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV) if dtype is None else torch.as_tensor(
        np.ascontiguousarray(x)).to(DEV, dtype)


def _rel(name, got, ref, bar=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), float(np.finfo(np.float32).tiny))
    ratio = float(np.abs(got - ref).max()) / (bar * scale)
    print(f"PARITY {name}: max |hip - ref64| / (1e-5 max |ref64|) = {ratio:.3g}")
    assert ratio <= 1.0, (name, ratio)


def _ulp_floor(ref):
    m = float(np.abs(ref).max()) if np.size(ref) else 0.0
    return 8.0 * float(np.spacing(np.float32(m))) if m > 0 else 8.0 * float(np.finfo(np.float32).tiny)


def _check(name, got, ref, e_ref, extra=0.0):
    """test_gpu_qmix.py's bar: |got - ref| <= plain + extra, plain = 4 max(e_ref, 8 ulp(max |ref|)); with an allowance all but
    0.1 % must also meet the plain bar alone."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    plain = 4.0 * max(float(e_ref), _ulp_floor(ref))
    tol = plain + extra
    err = np.abs(got - ref)
    ratio = float((err / tol).max())
    msg = f"PARITY {name}: max |hip - ref64| / tol = {ratio:.3g}"
    if np.ndim(extra) > 0:
        share = float((err <= plain).mean())
        msg += f", share within the plain bar {share:.6f}"
        assert share > 0.999, (name, share)
    print(msg)
    assert np.all(err <= tol), (name, ratio)


# ---- n-step walk ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ns_buffer(g):
    """The fixture's add script replayed into a joint-lane device buffer: agent k's lane carries reward column k."""
    B, S, D = (int(x) for x in g["ns_dims"])
    buf = DeviceVectorReplayBuffer(B * S, B, n_agent=D, obs_dim=3, device=DEV)
    for k in range(len(g["ns_env"])):
        z = np.zeros((1, D, 3), np.float32)
        buf.add(Batch(obs=z, act=np.zeros((1, D), np.int64), rew=g["ns_rew"][k:k + 1], terminated=g["ns_term"][k:k + 1],
                      truncated=g["ns_trunc"][k:k + 1], obs_next=z), buffer_ids=[int(g["ns_env"][k])])
    return buf


@pytest.mark.parametrize("n_step", [1, 3, 5])
@pytest.mark.parametrize("col", [0, 1])
def test_nstep_walk_matches_reference(g, ns_buffer, n_step, col):
    buf = ns_buffer
    assert np.array_equal(buf.sample_indices(0), g["ns_all"]) and np.array_equal(buf.unfinished_index(), g["ns_unfinished"])
    idx_n, mc, gpow, vmask = ops.nstep_return(buf.index, buf.term_store, buf.rew_store, _d(g["ns_indices"]), n_step,
                                              float(g["gamma"]), rew_col=col, term_col=col)
    p = f"ns_n{n_step}_c{col}_"
    assert np.array_equal(idx_n.cpu().numpy(), g[p + "idxn"])
    assert np.array_equal(vmask.cpu().numpy().astype(bool), g[p + "vmask"])
    _rel(p + "mc", mc.cpu().numpy(), g[p + "mc"])
    _rel(p + "gpow", gpow.cpu().numpy(), g[p + "gpow"])
    # the final returns through the TD head, with the fixture's table as the target network's output (one action)
    I = len(g["ns_indices"])
    tq = _d(g["ns_tq"])[idx_n].view(I, 1).contiguous()
    head = ops.dqn_td_head(torch.zeros(I, 1, device=DEV), tq, None, torch.zeros(I, dtype=torch.int64, device=DEV), mc, gpow,
                           vmask, is_double=False)
    _rel(p + "returns", head["returns"].cpu().numpy(), g[p + "returns"])


def test_nstep_walk_follows_vrb_next(g, ns_buffer):
    """idx_n equals n_step - 1 applications of tsm_vrb_next, for every stored index and its negative alias."""
    buf = ns_buffer
    idx = torch.arange(-buf.maxsize, buf.maxsize, device=DEV)
    cur = idx % buf.maxsize
    for n_step in (1, 2, 4, 9):
        idx_n = ops.nstep_return(buf.index, buf.term_store, buf.rew_store, idx, n_step, 0.9)[0]
        ref = cur
        for _ in range(n_step - 1):
            ref = buf.index.next(ref)
        assert torch.equal(idx_n, ref), n_step


# ---- TD head ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 5, 9])
def test_td_head_matches_reference(g, A):
    p = f"hd_A{A}_"
    B = len(g[p + "act"])
    assert B == 37
    q, on, tg = _d(g[p + "q"]), _d(g[p + "on"]), _d(g[p + "tg"])
    act, mc, gpow = _d(g[p + "act"]), _d(g[p + "mc"], torch.float32), _d(g[p + "gpow"], torch.float32)
    vmask, weight, mask = _d(g[p + "vmask"]), _d(g[p + "weight"]), _d(g[p + "mask"])
    slot = torch.zeros(2, device=DEV)
    worst = {}
    for c, case in enumerate(g["hd_cases"]):
        dbl, tgt, loss, msk = case[1] == "1", case[3] == "1", case.split("_")[1], case[-1] == "1"
        h = ops.dqn_td_head(q, on, tg if tgt else None, act, mc, gpow, vmask, mask_next=mask if msk else None,
                            weight=weight if loss == "msew" else None, is_double=dbl,
                            huber_delta=float(g["hd_huber_delta"]) if loss == "huber" else None)
        ops.qmix_finalize(h["partial"], B, slot)
        dq = h["dq"].cpu().numpy()
        sel = dq[np.arange(B), g[p + "act"]]
        off = dq.copy()
        off[np.arange(B), g[p + "act"]] = 0.0
        assert not off.any(), case   # exactly zero off the taken action
        for key, got, ref in (("td_error", h["td_error"].cpu().numpy(), g[p + "td"][4 * dbl + 2 * tgt + msk]),
                              ("dq", sel, g[p + "dqsel"][c]),
                              ("loss", [float(slot[0])], [g[p + "loss"][c, 0]])):
            ref = np.asarray(ref, np.float64)
            r = float(np.abs(np.asarray(got, np.float64) - ref).max()) / (1e-5 * max(float(np.abs(ref).max()), 1e-30))
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= 1.0, (case, key, r)
        assert float(slot[1]) == pytest.approx(float(g[p + "q"][np.arange(B), g[p + "act"]].astype(np.float64).mean()), rel=1e-5)
    for key, r in worst.items():
        print(f"PARITY hd A={A} {key} ({len(g['hd_cases'])} cases): max |hip - ref64| / (1e-5 max |ref64|) = {r:.3g}")


def test_td_head_poisons_an_action_outside_the_range(g):
    p = "hd_A5_"
    act = _d(g[p + "act"]).clone()
    act[4] = 5
    h = ops.dqn_td_head(_d(g[p + "q"]), _d(g[p + "on"]), None, act, _d(g[p + "mc"], torch.float32),
                        _d(g[p + "gpow"], torch.float32), _d(g[p + "vmask"]))
    assert torch.isnan(h["td_error"][4]) and not h["dq"][4].any() and not torch.isnan(h["td_error"][:4]).any()


def test_td_head_nan_logit_poisons_the_mask_offset_as_torch_does(g):
    """torch's min() / max() return a NaN logit, so the offset and with it every masked sum is NaN, and argmax takes entry 0."""
    p = "hd_A5_"
    on = g[p + "on"].copy()
    on[11, 2] = np.nan
    args = (g[p + "act"], g[p + "mc"], g[p + "gpow"], g[p + "vmask"])
    ref = td_head(g[p + "q"], on, g[p + "tg"], g[p + "mask"], *args, None, True, None)
    h = ops.dqn_td_head(_d(g[p + "q"]), _d(on), _d(g[p + "tg"]), _d(args[0]), _d(args[1], torch.float32),
                        _d(args[2], torch.float32), _d(args[3]), mask_next=_d(g[p + "mask"]))
    _rel("hd nan-offset td_error", h["td_error"].cpu().numpy(), ref["td_error"])
    exp = (g[p + "tg"][:, 0] * g[p + "vmask"]).astype(np.float64) * g[p + "gpow"] + g[p + "mc"]
    np.testing.assert_allclose(ref["returns"], exp, rtol=1e-12)


def test_egreedy_refuses_an_out_it_cannot_write_in_place():
    q = torch.zeros(8, 5, device=DEV)
    eps = torch.zeros(1, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        ops.dqn_egreedy(q, eps, 0, out=torch.zeros(8, 2, dtype=torch.int32, device=DEV)[:, 0])
    with pytest.raises(ValueError, match="at least 8"):
        ops.dqn_egreedy(q, eps, 0, out=torch.zeros(4, dtype=torch.int32, device=DEV))


# ---- full updates -------------------------------------------------------------------------------------------------------
def _dqn(init, dims, seed=0, **kw):
    net = FlatMLP(list(dims), "relu", device=DEV, seed=seed)
    if init is not None:
        net.flat.data.copy_(_d(np.asarray(init, np.float32)))
    pol = DiscreteQLearningPolicy(model=net, action_space=_Discrete(dims[-1]))
    return DQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), **kw)


def test_three_updates_match_reference(g):
    dims, B, n_env, S, n_step, freq, steps, T, RB, obs, obs_next, act = up_inputs(g)
    assert (dims, B, steps, freq) == ([6, 32, 32, 5], 37, 3, 2)
    buf = DeviceVectorReplayBuffer(n_env * S, n_env, n_agent=1, obs_dim=dims[0], device=DEV)
    for t in range(T):
        buf.add(Batch(obs=g["up_rows_obs"][t][:, None], act=g["up_rows_act"][t][:, None], rew=g["up_rows_rew"][t][:, None],
                      terminated=g["up_rows_term"][t], truncated=g["up_rows_trunc"][t],
                      obs_next=g["up_rows_obs_next"][t][:, None]), buffer_ids=np.arange(n_env))
    algo = _dqn(g["up_init"], dims, gamma=float(g["gamma"]), n_step_return_horizon=n_step, target_update_freq=freq)
    R = DqnRestatement(g["up_init"], dims, target_update_freq=freq)
    lr, cond, grad_tol = 1e-3, np.zeros(algo.policy.model.flat.numel()), None
    before = algo.target_flat.clone()
    changed = []
    for k in range(steps):
        idx = g[f"up_s{k}_indices"]
        batch = algo._preprocess_batch(Batch(), buf, idx)
        w_before = algo.policy.model.flat.data.clone()
        stats = algo._update_with_batch(batch)
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(g["gamma"]), 0)
        assert np.array_equal(batch.idx_n.cpu().numpy(), idx_n)
        r = R.update(obs[idx], act[idx], obs_next[idx_n], None, mc, gpow, vmask)
        cond += R.adam_cond()
        ref64, ref32 = (float(x) for x in g[f"up_s{k}_loss"])
        _check(f"up s{k} loss", [stats.loss], [ref64], abs(ref32 - ref64))     # the reference's own float64 run
        assert r["loss"] == pytest.approx(ref64, rel=1e-11)
        _check(f"up s{k} returns", batch.returns.cpu().numpy(), g[f"up_s{k}_returns"], float(g[f"up_s{k}_returns_eref"]))
        assert batch.weight.shape == (B,) and batch.weight.is_cuda   # td_error, for a prioritized buffer
        grad = algo._ws[B]["slabs"].double().sum(0).cpu().numpy()
        e = float(g[f"up_s{k}_grad_eref"])
        _check(f"up s{k} grad", grad, r["grads"], e)
        if grad_tol is None:
            grad_tol = 4.0 * max(e, _ulp_floor(r["grads"]))
        extra = np.minimum(cond * grad_tol, 2 * lr * (k + 1))
        w_hip = algo.policy.model.flat.double().cpu().numpy()
        _check(f"up s{k} weights", w_hip, R.weights(), float(g[f"up_s{k}_weights_eref"]), extra)
        didx = g[f"up_s{k}_weights_didx"]   # ... and the entries of the reference's float64 weights that the fixture keeps
        _check(f"up s{k} weights (reference entries)", w_hip[didx], g[f"up_s{k}_weights_dval"],
               float(g[f"up_s{k}_weights_eref"]), extra[didx])
        # the lagged copy: exactly at the calls the `_iter` rule names (0, 2, ...), and then the weights BEFORE the step
        changed.append(not torch.equal(algo.target_flat, before))
        if k % freq == 0:
            assert torch.equal(algo.target_flat, w_before), k
        before = algo.target_flat.clone()
        tidx = g[f"up_s{k}_targets_didx"]
        ref_changed = not np.array_equal(g[f"up_s{k}_targets_dval"],
                                         g[f"up_s{k - 1}_targets_dval"] if k else g["up_init"][tidx].astype(np.float64))
        assert changed[-1] == ref_changed, (k, changed)
    assert changed == [False, False, True] and algo._iter == steps


def test_update_samples_on_the_device_and_needs_a_training_step(g):
    dims = [6, 16, 5]
    buf = DeviceVectorReplayBuffer(32, 2, n_agent=1, obs_dim=6, device=DEV)
    rs = np.random.RandomState(0)
    for t in range(10):
        buf.add(Batch(obs=rs.randn(2, 1, 6).astype(np.float32), act=rs.randint(0, 5, (2, 1)), rew=rs.randn(2, 1).astype(np.float32),
                      terminated=rs.rand(2) < 0.2, truncated=np.zeros(2, bool), obs_next=rs.randn(2, 1, 6).astype(np.float32)))
    algo = _dqn(None, dims, n_step_return_horizon=2, target_update_freq=1, huber_loss_delta=1.0)
    with pytest.raises(RuntimeError, match="outside of a training step"):
        algo.update(buf, 16)
    algo.is_within_training_step = True
    w0 = algo.policy.model.flat.data.clone()
    stats = algo.update(buf, 16)
    assert np.isfinite(stats.loss) and not torch.equal(w0, algo.policy.model.flat.data)
    assert "loss" in stats.get_loss_stats_dict()
    sd = algo.state_dict()
    other = _dqn(None, dims, seed=5, n_step_return_horizon=2, target_update_freq=1, huber_loss_delta=1.0)
    other.load_state_dict(sd)
    assert torch.equal(other.policy.model.flat.data, algo.policy.model.flat.data) and other._iter == 1
    assert other.optim.step_count == 1 and torch.equal(other.optim.exp_avg, algo.optim.exp_avg)


# ---- epsilon-greedy ---------------------------------------------------------------------------------------------------
def _egreedy_inputs():
    rs = np.random.RandomState(4)
    R, A = 130, 5
    q = rs.standard_normal((R, A)).astype(np.float32)
    mask = np.zeros((R, A), bool)
    for r in range(R):
        mask[r, rs.choice(A, 1 + r % 4, replace=False)] = True   # 1 to 4 legal actions per row
    return R, A, q, mask


def test_egreedy_masked_argmax_and_draws():
    R, A, q, mask = _egreedy_inputs()
    qd, md = _d(q), _d(mask)
    eps0, eps1 = torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
    greedy = np.where(mask, q, -np.inf).argmax(1)
    assert np.array_equal(ops.dqn_egreedy(qd, eps0, 1, mask=md).cpu().numpy(), greedy)
    assert np.array_equal(ops.dqn_egreedy(qd, eps0, 1).cpu().numpy(), q.argmax(1))
    tie = q.copy()
    tie[:, 3] = tie[:, 1] = tie.max(1) + 1.0     # an exact tie: the first one wins
    assert (ops.dqn_egreedy(_d(tie), eps0, 1).cpu().numpy() == 1).all()
    a = ops.dqn_egreedy(qd, eps1, 7, offset=100, mask=md)
    an = a.cpu().numpy()
    assert mask[np.arange(R), an].all() and ((an >= 0) & (an < A)).all()          # no illegal action
    assert torch.equal(a, ops.dqn_egreedy(qd, eps1, 7, offset=100, mask=md))      # same (seed, offset): same actions
    assert not np.array_equal(an, greedy)
    head = ops.dqn_egreedy(qd[:64].contiguous(), eps1, 7, offset=100, mask=md[:64].contiguous())
    tail = ops.dqn_egreedy(qd[64:].contiguous(), eps1, 7, offset=164, mask=md[64:].contiguous())
    assert torch.equal(torch.cat([head, tail]), a)                                 # drawn in pieces = drawn at once
    off = torch.full((1,), 60, dtype=torch.int64, device=DEV)                     # a device-side counter adds to the offset
    assert torch.equal(ops.dqn_egreedy(qd, eps1, 7, offset=40, offset_dev=off, mask=md), a)
    assert not torch.equal(ops.dqn_egreedy(qd, eps1, 8, offset=100, mask=md), a)   # another seed
    half = ops.dqn_egreedy(qd, torch.full((1,), 0.5, device=DEV), 7, offset=100, mask=md).cpu().numpy()
    coin = half != greedy
    assert 0 < coin.sum() < R and np.array_equal(half[coin], an[coin])             # a row's draws do not depend on eps


def test_policy_forward_and_act_device_honour_the_mask():
    R, A, q, mask = _egreedy_inputs()
    net = FlatMLP([4, 16, A], "relu", device=DEV, seed=3)
    pol = DiscreteQLearningPolicy(model=net, action_space=_Discrete(A), eps_training=1.0, eps_inference=0.0, seed=11)
    obs = np.random.RandomState(1).standard_normal((R, 4)).astype(np.float32)
    out = pol(Batch(obs=Batch(obs=obs, mask=mask), info=Batch()))
    logits = out.logits.cpu().numpy()
    assert out.act.dtype == np.int64 and np.array_equal(out.act, np.where(mask, logits, -np.inf).argmax(1))
    assert np.array_equal(out.act, pol.compute_q_value(out.logits, mask).argmax(1).cpu().numpy())
    assert np.array_equal(pol(Batch(obs=obs, info=Batch())).act, logits.argmax(1))
    res = pol.act_device(_d(obs), mask=_d(mask))                       # inference: epsilon 0
    assert np.array_equal(res["act"].cpu().numpy(), out.act) and pol._sample_ctr == R
    pol.is_within_training_step = True                                  # training: epsilon 1, legal random actions
    a1 = pol.act_device(_d(obs), mask=_d(mask))["act"].cpu().numpy()
    assert mask[np.arange(R), a1].all() and not np.array_equal(a1, out.act)
    holder = dict(act=torch.full((R,), -7, dtype=torch.int32, device=DEV), logp=torch.ones(R, device=DEV),
                  value=torch.ones(R, device=DEV))
    assert pol.act_device(_d(obs), out=holder, mask=_d(mask)) is holder
    assert mask[np.arange(R), holder["act"].cpu().numpy()].all() and not holder["logp"].any() and not holder["value"].any()


# ---- MultiAgentOffPolicyAlgorithm ------------------------------------------------------------------------------------------
def _pair(dims, init=None, **kw):
    """Two lists of per-agent DQNs with equal weights: one for the multi-agent object, one for the per-agent runs."""
    mk = lambda: [_dqn(None if init is None else init[i], dims, seed=20 + i, **kw) for i in range(2)]  # noqa: E731
    return mk(), mk()


def test_multiagent_update_joint_lanes():
    rs = np.random.RandomState(8)
    N, E, T, D, A = 2, 4, 6, 5, 3
    buf = DeviceVectorReplayBuffer(E * 8, E, n_agent=N, obs_dim=D, device=DEV)
    for t in range(T):
        buf.add(Batch(obs=rs.randn(E, N, D).astype(np.float32), act=rs.randint(0, A, (E, N)), rew=rs.randn(E, N).astype(np.float32),
                      terminated=rs.rand(E) < 0.2, truncated=rs.rand(E) < 0.1, obs_next=rs.randn(E, N, D).astype(np.float32)))
    ours, alone = _pair([D, 16, A], n_step_return_horizon=3, target_update_freq=2)
    ma = MultiAgentOffPolicyAlgorithm(algorithms=ours, env=_Env(N))
    ma.is_within_training_step = True
    stats = ma.update(buf, 0).get_loss_stats_dict()
    idx = buf.sample_indices(0)
    for k in range(N):
        s = alone[k]._update_with_batch(alone[k]._preprocess_batch(Batch(), buf, idx, agent=k))
        assert stats[f"agent_{k}/loss"] == s.loss and np.isfinite(s.loss)
        assert torch.equal(ours[k].policy.model.flat.data, alone[k].policy.model.flat.data)
    assert stats["agent_0/loss"] != stats["agent_1/loss"]
    with pytest.raises(ValueError, match="which agent"):
        alone[0]._preprocess_batch(Batch(), buf, idx)
    ma.update(buf, 9)   # a sampled subset runs too


def test_multiagent_update_aec_matches_reference(g):
    N, n_env, S, D, A, n_step, T = (int(x) for x in g["ma_dims"][:7])
    dims = [int(x) for x in g["ma_dims"][7:]]
    env = _Env(N)
    buf = DeviceAECReplayBuffer(n_env * S, n_env, env.agents, obs_dim=D, n_act=A, device=DEV)
    for t in range(T):
        ids = np.array([env.agents[a] for a in g["ma_turn"][t]], dtype=object)
        nxt = np.array([env.agents[(a + 1) % N] for a in g["ma_turn"][t]], dtype=object)
        buf.add(Batch(obs=Batch(agent_id=ids, obs=g["ma_obs"][t], mask=g["ma_mask"][t]), act=g["ma_act"][t], rew=g["ma_rew"][t],
                      terminated=g["ma_term"][t], truncated=g["ma_trunc"][t],
                      obs_next=Batch(agent_id=nxt, obs=g["ma_obs_next"][t])), buffer_ids=np.arange(n_env))
    kw = dict(gamma=float(g["gamma"]), n_step_return_horizon=n_step, target_update_freq=3)
    ours, alone = _pair(dims, g["ma_init"], **kw)
    ma = MultiAgentOffPolicyAlgorithm(algorithms=ours, env=env)
    ma.is_within_training_step = True
    stats = ma.update(buf, 0).get_loss_stats_dict()
    idx = buf.sample_indices(0)
    who = buf[idx].obs.agent_id
    for k, agent in enumerate(env.agents):
        rows = idx[np.nonzero(who == agent)[0]]
        s = alone[k]._update_with_batch(alone[k]._preprocess_batch(Batch(), buf, rows, agent=k))
        assert stats[f"{agent}/loss"] == s.loss
        ref64, ref32 = float(g["ma_loss"][0, k]), float(g["ma_loss"][1, k])
        _check(f"ma {agent} loss", [s.loss], [ref64], abs(ref32 - ref64))
        assert torch.equal(ours[k].policy.model.flat.data, alone[k].policy.model.flat.data)
