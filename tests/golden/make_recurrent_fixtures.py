"""Generate tests/golden/recurrent.npz by RUNNING THE REFERENCE's `Recurrent` net and frame-stacked `VectorReplayBuffer`
(utils/net/common.py:372-458, data/buffer/buffer_base.py:495-635, manager.py:195-229, imported through oracle/ref_shim.py) in
float32 on the CPU.  Every array is data: parameters, inputs, add traces, indices and recorded results.

  a_*   Recurrent(layer_num=2, state_shape=6, action_shape=5, hidden_layer_size=32) on obs [7, 3, 6] from state None:
        a_p_<key> the parameters under their state_dict keys (a_keys: the key order), a_obs, a_out, a_hidden, a_cell
        [7, 2, 32], a_r the weights of the scalar sum(out * r), a_g_<key> its autograd gradients.
  b_*   the same net and obs from a given state b_h0, b_c0 [7, 2, 32]: b_out, b_hidden, b_cell, b_g_<key>.
  c_*   VectorReplayBuffer(24, 3, stack_num=4) under a recorded add trace (c_env, c_done, c_obs, c_obs_next per added row; obs
        rows are [2, 3]: two agents): sub-buffer 0 wraps once; episodes of length 1, 2 and 5 and open tails.  c_idx =
        sample_indices(0) with sample_avail off; c_stack_obs / c_stack_obs_next = buf[c_idx].obs / .obs_next [I, 4, 2, 3];
        c_prev = buf.prev(c_idx); c_avail = sample_indices(0) of the same trace with sample_avail on; the bookkeeping the walk
        reads: c_done_flat [24], c_last_index, c_lengths, c_insertion_idx, c_size [3].
Run from the repository root:  python tests/golden/make_recurrent_fixtures.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import ref_shim  # noqa: E402

ref_shim.install()

import torch  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)
from tianshou.algorithm.modelfree.dqn import DQN, DiscreteQLearningPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import Recurrent  # noqa: E402

from dqn_restatement import RestatedBuffer, nstep_walk  # noqa: E402
from recurrent_restatement import recurrent_dqn_step, recurrent_keys, stacked_indices  # noqa: E402

H, LAYERS, D, A, L, B = 32, 2, 6, 5, 3, 7
D_EPS = 1e-8   # Adam's eps in fixture d: torch's default


def net_sections(res: dict) -> None:
    torch.manual_seed(11)
    net = Recurrent(layer_num=LAYERS, state_shape=D, action_shape=A, hidden_layer_size=H)
    keys = list(net.state_dict().keys())
    assert keys == recurrent_keys(LAYERS), keys
    rs = np.random.RandomState(5)
    obs = rs.standard_normal((B, L, D)).astype(np.float32)
    r = rs.standard_normal((B, A)).astype(np.float32)
    h0 = (0.5 * rs.standard_normal((B, LAYERS, H))).astype(np.float32)
    c0 = rs.standard_normal((B, LAYERS, H)).astype(np.float32)
    res["a_keys"] = np.array(keys)
    res.update({f"a_p_{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()})
    res.update(a_obs=obs, a_r=r, b_h0=h0, b_c0=c0)
    for tag, state in (("a", None), ("b", Batch(hidden=torch.as_tensor(h0), cell=torch.as_tensor(c0)))):
        net.zero_grad()
        out, st = net(obs, state)
        (out * torch.as_tensor(r)).sum().backward()
        res.update({f"{tag}_out": out.detach().numpy().copy(), f"{tag}_hidden": st.hidden.numpy().copy(),
                    f"{tag}_cell": st.cell.numpy().copy()})
        res.update({f"{tag}_g_{k}": p.grad.numpy().copy() for k, p in net.named_parameters()})


def buffer_section(res: dict) -> None:
    n_buf, sub, stack = 3, 8, 4
    # (env, done) per added row: env 0 gets 11 rows (wraps once) with episodes of length 1, 2 and 5 and an open tail of 3 that
    # overwrites the first two; env 1 gets 6 rows: episodes of length 2 and 1, then an open tail; env 2 one open episode of 5
    plan = {0: [0, 2, 7], 1: [1, 2], 2: []}
    counts = {0: 11, 1: 6, 2: 5}
    trace = [(e, k in plan[e]) for k in range(11) for e in range(n_buf) if k < counts[e]]
    rs = np.random.RandomState(8)
    env = np.array([t[0] for t in trace], np.int64)
    done = np.array([t[1] for t in trace], bool)
    obs = rs.standard_normal((len(trace), 2, 3)).astype(np.float32)
    obs_next = rs.standard_normal((len(trace), 2, 3)).astype(np.float32)
    bufs = [VectorReplayBuffer(n_buf * sub, n_buf, stack_num=stack, sample_avail=av) for av in (False, True)]
    for k in range(len(trace)):
        for buf in bufs:
            buf.add(Batch(obs=obs[k:k + 1], act=np.zeros(1, int), rew=np.zeros(1), terminated=done[k:k + 1],
                          truncated=np.zeros(1, bool), obs_next=obs_next[k:k + 1]), buffer_ids=[int(env[k])])
    buf, buf_av = bufs
    idx = buf.sample_indices(0)
    got = buf[idx]
    assert got.obs.shape == (len(idx), stack, 2, 3)
    res.update(c_env=env, c_done=done, c_obs=obs, c_obs_next=obs_next, c_idx=idx.astype(np.int64), c_stack_obs=got.obs,
               c_stack_obs_next=got.obs_next, c_prev=buf.prev(idx).astype(np.int64),
               c_avail=buf_av.sample_indices(0).astype(np.int64), c_done_flat=np.asarray(buf.done, bool),
               c_last_index=np.asarray(buf.last_index, np.int64), c_lengths=np.asarray(buf._lengths, np.int64),
               c_insertion_idx=np.array([b._insertion_idx for b in buf.buffers], np.int64),
               c_size=np.array([b._size for b in buf.buffers], np.int64))
    assert 0 < len(res["c_avail"]) < len(idx)


def dqn_section(res: dict) -> None:
    n_env, S, T, Dd, Ad, Hd, Ld, n_step, gamma, lr, eps, Bd = 3, 16, 20, 6, 5, 32, 3, 2, 0.97, 1e-3, D_EPS, 24
    rs = np.random.RandomState(31)
    torch.manual_seed(31)
    rows = dict(obs=rs.standard_normal((T, n_env, Dd)).astype(np.float32), obs_next=rs.standard_normal((T, n_env, Dd)).astype(np.float32),
                act=rs.randint(0, Ad, (T, n_env)), rew=rs.standard_normal((T, n_env)).astype(np.float32),
                term=rs.rand(T, n_env) < 0.08, trunc=rs.rand(T, n_env) < 0.08)
    buf, RB = VectorReplayBuffer(n_env * S, n_env, stack_num=Ld), RestatedBuffer(n_env, S, 1)
    flat_obs, flat_next, flat_act = (np.zeros((n_env * S, Dd), np.float32), np.zeros((n_env * S, Dd), np.float32),
                                     np.zeros(n_env * S, np.int64))
    for t in range(T):
        buf.add(Batch(obs=rows["obs"][t], act=rows["act"][t], rew=rows["rew"][t].astype(np.float64), terminated=rows["term"][t],
                      truncated=rows["trunc"][t], obs_next=rows["obs_next"][t]), buffer_ids=np.arange(n_env))
        for e in range(n_env):
            cur = RB.add(e, rows["rew"][t, e], bool(rows["term"][t, e]), bool(rows["trunc"][t, e]))
            flat_obs[cur], flat_next[cur], flat_act[cur] = rows["obs"][t, e], rows["obs_next"][t, e], rows["act"][t, e]
    net = Recurrent(layer_num=1, state_shape=Dd, action_shape=Ad, hidden_layer_size=Hd)
    algo = DQN(policy=DiscreteQLearningPolicy(model=net, action_space=gym.spaces.Discrete(Ad)),
               optim=AdamOptimizerFactory(lr=lr, eps=eps), gamma=gamma, n_step_return_horizon=n_step, target_update_freq=1)
    with torch.no_grad():
        for p in algo.model_old.parameters():
            p.add_(0.05 * torch.randn_like(p))
    online = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    lagged = {k: v.detach().numpy().copy() for k, v in algo.model_old.module.state_dict().items()}
    assert list(online) == list(lagged) == recurrent_keys(1)
    idx = rs.choice(buf.sample_indices(0), Bd, replace=False).astype(np.int64)
    batch = algo._preprocess_batch(buf[idx], buf, idx)
    stats = algo._update_with_batch(batch)
    after = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    lag_after = {k: v.detach().numpy().copy() for k, v in algo.model_old.module.state_dict().items()}
    returns = batch.returns.detach().numpy().reshape(-1).astype(np.float64)
    # the restatement of the same step, from the trace alone
    idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, gamma, 0)
    walk = (RB.done, RB.last_index, RB.size, S)
    obs_st, nxt_st = flat_obs[stacked_indices(idx, Ld, *walk)], flat_next[stacked_indices(idx_n, Ld, *walk)]
    assert np.array_equal(obs_st, buf[idx].obs) and np.array_equal(nxt_st, buf[idx_n].obs_next)
    r = recurrent_dqn_step(online, lagged, obs_st, flat_act[idx], nxt_st, mc, gpow, vmask, 1, lr, eps)
    assert r["top2_gap"] > 1e-4, "a greedy tie within float32 rounding: change the seed"
    worst = max([abs(r["loss"] - stats.loss) / abs(r["loss"]), np.abs(r["returns"] - returns).max() / np.abs(r["returns"]).max()]
                + [np.abs(r["online"][k] - after[k]).max() / np.abs(r["online"][k]).max() for k in online])
    print(f"fixture d: loss {stats.loss:.6f}; worst |ref32 - re64| / max |re64| over loss, returns, parameter blocks = {worst:.3e}")
    assert worst <= 1e-6 and all(np.array_equal(lag_after[k], online[k]) for k in online)
    assert (np.abs(after["fc1.weight"] - online["fc1.weight"]) > 0).all()
    res.update(d_dims=np.array([n_env, S, T, Dd, Ad, Hd, Ld, n_step, Bd], np.int64), d_gamma=np.float64(gamma), d_lr=np.float64(lr),
               d_eps=np.float64(eps), d_idx=idx, d_loss=np.float64(stats.loss), d_returns=returns,
               **{f"d_rows_{k}": v for k, v in rows.items()}, **{f"d_p_{k}": v for k, v in online.items()},
               **{f"d_lag_{k}": v for k, v in lagged.items()}, **{f"d_q_{k}": v for k, v in after.items()},
               **{f"d_qlag_{k}": v for k, v in lag_after.items()})


def main() -> None:
    res: dict = {}
    net_sections(res)
    buffer_section(res)
    dqn_section(res)
    out = os.path.join(HERE, "recurrent.npz")
    np.savez_compressed(out, **res)
    print(f"wrote {out}: {len(res)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
