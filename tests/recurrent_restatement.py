"""float64 numpy restatement of the recurrent pieces, written from the equations (not from the kernels):

  * one LSTM layer forward / backward through time, torch's layout (gate order i, f, g, o; weight_hh [4H, H]);
  * the reference `Recurrent` net fc1 -> LSTM x layers -> fc2 on the last step (utils/net/common.py:372-458), forward and the
    gradient of sum(out * r) w.r.t. every parameter;
  * the frame-stacked index walk of ReplayBuffer.get / ReplayBufferManager.prev (buffer_base.py:533-590, manager.py:306-331)
    and `sample_indices` with `sample_avail` (buffer_base.py:495-531, manager.py:195-229).
"""
from __future__ import annotations

import numpy as np


def sigmoid(x):
    """Finite for every finite x: the exponent is never positive."""
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def lstm_layer_forward(x, w_ih, w_hh, b_ih, b_hh, h0=None, c0=None):
    """x [B, L, K] -> dict(h [B, L, H], h_prev, c, c_prev [B, L, H], gates [B, L, 4H] activated, h_n, c_n [B, H])."""
    x, w_ih, w_hh = np.asarray(x, np.float64), np.asarray(w_ih, np.float64), np.asarray(w_hh, np.float64)
    b = np.asarray(b_ih, np.float64) + np.asarray(b_hh, np.float64)
    B, L, _ = x.shape
    H = w_hh.shape[1]
    h = np.zeros((B, H)) if h0 is None else np.asarray(h0, np.float64).copy()
    c = np.zeros((B, H)) if c0 is None else np.asarray(c0, np.float64).copy()
    out = dict(h=np.zeros((B, L, H)), h_prev=np.zeros((B, L, H)), c=np.zeros((B, L, H)), c_prev=np.zeros((B, L, H)),
               gates=np.zeros((B, L, 4 * H)))
    for t in range(L):
        pre = x[:, t] @ w_ih.T + b + h @ w_hh.T
        i, f, o = sigmoid(pre[:, :H]), sigmoid(pre[:, H:2 * H]), sigmoid(pre[:, 3 * H:])
        g = np.tanh(pre[:, 2 * H:3 * H])
        out["h_prev"][:, t], out["c_prev"][:, t] = h, c
        c = f * c + i * g
        h = o * np.tanh(c)
        out["h"][:, t], out["c"][:, t] = h, c
        out["gates"][:, t] = np.concatenate([i, f, g, o], axis=1)
    out["h_n"], out["c_n"] = h, c
    return out


def lstm_layer_backward(fw, w_hh, d_h, d_hn=None, d_cn=None):
    """`fw` of lstm_layer_forward; d_h [B, L, H] arriving at every h_t from above; d_hn, d_cn at the final state.
    -> dict(d_gates [B, L, 4H] w.r.t. the pre-activations, d_h0, d_c0 [B, H])."""
    w_hh, d_h = np.asarray(w_hh, np.float64), np.asarray(d_h, np.float64)
    B, L, H = d_h.shape
    dh_rec = np.zeros((B, H)) if d_hn is None else np.asarray(d_hn, np.float64).copy()
    dc = np.zeros((B, H)) if d_cn is None else np.asarray(d_cn, np.float64).copy()
    d_gates = np.zeros((B, L, 4 * H))
    for t in range(L - 1, -1, -1):
        G = fw["gates"][:, t]
        i, f, g, o = G[:, :H], G[:, H:2 * H], G[:, 2 * H:3 * H], G[:, 3 * H:]
        tc = np.tanh(fw["c"][:, t])
        dh = d_h[:, t] + dh_rec
        dct = dc + dh * o * (1.0 - tc * tc)
        d_gates[:, t] = np.concatenate([dct * g * i * (1 - i), dct * fw["c_prev"][:, t] * f * (1 - f), dct * i * (1 - g * g),
                                        dh * tc * o * (1 - o)], axis=1)
        dc = dct * f
        dh_rec = d_gates[:, t] @ w_hh
    return dict(d_gates=d_gates, d_h0=dh_rec, d_c0=dc)


def lstm_layer_grads(fw, x, d_gates, w_ih):
    """-> (d weight_ih, d weight_hh, d bias (both biases), d_x [B, L, K])."""
    x = np.asarray(x, np.float64)
    dg = d_gates.reshape(-1, d_gates.shape[-1])
    return (dg.T @ x.reshape(dg.shape[0], -1), dg.T @ fw["h_prev"].reshape(dg.shape[0], -1), dg.sum(0),
            d_gates @ np.asarray(w_ih, np.float64))


def recurrent_keys(layer_num: int) -> list[str]:
    """The reference module's state_dict() order: nn.LSTM's parameters, then fc1, then fc2."""
    keys = [f"nn.{p}_l{k}" for k in range(layer_num) for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return keys + ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]


def recurrent_forward(params: dict, obs, layer_num: int, state=None):
    """params: {key: array} under `recurrent_keys`; obs [B, L, D] or [B, D]; state None or (hidden, cell) [B, layers, H].
    -> (out [B, A], (hidden, cell) [B, layers, H], what `recurrent_backward` needs)."""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    obs = np.asarray(obs, np.float64)
    if obs.ndim == 2:
        obs = obs[:, None]
    x = obs @ p["fc1.weight"].T + p["fc1.bias"]
    saved, xs, hn, cn = [], [], [], []
    for k in range(layer_num):
        h0 = None if state is None else np.asarray(state[0], np.float64)[:, k]
        c0 = None if state is None else np.asarray(state[1], np.float64)[:, k]
        fw = lstm_layer_forward(x, p[f"nn.weight_ih_l{k}"], p[f"nn.weight_hh_l{k}"], p[f"nn.bias_ih_l{k}"], p[f"nn.bias_hh_l{k}"],
                                h0, c0)
        xs.append(x)
        saved.append(fw)
        hn.append(fw["h_n"])
        cn.append(fw["c_n"])
        x = fw["h"]
    out = x[:, -1] @ p["fc2.weight"].T + p["fc2.bias"]
    return out, (np.stack(hn, 1), np.stack(cn, 1)), dict(obs=obs, xs=xs, layers=saved, top=x)


def recurrent_backward(params: dict, saved: dict, d_out, layer_num: int) -> dict:
    """Gradient of sum(out * d_out) w.r.t. every parameter -> {key: array}."""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    d_out = np.asarray(d_out, np.float64)
    g = {"fc2.weight": d_out.T @ saved["top"][:, -1], "fc2.bias": d_out.sum(0)}
    d_h = np.zeros_like(saved["top"])
    d_h[:, -1] = d_out @ p["fc2.weight"]
    for k in range(layer_num - 1, -1, -1):
        fw = saved["layers"][k]
        bw = lstm_layer_backward(fw, p[f"nn.weight_hh_l{k}"], d_h)
        dwi, dwh, db, d_h = lstm_layer_grads(fw, saved["xs"][k], bw["d_gates"], p[f"nn.weight_ih_l{k}"])
        g[f"nn.weight_ih_l{k}"], g[f"nn.weight_hh_l{k}"], g[f"nn.bias_ih_l{k}"], g[f"nn.bias_hh_l{k}"] = dwi, dwh, db, db
    d1 = d_h.reshape(-1, d_h.shape[-1])
    g["fc1.weight"], g["fc1.bias"] = d1.T @ saved["obs"].reshape(d1.shape[0], -1), d1.sum(0)
    return g


# ---- the stacked index walk ------------------------------------------------------------------------------------------------
def prev_index(index, done, last_index, lengths, sub_size: int):
    """ReplayBufferManager.prev (manager.py:306-331): done [buffer_num * sub_size] flat by reference index, last_index and
    lengths per sub-buffer."""
    index = np.asarray(index, np.int64) % (len(lengths) * sub_size)
    e = index // sub_size
    start = e * sub_size
    cur = np.maximum(np.asarray(lengths, np.int64)[e], 1)
    sub = (index - start - 1) % cur
    end = np.asarray(done, bool)[sub + start] | (sub + start == np.asarray(last_index, np.int64)[e])
    return (sub + end) % cur + start


def stacked_indices(index, stack_num: int, done, last_index, lengths, sub_size: int):
    """[I, stack_num] reference indices, oldest first (buffer_base.py:572-583)."""
    idx = np.asarray(index, np.int64).reshape(-1)
    cols = [idx]
    for _ in range(stack_num - 1):
        idx = prev_index(idx, done, last_index, lengths, sub_size)
        cols.append(idx)
    return np.stack(cols[::-1], axis=1)


def sample_indices_all(insertion_idx, size, done, last_index, lengths, sub_size: int, stack_num: int = 1, sample_avail: bool = False):
    """sample_indices(0) of a VectorReplayBuffer (manager.py:224-229 over buffer_base.py:511-531): per sub-buffer
    arange(ins, size) then arange(ins), plus its offset; with sample_avail and stack_num > 1 only the indices whose
    stack_num - 1 predecessors are all distinct."""
    out = []
    for e, (ins, sz) in enumerate(zip(np.asarray(insertion_idx, np.int64), np.asarray(size, np.int64))):
        if sz == 0:
            continue
        idx = np.concatenate([np.arange(ins, sz), np.arange(ins)]).astype(np.int64) + e * sub_size
        if sample_avail and stack_num > 1:
            prev = idx
            for _ in range(stack_num - 2):
                prev = prev_index(prev, done, last_index, lengths, sub_size)
            idx = idx[prev_index(prev, done, last_index, lengths, sub_size) != prev]
        out.append(idx)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


# ---- one DQN step on the recurrent net (dqn.py:365-404 around utils/net/common.py:372-458) -----------------------------------
def recurrent_dqn_step(online: dict, lagged: dict, obs, act, obs_next, mc, gpow, vmask, layer_num: int, lr: float,
                       eps: float = 1e-8, is_double: bool = True) -> dict:
    """One `_preprocess_batch` (after the n-step walk) + `_update_with_batch` with a lagged network and target_update_freq 1,
    from the equations: every forward starts from zero state; q' = online(obs_next), target = lagged(obs_next)[argmax q'] (double
    Q) or max lagged(obs_next); returns = mc + gpow * vmask * target; loss = mean (returns - q[act])^2; the lagged net takes the
    online weights of BEFORE the step (the `_iter` rule at 0); Adam's first step is w - lr g / (|g| + eps) (m^ = g, v^ = g^2).
    obs, obs_next [B, L, D] stacks.  -> dict(loss, returns, q, grads {key}, online {key} after the step, lagged {key} after)."""
    q, _, saved = recurrent_forward(online, obs, layer_num)
    qn_on = recurrent_forward(online, obs_next, layer_num)[0]
    qn_tg = recurrent_forward(lagged, obs_next, layer_num)[0]
    rows = np.arange(q.shape[0])
    target = qn_tg[rows, qn_on.argmax(1)] if is_double else qn_tg.max(1)
    returns = np.asarray(mc, np.float64) + np.asarray(gpow, np.float64) * np.asarray(vmask, bool) * target
    act = np.asarray(act, np.int64).reshape(-1)
    td = returns - q[rows, act]
    dq = np.zeros_like(q)
    dq[rows, act] = -2.0 * td / len(td)
    grads = recurrent_backward(online, saved, dq, layer_num)
    after = {k: np.asarray(online[k], np.float64) - lr * grads[k] / (np.abs(grads[k]) + eps) for k in grads}
    return dict(loss=float((td * td).mean()), returns=returns, q=q, grads=grads, online=after,
                lagged={k: np.asarray(online[k], np.float64).copy() for k in online}, top2_gap=float(np.diff(np.sort(qn_on, 1)[:, -2:], axis=1).min()))


def fixture_d_step(Z) -> dict:
    """Fixture d of tests/golden/recurrent.npz restated from its trace alone: the buffer rows by flat index, the n-step walk
    (dqn_restatement), the stacked index walk, then `recurrent_dqn_step`.  -> its dict + idx_n, obs, obs_next (the stacks), act."""
    from dqn_restatement import RestatedBuffer, nstep_walk

    n_env, S, T, D, A, H, L, n_step, B = (int(x) for x in Z["d_dims"])
    RB = RestatedBuffer(n_env, S, 1)
    obs, nxt, act = np.zeros((n_env * S, D), np.float32), np.zeros((n_env * S, D), np.float32), np.zeros(n_env * S, np.int64)
    for t in range(T):
        for e in range(n_env):
            cur = RB.add(e, Z["d_rows_rew"][t, e], bool(Z["d_rows_term"][t, e]), bool(Z["d_rows_trunc"][t, e]))
            obs[cur], nxt[cur], act[cur] = Z["d_rows_obs"][t, e], Z["d_rows_obs_next"][t, e], Z["d_rows_act"][t, e]
    idx = Z["d_idx"]
    idx_n, mc, gpow, vmask = nstep_walk(RB, idx, n_step, float(Z["d_gamma"]), 0)
    walk = (RB.done, RB.last_index, RB.size, S)
    keys = recurrent_keys(1)
    r = recurrent_dqn_step({k: Z[f"d_p_{k}"] for k in keys}, {k: Z[f"d_lag_{k}"] for k in keys},
                           obs[stacked_indices(idx, L, *walk)], act[idx], nxt[stacked_indices(idx_n, L, *walk)], mc, gpow, vmask, 1,
                           float(Z["d_lr"]), float(Z["d_eps"]))
    r.update(mc=mc, gpow=gpow, vmask=vmask, idx_n=idx_n, obs=obs[stacked_indices(idx, L, *walk)], obs_next=nxt[stacked_indices(idx_n, L, *walk)], act=act[idx])
    return r
