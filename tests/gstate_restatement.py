"""Float64 numpy restatement of the learned global states of CTDE: `GlobalStateConstructor` modes "attention" and "graph"
(reference ctde.py:268-280, 302-335), forward and backward, in the reference's own order of operations (per-agent projections,
THEN the mean over agents) and in the pooled order the device path takes (the mean, THEN the linear layer) -- and the attention
core alone under the kernel's contract (tsm_attn_pool_forward / _backward: qkv -> ctx, P; d_ctx -> d_qkv).

Weights are dicts under the reference module's state_dict keys.  tests/golden/gstate.npz pins all of it to the reference
(tests/test_gstate_restatement.py); the GPU tests compare the kernels and the nets with it.
"""
from __future__ import annotations

import numpy as np

HEADS = 4
ATT_KEYS = ("attention.in_proj_weight", "attention.in_proj_bias", "attention.out_proj.weight", "attention.out_proj.bias",
            "output_proj.weight", "output_proj.bias")
GRAPH_KEYS = ("gnn_layer1.weight", "gnn_layer1.bias", "gnn_layer2.weight", "gnn_layer2.bias")


def f64(x):
    return np.asarray(x, np.float64)


# ---- the attention core: what the kernels compute ---------------------------------------------------------------------------------
def split_heads(qkv):
    """qkv [B, N, 3 D] -> Q, K, V [B, 4, N, dh]."""
    qkv = f64(qkv)
    B, N, D3 = qkv.shape
    D = D3 // 3
    return tuple(qkv[:, :, k * D:(k + 1) * D].reshape(B, N, HEADS, D // HEADS).transpose(0, 2, 1, 3) for k in range(3))


def softmax_rows(S):
    e = np.exp(S - S.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def attn_scores(qkv):
    Q, K, _ = split_heads(qkv)
    return (Q / np.sqrt(Q.shape[-1])) @ K.transpose(0, 1, 3, 2)   # [B, 4, N, N]


def attn_heads(qkv):
    """-> (O [B, N, D]: the concatenated heads per query agent, P [B, 4, N, N])."""
    _, _, V = split_heads(qkv)
    P = softmax_rows(attn_scores(qkv))
    O = P @ V                                                      # [B, 4, N, dh]
    B, _, N, dh = O.shape
    return O.transpose(0, 2, 1, 3).reshape(B, N, HEADS * dh), P


def attn_core(qkv):
    """tsm_attn_pool_forward: -> (ctx [B, D] = mean over the query agents of the concatenated heads, P)."""
    O, P = attn_heads(qkv)
    return O.mean(axis=1), P


def attn_core_backward(d_ctx, qkv, P):
    """tsm_attn_pool_backward: -> d_qkv [B, N, 3 D]."""
    Q, K, V = split_heads(qkv)
    B, _, N, dh = Q.shape
    P, d_ctx = f64(P), f64(d_ctx)
    dO = np.broadcast_to((d_ctx / N).reshape(B, 1, HEADS, dh).transpose(0, 2, 1, 3), (B, HEADS, N, dh))
    dV = P.transpose(0, 1, 3, 2) @ dO
    dP = dO @ V.transpose(0, 1, 3, 2)
    dS = P * (dP - (P * dP).sum(axis=-1, keepdims=True))
    dQ = dS @ K / np.sqrt(dh)
    dK = dS.transpose(0, 1, 3, 2) @ Q / np.sqrt(dh)
    back = lambda x: x.transpose(0, 2, 1, 3).reshape(B, N, HEADS * dh)  # noqa: E731
    return np.concatenate([back(dQ), back(dK), back(dV)], axis=2)


# ---- mode "attention" ---------------------------------------------------------------------------------------------------------------
def attention_forward(w, obs, pooled: bool = True):
    """obs [B, N, D] -> (state [B, hidden], cache).  pooled False: the reference's order, out_proj on every agent, then the
    mean (ctde.py:308-312); True: the device path's, the mean before out_proj."""
    w = {k: f64(v) for k, v in w.items()}
    obs = f64(obs)
    qkv = obs @ w["attention.in_proj_weight"].T + w["attention.in_proj_bias"]
    Wo, bo = w["attention.out_proj.weight"], w["attention.out_proj.bias"]
    if pooled:
        ctx, P = attn_core(qkv)
        pooled_out = ctx @ Wo.T + bo
    else:
        O, P = attn_heads(qkv)
        ctx = O.mean(axis=1)
        pooled_out = (O @ Wo.T + bo).mean(axis=1)
    state = pooled_out @ w["output_proj.weight"].T + w["output_proj.bias"]
    return state, dict(obs=obs, qkv=qkv, P=P, ctx=ctx, pooled=pooled_out)


def attention_backward(w, cache, d_state):
    """-> {key: gradient} of sum(state * d_state)."""
    w = {k: f64(v) for k, v in w.items()}
    d_state = f64(d_state)
    obs, qkv = cache["obs"], cache["qkv"]
    g = {"output_proj.weight": d_state.T @ cache["pooled"], "output_proj.bias": d_state.sum(axis=0)}
    d_pooled = d_state @ w["output_proj.weight"]
    g["attention.out_proj.weight"], g["attention.out_proj.bias"] = d_pooled.T @ cache["ctx"], d_pooled.sum(axis=0)
    d_ctx = d_pooled @ w["attention.out_proj.weight"]
    d_qkv = attn_core_backward(d_ctx, qkv, cache["P"])
    g["attention.in_proj_weight"] = d_qkv.reshape(-1, d_qkv.shape[-1]).T @ obs.reshape(-1, obs.shape[-1])
    g["attention.in_proj_bias"] = d_qkv.sum(axis=(0, 1))
    return g


# ---- mode "graph" -------------------------------------------------------------------------------------------------------------------
def pool_coefficients(n_agents: int, adjacency=None):
    """c [N]: mean_n((A^ x)_n) = sum_m c_m x_m, A^ the row-normalised adjacency; None: 1 / N."""
    if adjacency is None:
        return np.full(n_agents, 1.0 / n_agents)
    A = f64(adjacency)
    return (A / A.sum(axis=1, keepdims=True)).sum(axis=0) / n_agents


def agent_pool(h, c, relu: bool = False):
    """tsm_agent_pool_forward: h [B, N, H] -> [B, H]."""
    h = f64(h)
    return np.einsum("n,bnk->bk", f64(c), np.maximum(h, 0.0) if relu else h)


def agent_pool_backward(d, c, h_relu=None):
    """tsm_agent_pool_backward: d [B, H] -> d_h [B, N, H]."""
    d_h = f64(c)[None, :, None] * f64(d)[:, None, :]
    return d_h if h_relu is None else d_h * (f64(h_relu) > 0)


def graph_forward(w, obs, adjacency=None, pooled: bool = True):
    """obs [B, N, D] -> (state [B, H], cache).  pooled False: the reference's order (ctde.py:320-335): aggregate, gnn_layer2 on
    every agent, the mean; True: ONE weighted sum over the agents, then gnn_layer2."""
    w = {k: f64(v) for k, v in w.items()}
    obs = f64(obs)
    N = obs.shape[1]
    pre = obs @ w["gnn_layer1.weight"].T + w["gnn_layer1.bias"]
    c = pool_coefficients(N, adjacency)
    if pooled:
        z = agent_pool(pre, c, relu=True)
        state = z @ w["gnn_layer2.weight"].T + w["gnn_layer2.bias"]
    else:
        h = np.maximum(pre, 0.0)
        if adjacency is not None:
            A = f64(adjacency)
            agg = np.einsum("nm,bmk->bnk", A, h) / A.sum(axis=-1)[None, :, None]
        else:
            agg = np.broadcast_to(h.mean(axis=1, keepdims=True), h.shape)
        state = (agg @ w["gnn_layer2.weight"].T + w["gnn_layer2.bias"]).mean(axis=1)
        z = agent_pool(pre, c, relu=True)
    return state, dict(obs=obs, pre=pre, z=z, c=c)


def graph_backward(w, cache, d_state):
    w = {k: f64(v) for k, v in w.items()}
    d_state = f64(d_state)
    obs, pre = cache["obs"], cache["pre"]
    g = {"gnn_layer2.weight": d_state.T @ cache["z"], "gnn_layer2.bias": d_state.sum(axis=0)}
    d_pre = agent_pool_backward(d_state @ w["gnn_layer2.weight"], cache["c"], h_relu=pre)
    g["gnn_layer1.weight"] = d_pre.reshape(-1, d_pre.shape[-1]).T @ obs.reshape(-1, obs.shape[-1])
    g["gnn_layer1.bias"] = d_pre.sum(axis=(0, 1))
    return g


def relu_gap(w, obs) -> float:
    """The smallest |pre-activation| of gnn_layer1 on obs: a fixture keeps it away from the kink."""
    return float(np.abs(f64(obs) @ f64(w["gnn_layer1.weight"]).T + f64(w["gnn_layer1.bias"])).min())
