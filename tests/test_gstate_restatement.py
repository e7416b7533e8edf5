"""CPU: the float64 restatement of the learned global states (tests/gstate_restatement.py) against the reference's own run
(tests/golden/gstate.npz, float64 results rounded to float32): forward and every parameter gradient of both modes, at 1e-6
relative per array; the pooling identities against the unpooled (reference) order; the attention core alone under the kernels'
contract against finite differences and against the unpooled chain."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gstate_restatement as R  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "gstate.npz"))
ATT = [f"at{i}_" for i in range(len(G["att_cases"]))]
GRAPH = [f"gr{i}_" for i in range(len(G["graph_cases"]))]


def _w(p, sub="w_"):
    return {str(k): G[f"{p}{sub}{k}"] for k in G[p + "keys"]}


def _close(a, b, what, tol=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-30), (what, np.abs(a - b).max(), np.abs(b).max())


def test_fixture_covers_the_cases_the_issue_names():
    assert {tuple(c) for c in G["att_cases"]} == {(3, 8, 16), (8, 48, 64), (1, 4, 5)}
    assert {int(c[3]) for c in G["graph_cases"]} == {0, 1}
    A = G["gr1_adjacency"]
    assert not np.allclose(A, A.T) and len(np.unique(A[A > 0])) > 2 and (np.diag(A) > 0).all()


@pytest.mark.parametrize("p", ATT)
def test_attention_follows_the_reference(p):
    w, obs = _w(p), G[p + "obs"]
    for pooled in (False, True):
        state, cache = R.attention_forward(w, obs, pooled=pooled)
        _close(state, G[p + "state"], (p, "state", pooled))
    for k, g in R.attention_backward(w, cache, G[p + "d_state"]).items():
        _close(g, G[f"{p}g_{k}"], (p, k))
    # the key bias moves nothing: a shift common to all keys leaves the softmax as it is
    D = obs.shape[2]
    assert np.abs(G[p + "g_attention.in_proj_bias"][D:2 * D]).max() <= 1e-12 + 1e-7 * np.abs(G[p + "g_attention.in_proj_bias"]).max()


@pytest.mark.parametrize("p", GRAPH)
def test_graph_follows_the_reference(p):
    w, obs = _w(p), G[p + "obs"]
    adj = G[p + "adjacency"] if p + "adjacency" in G else None
    for pooled in (False, True):
        state, cache = R.graph_forward(w, obs, adj, pooled=pooled)
        _close(state, G[p + "state"], (p, "state", pooled))
    for k, g in R.graph_backward(w, cache, G[p + "d_state"]).items():
        _close(g, G[f"{p}g_{k}"], (p, k))


@pytest.mark.parametrize("N,D", [(1, 4), (3, 8), (8, 48)])
def test_pooling_before_the_out_projection_is_the_unpooled_order(N, D):
    """mean_n(W O_n + b) = W mean_n O_n + b, to float64 rounding; and P's rows sum to one."""
    rs = np.random.RandomState(N * 100 + D)
    qkv, W, b = rs.standard_normal((6, N, 3 * D)), rs.standard_normal((D, D)), rs.standard_normal(D)
    O, P = R.attn_heads(qkv)
    ctx, P2 = R.attn_core(qkv)
    assert np.array_equal(P, P2) and np.allclose(P.sum(-1), 1.0, rtol=0, atol=1e-14)
    _close(ctx @ W.T + b, (O @ W.T + b).mean(axis=1), "pool", 1e-13)


def test_graph_pooling_coefficients_are_the_unpooled_aggregation():
    rs = np.random.RandomState(5)
    N, H = 5, 7
    A = rs.rand(N, N) + 0.1
    h, W, b = rs.standard_normal((4, N, H)), rs.standard_normal((H, H)), rs.standard_normal(H)
    c = R.pool_coefficients(N, A)
    agg = np.einsum("nm,bmk->bnk", A / A.sum(1, keepdims=True), h)
    _close(R.agent_pool(h, c) @ W.T + b, (agg @ W.T + b).mean(axis=1), "graph pool", 1e-13)
    assert np.isclose(c.sum(), 1.0) and np.allclose(R.pool_coefficients(N), 1.0 / N)
    d = rs.standard_normal((4, H))
    _close(R.agent_pool_backward(d, c), c[None, :, None] * d[:, None, :], "pool backward", 1e-15)
    assert (R.agent_pool_backward(d, c, h_relu=h)[h <= 0] == 0).all()


@pytest.mark.parametrize("N,D", [(1, 4), (2, 8), (3, 12)])
def test_attention_core_backward_is_the_derivative_of_its_forward(N, D):
    rs = np.random.RandomState(N + D)
    qkv, d_ctx = rs.standard_normal((2, N, 3 * D)), rs.standard_normal((2, D))
    ctx, P = R.attn_core(qkv)
    got = R.attn_core_backward(d_ctx, qkv, P)
    num, eps = np.zeros_like(qkv), 1e-6
    for i in np.ndindex(*qkv.shape):
        hi, lo = qkv.copy(), qkv.copy()
        hi[i] += eps
        lo[i] -= eps
        num[i] = ((R.attn_core(hi)[0] - R.attn_core(lo)[0]) * d_ctx).sum() / (2 * eps)
    _close(got, num, "d_qkv", 1e-6)


def test_softmax_keeps_its_head_at_saturation():
    """Scores more than 700 apart: the maximum is subtracted, so no overflow, exact zeros and a one."""
    qkv = np.zeros((1, 2, 12))
    qkv[0, :, 0:4] = 40.0                      # Q
    qkv[0, 0, 4:8], qkv[0, 1, 4:8] = 40.0, -40.0   # K: scores 1600 / sqrt(1) apart per head
    qkv[0, :, 8:12] = [[1, 2, 3, 4], [5, 6, 7, 8]]
    ctx, P = R.attn_core(qkv)
    assert np.isfinite(P).all() and (P[..., 0] == 1.0).all() and (P[..., 1] == 0.0).all()
    assert np.array_equal(ctx[0], [1, 2, 3, 4])
