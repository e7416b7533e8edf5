"""float64 numpy restatement of the dense MLP engine (csrc/dense.hip): forward, every layer's activation, the gradient of
sum(out * d_out) per layer and per block (dW_l, db_l) and the gradient with respect to the whole input.  Plain numpy module;
tests/test_host_dense_shapes.py pins it to torch float64 autograd, tests/test_gpu_dense_shapes.py holds the kernels to it.

Layout of the flat parameter vector = torch `parameters()` order, as in the header comment of dense.hip:
w0[d1, d0], b0[d1], w1[d2, d1], b1[d2], ...  The activation follows every layer but the last.  Its derivative is expressed
through the activation OUTPUT, as the kernel defines it (gemm_tile_dev.h: act_bwd): relu y > 0, tanh 1 - y^2, none 1.

The rows of a batch are independent, so the parameter gradient of the rows [r0, r1) alone is the gradient of that sub-batch
(`param_grad_rows`): what one gradient slab of tsm_mlp_backward must hold.
"""
from __future__ import annotations

import numpy as np

ACTS = ("relu", "tanh", "none")
KINK_MARGIN = 2e-6   # a ReLU pre-activation closer to 0 than this could land on the other side in float32
SEED_LIMIT = 20      # seeds tried by `first_kink_free`; tests/test_host_dense_shapes.py checks every relu case stays inside


def block_slices(dims) -> list:
    """[(slice of w_l, slice of b_l)] into the flat vector."""
    out, o = [], 0
    for i in range(len(dims) - 1):
        k, n = int(dims[i]), int(dims[i + 1])
        out.append((slice(o, o + n * k), slice(o + n * k, o + n * k + n)))
        o += n * k + n
    return out


def param_count(dims) -> int:
    return block_slices(dims)[-1][1].stop


def layers(flat, dims) -> list:
    """[(W [out, in], b [out])] views of a flat vector."""
    flat = np.asarray(flat)
    assert flat.shape == (param_count(dims),), (flat.shape, param_count(dims))
    return [(flat[w].reshape(int(dims[i + 1]), int(dims[i])), flat[b]) for i, (w, b) in enumerate(block_slices(dims))]


def _act(z, act):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "tanh":
        return np.tanh(z)
    assert act == "none", act
    return z


def _act_bwd(y, act):
    if act == "relu":
        return (y > 0).astype(np.float64)
    if act == "tanh":
        return 1.0 - y * y
    assert act == "none", act
    return np.ones_like(y)


def forward(dims, act, flat, x):
    """-> (pre-activations per layer, activations per layer); acts[-1] is the output (the last layer is linear)."""
    assert act in ACTS, act
    h = np.asarray(x, np.float64).reshape(-1, int(dims[0]))
    pre, acts, L = [], [], len(dims) - 1
    for i, (W, b) in enumerate(layers(np.asarray(flat, np.float64), dims)):
        z = h @ W.T + b
        h = _act(z, act) if i < L - 1 else z
        pre.append(z)
        acts.append(h)
    return pre, acts


def dense_reference(dims, act, flat_f32, x_f32, d_out_f32) -> dict:
    """float64 everything of one net on one batch: `out` [B, dims[-1]], `acts` (every layer's output), `pre` (every layer's
    pre-activation), `dW` / `db` per layer, `grad` (the same in the flat layout) and `dx` [B, dims[0]], the gradient of
    sum(out * d_out) with respect to the whole input."""
    dims = [int(d) for d in dims]
    x = np.asarray(x_f32, np.float64).reshape(-1, dims[0])
    flat = np.asarray(flat_f32, np.float64)
    pre, acts = forward(dims, act, flat, x)
    Wb = layers(flat, dims)
    L = len(dims) - 1
    dz = np.asarray(d_out_f32, np.float64).reshape(x.shape[0], dims[-1])
    dW, db = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        inp = x if l == 0 else acts[l - 1]
        dW[l], db[l] = dz.T @ inp, dz.sum(0)
        dz = dz @ Wb[l][0]
        if l > 0:
            dz = dz * _act_bwd(acts[l - 1], act)
    grad = np.concatenate([t.reshape(-1) for l in range(L) for t in (dW[l], db[l])])
    return dict(out=acts[-1], acts=acts, pre=pre, dW=dW, db=db, grad=grad, dx=dz)


def param_grad_rows(dims, act, flat_f32, x_f32, d_out_f32, r0: int, r1: int) -> np.ndarray:
    """The flat parameter gradient of the rows [r0, r1) alone (zeros for an empty range)."""
    if r1 <= r0:
        return np.zeros(param_count(dims))
    x = np.asarray(x_f32).reshape(-1, int(dims[0]))
    d_out = np.asarray(d_out_f32).reshape(x.shape[0], int(dims[-1]))
    return dense_reference(dims, act, flat_f32, x[r0:r1], d_out[r0:r1])["grad"]


def kink_distance(dims, act, flat_f32, x_f32) -> float:
    """The least |pre-activation| a ReLU sees (inf for the other activations and for one-layer nets)."""
    if act != "relu" or len(dims) < 3:
        return float("inf")
    pre, _ = forward(dims, act, flat_f32, x_f32)
    return min(float(np.abs(z).min()) for z in pre[:-1])


def first_kink_free(dims, act, make_inputs, limit: int = SEED_LIMIT):
    """-> (k, inputs): the first k in [0, limit) whose `make_inputs(k)` = (flat, x, d_out) keeps every ReLU pre-activation at
    least KINK_MARGIN from the kink, where a float32 rounding could flip the mask.  AssertionError past the limit."""
    for k in range(limit):
        inputs = make_inputs(k)
        if kink_distance(dims, act, inputs[0], inputs[1]) >= KINK_MARGIN:
            return k, inputs
    raise AssertionError(f"no seed in {limit} keeps the pre-activations of {dims} off the kink")
