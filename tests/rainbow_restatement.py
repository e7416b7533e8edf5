"""Float64 numpy restatement of the Rainbow path (reference rainbow.py:76-101; utils/net/discrete.py:351-375;
utils/net/common.py:355-364; lagged_network.py:81-87) -- the yardstick of the Rainbow tests.  Written from the description of
what the reference computes, step by step; pinned to the reference by tests/test_host_rainbow.py against
tests/golden/rainbow.npz.

  `net_layers`            [(in, out, noisy)] of a net in `parameters()` order: model, then Q, then V
  `compose`               the effective weights W = mu_W + sigma_W * (eps_q (x) eps_p), b = mu_b + sigma_b * eps_q per layer
  `noisy_grad`            the gradient over the effective layout mapped back onto the flat layout
  `dueling_combine` / `_backward`   q - mean_a q + v per atom, and its gradient
  `RainbowNetRestatement` forward and backward of the whole net on one flat vector
  `philox_normals`        Philox4x32-10 (tests/philox_restatement.py) + Box-Muller as tsm_noisy_sample forms its normals, in float64 or float32
  `RainbowRestatement`    the full update: both draws, the lagged copy of EVERY parameter with the `_iter` rule, C51's head
                          (tests/distq_restatement.py) on the one-step successors, Adam
"""
from __future__ import annotations

import numpy as np

from distq_restatement import c51_head, support_of
from philox_restatement import philox4


def net_layers(obs_dim, hidden, A, N, q_hidden=(), v_hidden=(), dueling=True, noisy=True):
    """-> (layers [(in, out, noisy)], chains: the widths of model / Q / V)."""
    if dueling:
        chains = [[obs_dim, *hidden], [hidden[-1], *q_hidden, A * N], [hidden[-1], *v_hidden, N]]
    else:
        chains = [[obs_dim, *hidden, A * N]]
    return [(c[i], c[i + 1], bool(noisy)) for c in chains for i in range(len(c) - 1)], chains


def layer_size(i, o, z):
    return 2 * i * o + 3 * o + i if z else i * o + o


def split_flat(flat, layers):
    """Per layer {name: view} of a flat vector."""
    out, p = [], 0
    for i, o, z in layers:
        names = ([("mu_W", (o, i)), ("sigma_W", (o, i)), ("mu_bias", (o,)), ("sigma_bias", (o,)), ("eps_p", (i,)), ("eps_q", (o,))]
                 if z else [("weight", (o, i)), ("bias", (o,))])
        d = {}
        for k, shp in names:
            n = int(np.prod(shp))
            d[k] = flat[p:p + n].reshape(shp)
            p += n
        out.append(d)
    assert p == flat.size
    return out


def noise_of(flat, layers):
    return np.concatenate([v[k].reshape(-1) for v in split_flat(flat, layers) for k in ("eps_p", "eps_q") if k in v] or [np.zeros(0)])


def set_noise(flat, layers, eps):
    eps, p = np.asarray(eps, np.float64).reshape(-1), 0
    for v in split_flat(flat, layers):
        for k in ("eps_p", "eps_q"):
            if k in v:
                v[k][...] = eps[p:p + v[k].size].reshape(v[k].shape)
                p += v[k].size
    assert p == eps.size


def effective(flat, layers, training):
    """[(W, b)] per layer."""
    out = []
    for v in split_flat(np.asarray(flat, np.float64), layers):
        if "weight" in v:
            out.append((v["weight"], v["bias"]))
        elif training:
            out.append((v["mu_W"] + v["sigma_W"] * np.outer(v["eps_q"], v["eps_p"]), v["mu_bias"] + v["sigma_bias"] * v["eps_q"]))
        else:
            out.append((v["mu_W"], v["mu_bias"]))
    return out


def compose(flat, layers, training):
    """The effective vector: W then b per layer."""
    return np.concatenate([x.reshape(-1) for W, b in effective(flat, layers, training) for x in (W, b)])


def noisy_grad(flat, layers, eff_grad, training):
    """eff_grad over the effective layout -> the gradient over the flat layout (noise slots 0)."""
    flat = np.asarray(flat, np.float64)
    out = np.zeros(flat.size)
    p = 0
    for v, g in zip(split_flat(flat, layers), split_flat(out, layers)):
        (o, i) = (v["weight"] if "weight" in v else v["mu_W"]).shape
        dW, db = eff_grad[p:p + o * i].reshape(o, i), eff_grad[p + o * i:p + o * i + o]
        p += o * i + o
        if "weight" in v:
            g["weight"][...], g["bias"][...] = dW, db
        else:
            g["mu_W"][...], g["mu_bias"][...] = dW, db
            if training:
                g["sigma_W"][...], g["sigma_bias"][...] = dW * np.outer(v["eps_q"], v["eps_p"]), db * v["eps_q"]
    return out


def dueling_combine(q, v, A, N):
    q, v = np.asarray(q, np.float64).reshape(-1, A, N), np.asarray(v, np.float64).reshape(-1, 1, N)
    return (q - q.mean(1, keepdims=True) + v).reshape(-1, A * N)


def dueling_combine_backward(d, A, N):
    d = np.asarray(d, np.float64).reshape(-1, A, N)
    s = d.sum(1)
    return (d - s[:, None, :] / A).reshape(-1, A * N), s


class RainbowNetRestatement:
    def __init__(self, obs_dim, hidden, A, N, q_hidden=(), v_hidden=(), dueling=True, noisy=True):
        self.layers, self.chains = net_layers(obs_dim, hidden, A, N, q_hidden, v_hidden, dueling, noisy)
        self.A, self.N, self.dueling = A, N, dueling
        self.P = sum(layer_size(*l) for l in self.layers)
        self.n_slots = sum(i + o for i, o, z in self.layers if z)

    @staticmethod
    def _chain(ws, x, last_relu):
        """-> (out, cache [(input, pre-activation, W, relu?)])."""
        cache = []
        for k, (W, b) in enumerate(ws):
            z = x @ W.T + b
            relu = k < len(ws) - 1 or last_relu
            cache.append((x, z, W, relu))
            x = np.maximum(z, 0.0) if relu else z
        return x, cache

    @staticmethod
    def _chain_backward(cache, d):
        """-> (d input, [dW, db per layer])."""
        grads = []
        for x, z, W, relu in reversed(cache):
            if relu:
                d = d * (z > 0)
            grads.append((d.T @ x, d.sum(0)))
            d = d @ W
        return d, grads[::-1]

    def forward(self, flat, x, training):
        """-> (raw [R, A * N], cache)."""
        ws = effective(flat, self.layers, training)
        n = [len(c) - 1 for c in self.chains]
        x = np.asarray(x, np.float64)
        if not self.dueling:
            out, c0 = self._chain(ws, x, False)
            return out, dict(chains=[c0], flat=np.array(flat, np.float64), training=training)
        f, c0 = self._chain(ws[:n[0]], x, True)
        q, c1 = self._chain(ws[n[0]:n[0] + n[1]], f, False)
        v, c2 = self._chain(ws[n[0] + n[1]:], f, False)
        return dueling_combine(q, v, self.A, self.N), dict(chains=[c0, c1, c2], flat=np.array(flat, np.float64), training=training)

    def backward(self, cache, d_out):
        """-> the gradient over the flat layout."""
        d_out = np.asarray(d_out, np.float64)
        cs = cache["chains"]
        if not self.dueling:
            _, g0 = self._chain_backward(cs[0], d_out)
            gs = g0
        else:
            d_q, d_v = dueling_combine_backward(d_out, self.A, self.N)
            d_fq, g1 = self._chain_backward(cs[1], d_q)
            d_fv, g2 = self._chain_backward(cs[2], d_v)
            _, g0 = self._chain_backward(cs[0], d_fq + d_fv)
            gs = g0 + g1 + g2
        eff_grad = np.concatenate([x.reshape(-1) for dW, db in gs for x in (dW, db)])
        return noisy_grad(cache["flat"], self.layers, eff_grad, cache["training"])

    @staticmethod
    def min_relu_gap(cache) -> float:
        """The smallest |pre-activation| in front of a ReLU of a forward."""
        return min([float(np.abs(z).min()) for c in cache["chains"] for _, z, _, relu in c if relu] or [np.inf])


# ---- Philox4x32-10 + Box-Muller -----------------------------------------------------------------------------------------
NOISE_KEY = 0x52424E4F4953455F


def philox_normals(seed: int, counter: int, n: int, dtype=np.float64) -> np.ndarray:
    """The n normals behind the first n noise slots of a draw at (seed, counter): slot s is word pair (s % 4) // 2 of block
    s // 4, cosine branch for even s, sine branch for odd s."""
    w = philox4((seed ^ NOISE_KEY) & (2**64 - 1), counter, np.arange(-(-n // 4)))
    two24 = dtype(16777216.0)
    u1 = ((w[:, 0::2] >> 8).astype(dtype) + dtype(1.0)) / two24
    u2 = (w[:, 1::2] >> 8).astype(dtype) / two24
    r = np.sqrt(dtype(-2.0) * np.log(u1))
    t = dtype(2.0 * np.pi) * u2
    z = np.stack([r * np.cos(t), r * np.sin(t)], 2)      # [blocks, pair, branch]
    return z.reshape(-1)[:n].astype(dtype)


def noisy_f(x):
    return np.sign(x) * np.sqrt(np.abs(x))


# ---- the full update -------------------------------------------------------------------------------------------------------
class RainbowRestatement:
    """RainbowDQN around a `RainbowNetRestatement`: flat vectors of the online and the lagged net, torch's Adam in numpy."""

    def __init__(self, init, net: RainbowNetRestatement, lr=1e-3, target_update_freq=0, v_min=-10.0, v_max=10.0):
        self.net, self.lr, self.freq = net, lr, int(target_update_freq)
        self.flat = np.array(init, np.float64)
        self.target = self.flat.copy() if self.freq > 0 else None
        self.m, self.v, self.t = np.zeros(net.P), np.zeros(net.P), 0
        self.v_min, self.v_max = float(v_min), float(v_max)
        self.support = support_of(v_min, v_max, net.N)
        self._iter = 0
        self.training = True

    def weights(self):
        return self.flat.copy()

    def targets(self):
        return self.target.copy()

    def adam_cond(self):
        return self.lr / (np.sqrt(self.v / (1.0 - 0.999 ** self.t)) + 1e-8)

    def update(self, obs, act, obs_next, mask_next, mc, gpow, vmask, weight=None, eps_online=None, eps_target=None) -> dict:
        """`obs_next`: the one-step successors of the sampled rows (C51's quirk).  eps_*: the draws of this update (None:
        a net without noise)."""
        L = self.net.layers
        if eps_online is not None:
            set_noise(self.flat, L, eps_online)
        if self.freq > 0 and eps_target is not None:
            set_noise(self.target, L, eps_target)
        if self.freq > 0 and self._iter % self.freq == 0:
            self.target[...] = self.flat          # every parameter, the noise included
        self._iter += 1
        on, c_on = self.net.forward(self.flat, obs_next, self.training)
        gap = self.net.min_relu_gap(c_on)
        tg = None
        if self.freq > 0:
            tg, c_tg = self.net.forward(self.target, obs_next, self.training)
            gap = min(gap, self.net.min_relu_gap(c_tg))
        raw, cache = self.net.forward(self.flat, obs, self.training)
        gap = min(gap, self.net.min_relu_gap(cache))
        h = c51_head(raw, on, tg, mask_next, act, mc, gpow, vmask, weight, self.support, self.v_min, self.v_max, self.net.A,
                     self.net.N)
        g = self.net.backward(cache, h["d_out"])
        h["grads"], h["relu_gap"] = g, gap
        self.t += 1
        self.m = 0.9 * self.m + (1 - 0.9) * g
        self.v = 0.999 * self.v + (1 - 0.999) * g * g
        denom = np.sqrt(self.v) / np.sqrt(1 - 0.999 ** self.t) + 1e-8
        self.flat = self.flat - (self.lr / (1 - 0.9 ** self.t)) * (self.m / denom)
        return h
