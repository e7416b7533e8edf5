"""Float64 numpy restatement of the BDQN path (reference bdqn.py:76-103, 155-224; BranchingNet, utils/net/common.py:557-678) --
the yardstick of the BDQN tests.  Written from the reference's description of what it computes; pinned to the reference's own
float64 run by tests/test_host_bdqn.py against tests/golden/bdqn.npz.  Nothing here calls the library.

  `BranchingNetRestatement`  forward / backward of the net on the project's flat layout [common | value | branches]: common and
                             value as `FlatMLP` (per layer W [out, in], b [out]), the K branches grouped (per layer W [K, in, out],
                             b [K, 1, out])
  `head`                     the branch-mean target, the return with its end-flag rule, the masked TD loss, d loss / d logits and,
                             through the combine's backward, d_adv [K, B, A] and d_v [B]
  `BdqnRestatement`          three-call learner: lagged copy by the `_iter` rule, Adam
  `bdqn_egreedy`             the device draw, over tests/philox_restatement.py
  `flat_from_reference` / `reference_from_flat`   the reference's per-parameter arrays (`parameters()` order, nn.Linear's
                             [out, in]) <-> the flat layout
"""
from __future__ import annotations

import numpy as np

from philox_restatement import philox4, u01
from sampling_restatement import counters, own


# ---- layout ------------------------------------------------------------------------------------------------------------------
def chains(D, common_hidden, value_hidden, action_hidden, A):
    H = common_hidden[-1]
    return [int(D), *common_hidden], [H, *value_hidden, 1], [H, *action_hidden, int(A)]


def mlp_split(flat, dims):
    """FlatMLP layout -> [(W [out, in], b [out])]."""
    out, o = [], 0
    for i in range(len(dims) - 1):
        k, n = dims[i], dims[i + 1]
        out.append((flat[o:o + n * k].reshape(n, k), flat[o + n * k:o + n * k + n]))
        o += n * k + n
    assert o == flat.size
    return out


def ens_split(flat, dims, K):
    """EnsembleLinear layout -> [(W [K, in, out], b [K, 1, out])]."""
    out, o = [], 0
    for i in range(len(dims) - 1):
        k, n = dims[i], dims[i + 1]
        out.append((flat[o:o + K * k * n].reshape(K, k, n), flat[o + K * k * n:o + K * (k * n + n)].reshape(K, 1, n)))
        o += K * (k * n + n)
    assert o == flat.size
    return out


def sizes(ch, K):
    n = lambda d: sum(d[i] * d[i + 1] + d[i + 1] for i in range(len(d) - 1))  # noqa: E731
    return n(ch[0]), n(ch[1]), K * n(ch[2])


def reference_shapes(ch, K):
    """The reference's parameter shapes in `parameters()` order: common, value, then branch by branch."""
    lin = lambda d: [s for i in range(len(d) - 1) for s in ((d[i + 1], d[i]), (d[i + 1],))]  # noqa: E731
    return lin(ch[0]) + lin(ch[1]) + lin(ch[2]) * K


def flat_from_reference(arrays, ch, K):
    arrays = [np.asarray(a, np.float64) for a in arrays]
    assert [a.shape for a in arrays] == reference_shapes(ch, K)
    n_c, n_v = 2 * (len(ch[0]) - 1), 2 * (len(ch[1]) - 1)
    L = len(ch[2]) - 1
    br = arrays[n_c + n_v:]
    parts = [a.reshape(-1) for a in arrays[:n_c + n_v]]
    for i in range(L):
        parts.append(np.stack([br[2 * L * k + 2 * i].T for k in range(K)]).reshape(-1))       # [K, in, out]
        parts.append(np.stack([br[2 * L * k + 2 * i + 1] for k in range(K)]).reshape(-1))     # [K, 1, out]
    return np.concatenate(parts)


def reference_from_flat(flat, ch, K):
    flat = np.asarray(flat, np.float64)
    n0, n1, _ = sizes(ch, K)
    out = [t for W, b in mlp_split(flat[:n0], ch[0]) + mlp_split(flat[n0:n0 + n1], ch[1]) for t in (W, b)]
    layers = ens_split(flat[n0 + n1:], ch[2], K)
    for k in range(K):
        for W, b in layers:
            out += [W[k].T, b[k, 0]]
    return out


# ---- the net -----------------------------------------------------------------------------------------------------------------
def _fwd(layers, x, grouped_k=None):
    hs, zs = [x], []
    for i, (W, b) in enumerate(layers):
        z = hs[-1] @ W.T + b if grouped_k is None else hs[-1] @ W[grouped_k] + b[grouped_k]
        zs.append(z)
        hs.append(np.maximum(z, 0.0) if i < len(layers) - 1 else z)
    return hs, zs


def _bwd(layers, hs, zs, d, grouped_k=None):
    grads = []
    for i in reversed(range(len(layers))):
        if i < len(layers) - 1:
            d = d * (zs[i] > 0)
        W = layers[i][0]
        grads.append((d.T @ hs[i] if grouped_k is None else hs[i].T @ d, d.sum(0)))
        d = d @ W if grouped_k is None else d @ W[grouped_k].T
    return grads[::-1], d


class BranchingNetRestatement:
    def __init__(self, flat, ch, K) -> None:
        self.ch, self.K, self.A = ch, int(K), ch[2][-1]
        self.n = sizes(ch, K)
        self.flat = np.array(flat, np.float64)
        assert self.flat.size == sum(self.n)
        self.kink = np.inf

    def parts(self):
        n0, n1, _ = self.n
        return (mlp_split(self.flat[:n0], self.ch[0]), mlp_split(self.flat[n0:n0 + n1], self.ch[1]),
                ens_split(self.flat[n0 + n1:], self.ch[2], self.K))

    def forward(self, x):
        """x [B, D] -> (logits [B, K, A], cache).  `kink` takes the smallest |ReLU pre-activation| seen."""
        x = np.asarray(x, np.float64)
        com, val, br = self.parts()
        ch, cz = _fwd(com, x)
        f = np.maximum(cz[-1], 0.0)   # the reference's common MLP ends in its activation
        vh, vz = _fwd(val, f)
        bs = [_fwd(br, f, k) for k in range(self.K)]
        adv = np.stack([h[-1] for h, _ in bs], 1)                      # [B, K, A]
        q = vh[-1][:, None, :] + (adv - adv.mean(2, keepdims=True))
        pre = cz + vz[:-1] + [z for _, zs in bs for z in zs[:-1]]
        self.kink = min([self.kink] + [float(np.abs(z).min()) for z in pre if z.size])
        return q, dict(ch=ch, cz=cz, f=f, vh=vh, vz=vz, bs=bs, adv=adv, v=vh[-1][:, 0])

    @staticmethod
    def combine_backward(d_q):
        """d loss / d logits [B, K, A] -> (d_adv [K, B, A], d_v [B])."""
        return (d_q - d_q.mean(2, keepdims=True)).transpose(1, 0, 2), d_q.sum((1, 2))

    def backward(self, cache, d_adv, d_v):
        """-> the gradient on the flat layout."""
        com, val, br = self.parts()
        gv, d_f = _bwd(val, cache["vh"], cache["vz"], np.asarray(d_v, np.float64).reshape(-1, 1))
        gb = []
        for k in range(self.K):
            g, d = _bwd(br, *cache["bs"][k], np.asarray(d_adv[k], np.float64), k)
            gb.append(g)
            d_f = d_f + d
        d_z = d_f * (cache["cz"][-1] > 0)
        hs, zs = cache["ch"], cache["cz"]
        gc, _ = _bwd(com, hs, zs, d_z)
        parts = [t.reshape(-1) for g in gc + gv for t in g]
        for i in range(len(br)):
            parts.append(np.stack([gb[k][i][0] for k in range(self.K)]).reshape(-1))
            parts.append(np.stack([gb[k][i][1] for k in range(self.K)]).reshape(-1))
        return np.concatenate(parts)


# ---- the head ----------------------------------------------------------------------------------------------------------------
def argmax_gap(x) -> float:
    """The smallest top-2 gap over the last axis (inf for one entry)."""
    x = np.asarray(x, np.float64)
    if x.shape[-1] < 2:
        return np.inf
    s = np.sort(x, -1)
    return float((s[..., -1] - s[..., -2]).min())


def head(q, qn_on, qn_tg, act, rew, end, gamma, weight=None, is_double=True):
    """q, qn_on [B, K, A]; qn_tg or None (the online values are the target values); act int [B, K]; rew [B]; end bool [B].
    -> dict(returns, prio, loss, q_taken, d_q [B, K, A], d_adv [K, B, A], d_v [B], gap)."""
    q, on = np.asarray(q, np.float64), np.asarray(qn_on, np.float64)
    tg = on if qn_tg is None else np.asarray(qn_tg, np.float64)
    B, K, A = q.shape
    act = np.asarray(act, np.int64).reshape(B, K)
    sel = on if is_double else tg
    a_star = sel.argmax(-1)                                                # first maximum
    tq = np.take_along_axis(tg, a_star[..., None], -1)[..., 0].mean(-1)    # mean over the branches
    returns = np.asarray(rew, np.float64) + gamma * tq * (1.0 - np.asarray(end, bool))
    taken = np.take_along_axis(q, act[..., None], -1)[..., 0]              # [B, K]
    td = returns[:, None] - taken
    w = np.ones(B) if weight is None else np.asarray(weight, np.float64)
    loss = float(((td ** 2).mean(-1) * w).mean())
    g = -2.0 * w[:, None] * td / (K * B)
    d_q = np.zeros_like(q)
    np.put_along_axis(d_q, act[..., None], g[..., None], -1)
    d_adv, d_v = BranchingNetRestatement.combine_backward(d_q)
    return dict(returns=returns, prio=td.sum(-1), loss=loss, q_taken=float(taken.mean()), d_q=d_q, d_adv=d_adv, d_v=d_v,
                gap=argmax_gap(sel))


# ---- the learner -------------------------------------------------------------------------------------------------------------
class BdqnRestatement:
    def __init__(self, flat, ch, K, gamma, lr=1e-3, target_update_freq=0, is_double=True, betas=(0.9, 0.999), eps=1e-8) -> None:
        self.net = BranchingNetRestatement(flat, ch, K)
        self.freq, self.is_double, self.gamma = int(target_update_freq), bool(is_double), float(gamma)
        self.old = BranchingNetRestatement(flat, ch, K) if self.freq > 0 else None
        self.lr, self.betas, self.eps = lr, betas, eps
        self.m, self.v, self.t, self._iter = np.zeros_like(self.net.flat), np.zeros_like(self.net.flat), 0, 0
        self.gap = np.inf

    @property
    def kink(self) -> float:
        return min(self.net.kink, self.old.kink if self.old is not None else np.inf, self.gap)

    def update(self, obs, act, obs_next, rew, end, weight=None) -> dict:
        """One `_preprocess_batch` + `_update_with_batch`: the target values with the weights as they are, then the `_iter`
        rule's copy, then the loss, its gradient and one Adam step."""
        on, _ = self.net.forward(obs_next)
        tg = self.old.forward(obs_next)[0] if self.old is not None else None
        if self.old is not None and self._iter % self.freq == 0:
            self.old.flat[:] = self.net.flat
        self._iter += 1
        q, cache = self.net.forward(obs)
        h = head(q, on, tg, act, rew, end, self.gamma, weight, self.is_double)
        self.gap = min(self.gap, h["gap"])
        h["q"], h["grads"] = q, self.net.backward(cache, h["d_adv"], h["d_v"])
        self.t += 1
        b1, b2 = self.betas
        self.m = b1 * self.m + (1 - b1) * h["grads"]
        self.v = b2 * self.v + (1 - b2) * h["grads"] ** 2
        self.net.flat -= self.lr / (1 - b1 ** self.t) * self.m / (np.sqrt(self.v) / np.sqrt(1 - b2 ** self.t) + self.eps)
        return h


# ---- acting ------------------------------------------------------------------------------------------------------------------
def bdqn_egreedy(q, eps, seed: int, offset: int = 0, offset_dev=None):
    """Row r at counter c + r: random where u01(word 0 of sub 0) < eps in float32; then branch k takes
    (word k % 4 of sub 1 + k / 4) * A >> 32; else the first maximum of every branch.
    -> (dict(act i32 [R, K], random [R]), the (key, counter, sub, word) the call owns)."""
    q = np.asarray(q, np.float32)
    R, K, A = q.shape
    ctr = counters(offset, offset_dev, np.arange(R))
    subs = np.arange(1 + (K + 3) // 4)
    w = philox4(seed, ctr[:, None], subs[None, :])                     # [R, subs, 4]
    coin = u01(w[:, 0, 0], np.float32) < np.float32(eps)
    rand = (w[:, 1:, :].reshape(R, -1)[:, :K].astype(np.uint64) * np.uint64(A)) >> np.uint64(32)
    act = np.where(coin[:, None], rand.astype(np.int64), q.argmax(-1)).astype(np.int32)
    used = own(seed, ctr, 0, (0,))
    for k in range(K):
        used |= own(seed, ctr, 1 + k // 4, (k % 4,))
    return dict(act=act, random=coin), used
