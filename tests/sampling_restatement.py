"""Every device sampling site restated in numpy from the comments of its kernel, over tests/philox_restatement.py.  Nothing here
calls the library.  One function per site, with the arguments of its `ops` entry point (a device counter is passed as its value);
each returns (what the site draws, `used`): `used` is the set of (key, counter, sub, word) the site OWNS at those arguments -- every
word it may read, whether or not this call's data made it read it.  `blocks_of(used)` drops the word.

  site                        key             block                                   words
  categorical_sample          seed            counter offset + row                    0: u = u01 * s, first j with u < cumsum exp(l - max)
  random_permutations         seed            counter ctr + p                         0..3 key a 6-round Feistel on 2 hb bits, cycle walking
  per_sample                  seed            counter offset + i                      0, 1: u = (w0 << 20 | w1 >> 12) / 2^52
  dqn_egreedy                 seed            counter c + r, sub 0                    0: the coin
                                              counter c + r, sub 1 + a / 4            a % 4: uniform[a]
  qmix_egreedy                seed            counter c + i                           1: agent i's coin, shared by all rows
                                              counter c + b N + i                     0: (w0 A) >> 32
  iqn_taus                    seed ^ TAU_KEY  counter c + r, sub s / 4                s % 4
  maddpg_act                  seed            counter c + idx                         0, 1: Box-Muller, cosine branch
  cac_normal                  seed ^ NORMAL_KEY  one counter, sub = element / 4       pairs (0, 1), (2, 3): cosine for even, sine for odd
  mpe_reset                   seed            (episode n_env + e) 8 + i               0, 1: agent xy; 2, 3: landmark xy
  mpe_tag_reset / _lanes      seed            (episode n_env + e) 16 + entity         0, 1: xy
"""
from __future__ import annotations

import numpy as np

from per_restatement import RestatedTree
from philox_restatement import M32, M64, philox4, u01

TAU_KEY = 0x5355415451495F4E        # csrc/iqn.hip kTauKey
NORMAL_KEY = 0x4341434E4F524D4C     # csrc/cac.hip kNormalKey


# ---- counters and ownership --------------------------------------------------------------------------------------------------
def dev_value(offset_dev) -> int:
    """The value behind a device counter: None (no counter) is 0."""
    return 0 if offset_dev is None else int(np.asarray(offset_dev).reshape(-1)[0]) & M64


def counters(offset: int, offset_dev, idx) -> np.ndarray:
    """offset + *offset_dev + idx in 64 bits, as the kernels' uint64_t sum: the carry of `+ idx` reaches the high word."""
    base = np.uint64((int(offset) + dev_value(offset_dev)) & M64)
    with np.errstate(over="ignore"):
        return base + np.asarray(idx).astype(np.uint64)


def own(key: int, ctrs, subs, words) -> set:
    """{(key, counter, sub, word)} for every counter x sub x word."""
    key = int(key) & M64
    return {(key, int(c), int(s), int(w)) for c in np.asarray(ctrs).reshape(-1) for s in np.atleast_1d(subs) for w in words}


def blocks_of(used: set) -> set:
    return {(k, c, s) for k, c, s, _ in used}


# ---- categorical -------------------------------------------------------------------------------------------------------------
def categorical_sample(logits, seed: int, offset: int = 0, deterministic: bool = False, offset_dev=None):
    """Row i: u = u01(word 0 at counter offset + i) * s, s = sum_j exp(l_j - max l); act = the first j with u < c_j, c the running
    sum, else A - 1; logp = l[act] - (max + log s).  All in float64.  `ambiguous` marks the rows in which u lies within
    8 A 2^-24 s of some c_j: there a float32 running sum may fall on the other side of u."""
    lg = np.asarray(logits, np.float64)
    B, A = lg.shape
    ctr = counters(offset, offset_dev, np.arange(B))
    m = lg.max(1, keepdims=True)
    e = np.exp(lg - m)
    s = e.sum(1)
    if deterministic:
        act = lg.argmax(1)
        amb = np.zeros(B, bool)
        u = np.zeros(B)
    else:
        u = u01(philox4(seed, ctr, 0)[:, 0]) * s
        c = np.cumsum(e, 1)
        below = u[:, None] < c
        act = np.where(below.any(1), below.argmax(1), A - 1)
        amb = (np.abs(u[:, None] - c) <= (8.0 * A * 2.0 ** -24 * s)[:, None]).any(1)
    logp = lg[np.arange(B), act] - (m[:, 0] + np.log(s))
    return dict(act=act.astype(np.int32), logp=logp, ambiguous=amb, u=u), own(seed, ctr, 0, (0,))


# ---- permutations ------------------------------------------------------------------------------------------------------------
def _mix32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def half_bits(n: int) -> int:
    """Half the width of the smallest even-width power-of-two domain >= n (at least 2 bits)."""
    bits = 0
    while (1 << bits) < n:
        bits += 1
    return 1 if bits < 2 else (bits + 1) // 2


def feistel_perm(n: int, key4) -> np.ndarray:
    """pi(i) for i in [0, n): a balanced 6-round Feistel network on 2 hb bits -- (l, r) <- (r, l ^ (mix32(r + key[round % 4] +
    0x9E3779B9 (round + 1)) & mask)) -- applied again while the image is >= n."""
    hb = half_bits(n)
    mask, hbu, m32 = np.uint64((1 << hb) - 1), np.uint64(hb), np.uint64(M32)
    k = [np.uint64(int(v)) for v in key4]
    x = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, bool)
    while todo.any():
        v = x[todo]
        l, r = v >> hbu, v & mask
        for rnd in range(6):
            f = _mix32((r + k[rnd & 3] + np.uint64((0x9E3779B9 * (rnd + 1)) & M32)) & m32) & mask
            l, r = r, l ^ f
        x[todo] = (l << hbu) | r
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


def random_permutations(n: int, n_perm: int, seed: int, counter: int = 0, counter_dev=None, scale: int = 1, group_size: int = 1,
                        offset_mul: int = 0):
    """out[p, i] = pi_p(i) * scale + (p // group_size) * offset_mul, pi_p keyed by the four words at counter ctr + p.  The
    `advance` form of the entry point draws the same numbers (and then adds to the device counter)."""
    ctr = counters(counter, counter_dev, np.arange(n_perm))
    keys = philox4(seed, ctr, 0)
    out = np.empty((n_perm, n), np.int64)
    for p in range(n_perm):
        out[p] = feistel_perm(n, keys[p]) * scale + (p // group_size) * offset_mul
    return out, own(seed, ctr, 0, range(4))


# ---- prioritized replay ------------------------------------------------------------------------------------------------------
def per_sample(tree, size: int, n: int, seed: int, offset: int = 0, offset_dev=None):
    """`tree`: the f64 [2 bound] sum tree.  Draw i: u = (w0 << 20 | w1 >> 12) / 2^52 at counter offset + i, then the reference's
    descent (tests/per_restatement.py) with the one float64 product u * tree[1]."""
    ctr = counters(offset, offset_dev, np.arange(n))
    w = philox4(seed, ctr, 0).astype(np.uint64)
    k = (w[:, 0] << np.uint64(20)) | (w[:, 1] >> np.uint64(12))
    u = k.astype(np.float64) * (1.0 / 4503599627370496.0)        # k < 2^52: exact
    t = RestatedTree(size)
    tree = np.asarray(tree, np.float64)
    assert tree.shape == t.tree.shape
    t.tree = tree
    return dict(index=t.prefix_sum_idx(u * tree[1]), u=u), own(seed, ctr, 0, (0, 1))


# ---- epsilon-greedy ----------------------------------------------------------------------------------------------------------
def dqn_random_action(uniform, mask_row) -> int:
    """(uniform[A] + mask).argmax() in float32, the first maximum."""
    v = np.asarray(uniform, np.float32) + (np.zeros(len(uniform), np.float32) if mask_row is None
                                           else (np.asarray(mask_row) != 0).astype(np.float32))
    return int(np.argmax(v))


def dqn_greedy_action(row, mask_row) -> int:
    """The first best legal entry; of a row without a legal entry, the first maximum of the raw row."""
    row = np.asarray(row, np.float32)
    legal = np.ones(len(row), bool) if mask_row is None else np.asarray(mask_row) != 0
    if not legal.any():
        return int(np.argmax(row))
    return int(np.flatnonzero(legal)[np.argmax(row[legal])])


def dqn_egreedy(q, eps, seed: int, offset: int = 0, offset_dev=None, mask=None):
    """Row r at counter c + r: random where u01(word 0 of sub 0) < eps, with uniform[a] = u01(word a % 4 of sub 1 + a / 4)."""
    q = np.asarray(q, np.float32)
    R, A = q.shape
    eps = np.float32(eps)
    ctr = counters(offset, offset_dev, np.arange(R))
    subs = np.arange(1 + (A + 3) // 4)
    w = philox4(seed, ctr[:, None], subs[None, :])                # [R, subs, 4]
    coin = u01(w[:, 0, 0], np.float32) < eps
    uni = u01(w[:, 1:, :].reshape(R, -1)[:, :A], np.float32)
    act = np.array([dqn_random_action(uni[r], None if mask is None else mask[r]) if coin[r]
                    else dqn_greedy_action(q[r], None if mask is None else mask[r]) for r in range(R)], np.int32)
    used = own(seed, ctr, 0, (0,))
    for a in range(A):
        used |= own(seed, ctr, 1 + a // 4, (a % 4,))
    return dict(act=act, random=coin, uniform=uni), used


def qmix_egreedy(q, eps, seed: int, offset: int = 0, offset_dev=None):
    """q: per agent [B, A].  Agent i's coin: word 1 at counter c + i, one for the call; where it says random, row b takes
    (word 0 at counter c + b N + i) * A >> 32; else the first maximum."""
    N = len(q)
    q = [np.asarray(x, np.float32) for x in q]
    B, A = q[0].shape
    eps = np.float32(eps)
    c_coin = counters(offset, offset_dev, np.arange(N))
    coin = u01(philox4(seed, c_coin, 0)[:, 1], np.float32) < eps
    c_act = counters(offset, offset_dev, np.arange(B * N)).reshape(B, N)
    rnd = (philox4(seed, c_act, 0)[..., 0].astype(np.uint64) * np.uint64(A)) >> np.uint64(32)
    greedy = np.stack([x.argmax(1) for x in q], 1)
    act = np.where(coin[None, :], rnd.astype(np.int64), greedy).astype(np.int32)
    return dict(act=act, random=coin, uniform_action=rnd.astype(np.int32)), own(seed, c_coin, 0, (1,)) | own(seed, c_act, 0, (0,))


# ---- IQN ---------------------------------------------------------------------------------------------------------------------
def iqn_taus(R: int, sample_size: int, seed: int, offset: int = 0, offset_dev=None):
    """taus[r, s] = u01(word s % 4 of block (counter c + r, sub s / 4)) under the key seed ^ TAU_KEY; float32, exact."""
    S = int(sample_size)
    key = (int(seed) ^ TAU_KEY) & M64
    ctr = counters(offset, offset_dev, np.arange(R))
    subs = np.arange((S + 3) // 4)
    w = philox4(key, ctr[:, None], subs[None, :])
    taus = u01(w.reshape(R, -1)[:, :S], np.float32)
    used = set()
    for s in range(S):
        used |= own(key, ctr, s // 4, (s % 4,))
    return taus, used


# ---- normals -----------------------------------------------------------------------------------------------------------------
def maddpg_act(mu, sigma, seed: int, offset: int = 0, offset_dev=None, low=None, high=None, dtype=np.float64):
    """mu: per agent [E, Ad] -> out [E N, Ad], row e N + i.  Element idx (row-major) at counter c + idx:
    z = sqrt(-2 log(1 - u01(w0))) cos(2 pi u01(w1)); out = mu + sigma z, clamped to [low, high].  sigma == 0 draws nothing."""
    N = len(mu)
    mu = np.stack([np.asarray(m, dtype) for m in mu], 1)                       # [E, N, Ad]
    E, _, Ad = mu.shape
    out = mu.reshape(E * N, Ad).copy()
    ctr = counters(offset, offset_dev, np.arange(E * N * Ad))
    sigma = dtype(sigma)
    if sigma != 0:
        w = philox4(seed, ctr, 0)
        u1 = dtype(1.0) - u01(w[:, 0], dtype)                                    # (0, 1]
        z = np.sqrt(dtype(-2.0) * np.log(u1)) * np.cos(dtype(6.28318530717958647692) * u01(w[:, 1], dtype))
        out = out + sigma * z.reshape(E * N, Ad).astype(dtype)
    if low is not None:
        out = np.minimum(np.maximum(out, np.asarray(low, dtype)[None, :]), np.asarray(high, dtype)[None, :])
    return out.astype(dtype), own(seed, ctr, 0, (0, 1))


def cac_normal(n: int, seed: int, offset: int = 0, offset_dev=None, dtype=np.float64):
    """Element j of the draw: word pair ((j % 4) / 2) of block (the ONE counter offset, sub j / 4) under the key seed ^ NORMAL_KEY;
    u1 = ((w >> 8) + 1) / 2^24 in (0, 1], u2 = u01; r cos(2 pi u2) for even j, r sin(2 pi u2) for odd j, r = sqrt(-2 log u1)."""
    key = (int(seed) ^ NORMAL_KEY) & M64
    ctr = counters(offset, offset_dev, np.zeros(1, np.int64))
    subs = np.arange((int(n) + 3) // 4)
    w = philox4(key, ctr[0], subs)
    u1 = ((w[:, 0::2] >> np.uint32(8)).astype(dtype) + dtype(1.0)) / dtype(16777216.0)
    t = dtype(6.28318530717958647692) * u01(w[:, 1::2], dtype)
    r = np.sqrt(dtype(-2.0) * np.log(u1))
    z = np.stack([r * np.cos(t), r * np.sin(t)], 2).reshape(-1)[:int(n)].astype(dtype)
    used = set()
    for j in range(int(n)):
        used |= own(key, ctr, j // 4, (2 * ((j % 4) // 2), 2 * ((j % 4) // 2) + 1))
    return z, used


# ---- the environments --------------------------------------------------------------------------------------------------------
def mpe_reset(seed: int, n_env: int, N: int, episode):
    """simple_spread: agent / landmark i of env e at counter (episode[e] n_env + e) 8 + i: agent xy = words 0, 1, landmark xy =
    words 2, 3, each u01 * 2 - 1 (exact in float32).  `episode`: the per-env episode number, an int or [n_env]."""
    ep = np.broadcast_to(np.asarray(episode, np.uint64), (n_env,))
    with np.errstate(over="ignore"):
        ctr = ((ep * np.uint64(n_env) + np.arange(n_env, dtype=np.uint64)) * np.uint64(8))[:, None] + np.arange(N, dtype=np.uint64)
    x = u01(philox4(seed, ctr, 0), np.float32) * np.float32(2.0) - np.float32(1.0)       # [E, N, 4]
    return dict(agent_pos=x[..., 0:2], landmark_pos=x[..., 2:4]), own(seed, ctr, 0, range(4))


def _tag_xy(seed, ctr, is_agent):
    """lo + (hi - lo) u in float64, lo / hi the float32 constants of the kernel: (-1, 1) for agents, (-0.9, 0.9) for obstacles."""
    hi = np.where(is_agent, 1.0, np.float64(np.float32(0.9)))
    u = u01(philox4(seed, ctr, 0)[..., 0:2])
    return -hi[..., None] + (2.0 * hi)[..., None] * u


def mpe_tag_reset(seed: int, n_env: int, n_adv: int, n_good: int, n_obst: int, episode):
    """simple_tag: entity i of env e (agents first, then obstacles) at counter (episode[e] n_env + e) 16 + i, xy = words 0, 1."""
    NA, NE = n_adv + n_good, n_adv + n_good + n_obst
    ep = np.broadcast_to(np.asarray(episode, np.uint64), (n_env,))
    with np.errstate(over="ignore"):
        ctr = ((ep * np.uint64(n_env) + np.arange(n_env, dtype=np.uint64)) * np.uint64(16))[:, None] + np.arange(NE, dtype=np.uint64)
    xy = _tag_xy(seed, ctr, np.broadcast_to(np.arange(NE) < NA, ctr.shape))
    return dict(agent_pos=xy[:, :NA], obstacle_pos=xy[:, NA:]), own(seed, ctr, 0, (0, 1))


def mpe_tag_reset_lanes(seed: int, n_env: int, n_adv: int, n_good: int, n_obst: int, episode):
    """The auto-reset of a finished env by its agent lanes: lane i draws agent i, then obstacles i, i + NA, i + 2 NA, ...; the
    counters are mpe_tag_reset's.  -> (positions, used, drawn): drawn[i] = the entities lane i draws."""
    NA = n_adv + n_good
    ep = np.broadcast_to(np.asarray(episode, np.uint64), (n_env,))
    with np.errstate(over="ignore"):
        base = (ep * np.uint64(n_env) + np.arange(n_env, dtype=np.uint64)) * np.uint64(16)
    ap, lp = np.full((n_env, NA, 2), np.nan), np.full((n_env, n_obst, 2), np.nan)
    used, drawn = set(), {}
    for i in range(NA):
        drawn[i] = [i]
        ap[:, i] = _tag_xy(seed, base + np.uint64(i), np.ones(n_env, bool))
        used |= own(seed, base + np.uint64(i), 0, (0, 1))
        for l in range(i, n_obst, NA):
            drawn[i].append(NA + l)
            lp[:, l] = _tag_xy(seed, base + np.uint64(NA + l), np.zeros(n_env, bool))
            used |= own(seed, base + np.uint64(NA + l), 0, (0, 1))
    return dict(agent_pos=ap, obstacle_pos=lp), used, drawn
