"""Philox4x32-10 restated in numpy (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the
generator behind every device draw of the project (csrc/philox.h).  Nothing here calls the library.

  `philox4x32_10`   the general function on counter words [..., 4] and key words [..., 2]; tests/test_host_sampling.py pins it
                    to the three Random123 known-answer vectors
  `philox4`         the project's use of it: counter words (low, high) of a 64-bit counter, `sub`, 0; key = (low, high) of the seed
  `u01`             the 24-bit uniform in [0, 1): (w >> 8) / 2^24 -- exact in float32 and in float64
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
MUL0, MUL1 = 0xD2511F53, 0xCD9E8D57          # the multipliers of counter words 0 and 2
WEYL0, WEYL1 = 0x9E3779B9, 0xBB67AE85        # the key schedule: added to key words 0 and 1 after every round
ROUNDS = 10


def philox4x32_10(counter_words, key_words) -> np.ndarray:
    """counter_words u32 [..., 4], key_words u32 [..., 2] (leading axes broadcast) -> u32 [..., 4].
    One round: (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); then the key moves on."""
    c = np.asarray(counter_words, np.uint64)
    k = np.asarray(key_words, np.uint64)
    assert c.shape[-1] == 4 and k.shape[-1] == 2
    assert (c <= M32).all() and (k <= M32).all(), "words are 32 bits"
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j], lead).copy() for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j], lead).copy() for j in range(2))
    m32, s32 = np.uint64(M32), np.uint64(32)
    for _ in range(ROUNDS):
        p0, p1 = np.uint64(MUL0) * c0, np.uint64(MUL1) * c2           # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(WEYL0)) & m32, (k1 + np.uint64(WEYL1)) & m32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def as_u64(x) -> np.ndarray:
    """Python ints (of any size) or an integer array -> uint64, reduced mod 2^64 as the kernels' uint64_t arithmetic is."""
    a = np.asarray(x)
    if a.dtype == object or a.dtype.kind not in "iu":
        a = np.asarray(x, dtype=object)
        return np.array([int(v) & M64 for v in a.reshape(-1)], np.uint64).reshape(a.shape)
    return a.astype(np.uint64)      # two's complement: a negative int64 is its value mod 2^64


def philox4(seed: int, counter, sub) -> np.ndarray:
    """-> u32 [broadcast(counter, sub), 4]: the four words of block (counter, sub) under the key `seed`.  `counter` and `sub`
    may be arrays; a caller forms `counter + i` in Python ints or uint64, so its carry into the high word is not lost."""
    counter, sub = as_u64(counter), as_u64(sub)
    assert (sub <= M32).all()
    shape = np.broadcast_shapes(counter.shape, sub.shape)
    counter, sub = np.broadcast_to(counter, shape), np.broadcast_to(sub, shape)
    cw = np.stack([counter & np.uint64(M32), counter >> np.uint64(32), sub, np.zeros(shape, np.uint64)], -1)
    seed = int(seed) & M64
    return philox4x32_10(cw, np.array([seed & M32, seed >> 32], np.uint64))


def u01(words, dtype=np.float64) -> np.ndarray:
    """(w >> 8) / 2^24 in [0, 1 - 2^-24]."""
    return (np.asarray(words, np.uint32) >> np.uint32(8)).astype(dtype) / dtype(16777216.0)
