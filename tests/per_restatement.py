"""Prioritized replay restated in numpy: the sum tree of tianshou/data/utils/segtree.py and the priority arithmetic of
tianshou/data/buffer/prio.py, written out element by element (no fancy-index assignment, no in-place vector updates), so that
what the kernels in csrc/segtree.hip have to reproduce is spelled out.  tests/golden/make_per_fixtures.py asserts that every
function here equals the reference on every section of tests/golden/per.npz; tests/test_host_per.py pins it to that file."""
from __future__ import annotations

import numpy as np

EPS = np.float32(np.finfo(np.float32).eps)


def bound_of(size: int) -> int:
    bound = 1
    while bound < size:
        bound *= 2
    return bound


class RestatedTree:
    """double tree[2 * bound]: leaf i at tree[bound + i], node k = tree[2k] + tree[2k + 1], tree[1] the total."""

    def __init__(self, size: int) -> None:
        self.size, self.bound = int(size), bound_of(size)
        self.tree = np.zeros(2 * self.bound, np.float64)

    def set(self, index, value) -> None:
        """`tree[index] = value`, the last of several entries with one index winning, then every ancestor of a written leaf,
        level by level: a parent is formed only once both of its children are final."""
        index = np.atleast_1d(np.asarray(index, np.int64))
        value = np.broadcast_to(np.asarray(value, np.float64), index.shape)
        assert (index >= 0).all() and (index < self.size).all()
        last = {}
        for i, leaf in enumerate(index):
            last[int(leaf)] = i
        for leaf, i in last.items():
            self.tree[self.bound + leaf] = value[i]
        nodes = {self.bound + leaf for leaf in last}
        while nodes and min(nodes) > 1:
            nodes = {k // 2 for k in nodes}
            for k in nodes:
                self.tree[k] = self.tree[2 * k] + self.tree[2 * k + 1]

    def prefix_sum_idx(self, value) -> np.ndarray:
        out = np.empty(len(value), np.int64)
        for j, v in enumerate(np.asarray(value, np.float64)):
            k = 1
            while k < self.bound:
                k *= 2
                left = self.tree[k]
                if left < v:          # strict
                    v = v - left
                    k += 1
            out[j] = k - self.bound
        return out

    def reduce(self, start: int = 0, end: int | None = None) -> float:
        if start == 0 and end is None:
            return float(self.tree[1])
        if end is None:
            end = self.size
        if end < 0:
            end += self.size
        start, end, result = start + self.bound - 1, end + self.bound, 0.0
        while end - start > 1:
            if start % 2 == 0:
                result += self.tree[start + 1]
            start //= 2
            if end % 2 == 1:
                result += self.tree[end - 1]
            end //= 2
        return float(result)


class RestatedPrio:
    """prio.py:39-90, 103-106 over a RestatedTree.  The power of update_weight is taken in float32 for float32 weights (numpy 2
    keeps `f32 ** python float` in f32) and the pair {max_prio, min_prio} holds 1.0 or float32 values."""

    def __init__(self, size: int, alpha: float, beta: float, weight_norm: bool = True) -> None:
        self.t = RestatedTree(size)
        self.alpha, self.beta, self.weight_norm = alpha, beta, weight_norm
        self.max_prio = self.min_prio = 1.0

    def init_weight(self, index) -> None:
        m = np.float32(self.max_prio)   # 1.0, or the float32 that update_weight folded in
        self.t.set(index, np.float64(m if self.alpha == 1.0 else m ** np.float32(self.alpha)))

    def update_weight(self, index, new_weight) -> None:
        w = np.abs(np.asarray(new_weight, np.float32)) + EPS
        self.t.set(index, (w if self.alpha == 1.0 else w ** np.float32(self.alpha)).astype(np.float64))
        self.max_prio = max(self.max_prio, float(w.max()))
        self.min_prio = min(self.min_prio, float(w.min()))

    def get_weight(self, index) -> np.ndarray:
        leaves = self.t.tree[self.t.bound + np.asarray(index, np.int64)]
        return (leaves / np.float64(self.min_prio)) ** (-self.beta)

    def batch_weight(self, index) -> np.ndarray:
        w = self.get_weight(index)
        return w / np.max(w) if self.weight_norm else w
