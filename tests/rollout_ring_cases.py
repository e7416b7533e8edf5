"""What a vector replay buffer whose sub-buffers are rings of S slots must hold after a run, stated in plain numpy from the run's
time-ordered truth: per-step rows `[T][n_env]...` of a stored field, the per-step done flags `[T][n_env]` and float32 rewards
`[T][n_env][N]`.  tests/test_gpu_rollout_ring.py takes the truth from a collect into a buffer large enough never to wrap and holds the
wrapped collects -- unfused adds and the persistent rollouts alike -- to these answers; tests/test_host_rollout_ring.py checks the
answers themselves against tests/golden/vrb_trace.npz and a hand-written trace.

`resets`: the steps t before whose add the buffer was `reset(keep_statistics=True)` (the trainer's sequence): insertion restarts at
slot 0, the stored rows stay, the running episode keeps its length and return."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import oracle as orc  # noqa: E402

orc.build()


def slot_of_step(T: int, S: int, resets=()) -> np.ndarray:
    """The slot step t's row goes to: steps since the last reset (or the start), modulo S."""
    base = np.zeros(T, np.int64)
    for r in sorted(resets):
        base[r:] = r
    return (np.arange(T) - base) % S


def expected_ring(rows, S: int, resets=(), init=0) -> np.ndarray:
    """[S][n_env]...: slot s of env e holds the row of the LAST step that went to slot s (without resets: the last t with
    t % S == s); a slot no step went to keeps `init`."""
    rows = np.asarray(rows)
    out = np.full((S,) + rows.shape[1:], init, rows.dtype)
    for t, s in enumerate(slot_of_step(len(rows), S, resets)):
        out[s] = rows[t]
    return out


def expected_index(done, rew, S: int, resets=()) -> dict:
    """Replay of `oracle.VectorReplayBufferIndex` (n_env sub-buffers of S slots, every env adds one row per step).  All exact: int64,
    and float64 sums of the float32 rewards in step order.
      per step  ptr / ep_idx / ep_len [T][n_env], ep_rew [T][n_env][N]  -- add()'s 4-tuple (manager.py:193)
      state     ins / size / ep_len / ep_start / last_index / lengths [n_env], ep_return [n_env][N] after the last step
      episodes  in (step, env) order: step, env, lens = rows in the buffer, (ptr - ep_idx) % S + 1 (collector.py:203), returns [.][N]"""
    done = np.asarray(done).astype(bool)
    rew = np.asarray(rew)
    assert rew.dtype == np.float32 and rew.ndim == 3 and done.shape == rew.shape[:2]
    T, E, N = rew.shape
    buf = orc.VectorReplayBufferIndex(E * S, E, N)
    assert buf.sub_size == S
    out = dict(ptr=np.zeros((T, E), np.int64), ep_idx=np.zeros((T, E), np.int64), ep_len=np.zeros((T, E), np.int64),
               ep_rew=np.zeros((T, E, N), np.float64))
    for t in range(T):
        if t in resets:
            buf.reset(keep_statistics=True)
        out["ptr"][t], out["ep_rew"][t], out["ep_len"][t], out["ep_idx"][t] = buf.add(rew[t].astype(np.float64), done[t])
    step, env = np.nonzero(done)   # row-major: (step, env) order
    out.update(state=buf.state(), step=step, env=env, lens=(out["ptr"][step, env] - out["ep_idx"][step, env]) % S + 1,
               returns=out["ep_rew"][step, env])
    return out


def episodes_between(exp: dict, t0: int, t1: int) -> tuple[np.ndarray, np.ndarray]:
    """(lens, returns) of the episodes that ended at steps t0 <= t < t1: one collect's statistics."""
    m = (exp["step"] >= t0) & (exp["step"] < t1)
    return exp["lens"][m], exp["returns"][m]


def pack_state(state: dict, flag: int = 0) -> np.ndarray:
    """The state as the device keeps it (csrc/vrb_dev.h: i64 ins | size | ep_len | ep_start | last_index | lengths | f64 ep_return
    | i64 error flag), as int64 words."""
    ints = np.concatenate([np.asarray(state[k], np.int64) for k in ("ins", "size", "ep_len", "ep_start", "last_index", "lengths")])
    return np.concatenate([ints, np.ascontiguousarray(state["ep_return"], np.float64).reshape(-1).view(np.int64),
                           np.array([flag], np.int64)])


def expected_next(done_ring, last_index, lengths, S: int) -> np.ndarray:
    """`next(index)` of every flat index (manager.py:334-358): the index itself where the stored row ends an episode or is the
    newest row of its sub-buffer, else the following slot of the sub-buffer's filled part.  done_ring [S][n_env]."""
    done_ring = np.asarray(done_ring).astype(bool)
    E = done_ring.shape[1]
    idx = np.arange(E * S)
    env, slot = idx // S, idx % S
    stay = done_ring[slot, env] | (idx == np.asarray(last_index)[env])
    return np.where(stay, slot, slot + 1) % np.maximum(np.asarray(lengths)[env], 1) + env * S
