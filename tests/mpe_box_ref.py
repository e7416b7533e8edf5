"""TEST INFRASTRUCTURE ONLY -- float64 yardstick of one Box-action step of simple_spread / simple_tag (test_gpu_mpe_box.py).
It adds the decode alone, F = ((a[2] - a[1]) accel, (a[4] - a[3]) accel), to the oracles: the action force enters a step only through
v' = v (1 - damping) + (F + contacts) dt and the contacts depend on positions alone, so a step under F is the oracle's noop step
from the velocity v + F dt / (1 - damping) (the same number up to float64 rounding, before the speed clamp)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import mpe_oracle as so  # noqa: E402
import mpe_tag_oracle  # noqa: E402


def make_world(kind: str, sizes: tuple, max_cycles: int):
    return so.SimpleSpreadWorld(sizes[0], max_cycles, 0.5) if kind == "spread" else mpe_tag_oracle.SimpleTagWorld(*sizes, max_cycles=max_cycles)


def step_box(w, a):
    """One step of world `w` under Box actions a [N, 5] -> the oracle's (obs, rew, terminated, truncated)."""
    a = np.asarray(a, np.float64)
    accel, dt, damping = (so.ACCEL, so.DT, so.DAMPING) if isinstance(w, so.SimpleSpreadWorld) else (w.accel[:, None], w.dt, w.damping)
    w.avel = w.avel + np.stack([a[:, 2] - a[:, 1], a[:, 4] - a[:, 3]], 1) * accel * dt / (1 - damping)
    return w.step(np.zeros(len(a), np.int64))


def decision_margin(w) -> float:
    """Distance of the state's nearest contact decision from its threshold (rewards count contacts)."""
    p = w.apos
    if isinstance(w, so.SimpleSpreadWorld):
        d = np.linalg.norm(p[:, None] - p[None], axis=-1)[~np.eye(len(p), dtype=bool)]
        return float(np.abs(d - 2 * so.AGENT_SIZE).min()) if d.size else np.inf
    na = w.n_adv
    return float(np.abs(np.linalg.norm(p[:na, None] - p[None, na:], axis=-1) - (w.size[:na, None] + w.size[None, na:w.NA])).min())
