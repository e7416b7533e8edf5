"""Generate tests/golden/ppo_checkpoint_layout.npz: the `state_dict()` layout of the on-policy learners of
tests/ppo_checkpoint_cases.py, built on the CPU at seed 3 with a planted optimizer state, so that a change of their checkpoint
plumbing can be held against it.  Per case:
  <name>/exp_avg/<i>, <name>/exp_avg_sq/<i>   the moments of parameter i as the checkpoint lists them
  <name>/ret_rms                              the return statistics of `tsm_engine`
and in `meta` (JSON): the ordered keys, the parameter shapes, [index, step] of every optimizer state entry, `param_groups[0]`
whole and the rest of `tsm_engine`.  Data only; run from the repository root:
  python tests/golden/make_ppo_checkpoint_fixtures.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from ppo_checkpoint_cases import CASES, record  # noqa: E402


def main() -> None:
    arrays, meta = {}, {}
    for name in CASES:
        a, meta[name] = record(name)
        arrays.update(a)
    out = os.path.join(HERE, "ppo_checkpoint_layout.npz")
    np.savez_compressed(out, meta=np.array(json.dumps(meta)), **arrays)
    print(f"wrote {out}: {len(CASES)} cases, {sum(v.size for v in arrays.values())} floats, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
