"""Generate tests/golden/flat_nets.npz: what the flat-parameter networks (tests/flat_net_cases.py) give at seed 3 on the CPU, so
that a change of their shared plumbing can be held against it.  Per case:
  <name>/flat     the flat parameter vector after construction (the init, bit for bit)
  <name>/lagged   the flat vector of `lagged_copy(net)`, where the class has twins
and in `meta` (JSON): the ordered keys and shapes of the reference checkpoint, and the ordered shapes of
`FlatAdam(net).state_dict()["state"]` after one step.  Data only; run from the repository root:
  python tests/golden/make_flat_net_fixtures.py
"""
from __future__ import annotations

import json
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from flat_net_cases import CASES, record  # noqa: E402
from tianshou_marl_amd.utils.net import FlatNet  # noqa: E402


def checkpoint_of(net) -> OrderedDict:
    """`to_reference_state_dict()`; for a net from before every class had one, the same entries from where it kept them:
    `reference_named_views()` (MLPActorCritic; DiscreteActorCritic, whose own export was nested by trunk) or the module's own
    `state_dict()` (QMIXMixer)."""
    if isinstance(net, FlatNet):
        return net.to_reference_state_dict()
    if hasattr(net, "reference_named_views"):
        return OrderedDict(net.reference_named_views())
    return net.state_dict()


def main() -> None:
    arrays, meta = {}, {}
    for name in CASES:
        a, meta[name] = record(name, checkpoint_of)
        arrays.update(a)
    out = os.path.join(HERE, "flat_nets.npz")
    np.savez_compressed(out, meta=np.array(json.dumps(meta)), **arrays)
    print(f"wrote {out}: {len(CASES)} cases, {sum(v.size for v in arrays.values())} floats, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
