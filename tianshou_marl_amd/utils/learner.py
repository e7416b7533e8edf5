"""What the learners' acting paths and update steps share on the host side: the Philox counter and the result dict of an
`act_device` call, the per-batch-size workspace with its gradient slabs, and the pinned slot the statistics land in."""
from __future__ import annotations

import torch

from .. import ops
from ..data.stats import ResultRing, pinned_slot


def sample_counter(policy, draws: int, row_offset: int, offset_dev) -> int:
    """The Philox counter of one `act_device` call: the policy's own plus `row_offset`; the policy's advances by the call's
    `draws` unless `offset_dev` (the env's device tick, which captured graphs advance) supplies the counter.  It advances
    here, before the sampling launch: a call that raises afterwards has still used up its counters."""
    ctr = policy._sample_ctr + row_offset
    if offset_dev is None:
        policy._sample_ctr += draws
    return ctr


def act_result(out: dict | None, act: torch.Tensor, logp: torch.Tensor | None = None, value: torch.Tensor | None = None,
               **extra) -> dict:
    """What `act_device` returns.  `logp` / `value` None: the policy does not produce them, they are 0.  With `out` (the
    collector's buffers, which the kernels wrote what they produce into) those fields of it are zeroed and `out` is returned;
    else a dict of `act` [rows, ...], f32 `logp` and `value` [rows] and the policy's `extra` fields."""
    if out is not None:
        for k, v in (("logp", logp), ("value", value)):
            if v is None:
                out[k].zero_()
        return out
    zeros = lambda: torch.zeros(act.shape[0], dtype=torch.float32, device=act.device)  # noqa: E731
    return dict(act=act, logp=zeros() if logp is None else logp, value=zeros() if value is None else value, **extra)


def slab_workspace(ws: dict, B: int, device, more=None, **widths: int) -> dict:
    """ws[B], a learner's workspace for batches of B rows, made on the first call at that B: `n_split` (ops.mlp_n_split), one
    f32 gradient slab array [n_split, width] per name in `widths`, then whatever else the learner keeps per B: `more()`."""
    w = ws.get(B)
    if w is None:
        n_split = ops.mlp_n_split(B)
        w = ws[B] = dict(n_split=n_split, **{k: torch.empty(n_split, n, dtype=torch.float32, device=device)
                                             for k, n in widths.items()})
        if more is not None:
            w.update(more())
    return w


def result_slot(w: dict, *shape: int) -> dict:
    """This call's slot of the workspace's `ResultRing`: pinned f32 `h` of `shape` for the statistics, `event`, `pending`."""
    return ResultRing.of(w, lambda: pinned_slot(*shape)).take("resolve", wait=False)
