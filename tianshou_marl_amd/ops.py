"""Tensor-level front-end of the C-ABI (one thin function per entry point of include/tsmarl.h).

Inputs/outputs are torch tensors that live in HBM; every function launches hand-written HIP
kernels through `_abi.call` on torch's current stream.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _abi
from ._abi import call, ptr, stream_ptr, tsm_field, tsm_ppo_cfg


def _chk(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t.contiguous()


def _dev_only(name: str, *tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{name} needs device (HIP) tensors; there is no CPU path")


def _out(name: str, out, shape, dtype, device, what: str = "out", size: str = "shape"):
    """The tensor a launch writes (`_chk` is for inputs: its copy of a strided `out` would take the result and the caller's
    tensor stay as it was).  None: a fresh `shape` of `dtype`.  Else `out` ITSELF, which must be a contiguous device tensor of
    `dtype` and, by `size`, "shape": of exactly `shape`; "numel": of any shape with as many entries; "min": with at least as many
    (the floor of memory safety, for buffers the caller slices from something larger)."""
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    n = math.prod(shape)
    fits = tuple(out.shape) == tuple(shape) if size == "shape" else out.numel() == n if size == "numel" else out.numel() >= n
    if out.dtype != dtype or not fits or not out.is_contiguous():
        want = list(shape) if size == "shape" else f"{'at least ' if size == 'min' else ''}{n} entries"
        raise ValueError(f"{name}: {what} must be {want}, contiguous {dtype}; got {list(out.shape)} {out.dtype}, strides "
                         f"{tuple(out.stride())}")
    _dev_only(name, out)
    return out


def _out_or_pinned(name: str, out, n: int, what: str = "out") -> int:
    """The address of a result of at least n f32 that the host reads: a device tensor, or pinned host memory (mapped: the kernel
    writes it directly, no D2H copy)."""
    if not (out.is_cuda or out.is_pinned()):
        raise RuntimeError(f"{name} needs device (HIP) tensors; there is no CPU path ({what} must be a device tensor or pinned "
                           f"host memory)")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < n:
        raise ValueError(f"{name}: {what} must be at least {n} contiguous f32")
    return out.data_ptr()


def _philox(name: str, seed: int, offset: int, offset_dev) -> tuple:
    """The three counter arguments of every sampling entry: the seed and the host's offset as u64 (Python ints of either sign
    wrap modulo 2**64) and the address of the device's offset word (None: NULL), which must live in HBM."""
    _dev_only(name, offset_dev)
    return seed & (2**64 - 1), offset & (2**64 - 1), ptr(offset_dev)


def _slab_dest(name: str, slabs, n_split: int, rows: int, pitch: int, extent: int, dev) -> tuple:
    """Where a backward's weight gradients land: slab s may be written over the floats [s * pitch, s * pitch + extent) behind
    the first element of `slabs`, which may be a view INTO the slabs of a larger joint vector.  n_split <= 0: `mlp_n_split(rows)`;
    slabs None: a fresh [n_split, pitch].  -> (n_split, slabs, pitch), no write of which leaves the tensor."""
    n_split, pitch = int(n_split) if n_split > 0 else mlp_n_split(rows), int(pitch)
    if not 1 <= n_split <= 65535:
        raise ValueError(f"{name}: n_split {n_split} outside [1, 65535]")
    if pitch < extent:
        raise ValueError(f"{name}: slab_stride {pitch} smaller than the parameter count {extent}, the floats of a slab")
    if slabs is None:
        return n_split, torch.empty(n_split, pitch, dtype=torch.float32, device=dev), pitch
    if slabs.dtype != torch.float32 or slabs.dim() < 1 or slabs.numel() == 0 or slabs.stride(-1) != 1:
        raise ValueError(f"{name}: slabs must be a non-empty f32 tensor, contiguous along the parameters")
    if slabs.dim() == 2 and n_split > slabs.shape[0]:
        raise ValueError(f"{name}: n_split {n_split} exceeds the {slabs.shape[0]} rows of slabs")
    reach = 1 + sum((n - 1) * st for n, st in zip(slabs.shape, slabs.stride()))
    if (n_split - 1) * pitch + extent > reach:
        raise ValueError(f"{name}: slabs reach {reach} floats; {n_split} slabs of {extent} floats at pitch {pitch} need "
                         f"{(n_split - 1) * pitch + extent}")
    _dev_only(name, slabs)
    return n_split, slabs, pitch


# --------------------------------------------------------------------------------------------
# GAE  (algorithm_base.py:651-717,1079-1134; a2c.py:132-146)
# --------------------------------------------------------------------------------------------
def gae_lanes(v_s, v_s_next, rew, terminated, truncated, gamma=0.99, gae_lambda=0.95, v_scale=1.0,
              lanes_per_env=1, env_start=None, env_len=None, out=None, rms=None, rms_eps=1e-8):
    """Per-lane GAE on time-major tensors [T, ...lanes]; returns (returns, adv) f32 tensors.

    terminated/truncated: u8/bool, either the lane shape [T, n_lane] or env-level [T, n_env].
    rms: device f64[3] {mean, var, count} of the return statistics -> v_scale = sqrt(var + rms_eps) read on device.
    """
    v_s = _chk(v_s, torch.float32, "v_s")
    T = v_s.shape[0]
    L = v_s[0].numel() if T > 0 else 0
    if T > 4096 and L <= 64:
        ensure_scan_workspace(v_s.device)
    v_s_next = _chk(v_s_next, torch.float32, "v_s_next")
    rew = _chk(rew, torch.float32, "rew")
    term = terminated.contiguous().view(torch.uint8) if terminated.dtype == torch.bool else _chk(terminated, torch.uint8, "terminated")
    trunc = truncated.contiguous().view(torch.uint8) if truncated.dtype == torch.bool else _chk(truncated, torch.uint8, "truncated")
    if v_s_next.shape != v_s.shape or rew.shape != v_s.shape:
        raise ValueError("gae_lanes: v_s, v_s_next, rew must have identical shapes")
    flags_per_lane = 1 if term.numel() == v_s.numel() else 0
    if not flags_per_lane and term.numel() * lanes_per_env != v_s.numel():
        raise ValueError("gae_lanes: flag tensors must be lane-shaped or env-shaped")
    if trunc.numel() != term.numel():
        raise ValueError("gae_lanes: terminated/truncated shape mismatch")
    ret, adv = (_out("gae_lanes", o, v_s.shape, torch.float32, v_s.device, nm, "min")
                for o, nm in zip(out or (None, None), ("out[0]", "out[1]")))
    if rms is not None:
        call("tsm_gae_lanes_rms", ptr(v_s), ptr(v_s_next), ptr(rew), ptr(term), ptr(trunc), flags_per_lane, T, L,
             lanes_per_env, ptr(env_start), ptr(env_len), float(gamma), float(gae_lambda),
             ptr(_chk(rms, torch.float64, "rms")), float(rms_eps), ptr(ret), ptr(adv), stream_ptr())
        return ret, adv
    call("tsm_gae_lanes", ptr(v_s), ptr(v_s_next), ptr(rew), ptr(term), ptr(trunc), flags_per_lane, T, L,
         lanes_per_env, ptr(env_start), ptr(env_len), float(gamma), float(gae_lambda), float(v_scale),
         ptr(ret), ptr(adv), stream_ptr())
    return ret, adv


_scan_ws: dict = {}   # device index -> (workspace, pinned error word)


def ensure_scan_workspace(device) -> bool:
    """Register the workspace of the parallel long-series GAE scan (include/tsmarl.h: tsm_gae_set_scan_workspace) once per DEVICE;
    not while a stream is capturing (the allocation would belong to that graph's pool).  Callers that capture graphs call it
    beforehand (PPO._warm_kernels)."""
    device = torch.device(device)
    idx = device.index if device.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
    if idx not in _scan_ws and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
        n = int(call("tsm_gae_scan_workspace_bytes"))
        with torch.cuda.device(idx):
            ws = torch.zeros(n, dtype=torch.uint8, device=torch.device("cuda", idx))
            err = torch.zeros(1, dtype=torch.int32, pin_memory=True)
            call("tsm_gae_set_scan_workspace", ws.data_ptr(), n)
            call("tsm_gae_set_scan_error_word", err.data_ptr())
        _scan_ws[idx] = (ws, err)
    return idx in _scan_ws


def gae_scan_failed() -> bool:
    """True once a parallel long-series scan gave up waiting for another workgroup's map (its returns are NaN from there on).
    A plain read of pinned host words: meaningful after the host has waited for the launch (the statistics' event)."""
    return any(int(err[0]) != 0 for _, err in _scan_ws.values())


def rms_update(returns, rms, rms_eps=1e-8, ids=None, work=None):
    """RunningMeanStd.update(returns * sqrt(var + eps)) on device (a2c.py:144-146); rms f64[3] is updated in place."""
    returns = _chk(returns, torch.float32, "returns").reshape(-1)
    n = returns.numel() if ids is None else ids.numel()
    if work is None:
        work = torch.empty(call("tsm_rms_update_work_elems", n), dtype=torch.float64, device=returns.device)
    call("tsm_rms_update", ptr(returns), ptr(ids), n, ptr(_out("rms_update", rms, (3,), torch.float64, None, "rms", "min")),
         float(rms_eps), ptr(work), stream_ptr())
    return rms


def mc_return_to_go_lanes(rew, gamma=0.99):
    rew = _chk(rew, torch.float32, "rew")
    out = torch.empty_like(rew)
    T = rew.shape[0]
    call("tsm_mc_return_to_go_lanes", ptr(rew), T, rew[0].numel() if T else 0, float(gamma), ptr(out), stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# VectorReplayBuffer index state (manager.py / buffer_base.py)
# --------------------------------------------------------------------------------------------
class VrbState:
    """Device-resident episode/index bookkeeping of a VectorReplayBuffer(total_size, buffer_num)."""

    def __init__(self, total_size: int, buffer_num: int, rew_dim: int = 1, device="cuda"):
        self.buffer_num = int(buffer_num)
        self.sub_size = -(-int(total_size) // self.buffer_num)  # ceil, vecbuf.py:35
        self.maxsize = self.sub_size * self.buffer_num
        self.rew_dim = max(1, int(rew_dim))
        self.device = torch.device(device)
        nbytes = call("tsm_vrb_state_bytes", self.buffer_num, self.rew_dim)
        self.state = torch.zeros(nbytes // 8, dtype=torch.int64, device=self.device)
        self.done_store = torch.zeros(self.sub_size, self.buffer_num, dtype=torch.uint8, device=self.device)
        self._scratch = torch.zeros(self.buffer_num + 1, dtype=torch.int64, device=self.device)
        self._n_out = torch.zeros(1, dtype=torch.int64, device=self.device)
        call("tsm_vrb_init", ptr(self.state), self.buffer_num, self.sub_size, self.rew_dim, stream_ptr())

    # views into the packed state (i64 [6][B] | f64 [B][D] | i64 flag)
    def _i64(self, k):
        B = self.buffer_num
        return self.state[k * B:(k + 1) * B]

    insertion_idx = property(lambda s: s._i64(0))
    size = property(lambda s: s._i64(1))
    last_index = property(lambda s: s._i64(4))
    lengths = property(lambda s: s._i64(5))

    def __len__(self) -> int:
        return int(self.lengths.sum().item())

    def reset(self, keep_statistics: bool = False) -> None:
        call("tsm_vrb_reset", ptr(self.state), self.buffer_num, self.sub_size, self.rew_dim,
             int(keep_statistics), stream_ptr())

    def add(self, rew, done, buffer_ids=None, fields=(), outs=None):
        """manager.py:131-193.  fields: iterable of (src[R, ...], dst[sub_size, buffer_num, ...]).
        outs: optional preallocated (ptr i64[R], ep_rew f64[R,D], ep_len i64[R], ep_idx i64[R])."""
        rew = _chk(rew, torch.float32, "rew").reshape(rew.shape[0], -1)
        R = rew.shape[0]
        if rew.shape[1] != self.rew_dim:
            raise ValueError(f"rew has {rew.shape[1]} columns, buffer was created with rew_dim={self.rew_dim}")
        done = done.contiguous().view(torch.uint8) if done.dtype == torch.bool else _chk(done, torch.uint8, "done")
        ids = None if buffer_ids is None else _chk(buffer_ids, torch.int64, "buffer_ids")
        dev = self.device
        ptr_out, ep_rew, ep_len, ep_idx = (
            _out("VrbState.add", o, shape, dt, dev, f"outs[{k}]", "min") for k, (o, shape, dt) in enumerate(zip(
                outs or (None,) * 4, ((R,), (R, self.rew_dim), (R,), (R,)), (torch.int64, torch.float64, torch.int64, torch.int64))))
        farr = (tsm_field * max(1, len(fields)))()
        keep = []
        for i, (src, dst) in enumerate(fields):
            src = src.contiguous()
            keep.append(src)
            rb = src[0].numel() * src.element_size() if R else dst[0, 0].numel() * dst.element_size()
            if dst[0, 0].numel() * dst.element_size() != rb:
                raise ValueError(f"field {i}: row size mismatch between source and store")
            farr[i] = tsm_field(ptr(src), ptr(dst), rb)
        call("tsm_vrb_add", ptr(self.state), self.buffer_num, self.sub_size, self.rew_dim, ptr(ids), R,
             ptr(rew), ptr(done), ptr(self.done_store), farr, len(fields), ptr(ptr_out), ptr(ep_rew),
             ptr(ep_len), ptr(ep_idx), stream_ptr())
        return ptr_out, ep_rew, ep_len, ep_idx

    def check(self) -> None:
        call("tsm_vrb_check", ptr(self.state), self.buffer_num, self.rew_dim, stream_ptr())

    def sample_indices_all(self) -> torch.Tensor:
        out = torch.empty(self.maxsize, dtype=torch.int64, device=self.device)
        call("tsm_vrb_sample_indices_all", ptr(self.state), self.buffer_num, self.sub_size, ptr(out),
             ptr(self._n_out), ptr(self._scratch), stream_ptr())
        return out[: int(self._n_out.item())]

    def unfinished_index(self) -> torch.Tensor:
        out = torch.empty(self.buffer_num, dtype=torch.int64, device=self.device)
        call("tsm_vrb_unfinished_index", ptr(self.state), self.buffer_num, self.sub_size,
             ptr(self.done_store), ptr(out), ptr(self._n_out), stream_ptr())
        return out[: int(self._n_out.item())]

    def _pn(self, name, index):
        index = _chk(torch.as_tensor(index, device=self.device), torch.int64, "index").reshape(-1)
        out = torch.empty_like(index)
        call(name, ptr(self.state), self.buffer_num, self.sub_size, ptr(self.done_store), ptr(index),
             index.numel(), ptr(out), stream_ptr())
        return out

    def prev(self, index):
        return self._pn("tsm_vrb_prev", index)

    def next(self, index):
        return self._pn("tsm_vrb_next", index)

    def gather(self, store: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
        """ReplayBuffer.__getitem__ for one field: rows of a [sub_size, buffer_num, ...] store by flat index."""
        index = _chk(index, torch.int64, "index").reshape(-1)
        row_shape = store.shape[2:]
        out = torch.empty((index.numel(), *row_shape), dtype=store.dtype, device=store.device)
        rb = store[0, 0].numel() * store.element_size()
        call("tsm_vrb_gather", ptr(store), self.buffer_num, self.sub_size, rb, ptr(index), index.numel(),
             ptr(out), stream_ptr())
        return out


    def gather_stacked(self, store: torch.Tensor, index: torch.Tensor, stack_num: int, lane: int | None = None) -> torch.Tensor:
        """ReplayBuffer.get(index, key, stack_num) for one field (buffer_base.py:533-590) in one launch: the rows of a
        [sub_size, buffer_num, ...] store at the `stack_num - 1` predecessors of `index` (prev's rule) and at `index`, oldest
        first -> [I, stack_num, ...].  `lane`: only store[:, :, lane] of a [sub_size, buffer_num, N, ...] store -> [I, stack_num,
        ...] without the agent axis.  Bit-identical to rounds of `prev` + `gather`."""
        _dev_only("gather_stacked", store, index)
        if int(stack_num) < 1:
            raise ValueError(f"gather_stacked: stack_num {stack_num} must be >= 1")
        if store.dim() < 2 or tuple(store.shape[:2]) != (self.sub_size, self.buffer_num) or not store.is_contiguous():
            raise ValueError(f"gather_stacked: store must be a contiguous [{self.sub_size}, {self.buffer_num}, ...]")
        index = _chk(index, torch.int64, "index").reshape(-1)
        rb = store[0, 0].numel() * store.element_size()
        row_shape, off, nb = tuple(store.shape[2:]), 0, rb
        if lane is not None:
            if store.dim() < 3 or not 0 <= int(lane) < store.shape[2]:
                raise ValueError(f"gather_stacked: lane {lane} outside the store's agent axis {tuple(store.shape[2:3])}")
            row_shape, nb = tuple(store.shape[3:]), rb // store.shape[2]
            off = int(lane) * nb
        out = torch.empty((index.numel(), int(stack_num), *row_shape), dtype=store.dtype, device=store.device)
        call("tsm_vrb_gather_stacked", ptr(self.state), self.buffer_num, self.sub_size, ptr(self.done_store), ptr(store), rb, off,
             nb, ptr(index), index.numel(), int(stack_num), ptr(out), stream_ptr())
        return out


# --------------------------------------------------------------------------------------------
# agent dispatch (marl.py:148,170-180,233)
# --------------------------------------------------------------------------------------------
def agent_index(agent_id: torch.Tensor, n_agent: int):
    """Stable partition of row numbers by agent -> (index[B] i64, offsets[n_agent+1] i64)."""
    agent_id = _chk(agent_id, torch.int32, "agent_id").reshape(-1)
    B = agent_id.numel()
    dev = agent_id.device
    index = torch.empty(B, dtype=torch.int64, device=dev)
    offsets = torch.empty(n_agent + 1, dtype=torch.int64, device=dev)
    n_blocks = max(1, -(-B // 1024))
    scratch = torch.empty(n_agent * n_blocks + 1, dtype=torch.int64, device=dev)
    call("tsm_agent_index", ptr(agent_id), B, n_agent, ptr(index), ptr(offsets), ptr(scratch), stream_ptr())
    return index, offsets


def scatter_rows(src: torch.Tensor, index: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst[index[i]] = src[i]"""
    src = src.contiguous()
    n = index.numel()
    rb = (src[0].numel() if n else 1) * src.element_size()
    call("tsm_scatter_rows", ptr(src), ptr(_chk(index, torch.int64, "index")), n, rb, ptr(dst), stream_ptr())
    return dst


def gather_rows(src: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """out[i] = src[index[i]]"""
    src = src.contiguous()
    n = index.numel()
    out = torch.empty((n, *src.shape[1:]), dtype=src.dtype, device=src.device)
    rb = src[0].numel() * src.element_size()
    call("tsm_gather_rows", ptr(src), ptr(_chk(index, torch.int64, "index")), n, rb, ptr(out), stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# categorical head (discrete.py:22-24; reinforce.py:183-189)
# --------------------------------------------------------------------------------------------
def categorical_sample(logits, seed: int, offset: int = 0, deterministic: bool = False, want_logp: bool = True,
                       offset_dev=None, out=None):
    """Categorical(logits).sample() / .mode + log-prob; `out` = optional preallocated (act i32[B], logp f32[B])."""
    logits = _chk(logits, torch.float32, "logits")
    B, A = logits.shape
    act, logp = out if out is not None else (None, None)
    act = _out("categorical_sample", act, (B,), torch.int32, logits.device, "act", "min")
    if logp is not None or (out is None and want_logp):
        logp = _out("categorical_sample", logp, (B,), torch.float32, logits.device, "logp", "min")
    call("tsm_categorical_sample", ptr(logits), B, A, *_philox("categorical_sample", seed, offset, offset_dev),
         int(deterministic), ptr(act), ptr(logp), stream_ptr())
    return act, logp


def categorical_logp_entropy(logits, act):
    logits = _chk(logits, torch.float32, "logits")
    act = _chk(act, torch.int32, "act")
    B, A = logits.shape
    logp = torch.empty(B, dtype=torch.float32, device=logits.device)
    ent = torch.empty(B, dtype=torch.float32, device=logits.device)
    call("tsm_categorical_logp_entropy", ptr(logits), ptr(act), B, A, ptr(logp), ptr(ent), stream_ptr())
    return logp, ent


# --------------------------------------------------------------------------------------------
# PPO loss (ppo.py:182-211)
# --------------------------------------------------------------------------------------------
def make_ppo_cfg(eps_clip=0.2, dual_clip=None, value_clip=False, adv_norm=True, vf_coef=0.5, ent_coef=0.01,
                 loss_kind=0, value_group=1):
    """loss_kind 0: PPO clip objective; 1: plain policy gradient -mean(logp * adv) (A2C / Reinforce); 2: the value term
    alone (ppo_value_loss).  value_group N > 1: one critic value per joint row of N agents (centralized critic)."""
    if loss_kind not in (0, 1, 2):
        raise ValueError(f"loss_kind must be 0 (PPO clip), 1 (policy gradient) or 2 (value term only), got {loss_kind}")
    return tsm_ppo_cfg(float(eps_clip), float(dual_clip or 0.0), float(vf_coef), float(ent_coef),
                       int(bool(value_clip)), int(bool(adv_norm)), int(loss_kind), int(value_group))


def ppo_adv_stats(adv, mb_start, perm=None, out=None, max_rows: int = 0, work=None):
    """Per-minibatch (mean, unbiased std) of adv[perm[mb_start[k]:mb_start[k+1]]] -> [n_mb, 2] f32.
    max_rows: host knowledge of the longest minibatch; above 8192 rows the chunks of a minibatch are reduced by separate
    workgroups (tsm_ppo_adv_stats_wide, work = f64 scratch kept alive by the caller when captured in a graph)."""
    adv = _chk(adv, torch.float32, "adv").reshape(-1)
    mb_start = _chk(mb_start, torch.int64, "mb_start")
    n_mb = mb_start.numel() - 1
    stats = _out("ppo_adv_stats", out, (n_mb, 2), torch.float32, adv.device, size="min")
    if max_rows > 8192:
        if work is None:
            work = torch.empty(call("tsm_ppo_adv_stats_work_elems", n_mb, max_rows), dtype=torch.float64, device=adv.device)
        call("tsm_ppo_adv_stats_wide", ptr(adv), ptr(perm), ptr(mb_start), n_mb, int(max_rows), ptr(work), ptr(stats),
             stream_ptr())
        return stats
    call("tsm_ppo_adv_stats", ptr(adv), ptr(perm), ptr(mb_start), n_mb, ptr(stats), stream_ptr())
    return stats


def ppo_packed_record_elems(obs_dim: int) -> int:
    """4-byte words of one packed 16-row tile record (include/tsmarl.h: tsm_ppo_pack_minibatches)."""
    return call("tsm_ppo_packed_record_elems", int(obs_dim))


def ppo_pack_workspace(sizes, obs_dim: int, device) -> dict:
    """Where `ppo_pack_minibatches` puts the rows of minibatches of `sizes` rows (host ints, in launch order), allocated once:
    `packed` [records, record words] f32, `tile_start` (device i64, first record of each minibatch) and the same on the host
    (`tile_start_host`, one entry more: the total).  `rows(k)` is minibatch k's slice of `packed`, the `packed=` argument of
    `ppo_update_fused`."""
    sizes = [int(m) for m in sizes]
    if not sizes or min(sizes) < 1 or max(sizes) > 8192:
        raise ValueError(f"ppo_pack_workspace: minibatches of 1..8192 rows (got {sizes[:4]}...)")
    starts = [0]
    for m in sizes:
        starts.append(starts[-1] + (m + 15) // 16)
    ws = dict(sizes=sizes, obs_dim=int(obs_dim), max_rows=max(sizes), tile_start_host=starts,
              tile_start=torch.as_tensor(starts[:-1], dtype=torch.int64, device=device),
              packed=torch.zeros(starts[-1], ppo_packed_record_elems(obs_dim), dtype=torch.float32, device=device))
    ws["rows"] = lambda k: ws["packed"][starts[k]:starts[k + 1]]
    return ws


def ppo_pack_minibatches(ws: dict, adv, mb_start, perm, obs, act, logp_old, returns, v_old=None, out=None, stats=True):
    """`ppo_adv_stats` of every minibatch AND the minibatches' rows gathered into `ws` (`ppo_pack_workspace`) in ONE launch:
    the gradient steps then read their 16-row tiles as contiguous records instead of chasing `perm` (`ppo_update_fused(packed=)`).
    v_old: v_s_old when the loss clips the value (None: the returns, which the kernel then ignores).  stats=False: rows only.
    Returns the statistics [n_mb, 2] (None without)."""
    adv = _chk(adv, torch.float32, "adv").reshape(-1)
    obs = _chk(obs, torch.float32, "obs")
    mb_start = _chk(mb_start, torch.int64, "mb_start")
    n_mb = mb_start.numel() - 1
    if n_mb != len(ws["sizes"]) or obs.shape[-1] != ws["obs_dim"]:
        raise ValueError(f"ppo_pack_minibatches: the workspace was made for {len(ws['sizes'])} minibatches of obs_dim "
                         f"{ws['obs_dim']}, got {n_mb} and {obs.shape[-1]}")
    n = obs.numel() // obs.shape[-1]
    returns = _chk(returns, torch.float32, "returns")
    v_old = returns if v_old is None else _chk(v_old, torch.float32, "v_old")
    for name, t in (("adv", adv), ("act", act), ("logp_old", logp_old), ("returns", returns), ("v_old", v_old)):
        if t.numel() != n:
            raise ValueError(f"ppo_pack_minibatches: {name} holds {t.numel()} values for {n} rows of obs")
    if perm is not None and _chk(perm, torch.int64, "perm").numel() < sum(ws["sizes"]):
        raise ValueError(f"ppo_pack_minibatches: perm holds {perm.numel()} row ids, the minibatches {sum(ws['sizes'])}")
    st = _out("ppo_pack_minibatches", out, (n_mb, 2), torch.float32, adv.device, size="min") if stats else None
    call("tsm_ppo_pack_minibatches", ptr(adv), ptr(perm), ptr(mb_start), n_mb, ws["max_rows"], ptr(st), ptr(obs), ws["obs_dim"],
         ptr(_chk(act, torch.int32, "act")), ptr(_chk(logp_old, torch.float32, "logp_old")), ptr(returns), ptr(v_old),
         ptr(ws["tile_start"]), ptr(ws["packed"]), stream_ptr())
    return st


def ppo_adv_stats_pack(stats, mb_start, out=None):
    """This rank's per-minibatch (mean, unbiased std) + row counts -> f64 [n_mb, 3] = (n, sum x, sum x^2): the additive
    form one all-reduce sums over data-parallel ranks (parallel.GradSync.merge_adv_stats_)."""
    stats = _chk(stats, torch.float32, "stats").reshape(-1, 2)
    mb_start = _chk(mb_start, torch.int64, "mb_start")
    n_mb = mb_start.numel() - 1
    if stats.shape[0] != n_mb:
        raise ValueError(f"ppo_adv_stats_pack: {stats.shape[0]} statistics rows for {n_mb} minibatches")
    pack = _out("ppo_adv_stats_pack", out, (n_mb, 3), torch.float64, stats.device, size="min")
    call("tsm_ppo_adv_stats_pack", ptr(stats), ptr(mb_start), n_mb, ptr(pack), stream_ptr())
    return pack


def ppo_adv_stats_unpack(pack, stats):
    """Summed (n, sum x, sum x^2) -> (mean, unbiased std) of the union, written into `stats` [n_mb, 2] f32 in place."""
    pack = _chk(pack, torch.float64, "pack").reshape(-1, 3)
    _out("ppo_adv_stats_unpack", stats, (pack.shape[0], 2), torch.float32, None, "stats", "numel")
    call("tsm_ppo_adv_stats_unpack", ptr(pack), pack.shape[0], ptr(stats), stream_ptr())
    return stats


def ppo_loss_fwd_bwd(logits, value, act, logp_old, adv, returns, cfg: tsm_ppo_cfg, adv_stats=None,
                     v_s_old=None, perm=None, first_row=0, finalize: bool = True):
    """One minibatch -> (dlogits[M,A], dvalue[M], scalars[4]={loss, clip, vf, ent}).
    finalize=False leaves the per-workgroup partial sums unfolded (returned in place of `scalars`): an epoch's
    statistics can then be folded once, as the fused path does (ppo_finalize_many)."""
    logits = _chk(logits, torch.float32, "logits")
    M, A = logits.shape
    value = _chk(value, torch.float32, "value").reshape(-1)
    dev = logits.device
    vg = max(1, int(cfg.value_group))
    if value.numel() * vg != M:
        raise ValueError(f"ppo_loss_fwd_bwd: {value.numel()} values for {M} samples with value_group={vg}")
    dlogits = torch.empty_like(logits)
    dvalue = torch.empty(M // vg, dtype=torch.float32, device=dev)
    partial = torch.empty(max(1, call("tsm_ppo_loss_partial_elems", M)), dtype=torch.float64, device=dev)
    scalars = torch.empty(4, dtype=torch.float32, device=dev)
    s = stream_ptr()
    call("tsm_ppo_loss_fwd_bwd", ptr(logits), ptr(value), ptr(_chk(act, torch.int32, "act")),
         ptr(_chk(logp_old, torch.float32, "logp_old")), ptr(_chk(adv, torch.float32, "adv")),
         ptr(_chk(returns, torch.float32, "returns")), ptr(v_s_old), ptr(perm), first_row, M, A,
         ptr(adv_stats), C.byref(cfg), ptr(dlogits), ptr(dvalue), ptr(partial), s)
    if not finalize:
        return dlogits, dvalue, partial
    if M > 0:
        call("tsm_ppo_loss_finalize", ptr(partial), M, C.byref(cfg), ptr(scalars), s)
    return dlogits, dvalue, scalars


# --------------------------------------------------------------------------------------------
# optimizer (algorithm_base.py:485-498; optim.py:91-111)
# --------------------------------------------------------------------------------------------
def adam_step(param, grad_slabs, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.0, max_grad_norm=None, work=None, step_dev=None, image=None, image_map=None, lr_dev=None,
              coef64=False):
    """In-place Adam on a flat f32 vector; grad_slabs [n_slab, n] are summed in slab order.  coef64: 1 - beta formed in f64
    and rounded once, as torch forms them (include/tsmarl.h: tsm_adam_step_coef64)."""
    n = param.numel()
    grad_slabs = _chk(grad_slabs, torch.float32, "grad_slabs").reshape(-1, n)
    if max_grad_norm and work is None:
        work = torch.empty(call("tsm_adam_work_elems", n), dtype=torch.float32, device=param.device)
    call("tsm_adam_step_coef64" if coef64 else "tsm_adam_step", ptr(param), ptr(grad_slabs), grad_slabs.shape[0], n, ptr(exp_avg),
         ptr(exp_avg_sq),
         int(step), ptr(step_dev), float(lr), ptr(lr_dev), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
         float(max_grad_norm or 0.0), ptr(work), ptr(image), ptr(image_map), stream_ptr())
    return param


def _slab_segs(segs, n: int):
    """[(slabs [n_slab, stride >= n_k], offset, n_k[, scale_dev[, frag_image[, col0]]]), ...] -> ctypes array of tsm_slab_seg.
    col0: the segment's gradients are columns [col0, col0 + n_k) of every slab row (a view into joint slabs).
    A segment's slabs tensor may be wider than its parameter count (a view into joint slabs): stride = its row pitch.
    scale_dev (optional device f32[1]): the segment's summed gradient is multiplied by it.
    frag_image (optional, `critic_w1_image` layout): the segment is a [128][n_k / 128] first-layer weight matrix whose
    updated values the optimizer also stores in fragment order."""
    arr = (_abi.tsm_slab_seg * len(segs))()
    for k, seg in enumerate(segs):
        sl, off, nk = seg[:3]
        sc = seg[3] if len(seg) > 3 else None
        img = seg[4] if len(seg) > 4 else None
        col0 = int(seg[5]) if len(seg) > 5 else 0   # the segment's gradients start at this column of every slab row
        sl = _chk(sl, torch.float32, "slabs")
        if sl.dim() != 2 or sl.shape[1] < col0 + nk:
            raise ValueError("slab segment: expected slabs [n_slab, >= col0 + n] for n = %d, got %s" % (nk, tuple(sl.shape)))
        k1 = kj = 0
        if img is not None:
            if nk % 128:
                raise ValueError("slab segment: a fragment image belongs to a [128][K1] weight matrix")
            k1 = nk // 128
            kj = call("tsm_critic_rows_w1_image_kj", k1)
            if _chk(img, torch.float32, "frag_image").numel() != call("tsm_critic_rows_w1_image_elems", k1):
                raise ValueError("slab segment: frag_image has the wrong size for K1 = %d" % k1)
        arr[k] = _abi.tsm_slab_seg(ptr(sl) + 4 * col0, int(off), int(nk), int(sl.shape[1]), int(sl.shape[0]), k1,
                                   ptr(None if sc is None else _chk(sc, torch.float32, "scale_dev")), ptr(img), kj, 0)
    return arr


def critic_w1_image(w0_flat, in_dim: int, out=None):
    """The first-layer weights w0 [128][in_dim] (the head of a critic's flat parameter vector) in the fragment order the
    one-launch critic gradient step loads with coalesced 16-B loads (include/tsmarl.h: tsm_critic_rows_w1_image)."""
    n = call("tsm_critic_rows_w1_image_elems", in_dim)
    if n < 0:
        raise ValueError(f"critic_w1_image: in_dim = {in_dim} is not served by the rows kernels")
    out = _out("critic_w1_image", out, (n,), torch.float32, w0_flat.device, size="min")
    call("tsm_critic_rows_w1_image", ptr(_chk(w0_flat, torch.float32, "w0")), in_dim, ptr(out), stream_ptr())
    return out


def adam_step_segs(param, segs, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                   max_grad_norm=None, work=None, step_dev=None, lr_dev=None):
    """`adam_step` for a flat vector whose parts have their own slab arrays: segs = [(slabs, offset, n), ...] tiling
    [0, param.numel()) in order.  One launch (+ one reduction launch when clipping; ONE norm over all segments)."""
    n = param.numel()
    if max_grad_norm and work is None:
        work = torch.empty(call("tsm_adam_work_elems", n), dtype=torch.float32, device=param.device)
    arr = _slab_segs(segs, n)
    call("tsm_adam_step_segs", ptr(param), arr, len(segs), n, ptr(exp_avg), ptr(exp_avg_sq), int(step), ptr(step_dev),
         float(lr), ptr(lr_dev), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
         float(max_grad_norm or 0.0), ptr(work), stream_ptr())
    return param


def reduce_slabs_segs(segs, n: int, out=None, scale: float = 1.0):
    """Flat gradient [n] = scale * per-segment slab sums (see adam_step_segs); one launch."""
    out = _out("reduce_slabs_segs", out, (n,), torch.float32, segs[0][0].device, size="min")
    call("tsm_reduce_slabs_segs", _slab_segs(segs, n), len(segs), n, float(scale), ptr(out), stream_ptr())
    return out


def reduce_slabs(grad_slabs, out=None, scale: float = 1.0):
    """Flat gradient = scale * sum of per-workgroup slabs [n_slab, n] (deterministic slab order)."""
    grad_slabs = _chk(grad_slabs, torch.float32, "grad_slabs")
    n_slab, n = grad_slabs.shape
    out = _out("reduce_slabs", out, (n,), torch.float32, grad_slabs.device, size="min")
    call("tsm_reduce_slabs", ptr(grad_slabs), n_slab, n, float(scale), ptr(out), stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# fused actor+critic MLP (reinforce.py:167-192, a2c.py:121-127, ppo.py:157-212)
# --------------------------------------------------------------------------------------------
POLICY_MODES = {"none": 0, "sample": 1, "mode": 2, "given": 3}


def policy_param_count(obs_dim: int, hidden: int, n_act: int) -> int:
    n = call("tsm_policy_param_count", obs_dim, hidden, n_act)
    if n < 0:
        raise ValueError(f"fused MLP does not support hidden={hidden}")
    return n


def policy_forward(params, obs, n_act: int, hidden: int = 64, mode: str = "none", seed: int = 0, offset: int = 0,
                   act=None, want_logits=True, want_value=True, want_logp=True, offset_dev=None, out=None,
                   image=None):
    """obs [B, D] f32 -> dict(logits[B,A], value[B], act[B] i32, logp[B]) via one fused kernel."""
    obs = _chk(obs, torch.float32, "obs")
    B, D = obs.shape
    dev = obs.device
    m = POLICY_MODES[mode]
    # preallocated outputs (graph capture): out = dict(logits, value, act, logp), entries may be None (not wanted)
    want = dict(logits=want_logits, value=want_value, act=m in (1, 2), logp=want_logp and m != 0) if out is None else \
        {k: out.get(k) is not None for k in ("logits", "value", "act", "logp")}
    res = {k: _out("policy_forward", (out or {}).get(k), (B, n_act) if k == "logits" else (B,),
                   torch.int32 if k == "act" else torch.float32, dev, k, "min") if want[k] else None for k in want}
    if m == 3:
        res["act"] = _chk(act, torch.int32, "act")
    call("tsm_policy_forward", ptr(_chk(params, torch.float32, "params")), ptr(image), D, hidden, n_act, ptr(obs), B, m,
         *_philox("policy_forward", seed, offset, offset_dev), ptr(res["logits"]), ptr(res["value"]), ptr(res["act"]),
         ptr(res["logp"]), stream_ptr())
    return res


def policy_image(obs_dim: int, hidden: int, n_act: int, device):
    """(zero image f32[elems], map i32[P]) of the padded LDS-layout parameter copy."""
    import numpy as np

    n_img = call("tsm_policy_image_elems", obs_dim, hidden, n_act)
    if n_img < 0:  # layout too small for the padded staging copy: kernels re-pack `params` themselves
        return None, None
    n_par = policy_param_count(obs_dim, hidden, n_act)
    m = np.zeros(n_par, np.int32)
    call("tsm_policy_image_map", obs_dim, hidden, n_act, m.ctypes.data_as(C.c_void_p))
    return torch.zeros(n_img, dtype=torch.float32, device=device), torch.from_numpy(m).to(device)


def scatter_image(params, image, image_map):
    if image is None:
        return None
    if not params.is_cuda:  # a host net (tests, checkpoint tools): the same placement, by indexing
        image[image_map.long()] = params
        return image
    call("tsm_scatter_image", ptr(params), params.numel(), ptr(image_map), ptr(image), stream_ptr())
    return image


def ppo_finalize_many(partial, stride_elems: int, n_blocks_dev, M_dev, cfg: tsm_ppo_cfg, scalars_out):
    """scalars_out[k] = {loss, clip, vf, ent} of gradient step k from its loss partials (one launch for all k).
    scalars_out may be a pinned host tensor (mapped memory: the kernel writes it directly, no D2H copy)."""
    call("tsm_ppo_finalize_many", ptr(partial), stride_elems, ptr(_chk(n_blocks_dev, torch.int32, "n_blocks")),
         ptr(_chk(M_dev, torch.int64, "M")), scalars_out.shape[0], C.byref(cfg),
         _out_or_pinned("ppo_finalize_many", scalars_out, 4 * scalars_out.shape[0], "scalars_out"), stream_ptr())
    return scalars_out


def ppo_update_grid(M: int, max_blocks: int = 0) -> int:
    if not max_blocks:
        max_blocks = int(os.environ.get("TSM_UPDATE_MAX_BLOCKS", "0"))  # (A/B timing of the slab count; default: the rule)
    return call("tsm_ppo_update_grid", M, max_blocks)


def ppo_update_fused(params, obs, act, logp_old, adv, returns, cfg: tsm_ppo_cfg, n_act: int, hidden: int = 64,
                     adv_stats=None, v_s_old=None, perm=None, first_row=0, M=None, n_blocks=None,
                     slabs=None, partial=None, scalars=None, opt_step_dev=None, image=None, want_scalars=True, packed=None):
    """One PPO gradient step up to the gradients -> (grad_slabs[n_blocks, P], scalars[4]).
    packed: the minibatch's rows as tile records (`ppo_pack_workspace(...)["rows"](k)`, written by `ppo_pack_minibatches` from
    these arrays and this perm) -- read instead of perm's rows when `image` is given; same bits."""
    obs = _chk(obs, torch.float32, "obs")
    D = obs.shape[-1]
    if M is None:
        M = perm.numel() if perm is not None else obs.shape[0] - first_row
    if n_blocks is None:
        n_blocks = ppo_update_grid(M)
    P = params.numel()
    dev = obs.device
    slabs, partial = _rows_slabs("ppo_update_fused", n_blocks, P, dev, slabs, partial)
    if perm is not None and perm.numel() < M:
        raise ValueError(f"ppo_update_fused: perm holds {perm.numel()} row ids, M = {M}")
    if scalars is not None or want_scalars:
        scalars = _out("ppo_update_fused", scalars, (4,), torch.float32, dev, "scalars", "min")
    args = (ptr(_chk(params, torch.float32, "params")), ptr(image), D, hidden, n_act, ptr(obs),
            ptr(_chk(act, torch.int32, "act")), ptr(_chk(logp_old, torch.float32, "logp_old")),
            ptr(_chk(adv, torch.float32, "adv")), ptr(_chk(returns, torch.float32, "returns")), ptr(v_s_old),
            ptr(perm), first_row, M, ptr(adv_stats), C.byref(cfg), n_blocks, ptr(slabs), ptr(partial), ptr(scalars),
            ptr(opt_step_dev))
    if packed is None:
        call("tsm_ppo_update_fused", *args, stream_ptr())
        return slabs, scalars
    need = (M + 15) // 16 * ppo_packed_record_elems(D)
    if _chk(packed, torch.float32, "packed").numel() < need:  # the kernel reads ceil(M / 16) records: never launch onto fewer
        raise ValueError(f"ppo_update_fused: packed holds {packed.numel()} words, {M} rows of width {D} need {need}")
    call("tsm_ppo_update_fused_packed", *args, ptr(packed), stream_ptr())
    return slabs, scalars


# ---- the 128-wide "rows" kernels (csrc/rows128_dev.h): what their wrappers check and allocate alike ----
def _two_layer_relu(hidden_sizes, act: str) -> int:
    """The width of two equal hidden layers under ReLU -- the only net the rows kernels are written for -- else 0."""
    hs = list(hidden_sizes)
    return hs[0] if act == "relu" and len(hs) == 2 and hs[0] == hs[1] else 0


def _mlp3_param_count(in_dim: int, hidden: int, n_out: int) -> int:
    """w0[H][in] b0[H] w1[H][H] b1[H] w2[n_out][H] b2[n_out]"""
    return hidden * in_dim + hidden + hidden * hidden + hidden + n_out * hidden + n_out


def _rows_ids(name: str, ids_name: str, ids, count_name: str, count, first_row: int, n_rows: int):
    """(count, ids) of a rows kernel's minibatch: the ids given (i64, at least `count` of them) or rows first_row + i;
    `count` defaults to every id, or to every row from first_row on."""
    if count is None:
        count = ids.numel() if ids is not None else n_rows - first_row
    if ids is not None:
        ids = _chk(ids, torch.int64, ids_name)
        if ids.numel() < count:
            raise ValueError(f"{name}: {ids_name} holds {ids.numel()} ids, {count_name} = {count}")
    return count, ids


def _rows_slabs(name: str, n_blocks: int, P: int, dev, slabs=None, partial=None):
    """(grad slabs f32 [n_blocks, P], loss partials f64 [n_blocks * 4]) of a gradient step: the caller's, if they are large
    enough, else new ones.  P = 0: the partials alone (the slabs live in the step's workspace)."""
    if P:  # the kernel writes n_blocks slabs of P floats: never launch into a smaller buffer
        slabs = _out(name, slabs, (n_blocks, P), torch.float32, dev, "slabs", "min")
    return slabs, _out(name, partial, (n_blocks * 4,), torch.float64, dev, "partial", "min")


def ppo_actor_rows_supported(obs_dim: int, hidden_sizes, n_act: int, act: str = "relu") -> bool:
    """Does the one-launch actor step (csrc/ppo_rows.hip) cover this actor?  obs -> 128 -> 128 -> n_act, ReLU."""
    H = _two_layer_relu(hidden_sizes, act)
    ok = bool(H) and bool(call("tsm_ppo_actor_rows_supported", obs_dim, H, n_act))
    if ok:
        _ppo_rows_init()
    return ok


_ppo_rows_ready = False


def _ppo_rows_init() -> None:
    """The rows kernels' LDS attributes, set when a host first asks whether they serve its nets -- at construction time,
    outside any stream capture (tsm_ppo_rows_init)."""
    global _ppo_rows_ready
    if not _ppo_rows_ready and torch.cuda.is_available():
        call("tsm_ppo_rows_init")
        _ppo_rows_ready = True


def ppo_actor_rows_grid(M: int) -> int:
    return call("tsm_ppo_actor_rows_grid", M)


def ppo_actor_rows_update(actor_params, obs, act, logp_old, adv, cfg: tsm_ppo_cfg, n_act: int, hidden: int = 128,
                          adv_stats=None, perm=None, first_row=0, M=None, n_blocks=None, slabs=None, partial=None,
                          opt_step_dev=None):
    """Actor half of one PPO gradient step in one launch -> (grad_slabs [n_blocks, P_actor], loss partials f64
    [n_blocks, 4] = {sum clip objective, 0, sum entropy, 0}).  opt_step_dev (device i64[1]): advanced by one."""
    obs = _chk(obs, torch.float32, "obs")
    D = obs.shape[-1]
    M, perm = _rows_ids("ppo_actor_rows_update", "perm", perm, "M", M, first_row, obs.shape[0])
    if n_blocks is None:
        n_blocks = ppo_actor_rows_grid(M)
    P = actor_params.numel()
    if P != call("tsm_ppo_actor_rows_param_count", D, hidden, n_act):
        raise ValueError(f"ppo_actor_rows_update: {P} actor parameters do not match obs {D} -> {hidden} -> {hidden} -> {n_act}")
    slabs, partial = _rows_slabs("ppo_actor_rows_update", n_blocks, P, obs.device, slabs, partial)
    call("tsm_ppo_actor_rows_update", ptr(_chk(actor_params, torch.float32, "actor_params")), D, hidden, n_act, ptr(obs),
         ptr(_chk(act, torch.int32, "act")), ptr(None if logp_old is None else _chk(logp_old, torch.float32, "logp_old")),
         ptr(None if adv is None else _chk(adv, torch.float32, "adv")), ptr(perm), first_row, M, ptr(adv_stats), C.byref(cfg),
         n_blocks, ptr(slabs), ptr(partial), ptr(opt_step_dev), stream_ptr())
    return slabs, partial


def ppo_critic_rows_supported(in_dim: int, hidden_sizes, n_agent: int, act: str = "relu") -> bool:
    """Does the one-launch critic step (csrc/ppo_rows.hip) cover this critic?  in_dim -> 128 -> 128 -> 1, ReLU."""
    H = _two_layer_relu(hidden_sizes, act)
    n_slice = -(-in_dim // 32)
    ok = bool(H) and n_slice in (1, 2, 3) and bool(call("tsm_ppo_critic_rows_supported", in_dim, H, n_agent))
    if ok:
        _ppo_rows_init()
    return ok


def ppo_critic_rows_grid(Mr: int) -> int:
    return call("tsm_ppo_critic_rows_grid", Mr)


def ppo_critic_rows_update(critic_params, obs_rows, returns, cfg: tsm_ppo_cfg, n_agent: int, hidden: int = 128, v_s_old=None,
                           rows=None, first_row=0, Mr=None, n_blocks=None, slabs=None, partial=None):
    """Critic half of one PPO gradient step in one launch -> (grad_slabs [n_blocks, P_critic], loss partials f64
    [n_blocks, 4] = {0, sum vf, 0, 0}).  obs_rows [n, in_dim]: the joint rows (in_dim = n_agent * obs_dim)."""
    obs_rows = _chk(obs_rows, torch.float32, "obs_rows")
    K1 = obs_rows.shape[-1]
    Mr, rows = _rows_ids("ppo_critic_rows_update", "rows", rows, "Mr", Mr, first_row, obs_rows.shape[0])
    if n_blocks is None:
        n_blocks = ppo_critic_rows_grid(Mr)
    P = critic_params.numel()
    if P != call("tsm_ppo_critic_rows_param_count", K1, hidden):
        raise ValueError(f"ppo_critic_rows_update: {P} critic parameters do not match {K1} -> {hidden} -> {hidden} -> 1")
    slabs, partial = _rows_slabs("ppo_critic_rows_update", n_blocks, P, obs_rows.device, slabs, partial)
    _critic_rows_init(K1, hidden)
    call("tsm_ppo_critic_rows_update", ptr(_chk(critic_params, torch.float32, "critic_params")), K1, hidden, n_agent,
         ptr(obs_rows), ptr(_chk(returns, torch.float32, "returns")), ptr(v_s_old), ptr(rows), first_row, Mr, C.byref(cfg),
         n_blocks, ptr(slabs), ptr(partial), stream_ptr())
    return slabs, partial


def critic_rows_forward_supported(in_dim: int, hidden_sizes, n_out: int = 1, act: str = "relu") -> bool:
    """Does the one-launch critic forward (csrc/critic_rows.hip) cover this critic?  in -> 128 -> 128 -> n_out <= 16, ReLU
    (n_out > 1: the value is the mean of the outputs)."""
    H = _two_layer_relu(hidden_sizes, act)
    return bool(H) and 1 <= n_out <= 16 and bool(call("tsm_critic_rows_forward_supported", in_dim, H))


_critic_rows_ready: set = set()


def _critic_rows_init(K1: int, hidden: int) -> None:
    """One-time function attributes (dynamic LDS size) of the one-launch critic kernels serving this input width; must
    happen outside any stream capture."""
    if (K1, hidden) in _critic_rows_ready:
        return
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("one-launch critic kernels: first use inside a stream capture; run them (or "
                           "ops.call('tsm_critic_rows_init', in_dim, hidden)) once before capturing")
    call("tsm_critic_rows_init", K1, hidden)
    _critic_rows_ready.add((K1, hidden))


def critic_rows_forward(critic_params, obs_rows, hidden: int = 128, rows=None, first_row: int = 0, Mr=None, run_if=None,
                        out=None, n_out: int = 1):
    """V(row) for Mr rows of obs_rows [n, in_dim] (row ids `rows`, or first_row + i) in ONE launch -> values [Mr]
    (n_out > 1: the mean of the critic's outputs).  run_if (device i32[1]): the launch is a no-op (and `out` is left
    as it is) when it holds 0."""
    obs_rows = _chk(obs_rows, torch.float32, "obs_rows")
    K1 = obs_rows.shape[-1]
    Mr, rows = _rows_ids("critic_rows_forward", "rows", rows, "Mr", Mr, first_row, obs_rows.shape[0])
    if rows is None and first_row + Mr > obs_rows.shape[0]:
        raise ValueError(f"critic_rows_forward: rows [{first_row}, {first_row + Mr}) exceed the {obs_rows.shape[0]} given")
    if critic_params.numel() != _mlp3_param_count(K1, hidden, n_out):
        raise ValueError(f"critic_rows_forward: {critic_params.numel()} parameters do not match {K1} -> {hidden} -> {hidden} -> {n_out}")
    _critic_rows_init(K1, hidden)
    out = _out("critic_rows_forward", out, (Mr,), torch.float32, obs_rows.device, size="min")
    call("tsm_critic_rows_forward", ptr(_chk(critic_params, torch.float32, "critic_params")), K1, hidden, n_out, ptr(obs_rows),
         ptr(rows), first_row, Mr,
         ptr(None if run_if is None else _chk(run_if, torch.int32, "run_if")), ptr(out), stream_ptr())
    return out


def critic_rows_grad_supported(in_dim: int, hidden_sizes, n_out: int = 1, act: str = "relu") -> bool:
    """Does the two-launch critic gradient step (csrc/critic_train.hip + critic_dw1.hip) cover this critic?"""
    return critic_rows_forward_supported(in_dim, hidden_sizes, n_out, act) and (in_dim % 4 == 0 or in_dim <= 64)


def _critic_grad_ws(K1: int, hidden: int, n_out: int, Mr: int, td: bool, dev, ws: dict | None, split_dw2: bool = False):
    """(n_blocks, n_chunks, dh1, rest slabs, w1 slabs, partial) for a gradient step of Mr rows; cached in `ws` (the
    buffers are what captured graphs hold on to).  split_dw2: + the published H1 / dH2 and the dW2 chunk slabs; the rest slabs
    start as zeros (their W2 columns are never written in that mode)."""
    nb = call("tsm_critic_rows_grad_grid", Mr, int(td))
    nc = call("tsm_critic_rows_dw1_chunks", Mr, K1)
    key = ("critic_grad", K1, hidden, n_out, Mr, td, bool(split_dw2))
    w = None if ws is None else ws.get(key)
    if w is None:
        n_rest = _mlp3_param_count(K1, hidden, n_out) - hidden * K1
        w = dict(nb=nb, nc=nc, dh1=torch.empty(Mr, hidden, dtype=torch.float32, device=dev),
                 rest=(torch.zeros if split_dw2 else torch.empty)(nb, n_rest, dtype=torch.float32, device=dev),
                 w1=torch.empty(nc, hidden * K1, dtype=torch.float32, device=dev),
                 partial=torch.zeros(nb * 4, dtype=torch.float64, device=dev))
        if split_dw2:
            w.update(h1=torch.empty(Mr, hidden, dtype=torch.float32, device=dev),
                     dh2=torch.empty(Mr, hidden, dtype=torch.float32, device=dev),
                     w2=torch.empty(nc, hidden * hidden, dtype=torch.float32, device=dev))
        if ws is not None:
            ws[key] = w
    return w


def _side_reductions(side):
    """[(slabs [n_slab, stride >= n], out [n]), ...] (at most two) -> (ctypes array or None, count): slab sets summed to one
    row each by extra workgroups of the dW1 launch (include/tsmarl.h: tsm_slab_reduce)."""
    if not side:
        return None, 0
    if len(side) > 2:
        raise ValueError("at most two side reductions ride on the dW1 launch")
    arr = (_abi.tsm_slab_reduce * len(side))()
    for k, (sl, out) in enumerate(side):
        sl, out = _chk(sl, torch.float32, "side slabs"), _out("side reduction", out, out.shape, torch.float32, None)
        if sl.dim() != 2 or out.numel() > sl.shape[1]:
            raise ValueError("side reduction: slabs [n_slab, >= n] and out [n] expected")
        arr[k] = _abi.tsm_slab_reduce(ptr(sl), out.numel(), int(sl.shape[1]), int(sl.shape[0]), 0, ptr(out))
    return arr, len(side)


def critic_rows_grad_ppo(critic_params, obs_rows, returns, cfg: tsm_ppo_cfg, n_agent: int, hidden: int = 128, v_s_old=None,
                         rows=None, first_row=0, Mr=None, partial=None, ws: dict | None = None, w1_image=None, side_reduce=None,
                         split_dw2: bool = False):
    """Critic half of one PPO gradient step on joint rows in two launches -> (w1_slabs [n_chunks, H * in_dim],
    rest_slabs [n_blocks, P - H * in_dim], partial f64 [n_blocks * 4] = {0, sum vf, 0, 0} per workgroup): feed the two slab
    arrays to `adam_step_segs` as segments (W1 first).  `partial`: where to leave the loss partials (>= n_blocks * 4).
    w1_image: the first-layer weights in fragment order (`critic_w1_image`; must hold the values of critic_params' w0).
    side_reduce: [(slabs, out), ...] -- other kernels' complete slab sets summed to one row each inside the dW1 launch; an
    entry whose slabs is the string "rest" names this step's own rest slabs.
    split_dw2: the first launch publishes H1 / dH2 instead of forming dW2 (a rank-32 update per tile as a 64 KB slab) and the
    second forms dW2 = dH2^T H1 over its row chunks beside dW1: the W2 gradient is then `ws[...]["w2"]` [n_chunks, H * H] and the
    W2 columns of `rest` stay zero -- `critic_grad_segs` lists the optimizer's segments for either mode."""
    obs_rows = _chk(obs_rows, torch.float32, "obs_rows")
    K1 = obs_rows.shape[-1]
    Mr, rows = _rows_ids("critic_rows_grad_ppo", "rows", rows, "Mr", Mr, first_row, obs_rows.shape[0])
    if critic_params.numel() != call("tsm_critic_rows_param_count", K1, hidden, 1):
        raise ValueError(f"critic_rows_grad_ppo: {critic_params.numel()} parameters do not match {K1} -> {hidden} -> {hidden} -> 1")
    _critic_rows_init(K1, hidden)
    w = _critic_grad_ws(K1, hidden, 1, Mr, False, obs_rows.device, ws, split_dw2)
    _, part = _rows_slabs("critic_rows_grad_ppo", w["nb"], 0, None, None, w["partial"] if partial is None else partial)
    call("tsm_critic_rows_grad_ppo", ptr(_chk(critic_params, torch.float32, "critic_params")), ptr(w1_image), K1, hidden, n_agent,
         ptr(obs_rows), ptr(_chk(returns, torch.float32, "returns")), ptr(v_s_old), ptr(rows), first_row, Mr, C.byref(cfg),
         w["nb"], ptr(w["dh1"]), ptr(w.get("h1")), ptr(w.get("dh2")), ptr(w["rest"]), ptr(part), stream_ptr())
    side = [(w["rest"] if isinstance(sl, str) else sl, out) for sl, out in (side_reduce or [])]
    arr, n_side = _side_reductions(side)
    call("tsm_critic_rows_dw1", ptr(w["dh1"]), ptr(obs_rows), K1, ptr(rows), first_row, 0, 0, Mr, w["nc"], ptr(w["w1"]),
         ptr(w.get("dh2")), ptr(w.get("h1")), ptr(w.get("w2")), arr, n_side, stream_ptr())
    return w["w1"], w["rest"], part


def critic_grad_segs(w: dict, offset: int, K1: int, hidden: int = 128, n_out: int = 1, w1_image=None, rest_row=None) -> list:
    """The optimizer's slab segments (`adam_step_segs` / `reduce_slabs_segs`) for the critic gradients a `critic_rows_grad_*`
    call left in workspace `w`, the critic's parameters starting at `offset` of the flat vector.  Plain mode: W1 chunk slabs |
    rest slabs (or `rest_row`, their side-reduced sum [1, n_rest]).  split_dw2 mode: W1 chunks | b1 (a column view of the rest
    slabs) | W2 chunks | b2, W3, b3 (another view)."""
    nW1, H = hidden * K1, hidden
    if "w2" not in w:
        rest = w["rest"] if rest_row is None else rest_row
        return [(w["w1"], offset, nW1, None, w1_image), (rest, offset + nW1, w["rest"].shape[1])]
    tail = H + n_out * H + n_out
    return [(w["w1"], offset, nW1, None, w1_image), (w["rest"], offset + nW1, H),
            (w["w2"], offset + nW1 + H, H * H), (w["rest"], offset + nW1 + H + H * H, tail, None, None, H + H * H)]


def critic_rows_grad_td(critic_params, joint_store, T: int, E: int, rew, terminated, agent: int, n_agent: int, v_last,
                        gamma: float, n_out: int, hidden: int = 128, partial=None, ws: dict | None = None, v_next_full=None,
                        use_full=None):
    """The critic half of CTDEPolicy.learn (ctde.py:149-172, 188-190) on CHAINED rows in two launches.
    joint_store f32 [T, E, in_dim] (time-major joint rows), rew f32 / terminated u8 [T, E, n_agent] (agent column `agent`),
    v_last f32 [E].  use_full (device i32[1]) != 0: targets take v_next_full [T * E] (env-major V(obs_next)) instead of the
    next row's value.  -> (w1_slabs, rest_slabs, partial f64 = {sum adv, sum sq, 0, 0} per workgroup)."""
    joint_store = _chk(joint_store, torch.float32, "joint_store")
    K1 = joint_store.shape[-1]
    B = T * E
    if joint_store.numel() < B * K1 or rew.numel() < B * n_agent or terminated.numel() < B * n_agent or v_last.numel() < E:
        raise ValueError("critic_rows_grad_td: store tensors are smaller than T x E")
    if critic_params.numel() != call("tsm_critic_rows_param_count", K1, hidden, n_out):
        raise ValueError(f"critic_rows_grad_td: {critic_params.numel()} parameters do not match {K1} -> {hidden} -> {hidden} -> {n_out}")
    _critic_rows_init(K1, hidden)
    w = _critic_grad_ws(K1, hidden, n_out, B, True, joint_store.device, ws)
    _, part = _rows_slabs("critic_rows_grad_td", w["nb"], 0, None, None, w["partial"] if partial is None else partial)
    term = terminated.view(torch.uint8) if terminated.dtype == torch.bool else _chk(terminated, torch.uint8, "terminated")
    call("tsm_critic_rows_grad_td", ptr(_chk(critic_params, torch.float32, "critic_params")), None, K1, hidden, n_out,
         ptr(joint_store), T, E, ptr(_chk(rew, torch.float32, "rew")), ptr(term), n_agent, agent,
         ptr(_chk(v_last, torch.float32, "v_last")), ptr(None if v_next_full is None else _chk(v_next_full, torch.float32, "v_next_full")),
         ptr(None if use_full is None else _chk(use_full, torch.int32, "use_full")), float(gamma), w["nb"], ptr(w["dh1"]),
         ptr(w["rest"]), ptr(part), stream_ptr())
    call("tsm_critic_rows_dw1", ptr(w["dh1"]), ptr(joint_store), K1, None, 0, T, E, B, w["nc"], ptr(w["w1"]), None, None, None,
         None, 0, stream_ptr())
    return w["w1"], w["rest"], part


def ctde_finalize(critic_partial, nb_c: int, actor_partial, nb_a: int, B: int, scalars_out, mean_adv_out):
    """{actor_loss, critic_loss} and mean(advantage) of CTDEPolicy.learn from the kernels' partial sums (one launch).
    scalars_out: device f32[2] or pinned host f32[2]; mean_adv_out: device f32[1]."""
    call("tsm_ctde_finalize", ptr(_chk(critic_partial, torch.float64, "critic_partial")), nb_c,
         ptr(_chk(actor_partial, torch.float64, "actor_partial")), nb_a, B, _out_or_pinned("ctde_finalize", scalars_out, 2, "scalars_out"),
         ptr(_out("ctde_finalize", mean_adv_out, (1,), torch.float32, None, "mean_adv_out", "min")), stream_ptr())
    return scalars_out


def ppo_value_loss(value, returns, cfg: tsm_ppo_cfg, M: int, v_s_old=None, perm=None, first_row=0, partial=None):
    """Value term of the PPO loss alone (loss_kind = 2) for M samples whose values are `value` (one per sample, or one
    per joint row with cfg.value_group = N) -> (dvalue [len(value)], loss partials f64 [blocks, 4] = {0, sum vf, 0, 0})."""
    value = _chk(value, torch.float32, "value").reshape(-1)
    vg = max(1, int(cfg.value_group))
    if value.numel() * vg != M:
        raise ValueError(f"ppo_value_loss: {value.numel()} values for {M} samples with value_group={vg}")
    if cfg.loss_kind != 2:
        raise ValueError("ppo_value_loss needs a cfg with loss_kind = 2")
    dev = value.device
    dvalue = torch.empty(value.numel(), dtype=torch.float32, device=dev)
    partial = _out("ppo_value_loss", partial, (call("tsm_ppo_loss_partial_elems", M),), torch.float64, dev, "partial", "min")
    call("tsm_ppo_loss_fwd_bwd", None, ptr(value), None, None, None, ptr(_chk(returns, torch.float32, "returns")),
         ptr(v_s_old), ptr(perm), first_row, M, 1, None, C.byref(cfg), None, ptr(dvalue), ptr(partial), stream_ptr())
    return dvalue, partial


def ppo_loss_partial_elems(M: int) -> int:
    return call("tsm_ppo_loss_partial_elems", M)


# --------------------------------------------------------------------------------------------
# CTDE (ctde.py:291-300)
# --------------------------------------------------------------------------------------------
def global_state(obs_by_agent, mode: str = "concatenate") -> torch.Tensor:
    """obs_by_agent: list of [B, D] f32 tensors in env.agents order."""
    if mode not in ("concatenate", "mean"):
        raise ValueError(f"unsupported global-state mode {mode!r} (concatenate | mean)")
    obs = [_chk(o, torch.float32, "obs") for o in obs_by_agent]
    N = len(obs)
    B, D = obs[0].shape
    arr = (C.c_void_p * N)(*[ptr(o) for o in obs])
    out = torch.empty((B, N * D) if mode == "concatenate" else (B, D), dtype=torch.float32, device=obs[0].device)
    call("tsm_global_state", arr, N, B, D, 0 if mode == "concatenate" else 1, ptr(out), stream_ptr())
    return out


def random_permutations(n: int, n_perm: int, seed: int, counter: int = 0, counter_dev=None, scale: int = 1,
                        group_size: int = 1, offset_mul: int = 0, out=None, device="cuda", advance: int = 0, done_ctr=None):
    """n_perm pseudo-random permutations of range(n) in one launch -> i64 [n_perm, n] (batch.py:1219 on device).
    out[p, i] = pi_p(i) * scale + (p // group_size) * offset_mul.
    advance > 0 (with counter_dev and done_ctr, a zeroed u32[1] of this call site): the launch itself adds `advance` to
    *counter_dev once every workgroup has read it -- the draws of counter = 0 followed by tsm_u64_add, in one launch."""
    if n < 0 or n_perm < 0:
        raise ValueError("random_permutations: negative size")
    out = _out("random_permutations", out, (n_perm, n), torch.int64, device, size="numel")
    seed, counter, ctr_p = _philox("random_permutations", seed, counter, counter_dev)
    if advance:
        if counter or counter_dev is None or done_ctr is None:
            raise ValueError("random_permutations: advance needs counter_dev and done_ctr, and no host counter")
        call("tsm_random_permutations_advance", n, n_perm, seed, ctr_p, int(advance),
             ptr(_out("random_permutations", done_ctr, (1,), torch.int32, None, "done_ctr", "min")), scale, group_size, offset_mul,
             ptr(out), stream_ptr())
        return out
    call("tsm_random_permutations", n, n_perm, seed, counter, ctr_p, scale, group_size, offset_mul, ptr(out), stream_ptr())
    return out


def ctde_td_head(q, q_next, rew, terminated, gamma: float, logits, act):
    """CTDEPolicy.learn loss head (ctde.py:149-185) -> (dq, dlogits, scalars[actor_loss, critic_loss])."""
    q, q_next = _chk(q, torch.float32, "q"), _chk(q_next, torch.float32, "q_next")
    B, n_out = q.shape
    logits = _chk(logits, torch.float32, "logits")
    A = logits.shape[1]
    dev = q.device
    dq, dlogits = torch.empty_like(q), torch.empty_like(logits)
    partial = torch.empty(call("tsm_ctde_head_partial_elems", B), dtype=torch.float64, device=dev)
    scalars = torch.empty(2, dtype=torch.float32, device=dev)
    call("tsm_ctde_td_head", ptr(q), ptr(q_next), n_out, ptr(_chk(rew, torch.float32, "rew").reshape(-1)),
         ptr(_chk(terminated, torch.uint8, "terminated").reshape(-1)), float(gamma), ptr(logits),
         ptr(_chk(act, torch.int64, "act").reshape(-1)), A, B, ptr(dq), ptr(dlogits), ptr(partial), ptr(scalars),
         stream_ptr())
    return dq, dlogits, scalars


# --------------------------------------------------------------------------------------------
# learned global states (ctde.py:230-343, modes "attention" and "graph"; csrc/gstate.hip)
# --------------------------------------------------------------------------------------------
def gstate_check(n_agents: int, obs_dim: int) -> None:
    """The bounds of the attention kernels (include/tsmarl.h): ValueError naming the limit."""
    N, D, heads = int(n_agents), int(obs_dim), _abi.GSTATE_HEADS
    if not 1 <= N <= _abi.GSTATE_MAX_AGENTS:
        raise ValueError(f"gstate: n_agents = {N}; the HIP kernels serve 1 to {_abi.GSTATE_MAX_AGENTS} agents")
    if D % heads or not heads <= D <= _abi.GSTATE_MAX_DIM:
        raise ValueError(f"gstate: obs_dim = {D}; the HIP kernels serve multiples of {heads} (the {heads} heads) from {heads} to "
                         f"{_abi.GSTATE_MAX_DIM}")


def _gstate_arg(name: str, nm: str, t, shape=None):
    """An f32 tensor, contiguous as it stands (no silent copy: the backward reads what the forward wrote), of `shape`.  Shapes
    and limits are checked before the device is: a host tensor reaches `_dev_only` with everything else in order."""
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: {nm} must be a contiguous float32 tensor, got {t.dtype}, strides {tuple(t.stride())}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {nm} must be {list(shape)}, got {list(t.shape)}")
    if nm == "qkv" and t.data_ptr() % 16:
        raise ValueError(f"{name}: qkv must be 16-byte aligned (the kernels stage it with 16-byte loads)")
    return t


def _pool_check(name: str, N: int, H: int, B: int) -> None:
    if not 1 <= N <= _abi.GSTATE_MAX_AGENTS:
        raise ValueError(f"{name}: n_agents = {N}; the HIP kernels serve 1 to {_abi.GSTATE_MAX_AGENTS} agents")
    if H < 1 or B < 1:
        raise ValueError(f"{name}: B = {B} rows of H = {H}; both at least 1")


def attn_pool_forward(qkv, n_agents: int):
    """The attention core and the mean over agents (tsm_attn_pool_forward): qkv f32 [B, N, 3 D] or [B * N, 3 D], the
    in-projection's output -> (ctx [B, D], P [B, 4, N, N])."""
    N = int(n_agents)
    _gstate_arg("attn_pool_forward", "qkv", qkv)
    if qkv.dim() not in (2, 3) or qkv.shape[-1] % 3 or qkv.numel() == 0:
        raise ValueError(f"attn_pool_forward: qkv must be a non-empty [B, N, 3 D] or [B N, 3 D], got {list(qkv.shape)}")
    D = qkv.shape[-1] // 3
    gstate_check(N, D)
    rows = qkv.numel() // (3 * D)
    if rows % N or (qkv.dim() == 3 and qkv.shape[1] != N):
        raise ValueError(f"attn_pool_forward: qkv {list(qkv.shape)} does not hold rows of n_agents = {N}")
    B = rows // N
    _dev_only("attn_pool_forward", qkv)
    ctx = torch.empty(B, D, dtype=torch.float32, device=qkv.device)
    P = torch.empty(B, _abi.GSTATE_HEADS, N, N, dtype=torch.float32, device=qkv.device)
    call("tsm_attn_pool_forward", ptr(qkv), B, N, D, ptr(ctx), ptr(P), stream_ptr())
    return ctx, P


def attn_pool_backward(d_ctx, qkv, P):
    """d_ctx [B, D], and the forward's qkv and P [B, 4, N, N] -> d_qkv [B, N, 3 D] (tsm_attn_pool_backward)."""
    _gstate_arg("attn_pool_backward", "P", P)
    if P.dim() != 4 or P.shape[1] != _abi.GSTATE_HEADS or P.shape[2] != P.shape[3] or P.numel() == 0:
        raise ValueError(f"attn_pool_backward: P must be a non-empty [B, {_abi.GSTATE_HEADS}, N, N], got {list(P.shape)}")
    B, N = P.shape[0], P.shape[2]
    _gstate_arg("attn_pool_backward", "d_ctx", d_ctx)
    if d_ctx.dim() != 2 or d_ctx.shape[0] != B:
        raise ValueError(f"attn_pool_backward: d_ctx must be [{B}, D], got {list(d_ctx.shape)}")
    D = d_ctx.shape[1]
    gstate_check(N, D)
    _gstate_arg("attn_pool_backward", "qkv", qkv)
    if qkv.numel() != B * N * 3 * D or qkv.shape[-1] != 3 * D:
        raise ValueError(f"attn_pool_backward: qkv must be [{B}, {N}, {3 * D}], got {list(qkv.shape)}")
    _dev_only("attn_pool_backward", d_ctx, qkv, P)
    d_qkv = torch.empty(B, N, 3 * D, dtype=torch.float32, device=qkv.device)
    call("tsm_attn_pool_backward", ptr(d_ctx), ptr(qkv), ptr(P), B, N, D, ptr(d_qkv), stream_ptr())
    return d_qkv


def agent_pool_forward(h, c, relu: bool = False):
    """h f32 [B, N, H], c f32 [N] -> [B, H] = sum_n c[n] f(h[:, n]) (tsm_agent_pool_forward); relu: f = max(., 0)."""
    _gstate_arg("agent_pool_forward", "h", h)
    if h.dim() != 3:
        raise ValueError(f"agent_pool_forward: h must be [B, N, H], got {list(h.shape)}")
    B, N, H = h.shape
    _pool_check("agent_pool_forward", N, H, B)
    _gstate_arg("agent_pool_forward", "c", c, (N,))
    _dev_only("agent_pool_forward", h, c)
    out = torch.empty(B, H, dtype=torch.float32, device=h.device)
    call("tsm_agent_pool_forward", ptr(h), ptr(c), B, N, H, int(bool(relu)), ptr(out), stream_ptr())
    return out


def agent_pool_backward(d, c, n_agents: int, h_relu=None):
    """d f32 [B, H], c f32 [N] -> d_h [B, N, H] = c[n] d (tsm_agent_pool_backward); h_relu [B, N, H], the input of a forward
    with relu: zero where it was not positive."""
    N = int(n_agents)
    _gstate_arg("agent_pool_backward", "d", d)
    if d.dim() != 2:
        raise ValueError(f"agent_pool_backward: d must be [B, H], got {list(d.shape)}")
    B, H = d.shape
    _pool_check("agent_pool_backward", N, H, B)
    _gstate_arg("agent_pool_backward", "c", c, (N,))
    if h_relu is not None:
        _gstate_arg("agent_pool_backward", "h_relu", h_relu, (B, N, H))
    _dev_only("agent_pool_backward", d, c, h_relu)
    d_h = torch.empty(B, N, H, dtype=torch.float32, device=d.device)
    call("tsm_agent_pool_backward", ptr(d), ptr(c), ptr(h_relu), B, N, H, ptr(d_h), stream_ptr())
    return d_h


# --------------------------------------------------------------------------------------------
# QMIX (ctde.py:417-725; csrc/qmix.hip)
# --------------------------------------------------------------------------------------------
QMIX_EMBED_DIMS = (32, 64)


def qmix_check(n_agents: int, embed_dim: int, n_act: int | None = None) -> None:
    """The bounds of the QMIX kernels (include/tsmarl.h): ValueError naming the limit."""
    if not 1 <= n_agents <= _abi.QMIX_MAX_AGENTS:
        raise ValueError(f"QMIX: n_agents = {n_agents}; the HIP kernels serve 1 to {_abi.QMIX_MAX_AGENTS} agents")
    if embed_dim not in QMIX_EMBED_DIMS:
        raise ValueError(f"QMIX: mixing_embed_dim = {embed_dim}; the HIP kernels serve {QMIX_EMBED_DIMS}")
    if n_act is not None and not 1 <= n_act <= 64:
        raise ValueError(f"QMIX: n_act = {n_act}; the HIP kernels serve 1 to 64 actions")


def qmix_partial_elems(B: int, embed_dim: int) -> int:
    return call("tsm_qmix_partial_elems", B, embed_dim)


def qmix_mix_td(q, q_next, act, rew, hyper, hyper_next, term, gamma: float, monotonic: bool = True, out=None,
                qtot_out=None):
    """Mixer forward on both sides + TD target + MSE + the mixer's backward (QMIXPolicy.learn, ctde.py:628-697).
    q, q_next: per agent [B, A] (online Q on obs, target Q on obs_next); act: per agent i64 [B]; rew: per agent f32 [B];
    hyper / hyper_next: (w1raw [B, N*E], b1 [B, E], w2raw [B, E], b2 [B, 1]) of the online / target hypernetworks;
    term: agent 0's terminated [B] (u8 / bool).  out: optional (dq list, (dw1, db1, dw2, db2), partial) to write into.
    qtot_out: optional f32 [B] that receives q_tot of every row.
    -> (dq [per agent [B, A]], (dw1, db1, dw2, db2), partial f64)."""
    N = len(q)
    B, A = q[0].shape
    E = hyper[1].shape[1]
    qmix_check(N, E, A)
    if not (len(q_next) == len(act) == len(rew) == N):
        raise ValueError("qmix_mix_td: q, q_next, act and rew need one entry per agent")
    for k, (x, x1) in enumerate(zip(q, q_next)):
        if tuple(x.shape) != (B, A) or tuple(x1.shape) != (B, A) or act[k].numel() != B or rew[k].numel() != B:
            raise ValueError(f"qmix_mix_td: agent {k}: expected Q [{B}, {A}], act [{B}], rew [{B}]")
    for h in (hyper, hyper_next):
        if (tuple(h[0].shape) != (B, N * E) or tuple(h[1].shape) != (B, E) or tuple(h[2].shape) != (B, E)
                or h[3].numel() != B):
            raise ValueError(f"qmix_mix_td: hypernetwork outputs must be [{B}, {N * E}], [{B}, {E}], [{B}, {E}], [{B}, 1]")
    term = term.contiguous().view(torch.uint8) if term.dtype == torch.bool else _chk(term, torch.uint8, "term")
    if term.numel() != B:
        raise ValueError(f"qmix_mix_td: term must have {B} entries")
    dev = q[0].device
    dq, grads, partial = out if out is not None else ([None] * N, (None,) * 4, None)
    dq = [_out("qmix_mix_td", x, (B, A), torch.float32, dev, "dq", "min") for x in dq]
    grads = tuple(_out("qmix_mix_td", x, (B, w), torch.float32, dev, "grad", "min") for x, w in zip(grads, (N * E, E, E, 1)))
    partial = _out("qmix_mix_td", partial, (qmix_partial_elems(B, E),), torch.float64, dev, "partial", "min")
    if qtot_out is not None:
        _out("qmix_mix_td", qtot_out, (B,), torch.float32, dev, "qtot_out", "min")
    ag = _abi.tsm_qmix_agents()
    for k in range(N):
        ag.q[k] = ptr(_chk(q[k], torch.float32, "q"))
        ag.q_next[k] = ptr(_chk(q_next[k], torch.float32, "q_next"))
        ag.act[k] = ptr(_chk(act[k], torch.int64, "act"))
        ag.rew[k] = ptr(_chk(rew[k], torch.float32, "rew"))
        ag.dq[k] = ptr(dq[k])
    hp = [ptr(_chk(x, torch.float32, "hyper")) for x in (*hyper, *hyper_next)]
    call("tsm_qmix_mix_td", C.byref(ag), N, A, B, E, *hp, ptr(term), float(gamma), int(bool(monotonic)),
         *map(ptr, grads), ptr(partial), ptr(qtot_out), stream_ptr())
    return dq, grads, partial


def qmix_finalize(partial, B: int, out):
    """{loss, q_values} of QMIXPolicy.learn from tsm_qmix_mix_td's partials (one launch).  out: device f32[2] or pinned
    host f32[2]."""
    partial = _chk(partial, torch.float64, "partial")
    call("tsm_qmix_finalize", ptr(partial), partial.numel() // 2, B, _out_or_pinned("qmix_finalize", out, 2), stream_ptr())
    return out


def qmix_egreedy(q, eps_dev, seed: int, offset: int = 0, offset_dev=None, out=None, row_stride: int | None = None):
    """Epsilon-greedy actions of QMIXPolicy.forward (ctde.py:606-612) on the device: q per agent [B, A] -> act i32 with
    act[b * row_stride + i] (default [B, N]).  One coin per (call, agent); eps read from the device scalar eps_dev."""
    N = len(q)
    B, A = q[0].shape
    qmix_check(N, 32, A)
    stride = N if row_stride is None else int(row_stride)
    if out is None:
        out = torch.empty(B, stride, dtype=torch.int32, device=q[0].device)
    _out("qmix_egreedy", out, ((B - 1) * stride + N if B else 0,), torch.int32, None, size="min")  # the last row's window ends there
    arr = (C.c_void_p * N)(*[ptr(_chk(x, torch.float32, "q")) for x in q])
    call("tsm_qmix_egreedy", arr, N, B, A, ptr(_chk(eps_dev, torch.float32, "eps_dev")),
         *_philox("qmix_egreedy", seed, offset, offset_dev), ptr(out), stride, stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# n-step targets and DQN (algorithm_base.py:720-815; dqn.py; csrc/nstep.hip, csrc/dqn.hip)
# --------------------------------------------------------------------------------------------
def _head_args(name: str, B: int, shaped: tuple, per_row: tuple, note: str = "") -> list:
    """The host checks every value-based head shares.  Each (nm, x, shape, dtype) of `shaped` must have that shape, each
    (nm, x, dtype) of `per_row` B entries; None is an argument left out.  dtype uint8 also takes bool, viewed as bytes.
    -> what call(...) needs, as `*map(ptr, args)`: the contiguous tensors, `shaped` then `per_row` (flattened), in the order
    given.  The list keeps a copy made here alive until the launch is queued."""
    for nm, x, shape, _ in shaped:
        if x is not None and tuple(x.shape) != tuple(shape):
            raise ValueError(f"{name}: {nm} must be {list(shape)}{note}")
    for nm, x, _ in per_row:
        if x is not None and x.numel() != B:
            raise ValueError(f"{name}: {nm} must have {B} entries")

    def conv(nm, x, dtype):
        if x is None:
            return None
        return x.contiguous().view(torch.uint8) if dtype == torch.uint8 and x.dtype == torch.bool else _chk(x, dtype, nm)

    return [conv(nm, x, dt) for nm, x, _, dt in shaped] + \
           [None if x is None else conv(nm, x, dt).reshape(-1) for nm, x, dt in per_row]


def _target_rows(act, mc, gpow, vmask, weight) -> tuple:
    """The per-row arguments of a head that forms the n-step target itself, in the entry points' order."""
    return (("act", act, torch.int64), ("mc", mc, torch.float32), ("gpow", gpow, torch.float32),
            ("vmask", vmask, torch.uint8), ("weight", weight, torch.float32))


def _head_partial(B: int, rows_per_block: int, dev) -> torch.Tensor:
    """f64 [2 * ceil(B / rows_per_block)]: a head's pair of sums per workgroup, for `qmix_finalize`."""
    return torch.empty(2 * -(-B // rows_per_block), dtype=torch.float64, device=dev)


def dqn_check(n_act: int, n_step: int = 1) -> None:
    """The bounds of the DQN kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_dqn_check", int(n_act), int(n_step))


def lstm_check(hidden: int, layer_num: int = 1, seq_len: int = 1) -> None:
    """The bounds of the LSTM kernels (include/tsmarl.h): hidden a multiple of 16 in [16, 128], layer_num >= 1, seq_len >= 1;
    ValueError naming the limit."""
    call("tsm_lstm_check", int(hidden), int(layer_num), int(seq_len))


def _f32(name: str, what: str, t, shape):
    """`t` (None passes) as a contiguous device f32 tensor of `shape`."""
    if t is None:
        return None
    _dev_only(name, t)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be a contiguous f32 {list(shape)}, got {list(t.shape)} {t.dtype}")
    return t


def _rows2(name: str, what: str, t, width: int) -> tuple:
    """A [M, width] f32 device matrix whose rows are contiguous and `ld` floats apart -> (t, M, ld)."""
    _dev_only(name, t)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != width or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < width):
        raise ValueError(f"{name}: {what} must be f32 [M, {width}] with contiguous rows, got {list(t.shape)} {t.dtype} strides "
                         f"{tuple(t.stride())}")
    return t, t.shape[0], (t.stride(0) if t.shape[0] > 1 else width)


def dense_linear(x, W, bias, out=None):
    """out [M, O] = x [M, K] W [O, K]^T + bias [O] on the dense engine; the rows of x may be strided (a step of a sequence)."""
    O, K = W.shape
    x, M, ldx = _rows2("dense_linear", "x", x, K)
    if M < 1:
        raise ValueError("dense_linear: empty batch")
    W, bias = _f32("dense_linear", "W", W, (O, K)), _f32("dense_linear", "bias", bias, (O,))
    out = _out("dense_linear", out, (M, O), torch.float32, x.device)
    call("tsm_dense_linear", x.data_ptr(), ldx, ptr(W), ptr(bias), M, K, O, ptr(out), stream_ptr())
    return out


def dense_dgrad(dz, W, out=None):
    """dx [M, K] = dz [M, O] W [O, K]; `out` may be a strided [M, K] view (its rows contiguous)."""
    O, K = W.shape
    dz = _f32("dense_dgrad", "dz", dz, (dz.shape[0], O))
    M = dz.shape[0]
    if M < 1:
        raise ValueError("dense_dgrad: empty batch")
    W = _f32("dense_dgrad", "W", W, (O, K))
    if out is None:
        out = torch.empty(M, K, dtype=torch.float32, device=dz.device)
    out, Mo, ld = _rows2("dense_dgrad", "out", out, K)
    if Mo != M:
        raise ValueError(f"dense_dgrad: out has {Mo} rows, dz {M}")
    call("tsm_dense_dgrad", ptr(dz), ptr(W), M, O, K, out.data_ptr(), ld, stream_ptr())
    return out


def dense_wgrad(dz, x, slabs, n_split: int, w_off: int, b_off: int):
    """Weight and bias gradient of one linear layer into the slabs of a flat parameter vector: slabs [n_split, P];
    slabs[:, w_off : w_off + O K] sums to dz^T x, slabs[:, b_off : b_off + O] to the column sums of dz."""
    dz = _f32("dense_wgrad", "dz", dz, tuple(dz.shape))
    if dz.dim() != 2 or dz.shape[0] < 1:
        raise ValueError("dense_wgrad: dz must be [M, O], M >= 1")
    M, O = dz.shape
    x, Mx, ldx = _rows2("dense_wgrad", "x", x, x.shape[-1])
    K = x.shape[1]
    if Mx != M:
        raise ValueError(f"dense_wgrad: x has {Mx} rows, dz {M}")
    _dev_only("dense_wgrad", slabs)
    if slabs.dtype != torch.float32 or slabs.dim() != 2 or not slabs.is_contiguous() or slabs.shape[0] != int(n_split) or n_split < 1:
        raise ValueError(f"dense_wgrad: slabs must be a contiguous f32 [{n_split}, P]")
    P = slabs.shape[1]
    if not (0 <= w_off and w_off + O * K <= P and 0 <= b_off and b_off + O <= P):
        raise ValueError(f"dense_wgrad: the blocks at {w_off} (+{O * K}) and {b_off} (+{O}) leave the {P} floats of a slab")
    call("tsm_dense_wgrad", ptr(dz), x.data_ptr(), ldx, M, O, K, int(n_split), ptr(slabs), P, int(w_off), int(b_off), stream_ptr())
    return slabs


def _lstm_state(name: str, what: str, t, B: int, H: int):
    """A state operand: None, or f32 rows [B, H] that are contiguous and one common pitch apart (a layer of [B, layers, H])."""
    if t is None:
        return None, 0
    t, M, ld = _rows2(name, what, t, H)
    if M != B:
        raise ValueError(f"{name}: {what} has {M} rows, the batch {B}")
    return t, ld


def _one_pitch(name: str, lds) -> int:
    lds = {ld for ld in lds if ld}
    if len(lds) > 1:
        raise ValueError(f"{name}: the state operands must share one row pitch, got {sorted(lds)}")
    return lds.pop() if lds else 0


def lstm_forward(proj, w_hh, bias=None, h0=None, c0=None, h_n=None, c_n=None, save: bool = True):
    """One LSTM layer through all L steps in one launch (include/tsmarl.h: tsm_lstm_forward).  proj [B, L, 4H] = the input
    projection with b_ih; bias [4H] = b_hh; h0, c0 [B, H] or None (zeros); h_n, c_n [B, H] outputs, fresh when None, and
    allowed to BE h0, c0 (the acting step).  State operands may be strided rows of a [B, layers, H] tensor.
    -> dict(h [B, L, H], h_n, c_n, and with `save`: h_prev [B, L, H], gates [B, L, 4H], c [B, L, H])."""
    _dev_only("lstm_forward", proj, w_hh, bias)
    if proj.dim() != 3 or proj.shape[2] % 4:
        raise ValueError(f"lstm_forward: proj must be [B, L, 4H], got {list(proj.shape)}")
    B, L, H = proj.shape[0], proj.shape[1], proj.shape[2] // 4
    lstm_check(H, 1, L)
    if B < 1:
        raise ValueError("lstm_forward: empty batch")
    proj, w_hh = _f32("lstm_forward", "proj", proj, (B, L, 4 * H)), _f32("lstm_forward", "w_hh", w_hh, (4 * H, H))
    bias = _f32("lstm_forward", "bias", bias, (4 * H,))
    dev = proj.device
    if h_n is None:
        h_n = torch.empty(B, H, dtype=torch.float32, device=dev)
    if c_n is None:
        c_n = torch.empty(B, H, dtype=torch.float32, device=dev)
    (h0, l0), (c0, l1) = _lstm_state("lstm_forward", "h0", h0, B, H), _lstm_state("lstm_forward", "c0", c0, B, H)
    (h_n, l2), (c_n, l3) = _lstm_state("lstm_forward", "h_n", h_n, B, H), _lstm_state("lstm_forward", "c_n", c_n, B, H)
    ld = _one_pitch("lstm_forward", (l0, l1, l2, l3))
    out = dict(h=torch.empty(B, L, H, dtype=torch.float32, device=dev), h_n=h_n, c_n=c_n)
    if save:
        out.update(h_prev=torch.empty(B, L, H, dtype=torch.float32, device=dev),
                   gates=torch.empty(B, L, 4 * H, dtype=torch.float32, device=dev),
                   c=torch.empty(B, L, H, dtype=torch.float32, device=dev))
    dp = lambda t: None if t is None else t.data_ptr()  # noqa: E731  (strided rows: `ptr` wants contiguous tensors)
    call("tsm_lstm_forward", ptr(proj), ptr(w_hh), ptr(bias), dp(h0), dp(c0), ld, B, L, H, ptr(out["h"]), ptr(out.get("h_prev")),
         ptr(out.get("gates")), ptr(out.get("c")), dp(h_n), dp(c_n), stream_ptr())
    return out


def lstm_backward(d_h, w_hh, gates, c, c0=None, d_hn=None, d_cn=None, want_state_grad: bool = False):
    """The backward through time of `lstm_forward` in one launch: d_h [B, L, H] arriving at every step from above, d_hn, d_cn
    [B, H] or None at the final state; gates, c as saved; c0 as given to the forward.
    -> dict(d_gates [B, L, 4H], and with `want_state_grad`: d_h0, d_c0 [B, H])."""
    _dev_only("lstm_backward", d_h, w_hh, gates, c)
    if d_h.dim() != 3:
        raise ValueError(f"lstm_backward: d_h must be [B, L, H], got {list(d_h.shape)}")
    B, L, H = d_h.shape
    lstm_check(H, 1, L)
    if B < 1:
        raise ValueError("lstm_backward: empty batch")
    d_h, w_hh = _f32("lstm_backward", "d_h", d_h, (B, L, H)), _f32("lstm_backward", "w_hh", w_hh, (4 * H, H))
    gates, c = _f32("lstm_backward", "gates", gates, (B, L, 4 * H)), _f32("lstm_backward", "c", c, (B, L, H))
    dev = d_h.device
    out = dict(d_gates=torch.empty(B, L, 4 * H, dtype=torch.float32, device=dev))
    if want_state_grad:
        out.update(d_h0=torch.empty(B, H, dtype=torch.float32, device=dev), d_c0=torch.empty(B, H, dtype=torch.float32, device=dev))
    states = [_lstm_state("lstm_backward", n, t, B, H) for n, t in (("c0", c0), ("d_hn", d_hn), ("d_cn", d_cn),
                                                                    ("d_h0", out.get("d_h0")), ("d_c0", out.get("d_c0")))]
    ld = _one_pitch("lstm_backward", [l for _, l in states])
    dp = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    c0, d_hn, d_cn, d_h0, d_c0 = (t for t, _ in states)
    call("tsm_lstm_backward", ptr(d_h), dp(d_hn), dp(d_cn), ptr(w_hh), ptr(gates), ptr(c), dp(c0), ld, B, L, H, ptr(out["d_gates"]),
         dp(d_h0), dp(d_c0), stream_ptr())
    return out


def lstm_state_reset(h, c, done, rows_per_env: int = 1) -> None:
    """Zero the state rows of finished envs in place (collector.py:977-979): h, c f32 [E * rows_per_env, ...], done u8 / bool
    [E].  One launch without a host read: safe inside a captured graph."""
    _dev_only("lstm_state_reset", h, c, done)
    done = done.contiguous().view(torch.uint8) if done.dtype == torch.bool else _chk(done, torch.uint8, "done")
    E, R = done.numel(), int(rows_per_env)
    if R < 1 or h.shape != c.shape or h.dtype != torch.float32 or c.dtype != torch.float32 or h.dim() < 2 or h.shape[0] != E * R \
            or not (h.is_contiguous() and c.is_contiguous()):
        raise ValueError(f"lstm_state_reset: h and c must be contiguous f32 [{E * R}, ...] for {E} envs of {R} rows")
    if E:
        call("tsm_lstm_state_reset", ptr(h), ptr(c), ptr(done), E, R, h[0].numel(), stream_ptr())


def nstep_return(index: "VrbState", term_store, rew_store, indices, n_step: int, gamma: float, rew_col: int = 0,
                 term_col: int = 0):
    """The n-step walk of Algorithm.compute_nstep_return (algorithm_base.py:773-806, 1195-1211) for flat `indices` i64 [I]
    over a device buffer: `index` its VrbState, term_store u8 [S, B, ...], rew_store f32 [S, B, ...]; rew_col / term_col
    pick the agent's column.  -> (idx_n i64 [I], mc f32 [I], gpow f32 [I], vmask u8 [I])."""
    _dev_only("nstep_return", term_store, rew_store, indices)
    S, B = index.sub_size, index.buffer_num
    term_store = _chk(term_store, torch.uint8, "term_store")
    rew_store = _chk(rew_store, torch.float32, "rew_store")
    if tuple(term_store.shape[:2]) != (S, B) or tuple(rew_store.shape[:2]) != (S, B):
        raise ValueError(f"nstep_return: the stores must be [{S}, {B}, ...]")
    indices = _chk(indices, torch.int64, "indices").reshape(-1)
    I, dev = indices.numel(), indices.device
    idx_n = torch.empty(I, dtype=torch.int64, device=dev)
    mc = torch.empty(I, dtype=torch.float32, device=dev)
    gpow = torch.empty(I, dtype=torch.float32, device=dev)
    vmask = torch.empty(I, dtype=torch.uint8, device=dev)
    call("tsm_nstep_return", ptr(index.state), B, S, ptr(index.done_store), ptr(term_store), term_store[0, 0].numel(),
         int(term_col), ptr(rew_store), rew_store[0, 0].numel(), int(rew_col), ptr(indices), I, int(n_step), float(gamma),
         ptr(idx_n), ptr(mc), ptr(gpow), ptr(vmask), stream_ptr())
    return idx_n, mc, gpow, vmask


def dqn_td_head(q, q_next_online, q_next_target, act, mc, gpow, vmask, mask_next=None, weight=None, is_double: bool = True,
                huber_delta: float | None = None):
    """DQN._target_q after its forwards + the n-step target + the TD loss and its gradient (dqn.py:365-402) in one launch.
    q, q_next_online [B, A]; q_next_target [B, A] or None (no target network); act i64 [B]; mc, gpow, vmask from
    nstep_return; mask_next u8 / bool [B, A] or None; weight f32 [B] or None.
    -> dict(returns [B], td_error [B], dq [B, A], partial f64): `qmix_finalize(partial, B, out)` gives {loss, mean q}."""
    _dev_only("dqn_td_head", q, q_next_online, q_next_target, act, mc, gpow, vmask, mask_next, weight)
    q = _chk(q, torch.float32, "q")
    if q.dim() != 2:
        raise ValueError("dqn_td_head: q must be [B, A]")
    B, A = q.shape
    dqn_check(A)
    if B < 1:
        raise ValueError("dqn_td_head: empty batch")
    args = _head_args("dqn_td_head", B, (("q_next_online", q_next_online, (B, A), torch.float32),
                                         ("q_next_target", q_next_target, (B, A), torch.float32),
                                         ("mask_next", mask_next, (B, A), torch.uint8)),
                      _target_rows(act, mc, gpow, vmask, weight))
    dev = q.device
    out = dict(returns=torch.empty(B, dtype=torch.float32, device=dev), td_error=torch.empty(B, dtype=torch.float32, device=dev),
               dq=torch.empty(B, A, dtype=torch.float32, device=dev), partial=_head_partial(B, _abi.DQN_ROWS_PER_BLOCK, dev))
    call("tsm_dqn_td_head", ptr(q), *map(ptr, args), B, A, int(bool(is_double)),
         float(huber_delta) if huber_delta is not None else 0.0, ptr(out["returns"]),
         ptr(out["td_error"]), ptr(out["dq"]), ptr(out["partial"]), stream_ptr())
    return out


def dqn_egreedy(q, eps_dev, seed: int, offset: int = 0, offset_dev=None, mask=None, out=None):
    """Masked epsilon-greedy actions (dqn.py:140-141, 153-171) on the device: q [R, A], mask u8 / bool [R, A] or None ->
    act i32 [R].  One coin per ROW; eps read from the device scalar eps_dev; row r draws at Philox counter offset + r."""
    _dev_only("dqn_egreedy", q, eps_dev, mask)
    q = _chk(q, torch.float32, "q")
    if q.dim() != 2:
        raise ValueError("dqn_egreedy: q must be [R, A]")
    R, A = q.shape
    dqn_check(A)
    mask, = _head_args("dqn_egreedy", R, (("mask", mask, (R, A), torch.uint8),), ())
    out = _out("dqn_egreedy", out, (R,), torch.int32, q.device, size="min")
    call("tsm_dqn_egreedy", ptr(q), ptr(mask), R, A, ptr(_chk(eps_dev, torch.float32, "eps_dev")),
         *_philox("dqn_egreedy", seed, offset, offset_dev), ptr(out), stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# Distributional Q-learning: C51 and QR-DQN (c51.py; qrdqn.py; csrc/distq.hip)
# --------------------------------------------------------------------------------------------
def distq_check(n_act: int, n_atoms: int) -> None:
    """The bounds of the distributional kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_distq_check", int(n_act), int(n_atoms))


def distq_values(raw, n_act: int, n_atoms: int, support=None, want_probs: bool = False):
    """C51Policy.compute_q_value's expectation (support f32 [N] given: softmax over atoms, then the sum with the support;
    c51.py:67) or QRDQNPolicy.compute_q_value's mean over quantiles (support None; qrdqn.py:20), before the action mask.
    raw [R, A * N] -> q [R, A], or (q, probs [R, A, N]) with want_probs (categorical only)."""
    _dev_only("distq_values", raw, support)
    raw = _chk(raw, torch.float32, "raw")
    A, N = int(n_act), int(n_atoms)
    distq_check(A, N)
    if raw.dim() != 2 or raw.shape[1] != A * N:
        raise ValueError(f"distq_values: raw must be [R, {A} * {N}]")
    if support is not None and support.numel() != N:
        raise ValueError(f"distq_values: support must have {N} entries")
    if want_probs and support is None:
        raise ValueError("distq_values: probabilities belong to the categorical mode (give the support)")
    R, dev = raw.shape[0], raw.device
    q = torch.empty(R, A, dtype=torch.float32, device=dev)
    probs = torch.empty(R, A, N, dtype=torch.float32, device=dev) if want_probs else None
    call("tsm_distq_values", ptr(raw), ptr(None if support is None else _chk(support, torch.float32, "support")), R, A, N,
         int(support is not None), ptr(q), ptr(probs), stream_ptr())
    return (q, probs) if want_probs else q


def _distq_head(name: str, entry: str, raw, q_next, raw_next, act, mc, gpow, vmask, aux, aux_name: str, mask_next, weight,
                extra: tuple):
    _dev_only(name, raw, q_next, raw_next, act, mc, gpow, vmask, aux, mask_next, weight)
    raw = _chk(raw, torch.float32, "raw")
    if q_next.dim() != 2 or raw.dim() != 2:
        raise ValueError(f"{name}: raw must be [B, A * N] and q_next [B, A]")
    B, A = q_next.shape
    N = aux.numel()
    distq_check(A, N)
    if B < 1:
        raise ValueError(f"{name}: empty batch")
    args = _head_args(name, B, (("raw", raw, (B, A * N), torch.float32), ("q_next", q_next, (B, A), torch.float32),
                                ("raw_next", raw_next, (B, A * N), torch.float32), ("mask_next", mask_next, (B, A), torch.uint8)),
                      _target_rows(act, mc, gpow, vmask, weight), note=f" ({aux_name} has {N} entries)")
    dev = raw.device
    out = dict(returns=torch.empty(B, N, dtype=torch.float32, device=dev), prio=torch.empty(B, dtype=torch.float32, device=dev),
               d_out=torch.empty(B, A * N, dtype=torch.float32, device=dev),
               partial=_head_partial(B, _abi.DISTQ_ROWS_PER_BLOCK, dev))
    call(entry, *map(ptr, args), ptr(_chk(aux, torch.float32, aux_name).reshape(-1)), B, A, N, *extra, ptr(out["returns"]), ptr(out["prio"]),
         ptr(out["d_out"]), ptr(out["partial"]), stream_ptr())
    return out


def c51_head(raw, q_next, raw_next, act, mc, gpow, vmask, support, v_min: float, v_max: float, mask_next=None, weight=None):
    """C51._target_dist after its forwards + the cross entropy of C51._update_with_batch and its gradient with respect to
    the raw outputs (c51.py:123-158) in one launch.  raw [B, A * N]: the online net on obs; q_next [B, A]: `distq_values` of
    the online net on the successor rows; raw_next [B, A * N]: the lagged net there (the online net's output when there is
    none); act i64 [B]; mc, gpow, vmask from nstep_return; support f32 [N]; mask_next u8 / bool [B, A] or None; weight
    f32 [B] or None.  -> dict(returns [B, N], prio [B], d_out [B, A * N], partial f64): `qmix_finalize(partial, B, out)`
    gives {loss, mean expected value of the taken action}."""
    if not float(v_min) < float(v_max):
        raise ValueError(f"c51_head: v_max should be larger than v_min, but got v_min={v_min} and v_max={v_max}")
    return _distq_head("c51_head", "tsm_c51_head", raw, q_next, raw_next, act, mc, gpow, vmask, support, "support", mask_next,
                       weight, (float(v_min), float(v_max)))


def qrdqn_head(raw, q_next, raw_next, act, mc, gpow, vmask, tau_hat, mask_next=None, weight=None):
    """QRDQN._target_q after its forwards + the quantile Huber loss of QRDQN._update_with_batch and its gradient
    (qrdqn.py:94-129) in one launch.  Arguments as `c51_head`, with q_next the mean over quantiles and tau_hat f32 [N] the
    quantile midpoints.  -> dict(returns [B, N], prio [B], d_out [B, A * N], partial f64)."""
    return _distq_head("qrdqn_head", "tsm_qrdqn_head", raw, q_next, raw_next, act, mc, gpow, vmask, tau_hat, "tau_hat",
                       mask_next, weight, ())


# --------------------------------------------------------------------------------------------
# Implicit Quantile Network (iqn.py; utils/net/discrete.py:127-217; csrc/iqn.hip)
# --------------------------------------------------------------------------------------------
def iqn_check(num_cosines: int, embedding_dim: int, sample_size: int = 2, n_act: int = 1) -> None:
    """The bounds of the IQN kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_iqn_check", int(num_cosines), int(embedding_dim), int(sample_size), int(n_act))


def iqn_taus(R: int, sample_size: int, seed: int, device, offset: int = 0, offset_dev=None, out=None):
    """`torch.rand(R, sample_size)` of ImplicitQuantileNetwork.forward (discrete.py:211) from Philox on the device: row r
    draws at counter offset + *offset_dev + r under a key of its own.  -> taus f32 [R, sample_size] in [0, 1)."""
    R, S = int(R), int(sample_size)
    iqn_check(4, 16, S)
    out = _out("iqn_taus", out, (R, S), torch.float32, device)
    call("tsm_iqn_taus", R, S, *_philox("iqn_taus", seed, offset, offset_dev), ptr(out), stream_ptr())
    return out


def _iqn_embed_shapes(name: str, f, taus, We, be):
    if f.dim() != 2 or taus.dim() != 2 or We.dim() != 2 or f.shape[0] != taus.shape[0]:
        raise ValueError(f"{name}: f must be [R, H], taus [R, S] and We [H, C]")
    (R, H), S, C = f.shape, taus.shape[1], We.shape[1]
    iqn_check(C, H, S)
    if We.shape[0] != H or be.numel() != H:
        raise ValueError(f"{name}: We must be [{H}, C] and be [{H}]")
    if R < 1:
        raise ValueError(f"{name}: empty batch")
    return R, S, C, H


def iqn_embed_forward(f, taus, We, be, relu_f: bool = False):
    """CosineEmbeddingNetwork.forward and its product with the features (discrete.py:145-161, 212-215) in one launch:
    f [R, H], taus [R, S], We [H, C], be [H] -> (e [R * S, H] = g(f[b]) * phi[b, s], phi [R * S, H] = relu(We cos + be));
    g = relu with relu_f (a preprocess net that ends in its activation, as the reference's Net), else the identity."""
    _dev_only("iqn_embed_forward", f, taus, We, be)
    R, S, C, H = _iqn_embed_shapes("iqn_embed_forward", f, taus, We, be)
    e = torch.empty(R * S, H, dtype=torch.float32, device=f.device)
    phi = torch.empty_like(e)
    call("tsm_iqn_embed_forward", ptr(_chk(f, torch.float32, "f")), ptr(_chk(taus, torch.float32, "taus")),
         ptr(_chk(We, torch.float32, "We")), ptr(_chk(be, torch.float32, "be")), R, S, C, H, int(bool(relu_f)), ptr(e), ptr(phi), stream_ptr())
    return e, phi


def iqn_embed_backward(d_e, f, phi, taus, We, be, n_split: int = 0, slabs=None, slab_stride: int = 0, w_off: int = 0,
                       b_off: int | None = None, relu_f: bool = False):
    """The backward of `iqn_embed_forward` in one launch: d_e [R * S, H] -> (d_f [R, H], slabs).  dWe / dbe fill n_split
    slabs at w_off / b_off of rows `slab_stride` apart (default: slabs of their own, [n_split, H * C + H])."""
    _dev_only("iqn_embed_backward", d_e, f, phi, taus, We, be)
    R, S, C, H = _iqn_embed_shapes("iqn_embed_backward", f, taus, We, be)
    if tuple(d_e.shape) != (R * S, H) or tuple(phi.shape) != (R * S, H):
        raise ValueError(f"iqn_embed_backward: d_e and phi must be [{R * S}, {H}]")
    if b_off is None:
        b_off = w_off + H * C
    end = max(w_off + H * C, b_off + H)   # a slab is written up to the end of the later block
    n_split, slabs, slab_stride = _slab_dest("iqn_embed_backward", slabs, n_split, R,
                                             slab_stride if slab_stride > 0 else end if slabs is None else slabs.stride(0), end, f.device)
    d_f = torch.empty(R, H, dtype=torch.float32, device=f.device)
    call("tsm_iqn_embed_backward", ptr(_chk(d_e, torch.float32, "d_e")), ptr(_chk(f, torch.float32, "f")),
         ptr(_chk(phi, torch.float32, "phi")), ptr(_chk(taus, torch.float32, "taus")), R, S, C, H, int(bool(relu_f)), ptr(d_f), int(n_split),
         slabs.data_ptr(), int(slab_stride), int(w_off), int(b_off), stream_ptr())
    return d_f, slabs


def iqn_values(out, sample_size: int, n_act: int):
    """QRDQNPolicy.compute_q_value's mean over the fractions (qrdqn.py:20) on the sample-major output: out [R * S, A] or
    [R, S, A] -> q [R, A], before the action mask."""
    _dev_only("iqn_values", out)
    S, A = int(sample_size), int(n_act)
    iqn_check(4, 16, S, A)
    out = _chk(out, torch.float32, "out")
    if out.numel() % (S * A) != 0 or out.shape[-1] != A:
        raise ValueError(f"iqn_values: out must be [R, {S}, {A}]")
    R = out.numel() // (S * A)
    q = torch.empty(R, A, dtype=torch.float32, device=out.device)
    call("tsm_iqn_values", ptr(out), R, S, A, ptr(q), stream_ptr())
    return q


def iqn_head(out, q_next, out_next, taus, act, mc, gpow, vmask, mask_next=None, weight=None):
    """QRDQN._target_q after its forwards + the quantile Huber loss of IQN._update_with_batch over per-row fractions and its
    gradient (qrdqn.py:94-106, iqn.py:160-181) in one launch.  out [B, N, A]: the online net on obs under taus [B, N];
    q_next [B, A]: `iqn_values` of the online net on the successor rows; out_next [B, N', A]: the lagged net there (that same
    online forward when there is none); act i64 [B]; mc, gpow, vmask from nstep_return; mask_next u8 / bool [B, A] or None;
    weight f32 [B] or None.  -> dict(returns [B, N'], prio [B], d_out [B, N, A], partial f64): `qmix_finalize(partial, B,
    out)` gives {loss, mean value of the taken action}."""
    _dev_only("iqn_head", out, q_next, out_next, taus, act, mc, gpow, vmask, mask_next, weight)
    if q_next.dim() != 2 or taus.dim() != 2 or out.dim() != 3 or out_next.dim() != 3:
        raise ValueError("iqn_head: out must be [B, N, A], out_next [B, N', A], q_next [B, A] and taus [B, N]")
    B, A = q_next.shape
    N, Np = taus.shape[1], out_next.shape[1]
    iqn_check(4, 16, N, A)
    iqn_check(4, 16, Np, A)
    if B < 1:
        raise ValueError("iqn_head: empty batch")
    args = _head_args("iqn_head", B, (("out", out, (B, N, A), torch.float32), ("q_next", q_next, (B, A), torch.float32),
                                      ("out_next", out_next, (B, Np, A), torch.float32),
                                      ("mask_next", mask_next, (B, A), torch.uint8), ("taus", taus, (B, N), torch.float32)),
                      _target_rows(act, mc, gpow, vmask, weight))
    dev = out.device
    res = dict(returns=torch.empty(B, Np, dtype=torch.float32, device=dev), prio=torch.empty(B, dtype=torch.float32, device=dev),
               d_out=torch.empty(B, N, A, dtype=torch.float32, device=dev), partial=_head_partial(B, _abi.IQN_ROWS_PER_BLOCK, dev))
    call("tsm_iqn_head", *map(ptr, args), B, A, N, Np, ptr(res["returns"]), ptr(res["prio"]), ptr(res["d_out"]), ptr(res["partial"]), stream_ptr())
    return res


# --------------------------------------------------------------------------------------------
# Fully parameterized Quantile Function (fqf.py; utils/net/discrete.py:220-315; csrc/fqf.hip)
# --------------------------------------------------------------------------------------------
def fqf_check(num_fractions: int, embedding_dim: int = 16, n_act: int = 1) -> None:
    """The bounds of the FQF kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_fqf_check", int(num_fractions), int(embedding_dim), int(n_act))


def _fqf_propose_shapes(name: str, f, N: int):
    if f.dim() != 2:
        raise ValueError(f"{name}: f must be [R, H]")
    R, H = f.shape
    fqf_check(N, H)
    if R < 1:
        raise ValueError(f"{name}: empty batch")
    return R, H


def fqf_propose(f, Wf, bf, relu_f: bool = False):
    """FractionProposalNetwork.forward (discrete.py:240-253) in one launch: f [R, H], Wf [N, H], bf [N] ->
    (taus [R, N + 1], tau_hats [R, N], logp [R, N], entropies [R]); g = relu with relu_f, else the identity."""
    _dev_only("fqf_propose", f, Wf, bf)
    if Wf.dim() != 2:
        raise ValueError("fqf_propose: Wf must be [N, H]")
    N = Wf.shape[0]
    R, H = _fqf_propose_shapes("fqf_propose", f, N)
    f, Wf, bf = _head_args("fqf_propose", R, (("f", f, (R, H), torch.float32), ("Wf", Wf, (N, H), torch.float32),
                                              ("bf", bf, (N,), torch.float32)), ())
    dev = f.device
    taus = torch.empty(R, N + 1, dtype=torch.float32, device=dev)
    tau_hats, logp = (torch.empty(R, N, dtype=torch.float32, device=dev) for _ in range(2))
    entropies = torch.empty(R, dtype=torch.float32, device=dev)
    call("tsm_fqf_propose", ptr(f), ptr(Wf), ptr(bf), R, N, H, int(bool(relu_f)), ptr(taus), ptr(tau_hats), ptr(logp),
         ptr(entropies), stream_ptr())
    return taus, tau_hats, logp, entropies


def fqf_propose_backward(d_logits, f, n_split: int = 0, slabs=None, slab_stride: int = 0, w_off: int = 0,
                         b_off: int | None = None, relu_f: bool = False):
    """The backward of `fqf_propose` from d_logits [R, N] in one launch -> slabs: dWf / dbf fill n_split slabs at w_off /
    b_off of rows `slab_stride` apart (default: slabs of their own, [n_split, N * H + N])."""
    _dev_only("fqf_propose_backward", d_logits, f)
    if d_logits.dim() != 2:
        raise ValueError("fqf_propose_backward: d_logits must be [R, N]")
    N = d_logits.shape[1]
    R, H = _fqf_propose_shapes("fqf_propose_backward", f, N)
    d_logits, f = _head_args("fqf_propose_backward", R, (("d_logits", d_logits, (R, N), torch.float32),
                                                         ("f", f, (R, H), torch.float32)), ())
    if b_off is None:
        b_off = w_off + N * H
    end = max(w_off + N * H, b_off + N)   # a slab is written up to the end of the later block
    n_split, slabs, slab_stride = _slab_dest("fqf_propose_backward", slabs, n_split, R,
                                             slab_stride if slab_stride > 0 else end if slabs is None else slabs.stride(0), end, f.device)
    call("tsm_fqf_propose_backward", ptr(d_logits), ptr(f), R, N, H, int(bool(relu_f)), int(n_split), slabs.data_ptr(),
         int(slab_stride), int(w_off), int(b_off), stream_ptr())
    return slabs


def fqf_values(out, taus, n_act: int):
    """The fraction-weighted sum of FQFPolicy.forward (fqf.py:94-97) on the sample-major output: out [R * N, A] or [R, N, A],
    taus [R, N + 1] -> q [R, A], before the action mask."""
    _dev_only("fqf_values", out, taus)
    if taus.dim() != 2:
        raise ValueError("fqf_values: taus must be [R, N + 1]")
    R, N, A = taus.shape[0], taus.shape[1] - 1, int(n_act)
    fqf_check(N, 16, A)
    if out.numel() != R * N * A or out.shape[-1] != A:
        raise ValueError(f"fqf_values: out must be [{R}, {N}, {A}]")
    out, taus = _head_args("fqf_values", R, (("out", out.reshape(R, N, A), (R, N, A), torch.float32),
                                             ("taus", taus, (R, N + 1), torch.float32)), ())
    q = torch.empty(R, A, dtype=torch.float32, device=out.device)
    call("tsm_fqf_values", ptr(out), ptr(taus), R, N, A, ptr(q), stream_ptr())
    return q


def fqf_head(out, out_tau, q_next, out_next, taus, tau_hats, logp, entropies, act, mc, gpow, vmask, mask_next=None, weight=None,
             ent_coef: float = 0.0):
    """FQF._target_q after its forwards + both losses of FQF._update_with_batch and their gradients (fqf.py:178-193, 201-247) in
    one launch.  out [B, N, A]: the online net on obs at tau_hats [B, N]; out_tau [B, N - 1, A]: at the interior fractions taus[:, 1:-1] of
    taus [B, N + 1];
    q_next [B, A]: `fqf_values` of the online net on the successor rows; out_next [B, N, A]: the lagged net there (that same
    online forward when there is none); logp [B, N], entropies [B] from `fqf_propose`; the rest as `iqn_head`.
    -> dict(returns [B, N], prio [B], d_out [B, N, A], d_logits [B, N], partial, partial_frac f64): `qmix_finalize` gives
    {quantile loss, mean value of the taken action} and {fraction loss, entropy loss}."""
    _dev_only("fqf_head", out, out_tau, q_next, out_next, taus, tau_hats, logp, entropies, act, mc, gpow, vmask, mask_next, weight)
    if q_next.dim() != 2 or tau_hats.dim() != 2:
        raise ValueError("fqf_head: q_next must be [B, A] and tau_hats [B, N]")
    (B, A), N = q_next.shape, tau_hats.shape[1]
    fqf_check(N, 16, A)
    if B < 1:
        raise ValueError("fqf_head: empty batch")
    args = _head_args("fqf_head", B, (("out", out, (B, N, A), torch.float32), ("out_tau", out_tau, (B, N - 1, A), torch.float32),
                                      ("q_next", q_next, (B, A), torch.float32), ("out_next", out_next, (B, N, A), torch.float32),
                                      ("mask_next", mask_next, (B, A), torch.uint8), ("taus", taus, (B, N + 1), torch.float32),
                                      ("tau_hats", tau_hats, (B, N), torch.float32),
                                      ("logp", logp, (B, N), torch.float32)),
                      (("entropies", entropies, torch.float32),) + _target_rows(act, mc, gpow, vmask, weight))
    dev = q_next.device
    res = dict(returns=torch.empty(B, N, dtype=torch.float32, device=dev), prio=torch.empty(B, dtype=torch.float32, device=dev),
               d_out=torch.empty(B, N, A, dtype=torch.float32, device=dev), d_logits=torch.empty(B, N, dtype=torch.float32, device=dev),
               partial=_head_partial(B, _abi.IQN_ROWS_PER_BLOCK, dev), partial_frac=_head_partial(B, _abi.IQN_ROWS_PER_BLOCK, dev))
    call("tsm_fqf_head", *map(ptr, args), float(ent_coef), B, A, N, ptr(res["returns"]), ptr(res["prio"]), ptr(res["d_out"]),
         ptr(res["d_logits"]), ptr(res["partial"]), ptr(res["partial_frac"]), stream_ptr())
    return res


# --------------------------------------------------------------------------------------------
# Rainbow: NoisyLinear layers and dueling streams (rainbow.py; utils/net/discrete.py:318-375; common.py:319-364;
# csrc/rainbow.hip)
# --------------------------------------------------------------------------------------------
def noisy_net_table(layers) -> _abi.tsm_noisy_net:
    """The layer table of include/tsmarl.h for `layers` = [(in, out, noisy)] in the net's `parameters()` order: every layer's
    offsets in the flat vector, in the effective vector and among the noise slots, and the three totals."""
    layers = [(int(i), int(o), int(bool(z))) for i, o, z in layers]
    if not 1 <= len(layers) <= _abi.NOISY_MAX_LAYERS:
        raise ValueError(f"noisy_net_table: {len(layers)} layers outside [1, {_abi.NOISY_MAX_LAYERS}]")
    t = _abi.tsm_noisy_net()
    t.n_layers = len(layers)
    off = eff = slot = 0
    for l, (i, o, z) in enumerate(layers):
        L = t.layer[l]
        L.off, L.eff_off, L.slot_off, L.n_in, L.n_out, L.noisy = off, eff, slot, i, o, z
        off += 2 * i * o + 3 * o + i if z else i * o + o
        eff += i * o + o
        slot += i + o if z else 0
    t.P, t.P_eff, t.n_slots = off, eff, slot
    return t


def rainbow_check(table: _abi.tsm_noisy_net) -> None:
    """The bounds of a layer table (include/tsmarl.h: tsm_rainbow_check): ValueError naming the limit.  Needs no device."""
    call("tsm_rainbow_check", C.byref(table))


def _noisy_flat(name: str, table, flat):
    rainbow_check(table)
    _dev_only(name, flat)
    flat = _chk(flat, torch.float32, "flat")
    if flat.dim() != 1 or flat.numel() != table.P:
        raise ValueError(f"{name}: flat must be a vector of {table.P} elements")
    return flat


def noisy_sample(table, flat, seed: int, offset: int = 0, offset_dev=None):
    """NoisyLinear.sample (discrete.py:358-365) for every noisy layer of the net, in place in `flat`: slot s gets
    sign(x) sqrt(|x|), x ~ N(0, 1) from Philox at counter offset + *offset_dev under a key of its own."""
    rainbow_check(table)
    _out("noisy_sample", flat, (table.P,), torch.float32, None, "flat")   # (written in place)
    call("tsm_noisy_sample", C.byref(table), ptr(flat), *_philox("noisy_sample", seed, offset, offset_dev), stream_ptr())
    return flat


def noisy_compose(table, flat, training: bool, out=None):
    """The effective parameters of every layer (discrete.py:368-373) -> eff f32 [P_eff] in `FlatMLP` layout."""
    flat = _noisy_flat("noisy_compose", table, flat)
    out = _out("noisy_compose", out, (table.P_eff,), torch.float32, flat.device)
    call("tsm_noisy_compose", C.byref(table), ptr(flat), int(bool(training)), ptr(out), stream_ptr())
    return out


def noisy_grad(table, flat, eff_slabs, training: bool, slabs=None):
    """Gradient slabs over the effective layout [n_split, P_eff] -> slabs over the flat layout [n_split, P], slab by slab:
    d mu = d, d sigma = d * noise (zeros when not training), the noise slots +0.0."""
    flat = _noisy_flat("noisy_grad", table, flat)
    _dev_only("noisy_grad", eff_slabs)
    eff_slabs = _chk(eff_slabs, torch.float32, "eff_slabs")
    if eff_slabs.dim() != 2 or eff_slabs.shape[1] != table.P_eff or eff_slabs.shape[0] < 1:
        raise ValueError(f"noisy_grad: eff_slabs must be [n_split, {table.P_eff}]")
    n_split = eff_slabs.shape[0]
    slabs = _out("noisy_grad", slabs, (n_split, table.P), torch.float32, flat.device, "slabs")
    call("tsm_noisy_grad", C.byref(table), ptr(flat), ptr(eff_slabs), n_split, int(bool(training)), ptr(slabs), stream_ptr())
    return slabs


def _dueling_shapes(name: str, x, n_act: int, n_atoms: int):
    A, N = int(n_act), int(n_atoms)
    distq_check(A, N)
    if x.dim() != 2 or x.shape[1] != A * N:
        raise ValueError(f"{name}: the action stream must be [R, {A} * {N}]")
    return x.shape[0], A, N


def dueling_combine(q, v, n_act: int, n_atoms: int):
    """`q - q.mean(dim=1, keepdim=True) + v` (common.py:360-364): q [R, A * N], v [R, N] -> out [R, A * N], the raw output the
    distributional heads take."""
    R, A, N = _dueling_shapes("dueling_combine", q, n_act, n_atoms)
    if tuple(v.shape) != (R, N):
        raise ValueError(f"dueling_combine: v must be [{R}, {N}]")
    _dev_only("dueling_combine", q, v)
    out = torch.empty(R, A * N, dtype=torch.float32, device=q.device)
    call("tsm_dueling_combine", ptr(_chk(q, torch.float32, "q")), ptr(_chk(v, torch.float32, "v")), R, A, N, ptr(out), stream_ptr())
    return out


def dueling_combine_backward(d_out, n_act: int, n_atoms: int):
    """The backward of `dueling_combine`: d_out [R, A * N] -> (d_q [R, A * N], d_v [R, N])."""
    R, A, N = _dueling_shapes("dueling_combine_backward", d_out, n_act, n_atoms)
    _dev_only("dueling_combine_backward", d_out)
    d_q = torch.empty(R, A * N, dtype=torch.float32, device=d_out.device)
    d_v = torch.empty(R, N, dtype=torch.float32, device=d_out.device)
    call("tsm_dueling_combine_backward", ptr(_chk(d_out, torch.float32, "d_out")), R, A, N, ptr(d_q), ptr(d_v), stream_ptr())
    return d_q, d_v


def dueling_features(z):
    """The last activation of the dueling net's trunk: z [R, H] -> relu(z)."""
    _dev_only("dueling_features", z)
    z = _chk(z, torch.float32, "z")
    f = torch.empty_like(z)
    call("tsm_dueling_features", ptr(z), z.numel(), ptr(f), stream_ptr())
    return f


def dueling_features_backward(z, d_fq, d_fv):
    """The two streams' input gradients joined behind the trunk's last activation: d_z = z > 0 ? d_fq + d_fv : 0."""
    _dev_only("dueling_features_backward", z, d_fq, d_fv)
    if tuple(d_fq.shape) != tuple(z.shape) or tuple(d_fv.shape) != tuple(z.shape):
        raise ValueError(f"dueling_features_backward: both gradients must be {list(z.shape)}")
    z = _chk(z, torch.float32, "z")
    d_z = torch.empty_like(z)
    call("tsm_dueling_features_backward", ptr(z), ptr(_chk(d_fq, torch.float32, "d_fq")), ptr(_chk(d_fv, torch.float32, "d_fv")),
         z.numel(), ptr(d_z), stream_ptr())
    return d_z


# --------------------------------------------------------------------------------------------
# Discrete SAC (discrete_sac.py; sac.py Alpha / AutoAlpha; csrc/dsac.hip)
# --------------------------------------------------------------------------------------------
def dsac_check(n_act: int, n_step: int = 1) -> None:
    """The bounds of the Discrete SAC kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_dsac_check", int(n_act), int(n_step))


def _dsac_rows(name: str, first, others: dict, per_row: tuple = ()):
    """[B, A] of `first`; every f32 tensor of `others` must have that shape, every (nm, x, dtype) of `per_row` B entries.
    -> (B, A, the contiguous tensors of first, others and per_row in that order, as `_head_args`)."""
    first = _chk(first, torch.float32, "logits / q")
    if first.dim() != 2:
        raise ValueError(f"{name}: logits and Q values must be [B, A]")
    B, A = first.shape
    dsac_check(A)
    if B < 1:
        raise ValueError(f"{name}: empty batch")
    return B, A, [first] + _head_args(name, B, tuple((nm, x, (B, A), torch.float32) for nm, x in others.items()), per_row)


def dsac_target(logits_next, q1_next_old, q2_next_old, alpha_dev, mc, gpow, vmask):
    """DiscreteSAC._target_q_compute_value after its forwards + the n-step target (discrete_sac.py:147-155,
    algorithm_base.py:1213-1215) in one launch.  logits_next [B, A]: the online actor on obs_next[idx_n]; q1_next_old,
    q2_next_old [B, A]: the lagged critics there; alpha_dev f32 [1]; mc, gpow, vmask from nstep_return.  -> returns f32 [B]."""
    _dev_only("dsac_target", logits_next, q1_next_old, q2_next_old, alpha_dev, mc, gpow, vmask)
    B, A, args = _dsac_rows("dsac_target", logits_next, dict(q1_next_old=q1_next_old, q2_next_old=q2_next_old),
                            (("mc", mc, torch.float32), ("gpow", gpow, torch.float32), ("vmask", vmask, torch.uint8)))
    returns = torch.empty(B, dtype=torch.float32, device=logits_next.device)
    call("tsm_dsac_target", *map(ptr, args[:3]), ptr(_chk(alpha_dev, torch.float32, "alpha_dev")), *map(ptr, args[3:]), B, A,
         ptr(returns), stream_ptr())
    return returns


def dsac_critic_head(q1, q2, act, returns, weight=None):
    """Both critic losses of DiscreteSAC._update_with_batch and their gradients (discrete_sac.py:162-174) in one launch.
    q1, q2 [B, A]: the critics on obs; act i64 [B]; returns f32 [B]; weight f32 [B] or None.
    -> dict(dq1, dq2 [B, A], prio [B] = (td1 + td2) / 2 with td = q[act] - returns, partial f64):
    `qmix_finalize(partial, B, out)` gives {critic1_loss, critic2_loss}."""
    _dev_only("dsac_critic_head", q1, q2, act, returns, weight)
    B, A, args = _dsac_rows("dsac_critic_head", q1, dict(q2=q2), (("act", act, torch.int64), ("returns", returns, torch.float32),
                                                                  ("weight", weight, torch.float32)))
    dev = q1.device
    out = dict(dq1=torch.empty(B, A, dtype=torch.float32, device=dev), dq2=torch.empty(B, A, dtype=torch.float32, device=dev),
               prio=torch.empty(B, dtype=torch.float32, device=dev), partial=_head_partial(B, _abi.DSAC_ROWS_PER_BLOCK, dev))
    call("tsm_dsac_critic_head", *map(ptr, args), B, A, ptr(out["dq1"]), ptr(out["dq2"]), ptr(out["prio"]), ptr(out["partial"]),
         stream_ptr())
    return out


def dsac_actor_head(logits, q1, q2, alpha_dev):
    """The actor loss of DiscreteSAC._update_with_batch with its backward down to the logits, and the entropy AutoAlpha
    reads (discrete_sac.py:177-184) in one launch.  logits [B, A]: the actor on obs; q1, q2 [B, A]: the critics on obs after
    their steps; alpha_dev f32 [1].  -> dict(entropy [B], d_logits [B, A], partial f64): `qmix_finalize(partial, B, out)`
    gives {actor_loss, mean entropy}."""
    _dev_only("dsac_actor_head", logits, q1, q2, alpha_dev)
    B, A, args = _dsac_rows("dsac_actor_head", logits, dict(q1=q1, q2=q2))
    dev = logits.device
    out = dict(entropy=torch.empty(B, dtype=torch.float32, device=dev), d_logits=torch.empty(B, A, dtype=torch.float32, device=dev),
               partial=_head_partial(B, _abi.DSAC_ROWS_PER_BLOCK, dev))
    call("tsm_dsac_actor_head", *map(ptr, args), ptr(_chk(alpha_dev, torch.float32, "alpha_dev")), B, A, ptr(out["entropy"]),
         ptr(out["d_logits"]), ptr(out["partial"]), stream_ptr())
    return out


def dsac_alpha_step(entropy_partial, B: int, log_alpha, exp_avg, exp_avg_sq, step, target_entropy: float, alpha_dev, out,
                    lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
    """AutoAlpha.update (sac.py:203-209) on device scalars, one launch: entropy_partial f64: `dsac_actor_head`'s partials over
    B rows (the mean entropy is formed from them in float64); log_alpha, exp_avg, exp_avg_sq f32 [1] and step i64 [1] in
    HBM, updated in place; alpha_dev f32 [1] <- exp(log_alpha); out f32 [2] (device or pinned host memory) <- {alpha_loss,
    the new alpha}."""
    _dev_only("dsac_alpha_step", entropy_partial)
    out_p = _out_or_pinned("dsac_alpha_step", out, 2)
    entropy_partial = _chk(entropy_partial, torch.float64, "entropy_partial")
    if entropy_partial.numel() < 2 or entropy_partial.numel() % 2:
        raise ValueError("dsac_alpha_step: entropy_partial must hold pairs of {loss, entropy} sums")
    state = [_out("dsac_alpha_step", t, (1,), dt, None, nm, "min")   # (all four updated in place, alpha_dev written)
             for nm, t, dt in (("log_alpha", log_alpha, torch.float32), ("exp_avg", exp_avg, torch.float32),
                               ("exp_avg_sq", exp_avg_sq, torch.float32), ("step", step, torch.int64), ("alpha_dev", alpha_dev, torch.float32))]
    call("tsm_dsac_alpha_step", ptr(entropy_partial), entropy_partial.numel() // 2, int(B), *map(ptr, state[:4]), float(target_entropy),
         float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), ptr(state[4]), out_p, stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# ICM (modelbased/icm.py; IntrinsicCuriosityModule, utils/net/discrete.py:378-429; csrc/icm.hip)
# --------------------------------------------------------------------------------------------
def icm_check(feature_dim: int, n_act: int) -> None:
    """The bounds of the ICM kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_icm_check", int(feature_dim), int(n_act))


def _icm_phi(name: str, phi, act):
    """phi f32 [2R, F] (obs of row r at 2r, obs_next at 2r + 1), act i64 [R] -> (R, F, phi, act), contiguous."""
    phi = _chk(phi, torch.float32, "phi")
    if phi.dim() != 2 or phi.shape[0] < 2 or phi.shape[0] % 2:
        raise ValueError(f"{name}: phi must be [2 R, feature_dim], the rows of obs and obs_next interleaved")
    R, F = phi.shape[0] // 2, phi.shape[1]
    if act.numel() != R:
        raise ValueError(f"{name}: act must have {R} entries")
    return R, F, phi, _chk(act, torch.int64, "act").reshape(-1)


def icm_rows(phi, act, n_act: int, out=None):
    """The forward model's input (discrete.py:424-426) in one launch: phi [2R, F], act i64 [R]
    -> x_fwd f32 [R, F + n_act] = [phi[2r] | one_hot(act[r])]; an action outside [0, n_act) gives an all-zero one-hot."""
    _dev_only("icm_rows", phi, act)
    R, F, phi, act = _icm_phi("icm_rows", phi, act)
    icm_check(F, n_act)
    out = _out("icm_rows", out, (R, F + int(n_act)), torch.float32, phi.device)
    call("tsm_icm_rows", ptr(phi), ptr(act), R, F, int(n_act), ptr(out), stream_ptr())
    return out


def icm_head(phi2_hat, phi, act_hat, act, reward_scale: float, forward_loss_weight: float, lr_scale: float, rew_io=None, ids=None):
    """The ICM's row-wise head in one launch (include/tsmarl.h: tsm_icm_head).  phi2_hat [R, F]: the forward model's output; phi
    [2R, F]: the feature net's (phi2 = its odd rows, read in place); act_hat [R, A]: the inverse model's output; act i64 [R].
    rew_io f32 (any shape, contiguous) with ids i64 [R] or None: `rew_io.view(-1)[ids[r] or r] += mse[r] * reward_scale` in
    float32, in place; the ids must be distinct and inside rew_io.
    -> dict(mse [R], d_phi2_hat, d_phi2_fwd [R, F], d_act_hat [R, A], partial f64): `qmix_finalize(partial, R, out)` gives
    {icm_forward_loss, icm_inverse_loss}."""
    _dev_only("icm_head", phi2_hat, phi, act_hat, act, ids)
    R, F, phi, act = _icm_phi("icm_head", phi, act)
    act_hat = _chk(act_hat, torch.float32, "act_hat")
    if act_hat.dim() != 2 or act_hat.shape[0] != R:
        raise ValueError(f"icm_head: act_hat must be [{R}, n_act]")
    A = act_hat.shape[1]
    icm_check(F, A)
    phi2_hat = _chk(phi2_hat, torch.float32, "phi2_hat")
    if tuple(phi2_hat.shape) != (R, F):
        raise ValueError(f"icm_head: phi2_hat must be [{R}, {F}]")
    if ids is not None:
        if rew_io is None or ids.numel() != R:
            raise ValueError(f"icm_head: ids needs rew_io and must have {R} entries")
        ids = _chk(ids, torch.int64, "ids").reshape(-1)
    if rew_io is not None:   # (written in place)
        _out("icm_head", rew_io, (R if ids is None else 0,), torch.float32, None, "rew_io", "min")
    dev = phi.device
    out = dict(mse=torch.empty(R, dtype=torch.float32, device=dev), d_phi2_hat=torch.empty(R, F, dtype=torch.float32, device=dev),
               d_phi2_fwd=torch.empty(R, F, dtype=torch.float32, device=dev), d_act_hat=torch.empty(R, A, dtype=torch.float32, device=dev),
               partial=_head_partial(R, _abi.ICM_ROWS_PER_BLOCK, dev))
    call("tsm_icm_head", ptr(phi2_hat), phi.data_ptr() + 4 * F, 2 * F, ptr(act_hat), ptr(act), ptr(rew_io), ptr(ids), R, F, A,
         float(reward_scale), float(forward_loss_weight), float(lr_scale), ptr(out["mse"]), ptr(out["d_phi2_hat"]),
         ptr(out["d_phi2_fwd"]), ptr(out["d_act_hat"]), ptr(out["partial"]), stream_ptr())
    return out


def icm_join_grad(g_fwd, g_inv, d_phi2_fwd, out=None):
    """The feature net's d_out [2R, F] in one launch: row 2r = g_fwd[r] + g_inv[r, :F], row 2r + 1 = g_inv[r, F:] + d_phi2_fwd[r]
    (float32 sums in that order).  g_fwd [R, F]: the forward model's input gradient over its first F columns; g_inv [R, 2F]: the
    inverse model's; out None: g_inv's own memory (the two share their layout)."""
    _dev_only("icm_join_grad", g_fwd, g_inv, d_phi2_fwd)
    g_fwd, g_inv, d_phi2_fwd = (_chk(x, torch.float32, n) for x, n in ((g_fwd, "g_fwd"), (g_inv, "g_inv"), (d_phi2_fwd, "d_phi2_fwd")))
    if g_fwd.dim() != 2 or g_fwd.shape[0] < 1:
        raise ValueError("icm_join_grad: g_fwd must be [R, feature_dim]")
    R, F = g_fwd.shape
    icm_check(F, 1)
    if tuple(g_inv.shape) != (R, 2 * F) or tuple(d_phi2_fwd.shape) != (R, F):
        raise ValueError(f"icm_join_grad: g_inv must be [{R}, {2 * F}] and d_phi2_fwd [{R}, {F}]")
    out = g_inv if out is None else _out("icm_join_grad", out, (2 * R, F), torch.float32, None, size="numel")
    call("tsm_icm_join_grad", ptr(g_fwd), ptr(g_inv), ptr(d_phi2_fwd), R, F, ptr(out), stream_ptr())
    return out.view(2 * R, F)


# --------------------------------------------------------------------------------------------
# GAIL (imitation/gail.py; csrc/gail.hip)
# --------------------------------------------------------------------------------------------
def gail_check(obs_dim: int, n_act: int) -> None:
    """The bounds of the GAIL kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_gail_check", int(obs_dim), int(n_act))


def _gail_ids(name: str, ids, R: int | None = None):
    if ids is None:
        return None
    if R is not None and ids.numel() != R:
        raise ValueError(f"{name}: ids must have {R} entries")
    return _chk(ids, torch.int64, "ids").reshape(-1)


def gail_draw(valid, n_valid: int, n_agent: int, R: int, seed: int, counter: int = 0, counter_dev=None, out=None, device="cuda"):
    """`expert_buffer.sample(R)` (gail.py:227) as pair ids, uniform with replacement, in one launch: draw i is Philox word 0 at
    counter + *counter_dev + i under the key seed ^ kGailKey, j = (w0 n_valid n_agent) >> 32,
    -> i64 [R]: (valid[j // n_agent] or j // n_agent) * n_agent + j % n_agent.  valid: i64 [n_valid] store rows, or None."""
    _dev_only("gail_draw", valid)
    if valid is not None:
        valid = _chk(valid, torch.int64, "valid").reshape(-1)
        if valid.numel() != int(n_valid):
            raise ValueError(f"gail_draw: valid must have {int(n_valid)} entries")
        device = valid.device
    out = _out("gail_draw", out, (max(int(R), 0),), torch.int64, device, size="numel")
    call("tsm_gail_draw", ptr(valid), int(n_valid), int(n_agent), int(R), *_philox("gail_draw", seed, counter, counter_dev), ptr(out),
         stream_ptr())
    return out


def gail_rows(obs, act, n_act: int, ids=None, R: int | None = None, out=None):
    """The discriminator's input (gail.py:208-212, one-hot actions) in one launch.  obs f32 [.., D] and act i32 [..]: the
    buffer's stores, read in place as [P, D] and [P]; ids i64 [R] or None (the first R pairs, R = P by default)
    -> out f32 [R, D + n_act] = [obs[p] | one_hot(act[p])]; `out` may be R rows of a taller matrix.  The ids must lie in [0, P)."""
    _dev_only("gail_rows", obs, act, ids)
    obs, act = _chk(obs, torch.float32, "obs"), _chk(act, torch.int32, "act")
    D = obs.shape[-1] if obs.dim() >= 1 else 0
    P = act.numel()
    if obs.dim() < 2 or obs.numel() != P * D:
        raise ValueError("gail_rows: obs must be [.., obs_dim] and act hold one action per row of it")
    gail_check(D, n_act)
    ids = _gail_ids("gail_rows", ids, R)
    R = int(R if R is not None else (ids.numel() if ids is not None else P))
    if ids is None and R > P:
        raise ValueError(f"gail_rows: R = {R} rows asked of {P} pairs")
    out = _out("gail_rows", out, (R, D + int(n_act)), torch.float32, obs.device)
    call("tsm_gail_rows", ptr(obs), ptr(act), ptr(ids), R, D, int(n_act), ptr(out), stream_ptr())
    return out


def gail_reward(logits, rew_io, ids=None):
    """`batch.rew = -F.logsigmoid(-disc(batch))` (gail.py:204-205) in place: rew_io.view(-1)[ids[r] or r] = softplus(logits[r]),
    an overwrite.  The ids must be distinct and inside rew_io."""
    _dev_only("gail_reward", logits, ids)
    logits = _chk(logits, torch.float32, "logits").reshape(-1)
    R = logits.numel()
    ids = _gail_ids("gail_reward", ids, R)
    _out("gail_reward", rew_io, (R if ids is None else 0,), torch.float32, None, "rew_io", "min")   # (written in place)
    call("tsm_gail_reward", ptr(logits), ptr(ids), R, ptr(rew_io), stream_ptr())
    return rew_io


def gail_head(logits, Rp: int, d_logits=None, partial=None):
    """The discriminator loss's row-wise head in one launch (include/tsmarl.h: tsm_gail_head).  logits f32 [Rp + Re]: the policy
    rows, then the expert rows -> dict(d_logits f32 [Rp + Re], partial f64 [4 * blocks]) for `gail_finalize`."""
    _dev_only("gail_head", logits)
    logits = _chk(logits, torch.float32, "logits").reshape(-1)
    n = logits.numel()
    Rp, Re = int(Rp), n - int(Rp)
    nb = max(-(-n // _abi.GAIL_ROWS_PER_BLOCK), 1)
    d_logits = _out("gail_head", d_logits, (n,), torch.float32, logits.device, "d_logits", "numel")
    partial = _out("gail_head", partial, (4 * nb,), torch.float64, logits.device, "partial", "numel")
    call("tsm_gail_head", ptr(logits), Rp, Re, ptr(d_logits), ptr(partial), stream_ptr())
    return dict(d_logits=d_logits, partial=partial)


def gail_finalize(partial, Rp: int, Re: int, out=None):
    """{loss_disc, acc_pi, acc_exp} of one discriminator step from `gail_head`'s partials (one launch).  out: device f32 [3] or
    pinned host f32 [3] (None: a new device tensor)."""
    _dev_only("gail_finalize", partial)
    partial = _chk(partial, torch.float64, "partial").reshape(-1)
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=partial.device)
    if out.numel() != 3:
        raise ValueError("gail_finalize: out must be 3 contiguous f32")
    call("tsm_gail_finalize", ptr(partial), partial.numel() // 4, int(Rp), int(Re), _out_or_pinned("gail_finalize", out, 3), stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# Continuous-action actor-critics: DDPG, TD3, SAC (ddpg.py, td3.py, sac.py, utils/net/continuous.py; csrc/cac.hip)
# --------------------------------------------------------------------------------------------
def cac_check(act_dim: int, n_step: int = 1) -> None:
    """The bounds of the continuous actor-critic kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_cac_check", int(act_dim), int(n_step))


def cac_normal(n: int, seed: int, offset: int = 0, offset_dev=None, device="cuda", out=None):
    """n standard normals f32 from Philox (seed, offset + *offset_dev) under this draw's own key."""
    out = _out("cac_normal", out, (int(n),), torch.float32, device, size="numel")
    call("tsm_cac_normal", ptr(out), int(n), *_philox("cac_normal", seed, offset, offset_dev), stream_ptr())
    return out


def _cac_raw(name: str, raw, width: int | None = None):
    """raw [B, Ad * k] f32 contiguous in HBM -> (raw, B, width of a row)."""
    _dev_only(name, raw)
    if raw.dim() != 2 or raw.shape[0] < 1 or not raw.is_contiguous() or raw.dtype != torch.float32:
        raise ValueError(f"{name}: the actor's raw output must be a contiguous f32 [B, n] with B >= 1")
    if width is not None and raw.shape[1] != width:
        raise ValueError(f"{name}: expected rows of {width} floats, got {raw.shape[1]}")
    return raw, raw.shape[0], raw.shape[1]


def _cac_rows_out(name: str, out, B: int, Ad: int, col0: int):
    """The critic-input rows an action is written into: out [B, W] (None: a new [B, Ad], col0 = 0) -> (out, W)."""
    if out is None:
        if col0 != 0:
            raise ValueError(f"{name}: col0 needs out")
        return None, Ad
    _dev_only(name, out)
    if out.dim() != 2 or out.shape[0] != B or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous f32 [{B}, W]")
    if not 0 <= col0 <= out.shape[1] - Ad:
        raise ValueError(f"{name}: columns [{col0}, {col0 + Ad}) leave the row of {out.shape[1]} floats")
    return out, out.shape[1]


def _cac_z(name: str, z, B: int, Ad: int):
    if z is None:
        return None
    _dev_only(name, z)
    if tuple(z.shape) != (B, Ad):
        raise ValueError(f"{name}: z must be [{B}, {Ad}]")
    return _chk(z, torch.float32, "z")


def cac_det_action(raw, max_action: float = 1.0, z=None, policy_noise: float = 0.0, noise_clip: float = 0.0, out=None,
                   col0: int = 0, want_backward: bool = False):
    """`max_action * tanh(raw)` (continuous.py:86-88), with z also TD3's smoothing noise clamp(policy_noise * z, +-noise_clip)
    (td3.py:196-199; noise_clip <= 0: no clamp), written into columns [col0, col0 + Ad) of out [B, W] (None: a new [B, Ad]).
    -> out, or (out, 1 - tanh^2 [B, Ad]) with want_backward."""
    raw, B, Ad = _cac_raw("cac_det_action", raw)
    cac_check(Ad)
    out, W = _cac_rows_out("cac_det_action", out, B, Ad, col0)
    if out is None:
        out = torch.empty(B, Ad, dtype=torch.float32, device=raw.device)
    z = _cac_z("cac_det_action", z, B, Ad)
    omt2 = torch.empty(B, Ad, dtype=torch.float32, device=raw.device) if want_backward else None
    call("tsm_cac_det_action", ptr(raw), ptr(z), B, Ad, float(max_action), float(policy_noise), float(noise_clip), ptr(out), W,
         int(col0), ptr(omt2), stream_ptr())
    return (out, omt2) if want_backward else out


def _sac_raw(name: str, raw, sigma_param):
    """The probabilistic actor's output: raw [B, 2 Ad] = [mu_raw | sigma_raw] (conditioned sigma), or raw [B, Ad] beside
    sigma_param f32 [Ad].  -> (raw, B, Ad, ld, the sigma tensor, its pointer, ld_sigma)."""
    if sigma_param is None:
        raw, B, n = _cac_raw(name, raw)
        if n % 2:
            raise ValueError(f"{name}: a conditioned-sigma actor emits [mu_raw | sigma_raw], an even number of columns")
        return raw, B, n // 2, n, raw, raw.data_ptr() + 4 * (n // 2), n
    raw, B, n = _cac_raw(name, raw)
    _dev_only(name, sigma_param)
    sg = _chk(sigma_param, torch.float32, "sigma_param").reshape(-1)
    if sg.numel() != n:
        raise ValueError(f"{name}: sigma_param must have {n} entries")
    return raw, B, n, n, sg, sg.data_ptr(), 0


def sac_action(raw, z=None, max_action: float = 1.0, unbounded: bool = False, sigma_param=None, out=None, col0: int = 0):
    """ContinuousActorProbabilistic.forward's epilogue and SACPolicy.forward (continuous.py:238-247, sac.py:114-123): raw as
    `_sac_raw` takes it, z [B, Ad] standard normals (None: the mode).  -> (act = tanh(mu + sigma z) in columns
    [col0, col0 + Ad) of out [B, W] (None: a new [B, Ad]), logp f32 [B])."""
    raw, B, Ad, ld, sg, sg_ptr, ld_s = _sac_raw("sac_action", raw, sigma_param)
    cac_check(Ad)
    out, W = _cac_rows_out("sac_action", out, B, Ad, col0)
    if out is None:
        out = torch.empty(B, Ad, dtype=torch.float32, device=raw.device)
    z = _cac_z("sac_action", z, B, Ad)
    logp = torch.empty(B, dtype=torch.float32, device=raw.device)
    call("tsm_sac_action", ptr(raw), ld, sg_ptr, ld_s, ptr(z), B, Ad, float(max_action), int(bool(unbounded)), ptr(out), W,
         int(col0), ptr(logp), stream_ptr())
    return out, logp


def cac_col_sum(d, slabs):
    """The gradient of a state-independent sigma row: d f32 [B, Ad] (`sac_actor_head`'s d_sigma) -> slabs [n_split, Ad], a
    (strided) view of the sigma columns of the actor's gradient slabs: slab 0 <- the column sums, the others zero."""
    _dev_only("cac_col_sum", d, slabs)
    if d.dim() != 2 or d.shape[0] < 1:
        raise ValueError("cac_col_sum: d must be [B, Ad] with B >= 1")
    B, Ad = d.shape
    cac_check(Ad)
    d = _cac_grad("cac_col_sum", d, B, Ad, "d")
    if slabs.dim() != 2 or slabs.shape[1] != Ad or slabs.dtype != torch.float32 or slabs.stride(1) != 1 or slabs.shape[0] < 1:
        raise ValueError(f"cac_col_sum: slabs must be f32 [n_split, {Ad}] with unit column stride")
    call("tsm_cac_col_sum", ptr(d), Ad, B, Ad, slabs.shape[0], slabs.data_ptr(), slabs.stride(0) if slabs.shape[0] > 1 else Ad,
         stream_ptr())
    return slabs


def cac_target(q1_next, q2_next, mc, gpow, vmask, logp_next=None, alpha_dev=None, out=None):
    """min of the lagged critics (q2_next None: the single critic), minus alpha * logp_next for SAC, then the n-step line
    (td3.py:94-102, sac.py:298-302, algorithm_base.py:1213-1215).  -> returns f32 [B]."""
    _dev_only("cac_target", q1_next, q2_next, mc, gpow, vmask, logp_next, alpha_dev)
    B = q1_next.numel()
    if B < 1:
        raise ValueError("cac_target: empty batch")
    if (logp_next is None) != (alpha_dev is None):
        raise ValueError("cac_target: logp_next and alpha_dev come together")
    args = _head_args("cac_target", B, (), (("q1_next", q1_next, torch.float32), ("q2_next", q2_next, torch.float32),
                                            ("logp_next", logp_next, torch.float32), ("mc", mc, torch.float32),
                                            ("gpow", gpow, torch.float32), ("vmask", vmask, torch.uint8)))
    out = _out("cac_target", out, (B,), torch.float32, q1_next.device, size="numel")
    call("tsm_cac_target", *map(ptr, args[:3]), ptr(None if alpha_dev is None else _chk(alpha_dev, torch.float32, "alpha_dev")),
         *map(ptr, args[3:]), B, ptr(out), stream_ptr())
    return out


def cac_critic_head(q1, q2, returns, weight=None):
    """_minimize_critic_squared_loss between the forward and the step (ddpg.py:267-285) for one critic (q2 None) or two.
    -> dict(dq1, dq2 [B] (dq2 None with one critic), prio [B] = td1 or (td1 + td2) / 2 with td = q - returns, partial f64):
    `qmix_finalize(partial, B, out)` gives {critic1_loss, critic2_loss}."""
    _dev_only("cac_critic_head", q1, q2, returns, weight)
    B = q1.numel()
    if B < 1:
        raise ValueError("cac_critic_head: empty batch")
    args = _head_args("cac_critic_head", B, (), (("q1", q1, torch.float32), ("q2", q2, torch.float32),
                                                 ("returns", returns, torch.float32), ("weight", weight, torch.float32)))
    dev = q1.device
    out = dict(dq1=torch.empty(B, dtype=torch.float32, device=dev),
               dq2=None if q2 is None else torch.empty(B, dtype=torch.float32, device=dev),
               prio=torch.empty(B, dtype=torch.float32, device=dev), partial=_head_partial(B, _abi.CAC_ROWS_PER_BLOCK, dev))
    call("tsm_cac_critic_head", *map(ptr, args), B, ptr(out["dq1"]), ptr(out["dq2"]), ptr(out["prio"]), ptr(out["partial"]),
         stream_ptr())
    return out


def _cac_grad(name: str, g, B: int, Ad: int, what: str):
    _dev_only(name, g)
    if tuple(g.shape) != (B, Ad):
        raise ValueError(f"{name}: {what} must be [{B}, {Ad}]")
    return _chk(g, torch.float32, what)


def cac_det_actor_head(dq_da, one_minus_tanh2, q_pi, max_action: float = 1.0, out=None):
    """actor_loss = -mean Q(s, pi(s)) and its gradient w.r.t. the actor's raw output (ddpg.py:406, td3.py:216): dq_da [B, Ad]
    = d Q / d a (`mlp_input_grad` with d_out = 1), one_minus_tanh2 from `cac_det_action`, q_pi [B].
    -> dict(d_raw [B, Ad], partial f64): `qmix_finalize(partial, B, out)` gives {actor_loss, 0}."""
    _dev_only("cac_det_actor_head", dq_da, one_minus_tanh2, q_pi)
    if dq_da.dim() != 2 or dq_da.shape[0] < 1:
        raise ValueError("cac_det_actor_head: dq_da must be [B, Ad] with B >= 1")
    B, Ad = dq_da.shape
    cac_check(Ad)
    dq_da = _cac_grad("cac_det_actor_head", dq_da, B, Ad, "dq_da")
    omt2 = _cac_grad("cac_det_actor_head", one_minus_tanh2, B, Ad, "one_minus_tanh2")
    (q_pi,) = _head_args("cac_det_actor_head", B, (), (("q_pi", q_pi, torch.float32),))
    out = _out("cac_det_actor_head", out, (B, Ad), torch.float32, dq_da.device)
    partial = _head_partial(B, _abi.CAC_ROWS_PER_BLOCK, dq_da.device)
    call("tsm_cac_det_actor_head", ptr(dq_da), Ad, ptr(omt2), ptr(q_pi), B, Ad, float(max_action), ptr(out), ptr(partial),
         stream_ptr())
    return dict(d_raw=out, partial=partial)


def sac_actor_head(raw, z, q1a, q2a, dq1_da, dq2_da, alpha_dev, max_action: float = 1.0, unbounded: bool = False,
                   sigma_param=None, out=None):
    """SAC's actor loss mean(alpha logp - min(q1a, q2a)) with its closed-form backward (sac.py:315-322) and the entropy
    AutoAlpha reads (:325).  raw, z, sigma_param as `sac_action` took them; q1a, q2a [B] (q2a None: one critic) and their
    input gradients dq1_da, dq2_da [B, Ad] with d_out = 1.  -> dict(d_raw (the shape of raw: [d mu_raw | d sigma_raw] with
    conditioned sigma), d_sigma ([B, Ad] per row for a sigma_param, else None), logp [B], partial f64):
    `qmix_finalize` gives {actor_loss, mean -logp}; the partials are what `AutoAlpha.step_device` takes."""
    raw, B, Ad, ld, sg, sg_ptr, ld_s = _sac_raw("sac_actor_head", raw, sigma_param)
    cac_check(Ad)
    _dev_only("sac_actor_head", q1a, q2a, alpha_dev)
    if (q2a is None) != (dq2_da is None):
        raise ValueError("sac_actor_head: q2a and dq2_da come together")
    z = _cac_z("sac_actor_head", z, B, Ad)
    g1 = _cac_grad("sac_actor_head", dq1_da, B, Ad, "dq1_da")
    g2 = None if dq2_da is None else _cac_grad("sac_actor_head", dq2_da, B, Ad, "dq2_da")
    q1a, q2a = _head_args("sac_actor_head", B, (), (("q1a", q1a, torch.float32), ("q2a", q2a, torch.float32)))
    dev = raw.device
    out = _out("sac_actor_head", out, raw.shape, torch.float32, dev)
    d_sigma = torch.empty(B, Ad, dtype=torch.float32, device=dev) if sigma_param is not None else None
    ds_ptr = out.data_ptr() + 4 * Ad if d_sigma is None else d_sigma.data_ptr()
    logp = torch.empty(B, dtype=torch.float32, device=dev)
    partial = _head_partial(B, _abi.CAC_ROWS_PER_BLOCK, dev)
    # one pitch serves d_mu and d_sigma: 2 Ad inside `out`, or Ad in `out` and in d_sigma's own array
    call("tsm_sac_actor_head", ptr(raw), ld, sg_ptr, ld_s, ptr(z), ptr(q1a), ptr(q2a), ptr(g1), ptr(g2), Ad,
         ptr(_chk(alpha_dev, torch.float32, "alpha_dev")), B, Ad, float(max_action), int(bool(unbounded)), ptr(out), ds_ptr, ld,
         ptr(logp), ptr(partial), stream_ptr())
    return dict(d_raw=out, d_sigma=d_sigma, logp=logp, partial=partial)


# --------------------------------------------------------------------------------------------
# Offline continuous learners: CQL / Cal-QL and TD3+BC (imitation/cql.py, td3_bc.py; csrc/cql.hip)
# --------------------------------------------------------------------------------------------
def cql_check(act_dim: int, num_repeat: int = 1) -> None:
    """The bounds of the CQL kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_cql_check", int(act_dim), int(num_repeat))


def cql_uniform(n: int, lo: float, hi: float, seed: int, offset: int = 0, offset_dev=None, device="cuda", out=None):
    """n uniforms f32 in [lo, hi) (`uniform_(lo, hi)`, cql.py:303-307) from Philox (seed, offset + *offset_dev) under this
    draw's own key; lo == hi gives lo."""
    out = _out("cql_uniform", out, (int(n),), torch.float32, device, size="numel")
    call("tsm_cql_uniform", ptr(out), int(n), float(lo), float(hi), *_philox("cql_uniform", seed, offset, offset_dev), stream_ptr())
    return out


def cql_rows(obs, obs_next, act, rand_act, num_repeat: int, out=None, actor_rows=None):
    """The critics' stacked row block and the actor's rows of one CQL update in one launch (include/tsmarl.h: tsm_cql_rows).
    obs, obs_next [B, D], act [B, Ad], rand_act [B R, Ad] -> (x [B + 3 B R, D + Ad], actor_rows [2 B R, D]); the action columns
    of x's last 2 B R rows are left as they are, for `sac_action(out=x[B + B R:], col0=D)`."""
    _dev_only("cql_rows", obs, obs_next, act, rand_act)
    obs, obs_next, act, rand_act = (_chk(t, torch.float32, nm) for t, nm in ((obs, "obs"), (obs_next, "obs_next"), (act, "act"),
                                                                              (rand_act, "rand_act")))
    if obs.dim() != 2 or act.dim() != 2 or obs.shape[0] < 1 or act.shape[0] != obs.shape[0]:
        raise ValueError("cql_rows: obs must be [B, D] and act [B, Ad] with B >= 1")
    (B, D), Ad, R = obs.shape, act.shape[1], int(num_repeat)
    cql_check(Ad, R)
    if tuple(obs_next.shape) != (B, D) or tuple(rand_act.shape) != (B * R, Ad):
        raise ValueError(f"cql_rows: obs_next must be [{B}, {D}] and rand_act [{B * R}, {Ad}]")
    out = _out("cql_rows", out, (B + 3 * B * R, D + Ad), torch.float32, obs.device)
    actor_rows = _out("cql_rows", actor_rows, (2 * B * R, D), torch.float32, obs.device, "actor_rows")
    call("tsm_cql_rows", ptr(obs), ptr(obs_next), ptr(act), ptr(rand_act), B, R, D, Ad, ptr(out), ptr(actor_rows), stream_ptr())
    return out, actor_rows


def cql_head(q1, q2, target, logp_cur, logp_next, num_repeat: int, act_dim: int, calib=None, temperature: float = 1.0,
             cql_weight: float = 1.0, alpha_min: float = 0.0, alpha_max: float = 1e6, log_alpha=None):
    """Both critics' CQL loss between the forward on `cql_rows`' block and the backward (include/tsmarl.h: tsm_cql_head), one
    launch.  q1, q2 [B + 3 B R]; target [B]; logp_cur, logp_next [B R]; calib [B] or None; log_alpha f32 [1] in HBM or None
    (no multiplier).  -> dict(dq1, dq2 [B + 3 B R], partial f64) for `cql_finalize`."""
    _dev_only("cql_head", q1, q2, target, logp_cur, logp_next, calib, log_alpha)
    B, R = target.numel(), int(num_repeat)
    cql_check(act_dim, R)
    if B < 1:
        raise ValueError("cql_head: empty batch")
    n = B + 3 * B * R
    q1, q2 = _head_args("cql_head", n, (), (("q1", q1, torch.float32), ("q2", q2, torch.float32)))
    (target, calib) = _head_args("cql_head", B, (), (("target", target, torch.float32), ("calib", calib, torch.float32)))
    lpc, lpn = _head_args("cql_head", B * R, (), (("logp_cur", logp_cur, torch.float32), ("logp_next", logp_next, torch.float32)))
    dev = q1.device
    out = dict(dq1=torch.empty(n, dtype=torch.float32, device=dev), dq2=torch.empty(n, dtype=torch.float32, device=dev),
               partial=torch.empty(6 * -(-B * R // _abi.CQL_ROWS_PER_BLOCK), dtype=torch.float64, device=dev))
    # np.log(0.5 ** act.shape[-1]) (cql.py:236) in float64, as numpy forms it
    call("tsm_cql_head", ptr(q1), ptr(q2), ptr(target), ptr(lpc), ptr(lpn), ptr(calib), B, R, math.log(0.5 ** int(act_dim)),
         float(temperature), float(cql_weight), float(alpha_min), float(alpha_max),
         ptr(None if log_alpha is None else _chk(log_alpha, torch.float32, "log_alpha")), ptr(out["dq1"]), ptr(out["dq2"]),
         ptr(out["partial"]), stream_ptr())
    return out


def cql_finalize(partial, B: int, num_repeat: int, out, cql_weight: float = 1.0, lagrange_threshold: float = 10.0,
                 alpha_min: float = 0.0, alpha_max: float = 1e6, log_alpha=None, exp_avg=None, exp_avg_sq=None, step=None,
                 lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8):
    """The scalars of one CQL critic loss from `cql_head`'s partials and the multiplier's Adam step, one launch
    (include/tsmarl.h: tsm_cql_finalize).  out f32 [6] (HBM or pinned) <- {critic1_loss, critic2_loss, cql_alpha,
    cql_alpha_loss, d cql_alpha_loss / d log_alpha, log_alpha after the step}.  log_alpha f32 [1] in HBM or None; exp_avg,
    exp_avg_sq f32 [1], step i64 [1] in HBM, updated in place, or all None: no step."""
    _dev_only("cql_finalize", partial, log_alpha, exp_avg, exp_avg_sq, step)
    partial = _chk(partial, torch.float64, "partial").reshape(-1)
    if partial.numel() < 6 or partial.numel() % 6:
        raise ValueError("cql_finalize: partial must hold six sums per workgroup")
    state = (exp_avg, exp_avg_sq, step)
    if any(s is None for s in state) != all(s is None for s in state) or (exp_avg is not None and log_alpha is None):
        raise ValueError("cql_finalize: exp_avg, exp_avg_sq and step come together, with log_alpha")
    if log_alpha is not None:   # (stepped in place)
        _out("cql_finalize", log_alpha, (1,), torch.float32, None, "log_alpha", "min")
    if exp_avg is not None:
        for nm, t, dt in (("exp_avg", exp_avg, torch.float32), ("exp_avg_sq", exp_avg_sq, torch.float32), ("step", step, torch.int64)):
            _out("cql_finalize", t, (1,), dt, None, nm, "min")
    call("tsm_cql_finalize", ptr(partial), partial.numel() // 6, int(B), int(num_repeat), float(cql_weight), float(lagrange_threshold),
         float(alpha_min), float(alpha_max), ptr(log_alpha), ptr(exp_avg), ptr(exp_avg_sq), ptr(step), float(lr), float(betas[0]),
         float(betas[1]), float(eps), _out_or_pinned("cql_finalize", out, 6), stream_ptr())
    return out


def td3bc_actor_head(dq_da, one_minus_tanh2, q_pi, act_pi, act_data, alpha: float, max_action: float = 1.0, out=None):
    """TD3+BC's actor loss -lmbda mean Q(s, pi(s)) + mse(pi(s), a), lmbda = alpha / mean |Q|, and its gradient w.r.t. the
    actor's raw output (td3_bc.py:113-119), two launches (include/tsmarl.h: tsm_td3bc_actor_head).  dq_da,
    one_minus_tanh2, act_data [B, Ad]; q_pi [B]; act_pi [B, Ad]: the policy's action, which may be the action columns of the
    critic's rows (a column slice).  -> dict(d_raw [B, Ad], partial f64): `qmix_finalize(partial, B, out)` gives {actor_loss, 0}."""
    _dev_only("td3bc_actor_head", dq_da, one_minus_tanh2, q_pi, act_pi, act_data)
    if dq_da.dim() != 2 or dq_da.shape[0] < 1:
        raise ValueError("td3bc_actor_head: dq_da must be [B, Ad] with B >= 1")
    B, Ad = dq_da.shape
    cac_check(Ad)
    dq_da = _cac_grad("td3bc_actor_head", dq_da, B, Ad, "dq_da")
    omt2 = _cac_grad("td3bc_actor_head", one_minus_tanh2, B, Ad, "one_minus_tanh2")
    act_data = _cac_grad("td3bc_actor_head", act_data, B, Ad, "act_data")
    if tuple(act_pi.shape) != (B, Ad) or act_pi.dtype != torch.float32 or act_pi.stride(1) != 1 or (B > 1 and act_pi.stride(0) < Ad):
        raise ValueError(f"td3bc_actor_head: act_pi must be f32 [{B}, {Ad}] with unit column stride")
    (q_pi,) = _head_args("td3bc_actor_head", B, (), (("q_pi", q_pi, torch.float32),))
    dev = dq_da.device
    out = _out("td3bc_actor_head", out, (B, Ad), torch.float32, dev)
    partial, qsum = _head_partial(B, _abi.CAC_ROWS_PER_BLOCK, dev), torch.empty(2, dtype=torch.float64, device=dev)
    call("tsm_td3bc_actor_head", ptr(dq_da), Ad, ptr(omt2), ptr(q_pi), act_pi.data_ptr(), act_pi.stride(0) if B > 1 else Ad,
         ptr(act_data), B, Ad, float(max_action), float(alpha), ptr(qsum), ptr(out), ptr(partial), stream_ptr())
    return dict(d_raw=out, partial=partial, qsum=qsum)


# --------------------------------------------------------------------------------------------
# BCQ (imitation/bcq.py, utils/net/continuous.py:395-513; csrc/bcq.hip)
# --------------------------------------------------------------------------------------------
def bcq_check(act_dim: int, latent_dim: int = 1, num_sampled: int = 1) -> None:
    """The bounds of the BCQ kernels (include/tsmarl.h): ValueError naming the limit.  For constructors: every entry point
    checks its own arguments, so the wrappers below do not call it."""
    call("tsm_bcq_check", int(act_dim), int(latent_dim), int(num_sampled))


def _bcq_rows(name: str, what: str, t, rows: int | None = None, width: int | None = None):
    """`t` as a contiguous device f32 [rows, width] (None: any, at least one row and one column) -> (t, rows, width)."""
    _dev_only(name, t)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or (rows is not None and t.shape[0] != rows) or \
            (width is not None and t.shape[1] != width):
        want = ["n" if rows is None else rows, "width" if width is None else width]
        raise ValueError(f"{name}: {what} must be {want}, got {list(t.shape)}")
    return _chk(t, torch.float32, what), t.shape[0], t.shape[1]


def bcq_latent(head, eps, obs, out=None):
    """The VAE's reparameterised latent beside its observation (include/tsmarl.h: tsm_bcq_latent): head [B, 2 L] = [mean | raw
    log_std], eps [B, L], obs [B, D] -> (x_dec [B, D + L] = [obs | mean + std eps], std [B, L])."""
    eps, B, L = _bcq_rows("bcq_latent", "eps", eps)
    head, _, _ = _bcq_rows("bcq_latent", "head", head, B, 2 * L)
    obs, _, D = _bcq_rows("bcq_latent", "obs", obs, B)
    out = _out("bcq_latent", out, (B, D + L), torch.float32, obs.device)
    std = torch.empty(B, L, dtype=torch.float32, device=obs.device)
    call("tsm_bcq_latent", ptr(head), ptr(eps), ptr(obs), B, D, L, ptr(out), ptr(std), stream_ptr())
    return out, std


def bcq_decode_rows(src_a, rep_a: int, src_b, z, out=None):
    """The decoder's rows for `decode(obs)` with fresh clamped normals, two groups in one launch (include/tsmarl.h:
    tsm_bcq_decode_rows): src_a [n_a, D] each repeated rep_a times, src_b [n_b, D] or None, z [n_a rep_a + n_b, L]
    -> [n_a rep_a + n_b, D + L]."""
    src_a, n_a, D = _bcq_rows("bcq_decode_rows", "src_a", src_a)
    n_b = 0
    if src_b is not None:
        src_b, n_b, _ = _bcq_rows("bcq_decode_rows", "src_b", src_b, None, D)
    n = n_a * max(int(rep_a), 0) + n_b
    z, _, L = _bcq_rows("bcq_decode_rows", "z", z, n)
    out = _out("bcq_decode_rows", out, (n, D + L), torch.float32, src_a.device)
    call("tsm_bcq_decode_rows", ptr(src_a), n_a, int(rep_a), ptr(src_b), n_b, ptr(z), D, L, ptr(out), stream_ptr())
    return out


def bcq_action_rows(raw, x_dec, obs_dim: int, max_action: float = 1.0, out=None):
    """`max_action * tanh(raw)` beside the observation of the decoder's rows (include/tsmarl.h: tsm_bcq_action_rows): raw
    [n, Ad], x_dec [n, D + L] -> [n, D + Ad]."""
    raw, n, Ad = _bcq_rows("bcq_action_rows", "raw", raw)
    x_dec, _, Wd = _bcq_rows("bcq_action_rows", "x_dec", x_dec, n)
    D = int(obs_dim)
    if not 1 <= D < Wd:
        raise ValueError(f"bcq_action_rows: obs_dim = {D} outside [1, {Wd}), the decoder rows' width")
    out = _out("bcq_action_rows", out, (n, D + Ad), torch.float32, raw.device)
    call("tsm_bcq_action_rows", ptr(raw), ptr(x_dec), n, D, Wd - D, Ad, float(max_action), ptr(out), stream_ptr())
    return out


def bcq_target(q1, q2, rew, vmask, num_sampled: int, gamma: float, lmbda: float, out=None):
    """bcq.py:223-237 (include/tsmarl.h: tsm_bcq_target): q1, q2 [B K] of the lagged critics, rew [B], vmask [B] -> target [B]."""
    _dev_only("bcq_target", q1, q2, rew, vmask)
    B, K = rew.numel(), int(num_sampled)
    if B < 1:
        raise ValueError("bcq_target: empty batch")
    q1, q2 = _head_args("bcq_target", B * K, (), (("q1", q1, torch.float32), ("q2", q2, torch.float32)))
    rew, vmask = _head_args("bcq_target", B, (), (("rew", rew, torch.float32), ("vmask", vmask, torch.uint8)))
    out = _out("bcq_target", out, (B,), torch.float32, q1.device, size="numel")
    call("tsm_bcq_target", ptr(q1), ptr(q2), ptr(rew), ptr(vmask), B, K, float(gamma), float(lmbda), ptr(out), stream_ptr())
    return out


def bcq_vae_head(raw_dec, act, head, max_action: float = 1.0, out=None):
    """vae_loss = mse(act, recon) + KL / 2 and its gradient at the decoder's raw output (include/tsmarl.h: tsm_bcq_vae_head):
    raw_dec, act [B, Ad], head [B, 2 L] -> dict(d_raw [B, Ad], partial f64): `qmix_finalize(partial, B, out)` gives
    {vae_loss, KL_loss}."""
    raw_dec, B, Ad = _bcq_rows("bcq_vae_head", "raw_dec", raw_dec)
    act, _, _ = _bcq_rows("bcq_vae_head", "act", act, B, Ad)
    head, _, L2 = _bcq_rows("bcq_vae_head", "head", head, B)
    if L2 % 2:
        raise ValueError("bcq_vae_head: head is [mean | log_std], an even number of columns")
    out = _out("bcq_vae_head", out, (B, Ad), torch.float32, raw_dec.device)
    partial = _head_partial(B, _abi.CAC_ROWS_PER_BLOCK, raw_dec.device)
    call("tsm_bcq_vae_head", ptr(raw_dec), ptr(act), ptr(head), B, Ad, L2 // 2, float(max_action), ptr(out), ptr(partial),
         stream_ptr())
    return dict(d_raw=out, partial=partial)


def bcq_latent_grad(dz, head, eps, out=None):
    """The decoder's input gradient dz [B, L] -> the gradient of the encoder's output [B, 2 L] (include/tsmarl.h:
    tsm_bcq_latent_grad); head, eps as `bcq_latent` took them."""
    eps, B, L = _bcq_rows("bcq_latent_grad", "eps", eps)
    dz, _, _ = _bcq_rows("bcq_latent_grad", "dz", dz, B, L)
    head, _, _ = _bcq_rows("bcq_latent_grad", "head", head, B, 2 * L)
    out = _out("bcq_latent_grad", out, (B, 2 * L), torch.float32, dz.device)
    call("tsm_bcq_latent_grad", ptr(dz), ptr(head), ptr(eps), B, L, ptr(out), stream_ptr())
    return out


def bcq_perturb(raw_p, x_in, phi: float, max_action: float = 1.0, out=None, want_factor: bool = True):
    """Perturbation.forward behind its net (include/tsmarl.h: tsm_bcq_perturb): raw_p [n, Ad], x_in [n, D + Ad] the rows the
    net read -> (x_out [n, D + Ad] with the perturbed, clamped action, factor [n, Ad] for `cac_det_actor_head` or None)."""
    raw_p, n, Ad = _bcq_rows("bcq_perturb", "raw_p", raw_p)
    x_in, _, W = _bcq_rows("bcq_perturb", "x_in", x_in, n)
    if W <= Ad:
        raise ValueError(f"bcq_perturb: rows of {W} floats hold no observation beside {Ad} action components")
    out = _out("bcq_perturb", out, (n, W), torch.float32, raw_p.device)
    if out.data_ptr() == x_in.data_ptr():
        raise ValueError("bcq_perturb: out must not be x_in")
    factor = torch.empty(n, Ad, dtype=torch.float32, device=raw_p.device) if want_factor else None
    call("tsm_bcq_perturb", ptr(raw_p), ptr(x_in), n, W - Ad, Ad, float(phi), float(max_action), ptr(out), ptr(factor),
         stream_ptr())
    return out, factor


def bcq_select(q, rows, num_sampled: int, col0: int, act_dim: int, out=None):
    """The candidate of the first maximal q per group of `num_sampled` (include/tsmarl.h: tsm_bcq_select): q [n S], rows
    [n S, W] whose columns [col0, col0 + act_dim) hold the candidates -> (act [n, act_dim], index i32 [n])."""
    _dev_only("bcq_select", q)
    rows, nS, W = _bcq_rows("bcq_select", "rows", rows)
    S, Ad = int(num_sampled), int(act_dim)
    if S < 1 or nS % S or not 0 <= col0 <= W - Ad:
        raise ValueError(f"bcq_select: {nS} rows of {W} floats for groups of {S} and columns [{col0}, {col0 + Ad})")
    (q,) = _head_args("bcq_select", nS, (), (("q", q, torch.float32),))
    n = nS // S
    out = _out("bcq_select", out, (n, Ad), torch.float32, rows.device)
    index = torch.empty(n, dtype=torch.int32, device=rows.device)
    call("tsm_bcq_select", ptr(q), ptr(rows), W, int(col0), n, S, Ad, ptr(out), ptr(index), stream_ptr())
    return out, index


# --------------------------------------------------------------------------------------------
# REDQ (redq.py; csrc/redq.hip)
# --------------------------------------------------------------------------------------------
def redq_subset_mask(indices, ensemble_size: int) -> int:
    """The u64 subset mask of `tsm_redq_target`: bit e set for every member index e of `indices` (distinct, in [0, E))."""
    idx = [int(i) for i in indices]
    if not idx or len(set(idx)) != len(idx) or min(idx) < 0 or max(idx) >= int(ensemble_size) or ensemble_size > _abi.ENS_MAX_MEMBERS:
        raise ValueError(f"redq_subset_mask: {idx} is not a set of distinct members of an ensemble of {ensemble_size} "
                         f"(at most {_abi.ENS_MAX_MEMBERS})")
    mask = 0
    for i in idx:
        mask |= 1 << i
    return mask


def _redq_q(name: str, q):
    _dev_only(name, q)
    if q.dim() == 3 and q.shape[2] == 1:
        q = q[:, :, 0]
    if q.dim() != 2 or q.shape[1] < 1:
        raise ValueError(f"{name}: q must be [E, B] (or [E, B, 1]) with B >= 1")
    return _chk(q, torch.float32, "q"), q.shape[0], q.shape[1]


def redq_target(q_next, subset_mask: int, mode: str, mc, gpow, vmask, logp_next=None, alpha_dev=None, out=None):
    """The subset's min or mean of the lagged ensemble q_next [E, B], minus alpha * logp_next, then the n-step line
    (redq.py:254-269, algorithm_base.py:1213-1215).  -> returns f32 [B]."""
    q_next, E, B = _redq_q("redq_target", q_next)
    _dev_only("redq_target", mc, gpow, vmask, logp_next, alpha_dev)
    if mode not in ("min", "mean"):
        raise ValueError(f"Unsupported target_mode: {mode}")
    if (logp_next is None) != (alpha_dev is None):
        raise ValueError("redq_target: logp_next and alpha_dev come together")
    args = _head_args("redq_target", B, (), (("logp_next", logp_next, torch.float32), ("mc", mc, torch.float32),
                                             ("gpow", gpow, torch.float32), ("vmask", vmask, torch.uint8)))
    out = _out("redq_target", out, (B,), torch.float32, q_next.device, size="numel")
    call("tsm_redq_target", ptr(q_next), E, int(subset_mask) % 2**64, 0 if mode == "min" else 1, ptr(args[0]),
         ptr(None if alpha_dev is None else _chk(alpha_dev, torch.float32, "alpha_dev")), *map(ptr, args[1:]), B, ptr(out),
         stream_ptr())
    return out


def redq_critic_head(q, returns, weight=None):
    """redq.py:273-279 between the forward and the step: q [E, B].  -> dict(dq [E, B] = 2 w td / (E B), prio [B] = the signed
    ensemble mean of td = q - returns, partial f64): `qmix_finalize(partial, E * B, out)` gives {critic_loss, 0}."""
    q, E, B = _redq_q("redq_critic_head", q)
    _dev_only("redq_critic_head", returns, weight)
    args = _head_args("redq_critic_head", B, (), (("returns", returns, torch.float32), ("weight", weight, torch.float32)))
    dev = q.device
    out = dict(dq=torch.empty(E, B, dtype=torch.float32, device=dev), prio=torch.empty(B, dtype=torch.float32, device=dev),
               partial=_head_partial(B, _abi.REDQ_ROWS_PER_BLOCK, dev))
    call("tsm_redq_critic_head", ptr(q), E, *map(ptr, args), B, ptr(out["dq"]), ptr(out["prio"]), ptr(out["partial"]),
         stream_ptr())
    return out


def redq_mean_q(q, out=None):
    """critic(obs, a).mean(dim=0) (redq.py:287): q [E, B] -> f32 [B], the members summed in order."""
    q, E, B = _redq_q("redq_mean_q", q)
    out = _out("redq_mean_q", out, (B,), torch.float32, q.device, size="numel")
    call("tsm_redq_mean_q", ptr(q), E, B, ptr(out), stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# BDQN (bdqn.py; BranchingNet, utils/net/common.py:557-678; csrc/bdqn.hip)
# --------------------------------------------------------------------------------------------
def bdqn_check(num_branches: int, action_per_branch: int) -> None:
    """The bounds of the BDQN kernels (include/tsmarl.h): ValueError naming the limit."""
    call("tsm_bdqn_check", int(num_branches), int(action_per_branch))


def _bdqn_q(name: str, q):
    _dev_only(name, q)
    if q.dim() != 3:
        raise ValueError(f"{name}: q must be [B, K, A]")
    bdqn_check(q.shape[1], q.shape[2])
    return _chk(q, torch.float32, "q"), q.shape[0], q.shape[1], q.shape[2]


def bdqn_combine(adv, v):
    """BranchingNet.forward after its MLPs (common.py:669-677): adv [K, B, A] (the ensemble's output block), v [B] or [B, 1]
    -> q [B, K, A] = v + adv - mean_a adv."""
    _dev_only("bdqn_combine", adv, v)
    if adv.dim() != 3 or adv.shape[1] < 1:
        raise ValueError("bdqn_combine: adv must be [K, B, A] with B >= 1")
    K, B, A = adv.shape
    bdqn_check(K, A)
    if v.numel() != B:
        raise ValueError(f"bdqn_combine: v must have {B} entries")
    q = torch.empty(B, K, A, dtype=torch.float32, device=adv.device)
    call("tsm_bdqn_combine", ptr(_chk(adv, torch.float32, "adv")), ptr(_chk(v, torch.float32, "v").reshape(-1)), B, K, A, ptr(q),
         stream_ptr())
    return q


def bdqn_head(q, q_next_online, q_next_target, act, rew, end, gamma: float, weight=None, is_double: bool = True):
    """BDQN._target_q after its forwards, _compute_return and the masked TD loss with its gradient (bdqn.py:155-195, 211-221)
    in one launch.  q, q_next_online [B, K, A]; q_next_target [B, K, A] or None (no lagged network); act i32 [B, K]; rew f32
    [B]; end u8 / bool [B]; weight f32 [B] or None.
    -> dict(returns [B], prio [B] = sum_k td, d_adv [K, B, A], d_v [B], partial f64): `qmix_finalize(partial, B, out)` gives
    {loss, the mean taken q}."""
    q, B, K, A = _bdqn_q("bdqn_head", q)
    _dev_only("bdqn_head", q_next_online, q_next_target, act, rew, end, weight)
    if B < 1:
        raise ValueError("bdqn_head: empty batch")
    args = _head_args("bdqn_head", B, (("q_next_online", q_next_online, (B, K, A), torch.float32),
                                       ("q_next_target", q_next_target, (B, K, A), torch.float32),
                                       ("act", act, (B, K), torch.int32)),
                      (("rew", rew, torch.float32), ("end", end, torch.uint8), ("weight", weight, torch.float32)))
    dev = q.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    out = dict(returns=f(B), prio=f(B), d_adv=f(K, B, A), d_v=f(B), partial=_head_partial(B, _abi.BDQN_ROWS_PER_BLOCK, dev))
    call("tsm_bdqn_head", ptr(q), *map(ptr, args), B, K, A, float(gamma), int(bool(is_double)), ptr(out["returns"]),
         ptr(out["prio"]), ptr(out["d_adv"]), ptr(out["d_v"]), ptr(out["partial"]), stream_ptr())
    return out


def bdqn_egreedy(q, eps_dev, seed: int, offset: int = 0, offset_dev=None, out=None):
    """Per-branch epsilon-greedy actions (bdqn.py:76, 80-103) on the device: q [R, K, A] -> act i32 [R, K].  One coin per ROW;
    eps read from the device scalar eps_dev; row r draws at Philox counter offset + r."""
    q, R, K, A = _bdqn_q("bdqn_egreedy", q)
    _dev_only("bdqn_egreedy", eps_dev)
    out = _out("bdqn_egreedy", out, (R, K), torch.int32, q.device, size="min")
    call("tsm_bdqn_egreedy", ptr(q), R, K, A, ptr(_chk(eps_dev, torch.float32, "eps_dev")),
         *_philox("bdqn_egreedy", seed, offset, offset_dev), ptr(out), stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# Prioritized replay (data/utils/segtree.py, data/buffer/prio.py; csrc/segtree.hip)
# --------------------------------------------------------------------------------------------
def segtree_bound(size: int) -> int:
    """The smallest power of two >= size (segtree.py:20-22); ValueError outside [1, 2^30]."""
    bound = call("tsm_segtree_bound", int(size))
    if bound < 0:
        raise ValueError(f"segment tree: size = {size} outside [1, 2^30]")
    return bound


def _tree_index(t: "DeviceSegmentTree", name: str, index) -> torch.Tensor:
    _dev_only(name, index)
    return _chk(index, torch.int64, "index").reshape(-1)


def segtree_set(t: "DeviceSegmentTree", index, value) -> None:
    """`_setitem` (segtree.py:95-101): leaves index i64 [n] <- value f64 [n] or [1] (one for all), then their ancestors, in one
    launch.  Of several entries with one index the last wins."""
    index = _tree_index(t, "segtree_set", index)
    _dev_only("segtree_set", value)
    value = _chk(value, torch.float64, "value").reshape(-1)
    call("tsm_segtree_set", ptr(t.tree), ptr(t.mark), t.size, ptr(index), index.numel(), ptr(value), value.numel(),
         ptr(t.err), stream_ptr())


def segtree_prefix_sum_idx(t: "DeviceSegmentTree", value) -> torch.Tensor:
    """`_get_prefix_sum_idx` (segtree.py:119-134): value f64 [n] -> leaf indices i64 [n]."""
    _dev_only("segtree_prefix_sum_idx", value)
    value = _chk(value, torch.float64, "value").reshape(-1)
    out = torch.empty(value.numel(), dtype=torch.int64, device=value.device)
    call("tsm_segtree_prefix_sum_idx", ptr(t.tree), t.size, ptr(value), value.numel(), ptr(out), stream_ptr())
    return out


def segtree_reduce(t: "DeviceSegmentTree", start: int, end: int) -> torch.Tensor:
    """`_reduce` (segtree.py:104-116): the sum of leaves [start, end) -> f64 [1] in HBM."""
    out = torch.empty(1, dtype=torch.float64, device=t.tree.device)
    call("tsm_segtree_reduce", ptr(t.tree), t.size, int(start), int(end), ptr(out), stream_ptr())
    return out


def segtree_check(t: "DeviceSegmentTree") -> None:
    """ValueError if a launch since the last check met an index outside [0, size) (one synchronisation)."""
    call("tsm_segtree_check", ptr(t.err), stream_ptr())


def per_sample(t: "DeviceSegmentTree", n: int, seed: int, offset: int = 0, offset_dev=None) -> torch.Tensor:
    """prio.py:63-66 in one launch: n leaf indices i64 drawn in proportion to the leaves; draw i at Philox counter offset +
    *offset_dev + i."""
    out = torch.empty(int(n), dtype=torch.int64, device=t.tree.device)
    call("tsm_per_sample", ptr(t.tree), t.size, int(n), *_philox("per_sample", seed, offset, offset_dev), ptr(out), stream_ptr())
    return out


def per_update_weight(t: "DeviceSegmentTree", index, td, alpha: float, prio) -> None:
    """prio.py:81-90: leaves index <- (|td| + eps) ** alpha in float32, and prio f64 [2] = {max_prio, min_prio} folded."""
    index = _tree_index(t, "per_update_weight", index)
    _dev_only("per_update_weight", td)
    td = _chk(td, torch.float32, "td").reshape(-1)
    if td.numel() != index.numel():
        raise ValueError(f"per_update_weight: {td.numel()} weights for {index.numel()} indices")
    call("tsm_per_update_weight", ptr(t.tree), ptr(t.mark), t.size, ptr(index), ptr(td), index.numel(), float(alpha),
         ptr(_out("per_update_weight", prio, (2,), torch.float64, None, "prio", "min")), ptr(t.err), stream_ptr())


def per_init_weight(t: "DeviceSegmentTree", index, alpha: float, prio) -> None:
    """prio.py:46-47: leaves index <- max_prio ** alpha, max_prio read on the device."""
    index = _tree_index(t, "per_init_weight", index)
    _dev_only("per_init_weight", prio)
    call("tsm_per_init_weight", ptr(t.tree), ptr(t.mark), t.size, ptr(index), index.numel(), float(alpha),
         ptr(_chk(prio, torch.float64, "prio")), ptr(t.err), stream_ptr())


def per_get_weight(t: "DeviceSegmentTree", index, beta: float, weight_norm: bool, prio):
    """prio.py:69-79, 103-106: (leaf / min_prio) ** (-beta), over the batch maximum when weight_norm -> (f32 [n], f64 [n])."""
    index = _tree_index(t, "per_get_weight", index)
    _dev_only("per_get_weight", prio)
    n, dev = index.numel(), index.device
    out32 = torch.empty(n, dtype=torch.float32, device=dev)
    out64 = torch.empty(n, dtype=torch.float64, device=dev)
    call("tsm_per_get_weight", ptr(t.tree), t.size, ptr(index), n, float(beta), int(bool(weight_norm)),
         ptr(_chk(prio, torch.float64, "prio")), ptr(out32), ptr(out64), ptr(t.err), stream_ptr())
    return out32, out64


class DeviceSegmentTree:
    """`SegmentTree(size)` (segtree.py:5-93) in HBM: `tree` f64 [2 * bound] in the reference's layout."""

    def __init__(self, size: int, device="cuda") -> None:
        self.size = int(size)
        self.bound = segtree_bound(self.size)
        self.device = torch.device(device)
        self.tree = torch.zeros(2 * self.bound, dtype=torch.float64, device=self.device)
        self.mark = torch.full((self.bound,), -1, dtype=torch.int32, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int64, device=self.device)

    def __len__(self) -> int:
        return self.size

    def _dev(self, x, dtype) -> torch.Tensor:
        # (dtype given to as_tensor: a Python float would otherwise pass through torch's default float32 and lose bits)
        return torch.as_tensor(x, dtype=dtype).to(self.device).reshape(-1)

    def __getitem__(self, index) -> torch.Tensor:
        return self.tree[self._dev(index, torch.int64) + self.bound]

    def __setitem__(self, index, value) -> None:
        segtree_set(self, self._dev(index, torch.int64), self._dev(value, torch.float64))

    def reduce(self, start: int = 0, end: int | None = None) -> torch.Tensor:
        if start == 0 and end is None:
            return self.tree[1:2]
        if end is None:
            end = self.size
        if end < 0:
            end += self.size
        return segtree_reduce(self, start, end)

    def get_prefix_sum_idx(self, value) -> torch.Tensor:
        return segtree_prefix_sum_idx(self, self._dev(value, torch.float64))

    def check(self) -> None:
        segtree_check(self)


# --------------------------------------------------------------------------------------------
# MADDPG (ctde.py:728-955; csrc/maddpg.hip)
# --------------------------------------------------------------------------------------------
def maddpg_check(n_agents: int, act_dim: int | None = None) -> None:
    """The bounds of the MADDPG kernels (include/tsmarl.h): ValueError naming the limit."""
    if not 1 <= n_agents <= _abi.MADDPG_MAX_AGENTS:
        raise ValueError(f"MADDPG: n_agents = {n_agents}; the HIP kernels serve 1 to {_abi.MADDPG_MAX_AGENTS} agents")
    if act_dim is not None and act_dim < 1:
        raise ValueError(f"MADDPG: act_dim = {act_dim}; at least one action component is needed")


def _ptr_array(ts, name: str):
    return (C.c_void_p * len(ts))(*[ptr(_chk(t, torch.float32, name)) for t in ts])


def maddpg_joint_rows(obs, act, replace=None, out=None):
    """The centralized critics' inputs (ctde.py:875-880, 888, 893, 913-919) in one launch.  obs: per agent [B, D]; act: per
    agent [B, Ad].  replace=None -> [B, W] rows [obs_0 .. obs_{N-1} | act_0 .. act_{N-1}], W = N (D + Ad); replace = per
    agent [B, Ad] -> [N, B, W], matrix m carrying replace[m] in agent m's action slot."""
    N = len(obs)
    B, D = obs[0].shape
    Ad = act[0].shape[1]
    maddpg_check(N, Ad)
    if len(act) != N or (replace is not None and len(replace) != N):
        raise ValueError("maddpg_joint_rows: obs, act and replace need one entry per agent")
    for k in range(N):
        if tuple(obs[k].shape) != (B, D) or tuple(act[k].shape) != (B, Ad) or (
                replace is not None and tuple(replace[k].shape) != (B, Ad)):
            raise ValueError(f"maddpg_joint_rows: agent {k}: expected obs [{B}, {D}], act [{B}, {Ad}]")
    W = N * (D + Ad)
    shape = (B, W) if replace is None else (N, B, W)
    out = _out("maddpg_joint_rows", out, shape, torch.float32, obs[0].device)
    call("tsm_maddpg_joint_rows", _ptr_array(obs, "obs"), _ptr_array(act, "act"),
         None if replace is None else _ptr_array(replace, "replace"), N, B, D, Ad, ptr(out), stream_ptr())
    return out


def maddpg_partial_elems(B: int, n_agents: int) -> int:
    return call("tsm_maddpg_partial_elems", B, n_agents)


def maddpg_td(q, q_next, rew, term, gamma: float, out=None):
    """TD target, MSE and its gradient for every agent in one launch (ctde.py:895-898).  Per agent: q, q_next, rew f32 [B]
    (or [B, 1]), term u8 / bool [B] -- agent i's OWN flags.  -> (dq per agent [B], partial f64)."""
    N = len(q)
    B = q[0].numel()
    maddpg_check(N)
    if not (len(q_next) == len(rew) == len(term) == N):
        raise ValueError("maddpg_td: q, q_next, rew and term need one entry per agent")
    term = [t.contiguous().view(torch.uint8) if t.dtype == torch.bool else _chk(t, torch.uint8, "term") for t in term]
    for k in range(N):
        if not (q[k].numel() == q_next[k].numel() == rew[k].numel() == term[k].numel() == B):
            raise ValueError(f"maddpg_td: agent {k}: every array needs {B} entries")
    dev = q[0].device
    dq, partial = out if out is not None else ([None] * N, None)
    dq = [_out("maddpg_td", x, (B,), torch.float32, dev, "dq", "min") for x in dq]
    partial = _out("maddpg_td", partial, (maddpg_partial_elems(B, N),), torch.float64, dev, "partial", "min")
    ag = _abi.tsm_maddpg_agents()
    for k in range(N):
        ag.q[k] = ptr(_chk(q[k], torch.float32, "q"))
        ag.q_next[k] = ptr(_chk(q_next[k], torch.float32, "q_next"))
        ag.rew[k] = ptr(_chk(rew[k], torch.float32, "rew"))
        ag.term[k] = ptr(term[k])
        ag.dq[k] = ptr(dq[k])
    call("tsm_maddpg_td", C.byref(ag), N, B, float(gamma), ptr(partial), stream_ptr())
    return dq, partial


def maddpg_finalize(partial, q_pi, B: int, out):
    """out[2 i] = actor_loss_i = -mean(q_pi[i]), out[2 i + 1] = critic_loss_i from tsm_maddpg_td's partials (one launch,
    fixed summation order).  out: device f32 [2 N] or pinned host f32 [2 N]."""
    N = len(q_pi)
    maddpg_check(N)
    if any(x.numel() != B for x in q_pi):
        raise ValueError(f"maddpg_finalize: every q_pi needs {B} entries")
    partial = _chk(partial, torch.float64, "partial")
    call("tsm_maddpg_finalize", ptr(partial), partial.numel() // N, _ptr_array(q_pi, "q_pi"), N, B,
         _out_or_pinned("maddpg_finalize", out, 2 * N), stream_ptr())
    return out


def maddpg_act(mu, sigma_dev, seed: int, offset: int = 0, offset_dev=None, low=None, high=None, out=None):
    """The acting epilogue: mu per agent [E, Ad] -> act f32 [E * N, Ad] (row e * N + i), plus *sigma_dev times a standard
    normal draw, clamped to [low, high] (device f32 [Ad], both or neither)."""
    N = len(mu)
    E, Ad = mu[0].shape
    maddpg_check(N, Ad)
    if any(tuple(m.shape) != (E, Ad) for m in mu):
        raise ValueError(f"maddpg_act: every actor output must be [{E}, {Ad}]")
    if (low is None) != (high is None) or (low is not None and (low.numel() != Ad or high.numel() != Ad)):
        raise ValueError(f"maddpg_act: low and high come together, {Ad} entries each")
    out = _out("maddpg_act", out, (E * N, Ad), torch.float32, mu[0].device, size="numel")
    call("tsm_maddpg_act", _ptr_array(mu, "mu"), N, E, Ad, ptr(_chk(sigma_dev, torch.float32, "sigma_dev")),
         *_philox("maddpg_act", seed, offset, offset_dev), ptr(None if low is None else _chk(low, torch.float32, "low")),
         ptr(None if high is None else _chk(high, torch.float32, "high")), ptr(out), stream_ptr())
    return out


def polyak(target, param, tau: float):
    """target <- tau * param + (1 - tau) * target in place (update_target_networks, ctde.py:936-955), bit for bit the torch
    expression on f32 device tensors."""
    param = _chk(param, torch.float32, "param")
    _out("polyak", target, (param.numel(),), torch.float32, None, "target", "numel")   # (written in place)
    call("tsm_polyak", ptr(target), ptr(param), target.numel(), float(tau), stream_ptr())
    return target


# --------------------------------------------------------------------------------------------
# fully-connected networks of arbitrary width (csrc/dense.hip)
# --------------------------------------------------------------------------------------------
_ACT = {"none": 0, None: 0, "relu": 1, "tanh": 2}


def mlp_desc(dims, act: str = "relu") -> _abi.tsm_mlp_desc:
    dims = [int(d) for d in dims]
    if not 2 <= len(dims) <= 9:
        raise ValueError("mlp_desc: between 1 and 8 layers")
    d = _abi.tsm_mlp_desc()
    d.n_layers, d.act = len(dims) - 1, _ACT[act]
    for i, v in enumerate(dims):
        d.dims[i] = v
    return d


def mlp_param_count(desc) -> int:
    return call("tsm_mlp_param_count", C.byref(desc))


def _mlp_args(name: str, desc, params, x, acts=None, d_out=None):
    """The host checks the dense entries share, before any launch: device f32 tensors, x [B, dims[0]], a parameter vector that
    holds the net (the net reads its head: an actor keeps its sigma_param behind the layers) and, where given, `acts` of
    tsm_mlp_act_elems floats and `d_out` [B, dims[-1]].  -> (params, x, B, n_act, the net's parameter count)."""
    _dev_only(name, params, x, acts, d_out)
    x = _chk(x, torch.float32, "x")
    if x.dim() != 2 or x.shape[1] != desc.dims[0]:
        raise ValueError(f"{name}: input width != dims[0]: x must be [B, {desc.dims[0]}], got {tuple(x.shape)}")
    B = x.shape[0]
    n_param = mlp_param_count(desc)
    if n_param < 0:
        _abi.check(_abi.TSM_ERR_INVALID)
    if params.numel() < n_param:
        raise ValueError(f"{name}: params must hold the net's {n_param} floats, got {params.numel()}")
    n_act = call("tsm_mlp_act_elems", C.byref(desc), B)
    if acts is not None and (acts.dtype != torch.float32 or not acts.is_contiguous() or acts.numel() != n_act):
        raise ValueError(f"{name}: acts must be a contiguous f32 buffer of {n_act} floats, the activations of {B} rows")
    if d_out is not None and (d_out.dtype != torch.float32 or d_out.numel() != B * desc.dims[desc.n_layers]):
        raise ValueError(f"{name}: d_out must be f32 [{B}, {desc.dims[desc.n_layers]}]")
    return _chk(params, torch.float32, "params"), x, B, n_act, n_param


def mlp_forward(desc, params, x, acts=None):
    """-> (out [B, dims[-1]] view of the last activation block, acts buffer)."""
    params, x, B, n, _ = _mlp_args("mlp_forward", desc, params, x, acts)
    if acts is None:
        acts = torch.empty(n, dtype=torch.float32, device=x.device)
    call("tsm_mlp_forward", C.byref(desc), ptr(params), ptr(x), B, ptr(acts), stream_ptr())
    O = desc.dims[desc.n_layers]
    return acts[n - B * O:].view(B, O), acts


def mlp_forward_cond(desc, params, x, run_if, acts=None):
    """`mlp_forward` whose launches are no-ops when the device flag `run_if` (i32[1]) is zero -- a pass a captured graph
    holds but only some inputs need (value_next_select).  The returned tensors hold garbage when it did not run."""
    params, x, B, n, _ = _mlp_args("mlp_forward_cond", desc, params, x, acts)
    _dev_only("mlp_forward_cond", run_if)
    if run_if.numel() < 1:
        raise ValueError("mlp_forward_cond: run_if must hold one i32 flag")
    if acts is None:
        acts = torch.empty(n, dtype=torch.float32, device=x.device)
    call("tsm_mlp_forward_cond", C.byref(desc), ptr(params), ptr(x), B, ptr(acts), ptr(_chk(run_if, torch.int32, "run_if")),
         stream_ptr())
    O = desc.dims[desc.n_layers]
    return acts[n - B * O:].view(B, O), acts


_GATHER_KINDS = {torch.float32: 0, torch.int32: 1, torch.int64: 2, torch.uint8: 3, torch.bool: 3}


def gather_fields(fields: list, prepared: list | None = None) -> list:
    """Several row-gathers with element conversion in ONE launch (include/tsmarl.h: tsm_gather_fields).  A field is
    `(src, dst)` -- both contiguous, equal numel: a converting copy -- or `(src, dst, T, E, src_row_stride, src_offset)`: dst row
    r = e * T + t (env-major) reads `width = dst.numel() // (T * E)` elements at src row t * E + e (`src` a contiguous time-major
    store, strides in elements).  f32 -> f32; int32 / int64 / uint8 / bool -> int32 / int64 / float32 / uint8 / bool.
    Returns the prepared descriptor arrays: pass them back as `prepared` (with fields=None) to launch the SAME gathers again
    without rebuilding them -- for call sites whose sources and destinations are static allocations (per-call host cost: one
    ctypes call instead of ~30 us of descriptor building)."""
    if prepared is not None:
        for arr, n in prepared:
            call("tsm_gather_fields", arr, n, stream_ptr())
        return prepared
    done = []
    for k0 in range(0, len(fields), _abi.MAX_GATHER_FIELDS):
        chunk = fields[k0:k0 + _abi.MAX_GATHER_FIELDS]
        arr = (_abi.tsm_gather_field * len(chunk))()
        for k, fd in enumerate(chunk):
            src, dst = fd[0], fd[1]
            if not (src.is_contiguous() and dst.is_contiguous() and src.is_cuda and dst.is_cuda):
                raise ValueError("gather_fields: contiguous device tensors only")
            if src.dtype not in _GATHER_KINDS or dst.dtype not in _GATHER_KINDS:
                raise TypeError(f"gather_fields: {src.dtype} -> {dst.dtype} is not supported")
            if len(fd) == 2:
                if src.numel() != dst.numel():
                    raise ValueError("gather_fields: a converting copy needs equal sizes")
                n_rows, width, T, E, stride, off = dst.numel(), 1, 0, 0, 1, 0
            else:
                T, E, stride, off = (int(x) for x in fd[2:6])
                n_rows = T * E
                width = dst.numel() // max(n_rows, 1)
                if width * n_rows != dst.numel() or (n_rows and ((T * E - 1) * stride + off + width) > src.numel()):
                    raise ValueError("gather_fields: the mapping leaves the source or does not tile the destination")
            arr[k] = _abi.tsm_gather_field(src.data_ptr(), dst.data_ptr(), n_rows, T, E, stride, off, width,
                                           _GATHER_KINDS[src.dtype], _GATHER_KINDS[dst.dtype], 0)
        call("tsm_gather_fields", arr, len(chunk), stream_ptr())
        done.append((arr, len(chunk)))
    return done


def any_nonzero_u8(x, out=None):
    """Device flag i32[1] = 1 if any byte of `x` (u8 / bool, contiguous) is non-zero."""
    x = _chk(x, torch.uint8, "x")
    flag = _out("any_nonzero_u8", out, (1,), torch.int32, x.device, size="min")
    call("tsm_any_nonzero_u8", ptr(x), x.numel(), ptr(flag), stream_ptr())
    return flag


def value_next_select(v_s, v_last, v_full, flag, T: int, U: int, out=None):
    """V(obs_next) [T, U] of chained rows: v_s shifted by one slot + the last slot's own values `v_last` [U], or the full
    pass `v_full` [T, U] when `flag` says an episode ended before the last slot (include/tsmarl.h)."""
    v_s, v_last, v_full = (_chk(t, torch.float32, n) for t, n in ((v_s, "v_s"), (v_last, "v_last"), (v_full, "v_full")))
    if v_s.numel() != T * U or v_full.numel() != T * U or v_last.numel() != U:
        raise ValueError("value_next_select: shapes do not match T x U")
    res = _out("value_next_select", out, (T, U), torch.float32, v_s.device, size="min")
    call("tsm_value_next_select", ptr(v_s), ptr(v_last), ptr(v_full), ptr(_chk(flag, torch.int32, "flag")), T, U, ptr(res),
         stream_ptr())
    return res


def value_next_index(v_s, done, T: int, U: int, lanes_per_env: int = 1, out=None):
    """V(obs_next) [T, U] of a buffer without an obs_next store (ignore_obs_next, buffer_base.py:612-616): the next slot's
    V(obs), or the row's own at an episode end (`done` u8 [T, U / lanes_per_env]) and in the newest slot."""
    v_s = _chk(v_s, torch.float32, "v_s")
    done = done.contiguous().view(torch.uint8) if done.dtype == torch.bool else _chk(done, torch.uint8, "done")
    if v_s.numel() != T * U or done.numel() * lanes_per_env != T * U:
        raise ValueError("value_next_index: shapes do not match T x U")
    res = _out("value_next_index", out, (T, U), torch.float32, v_s.device, size="min")
    call("tsm_value_next_index", ptr(v_s), ptr(done), T, U, lanes_per_env, ptr(res), stream_ptr())
    return res


def value_next_select_env_major(v_s, v_last, v_full, flag, E: int, T: int, U: int, out=None):
    """`value_next_select` for env-major rows [E, T, U] (the per-agent batches of the MARL trainers)."""
    v_s, v_last, v_full = (_chk(t, torch.float32, n) for t, n in ((v_s, "v_s"), (v_last, "v_last"), (v_full, "v_full")))
    if v_s.numel() != E * T * U or v_full.numel() != E * T * U or v_last.numel() != E * U:
        raise ValueError("value_next_select_env_major: shapes do not match E x T x U")
    res = _out("value_next_select_env_major", out, (E * T, U), torch.float32, v_s.device, size="min")
    call("tsm_value_next_select_env_major", ptr(v_s), ptr(v_last), ptr(v_full), ptr(_chk(flag, torch.int32, "flag")), E, T, U,
         ptr(res), stream_ptr())
    return res


def mlp_n_split(B: int) -> int:
    """Default number of gradient slabs for a batch of B rows."""
    return max(1, min(64, -(-B // 256)))


def mlp_backward(desc, params, x, acts, d_out, n_split: int = 0, slabs=None, slab_stride: int = 0):
    """Gradient slabs [n_split, n_param] of sum(out * d_out) w.r.t. the flat parameter vector.
    `slabs` may point INTO the slabs of a larger joint parameter vector (slab_stride = its parameter count)."""
    params, x, B, _, n_param = _mlp_args("mlp_backward", desc, params, x, acts, d_out)
    if B < 1:
        raise ValueError("mlp_backward: batch must be >= 1")
    d_out = _chk(d_out, torch.float32, "d_out")
    # (fresh slabs are as wide as the caller's vector, which may hold more than the net)
    n_split, slabs, slab_stride = _slab_dest("mlp_backward", slabs, n_split, B,
                                             slab_stride or (params.numel() if slabs is None else n_param), n_param, x.device)
    d_acts = torch.empty_like(acts)
    call("tsm_mlp_backward", C.byref(desc), ptr(params), ptr(x), B, ptr(acts), ptr(d_out), ptr(d_acts), n_split,
         slabs.data_ptr(), slab_stride, stream_ptr())
    return slabs


def mlp_input_grad(desc, params, x, acts, d_out, col0: int, n_col: int, out=None, d_acts=None):
    """Gradient of sum(out * d_out) w.r.t. the input columns [col0, col0 + n_col) -> [B, n_col]; no weight gradients are
    computed (include/tsmarl.h: tsm_mlp_input_grad).  `acts`: the activations of mlp_forward on x."""
    if not (0 <= col0 and n_col >= 1 and col0 + n_col <= desc.dims[0]):
        raise ValueError(f"mlp_input_grad: columns [{col0}, {col0 + n_col}) leave the input width {desc.dims[0]}")
    params, x, B, n_act, _ = _mlp_args("mlp_input_grad", desc, params, x, acts, d_out)
    if B < 1:
        raise ValueError("mlp_input_grad: batch must be >= 1")
    d_out = _chk(d_out, torch.float32, "d_out")
    out = _out("mlp_input_grad", out, (B, n_col), torch.float32, x.device)
    d_acts = _out("mlp_input_grad", d_acts, (n_act,), torch.float32, x.device, "d_acts", "numel")   # a workspace the size of acts
    call("tsm_mlp_input_grad", C.byref(desc), ptr(params), ptr(x), B, ptr(acts), ptr(d_out), ptr(d_acts), col0, n_col, ptr(out),
         n_col, stream_ptr())
    return out


# --------------------------------------------------------------------------------------------
# grouped ensemble MLP: E nets of one shape, one launch per layer and role (utils/net/common.py:522-554; csrc/ensemble.hip)
# --------------------------------------------------------------------------------------------
def ens_mlp_param_count(desc, E: int) -> int:
    """Floats of the flat vector: per layer weight [E, in, out] then bias_weights [E, 1, out].  ValueError naming the limit
    for a bad descriptor or E outside [1, ENS_MAX_MEMBERS]."""
    n = call("tsm_ens_mlp_param_count", C.byref(desc), int(E))
    if n < 0:
        _abi.check(_abi.TSM_ERR_INVALID)
    return n


def _ens_args(name: str, desc, E: int, params, x):
    _dev_only(name, params, x)
    x = _chk(x, torch.float32, "x")
    if x.dim() != 2 or x.shape[1] != desc.dims[0]:
        raise ValueError(f"{name}: x must be [B, {desc.dims[0]}], the input all members share")
    if params.numel() != ens_mlp_param_count(desc, E):
        raise ValueError(f"{name}: params must hold {ens_mlp_param_count(desc, E)} floats for {E} members")
    return _chk(params, torch.float32, "params"), x, x.shape[0]


def ens_mlp_forward(desc, E: int, params, x, acts=None):
    """x [B, dims[0]] through all E members -> (out [E, B, dims[-1]] view of the last activation block, acts buffer)."""
    params, x, B = _ens_args("ens_mlp_forward", desc, E, params, x)
    n = call("tsm_ens_mlp_act_elems", C.byref(desc), int(E), B)
    acts = _out("ens_mlp_forward", acts, (n,), torch.float32, x.device, "acts", "min")
    call("tsm_ens_mlp_forward", C.byref(desc), int(E), ptr(params), ptr(x), B, ptr(acts), stream_ptr())
    O = desc.dims[desc.n_layers]
    return acts[n - E * B * O:].view(E, B, O), acts


def ens_mlp_backward(desc, E: int, params, x, acts, d_out, n_split: int = 0, slabs=None, slab_stride: int = 0):
    """Gradient slabs [n_split, n_param] of sum(out * d_out), d_out [E, B, dims[-1]], in the parameter layout."""
    params, x, B = _ens_args("ens_mlp_backward", desc, E, params, x)
    d_out = _chk(d_out, torch.float32, "d_out")
    if d_out.numel() != E * B * desc.dims[desc.n_layers]:
        raise ValueError(f"ens_mlp_backward: d_out must be [{E}, {B}, {desc.dims[desc.n_layers]}]")
    n_split, slabs, slab_stride = _slab_dest("ens_mlp_backward", slabs, n_split, B, slab_stride or params.numel(), params.numel(),
                                             x.device)
    d_acts = torch.empty_like(acts)
    call("tsm_ens_mlp_backward", C.byref(desc), int(E), ptr(params), ptr(x), B, ptr(acts), ptr(d_out), ptr(d_acts), n_split,
         slabs.data_ptr(), slab_stride, stream_ptr())
    return slabs


def ens_mlp_input_grad(desc, E: int, params, x, acts, d_out, col0: int, n_col: int, out=None):
    """Gradient of sum(out * d_out) w.r.t. the shared input's columns [col0, col0 + n_col) -> [B, n_col]: the sum over the
    members, in member order; no weight gradients."""
    params, x, B = _ens_args("ens_mlp_input_grad", desc, E, params, x)
    d_out = _chk(d_out, torch.float32, "d_out")
    if not (0 <= col0 and n_col >= 1 and col0 + n_col <= desc.dims[0]):
        raise ValueError(f"ens_mlp_input_grad: columns [{col0}, {col0 + n_col}) leave the input width {desc.dims[0]}")
    if d_out.numel() != E * B * desc.dims[desc.n_layers]:
        raise ValueError(f"ens_mlp_input_grad: d_out must be [{E}, {B}, {desc.dims[desc.n_layers]}]")
    out = _out("ens_mlp_input_grad", out, (B, n_col), torch.float32, x.device)
    d_acts = torch.empty_like(acts)
    call("tsm_ens_mlp_input_grad", C.byref(desc), int(E), ptr(params), ptr(x), B, ptr(acts), ptr(d_out), ptr(d_acts), col0, n_col,
         ptr(out), n_col, stream_ptr())
    return out


def device_info() -> dict:
    n_cu, wave, hbm = C.c_int(), C.c_int(), C.c_int64()
    name = C.create_string_buffer(64)
    call("tsm_device_info", C.byref(n_cu), C.byref(wave), C.byref(hbm), name)
    return dict(n_cu=n_cu.value, wave_size=wave.value, hbm_bytes=hbm.value, arch=name.value.decode())


KERNEL_OPTIONS = ("actor_tile", "split_bf16", "generic_kernels", "rollout_form")


_options_cache = None  # kernel_options() as last read: options change only through set_kernel_option (the environment defaults
                       # are resolved once, at first use), and the tuple is part of every per-call graph key


def kernel_option(name: str) -> int:
    """Value of a kernel selection option (include/tsmarl.h: tsm_kernel_option_get)."""
    v = C.c_int32()
    call("tsm_kernel_option_get", name.encode(), C.byref(v))
    return v.value


def set_kernel_option(name: str, value: int) -> int:
    """Override a kernel selection rule for this process; returns the previous value."""
    global _options_cache
    old = kernel_option(name)
    _options_cache = None
    call("tsm_kernel_option_set", name.encode(), int(value))
    return old


def kernel_options() -> tuple:
    """All option values in KERNEL_OPTIONS order: part of every launch-cache (hipGraph) key."""
    global _options_cache
    if _options_cache is None:
        _options_cache = tuple(kernel_option(n) for n in KERNEL_OPTIONS)
    return _options_cache


class graph_capture:
    """`with ops.graph_capture(graph[, pool=...]):` -- torch.cuda.graph with Python's cyclic garbage collector held off while the
    stream is capturing.  A collection that happens to run inside a capture and frees a device tensor or destroys another
    hipGraph is an operation the capturing stream does not permit: the process aborts ("Fatal Python error: Aborted ...
    Garbage-collecting", seen in the test suite once enough graph-holding objects had become garbage)."""

    def __init__(self, graph, pool=None):
        self._cm = torch.cuda.graph(graph) if pool is None else torch.cuda.graph(graph, pool=pool)
        self._was = False

    def __enter__(self):
        import gc

        self._was = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            return self._cm.__enter__()
        except BaseException:
            if self._was:
                gc.enable()
            raise

    def __exit__(self, *exc):
        import gc

        try:
            return self._cm.__exit__(*exc)
        finally:
            if self._was:
                gc.enable()


class gc_hold:
    """`with ops.gc_hold():` -- one collection now, none inside: for capture sites that drive `capture_begin` / `capture_end`
    themselves (a side stream, thread-local capture mode) and therefore cannot use `graph_capture`."""

    def __enter__(self):
        import gc

        self._was = gc.isenabled()
        gc.collect()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc

        if self._was:
            gc.enable()
        return False


def capture_steps(w: dict, make_steps, reduce_, segmented: bool = False, capture=None) -> None:
    """Capture a launch sequence written as a generator of synchronisation points: `make_steps()` launches everything in
    order and YIELDS each tensor that has to be summed over the ranks at that point; `reduce_(tensor)` sums it in place.
      * not segmented: ONE graph with the collectives inside (or none at all) -> w["graph"].  `capture(graph, fn)` captures
        where a plain `graph_capture` will not do (PPO._capture_graph: RCCL collectives on a side stream);
      * segmented (the backend's collectives cannot be captured -- gloo --, or the capture probe failed): every stretch
        between two collectives is its own hipGraph on ONE shared memory pool, replayed in capture order with the
        collectives run eagerly in between -> w["segments"] = [(graph, tensor to reduce behind it | None)].
    One definition of the sequence serves both forms, and the eager launches too (drive the generator with `reduce_`)."""
    if not segmented:
        graph = torch.cuda.CUDAGraph()

        def run():
            for t in make_steps():
                reduce_(t)

        if capture is None:
            with graph_capture(graph):
                run()
        else:
            capture(graph, run)
        w["graph"] = graph
        return
    pool = torch.cuda.graph_pool_handle()
    segs, gen, more = [], make_steps(), True
    while more:
        g_ = torch.cuda.CUDAGraph()
        t_ = None
        with graph_capture(g_, pool=pool):
            try:
                t_ = next(gen)
            except StopIteration:
                more = False
        segs.append((g_, t_))
    w["segments"] = segs


def replay_steps(w: dict, reduce_) -> None:
    """Replay what `capture_steps` left in `w`: the one graph, or the segments with their collectives in between."""
    if w.get("graph") is not None:
        w["graph"].replay()
        return
    for g_, t_ in w["segments"]:
        g_.replay()
        if t_ is not None:
            reduce_(t_)


class kernel_override:
    """`with ops.kernel_override(actor_tile=64): ...` -- options set inside, restored on exit."""

    def __init__(self, **opts: int):
        self._opts, self._old = opts, {}

    def __enter__(self):
        for k, v in self._opts.items():
            self._old[k] = set_kernel_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self._old.items():
            set_kernel_option(k, v)
        return False


__all__ = [n for n in dir() if not n.startswith("_")]
_ = _abi
