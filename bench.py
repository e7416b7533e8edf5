#!/usr/bin/env python3
"""bench.py -- headline benchmark of the rollout + update hot path (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic rollouts: collect T = max_cycles
vector steps of `n_env` simple_spread worlds per GPU (fused actor+critic+sampling, batched env step,
buffer index algebra + SoA scatter), then one PPO update on those rows (critic passes, GAE, minibatch
loop of fused forward/loss/backward + Adam).  Workload at N=1: BASELINE configs[1] (simple_spread N=3,
shared PPO, num_envs=1024, obs 18, A=5, T=25, MLP 64-64).  N>1: env shards per rank (weak scaling:
1024 envs per GPU, BASELINE configs[3]) with one RCCL all-reduce of the flat gradient per gradient step.
value = env-steps/s = (n_env * n_agent * T * n_gpus) / max-over-ranks step time.
Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the steps and prints the headline figure
(`value`, `ms_per_step`); `--full` adds, after the timed steps, the collect / update split, the replica check, the
rooflines and `cpu_baseline`.  `--dump-outputs DIR` writes what the last timed step computed (buffer rows, parameters,
episode returns, losses) as DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X_MICROARCH.md "HBM3E peak BW 8.0 TB/s spec"
MFMA_F32_PEAK = 157.3e12  # FLOP/s, MI355X_MICROARCH.md "Peak FP32 (matrix) 157.3 TFLOPS" (f32-input MFMA)
# (round 5, measured: profiles/r05_probe_mfma_f32_issue.txt -- the clock read directly, s_memtime / s_memrealtime around the loop)
PEAK_NOTE = ("the f32-MFMA peak is 2.4 GHz x 256 flop/clk/CU; the part holds 2.39-2.40 GHz under sustained f32-MFMA load on all 256 "
             "CUs, zero or random operands, and back-to-back v_mfma_f32_16x16x4_f32 / 32x32x2 issue at 0.99 of the nominal rate with 1, 2 "
             "or 4 waves per SIMD (profiles/r05_probe_mfma_f32_issue.txt; the 0.86 / 0.74 of r05_probe_mfma_valu_overlap.txt were that "
             "probe's own accumulator copies); f32 MFMAs and the f32 VALU instructions of the other wave of a SIMD take turns (0.856 us + "
             "0.360 us alone -> 1.200 us together), so frac = the share of SIMD cycles that issue useful MFMAs: no clock or issue discount")


def mlp_flops(dims) -> tuple[int, int]:
    """USEFUL flops per input row of an MLP `dims[0] -> ... -> dims[-1]` (multiply-add = 2; biases, activations, padding of
    narrow layers to MFMA tiles not counted): (forward, backward).  Backward = weight gradient of every layer + input
    gradient of every layer but the first (nothing consumes dX of layer 1, and no kernel here forms it):
    forward 2 sum(a b); backward 4 sum over layers >= 2 of (a b) + 2 dims[0] dims[1]."""
    pairs = list(zip(dims[:-1], dims[1:]))
    return 2 * sum(a * b for a, b in pairs), 4 * sum(a * b for a, b in pairs[1:]) + 2 * pairs[0][0] * pairs[0][1]


# Fields of the JSON line that are LOOKED UP in committed profiles of earlier runs of this same command (they need rocprofv3 passes
# the default run does not make): every file a lookup read, by field name.  Emitted as `profile_sources` on the line.
_SOURCES: dict = {}


def _source(field: str, path: str) -> None:
    _SOURCES.setdefault(field, [])
    rel = os.path.relpath(path, ROOT)
    if rel not in _SOURCES[field]:
        _SOURCES[field].append(rel)


# Environment variables / process-wide switches that change WHICH kernel an entry point launches (or arm diagnostics).  A run with
# any of them set is not the configuration the line claims: refused unless --allow-options, and then labelled "diagnostic".
KERNEL_ENV = ("TSM_DBG", "TSM_GENERIC_KERNELS", "TSM_ACTOR_TILE", "TSM_SPLIT_BF16", "TSM_ROLLOUT_FORM", "TSM_UPDATE_MAX_BLOCKS",
              "TSM_CRITIC_GEN", "TSM_CRITIC_SPLIT_DW2", "TSM_UPDATE_FORM")


def kernel_env_set() -> list:
    return [k for k in KERNEL_ENV if os.environ.get(k) not in (None, "")]


def kernel_configuration() -> dict:
    """What selects kernels in this process, read from the library itself (host state only, no device call): the run-time
    options (ops.kernel_options), the debug switches of csrc/mlp_fused.hip (update variant, slab store flavour) and whether phase
    stamps are armed (tsm_debug_set_stamps) -- plus the environment variables above."""
    import ctypes

    from tianshou_marl_amd import _abi, ops

    st = (ctypes.c_int32 * 4)()
    _abi.load().tsm_debug_get_state(st)
    cfg = dict(zip(ops.KERNEL_OPTIONS, ops.kernel_options()))
    cfg.update(update_variant=int(st[0]), slab_store=int(st[1]), stamps_armed=bool(st[2]), env=kernel_env_set())
    cfg["default"] = not any(v for k, v in cfg.items() if k != "default")
    return cfg


def guard_configuration(a, out: dict | None = None) -> None:
    """Refuse (exit code 3) a run whose kernel selection is not the default, unless --allow-options; with it, label the line."""
    env = kernel_env_set()
    if out is None:  # the early check: environment only, BEFORE anything touches the GPU
        if env and not a.allow_options:
            raise SystemExit("bench.py: refusing to run with %s set (kernel selection / diagnostics switches): the line would not be "
                             "the configuration it names.  Unset them, or pass --allow-options for a run labelled \"diagnostic\"."
                             % ", ".join(env))
        return
    cfg = kernel_configuration()
    out.setdefault("config", {})["kernel_options"] = cfg
    if not cfg["default"]:
        if not a.allow_options:
            raise SystemExit("bench.py: kernel options are not at their defaults (%s): pass --allow-options for a diagnostic run" % cfg)
        out["diagnostic"] = True


def in_situ_us(kernel: str, workload: str = "bench", grid: int | None = None, near_us: float | None = None):
    """Average duration (us) of `kernel` INSIDE the job's own launch sequence, from the committed rocprofv3 --kernel-trace
    --stats summary of that job (profiles/*_{workload}_kernel_stats.json, tools/summarize_profile.py); None if absent.
    grid (threads) / near_us pick the row where the summary lists the kernel at several grids or problem sizes."""
    import glob
    import math

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_%s_kernel_stats.json" % workload)))
    if not files:
        return None
    rows = [r for r in json.load(open(files[-1])).get("by_grid", []) if kernel in r["kernel"] and (grid is None or r["grid"] == grid)]
    if not rows:
        return None
    _source("in_situ_us_rocprof", files[-1])
    if near_us is not None:
        rows.sort(key=lambda r: abs(math.log(r["avg_us"] / near_us)))
    else:
        rows.sort(key=lambda r: -r["total_ms"])
    return round(rows[0]["avg_us"], 3)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # a step is ~0.7 ms: 200 timed steps keep the fill/drain of the 1-step host pipeline (~0.2 ms) below 0.2 %
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n-env", type=int, default=1024, help="envs per GPU")
    ap.add_argument("--n-agent", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=25)
    ap.add_argument("--minibatch", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--dispatch", default="per_agent", choices=["per_agent", "pooled"])
    ap.add_argument("--c3-dispatch", default="pooled", choices=["per_agent", "pooled"],
                    help="c3ppo: pooled = minibatches of joint rows (critic once per row); per_agent = MARLDispatcher order")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--allow-options", action="store_true",
                    help="run although kernel-selection options / TSM_* switches are not at their defaults; the line says \"diagnostic\": true")
    ap.add_argument("--no-batch64", action="store_true", help="skip the reference-default (batch 64) update timing")
    ap.add_argument("--ignore-obs-next", action="store_true",
                    help="c3ppo: a buffer without an obs_next store (VectorReplayBuffer(ignore_obs_next=True), buffer_base.py:612-616): "
                         "the rollout writes half the observation rows, V(obs_next) comes from V(obs) at next(index)")
    ap.add_argument("--no-c3-grid", action="store_true", help="skip the roofline_grid entries of the 4096 x 8 configuration")
    ap.add_argument("--pooled-grid", action="store_true",
                    help="extended roofline_grid: the fused gradient step at a pooled 65 536-row minibatch and GAE at the "
                         "synthetic horizons T = 2048 and 256")
    ap.add_argument("--cpu-envs", type=int, default=0, help="envs of the CPU baseline sample (0 = the GPU job's --n-env)")
    ap.add_argument("--tag-envs", type=int, default=512, help="tag: simple_tag envs per GPU (BASELINE configs[4]: 4096 over 8 GPUs)")
    ap.add_argument("--workload", default="c2", choices=["c2", "c3", "c3ppo", "tag"],
                    help="c2 (default, the headline line): simple_spread N=3 shared PPO; c3: N=8 CTDEPolicy, 4096 envs; "
                         "c3ppo: N=8 PPO with a centralized critic, 4096 envs")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check what the headline figure does not need: the collect / "
                         "update split, the replica check of N > 1, the batch-64 update, the kernel rooflines and their 4096 x 8 "
                         "grid, the CPU baseline (each --no-* switch above still drops its part)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    return ap.parse_args()


def build_job(a, device, rank):
    from tianshou_marl_amd.algorithm.ppo import PPO
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.utils.net import DiscreteActorCritic

    env = DeviceSimpleSpreadVectorEnv(a.n_env, a.n_agent, max_cycles=a.horizon, device=device, seed=1626 + rank)
    net = DiscreteActorCritic(env.obs_dim, env.n_act, 64, device=device, init="orthogonal", seed=1626)
    # (tools/soak_determinism.py --stable passes other PPO hyper-parameters; the bench itself keeps the reference defaults)
    algo = PPO(net=net, lr=3e-4, dispatch=a.dispatch, shuffle="device", seed=1626 + rank, async_stats=True,
               **getattr(a, "ppo_kwargs", {}))
    buf = DeviceVectorReplayBuffer(a.n_env * a.horizon, a.n_env, a.n_agent, env.obs_dim, device=device)
    col = Collector(algo, env, buf, async_stats=True)  # stats resolve lazily: no per-step host sync
    col.reset()
    return env, net, algo, buf, col


def _allreduce_path(sync) -> dict:
    """Which way the replicas' gradients travel, for the bench line's `config` (parallel.p2p_mode: the first-use handshake
    decides unless TSM_P2P_ALLREDUCE forces or forbids the peer-memory path)."""
    if sync is None:
        return {}
    from tianshou_marl_amd.parallel import p2p_mode

    if getattr(sync, "p2p", None) is not None:
        return {"gradient_all_reduce": "peer memory (one-shot LL exchange; handshake passed; TSM_P2P_ALLREDUCE mode %s)" % p2p_mode()}
    return {"gradient_all_reduce": "process group (%s) all-reduce (peer-memory mode %s%s)"
                                   % (sync.dist.get_backend(sync.group), p2p_mode(),
                                      "" if p2p_mode() == "off" else ": setup or handshake declined, see stderr")}


def _resolve(stats):
    """Read a statistics object now if it is a lazy one (eager paths return finished objects)."""
    r = getattr(stats, "resolve", None)
    if callable(r):
        r()


DUMP_LIMIT = 64 << 20        # --dump-outputs: bytes in all
DUMP_BUFFER_BYTES = 32 << 20  # of them for the buffer rows: a larger buffer is cut to a fixed, seeded sample of its rows


def buffer_outputs(buf) -> dict:
    """The rows the last collect wrote: every store of the buffer, [slot, env, agent] rows flattened.  All of them while they
    fit DUMP_BUFFER_BYTES, else the same fixed, seeded sample of rows from every store (the same rows from run to run)."""
    stores = {"obs": buf.obs_store, "obs_next": buf.obs_next_store, "act": buf.act_store, "rew": buf.rew_store,
              "terminated": buf.term_store, "truncated": buf.trunc_store, "logp": buf.logp_store, "v_s": buf.vs_store,
              "v_next": buf.vnext_store}
    rows = buf.act_store.numel()
    stores = {k: v.reshape(rows, -1) for k, v in stores.items() if v is not None}
    keep = min(rows, DUMP_BUFFER_BYTES // (4 * sum(v.shape[1] for v in stores.values())))
    if keep < rows:
        idx = torch.from_numpy(np.sort(np.random.default_rng(1626).choice(rows, keep, replace=False))).to(buf.act_store.device)
        stores = {k: v[idx] for k, v in stores.items()}
    return stores


def episode_outputs(cs) -> dict:
    """Returns and lengths of the episodes a collect finished (CollectStats)."""
    return {"episode_returns": np.asarray(cs.returns, np.float64), "episode_lens": np.asarray(cs.lens, np.float64)}


def scalar_outputs(prefix: str, stats) -> dict:
    """Every scalar of a statistics object (TrainingStats: its loss statistics) or of a (nested) dict of them, one array each."""
    if hasattr(stats, "get_loss_stats_dict"):
        stats = stats.get_loss_stats_dict()
    if hasattr(stats, "items"):
        out = {}
        for k, v in sorted(stats.items()):
            out.update(scalar_outputs("%s_%s" % (prefix, str(k).replace("/", "_")), v))
        return out
    return {prefix: np.array([float(stats)], np.float64)}


def dump_outputs(path: str, arrays: dict) -> None:
    """--dump-outputs: every array as path/<name>.npy, float64 kept as it is and everything else as float32."""
    out = {}
    for name, x in arrays.items():
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        out[name] = x.astype(np.float64 if x.dtype == np.float64 else np.float32)
    total = sum(x.nbytes for x in out.values())
    if total > DUMP_LIMIT:
        raise SystemExit("bench.py --dump-outputs: %d bytes of outputs, more than the %d allowed" % (total, DUMP_LIMIT))
    os.makedirs(path, exist_ok=True)
    for name, x in out.items():
        np.save(os.path.join(path, name + ".npy"), x)


def one_step(a, algo, buf, col):
    from tianshou_marl_amd.algorithm.ppo import policy_within_training_step

    with policy_within_training_step(algo):
        cs = col.collect(n_step=a.n_env * a.horizon)
        ts = algo.update(buf, a.minibatch, a.repeat)
    # A trainer reads the statistics of every step (trainer.py:1063-1104: collect stats feed the logger and the
    # stop/test criteria, training stats the logger).  Both objects are lazy: reading the collect statistics here,
    # after update() has been queued, waits for the rollout only, and the training statistics are read one step late,
    # so the device never idles while the host looks at numbers -- and the host never queues more than one step
    # ahead (an unbounded run-ahead makes the HIP runtime drain its queue every ~10 steps, a 2 ms stall each time).
    _resolve(cs)
    _resolve(getattr(algo, "_bench_prev_ts", None))
    algo._bench_prev_ts = ts
    col.reset_buffer(keep_statistics=True)  # trainer.py:1104
    return cs, ts


def phase_times(a, algo, buf, col, reps=5):
    """Per-phase device time (HIP events on the launch stream) outside the timed region."""
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.ppo import policy_within_training_step

    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t_col = t_upd = 0.0
    for _ in range(reps):
        e0, e1, e2 = ev(), ev(), ev()
        with policy_within_training_step(algo):
            e0.record()
            col.collect(n_step=a.n_env * a.horizon)
            e1.record()
            algo.update(buf, a.minibatch, a.repeat)
            e2.record()
        torch.cuda.synchronize()
        t_col += e0.elapsed_time(e1)
        t_upd += e1.elapsed_time(e2)
        col.reset_buffer(keep_statistics=True)
    return t_col / reps, t_upd / reps


def batch64_update(a, algo, buf, col, reps: int = 3) -> dict:
    """`PPO.update` at the REFERENCE's own defaults (trainer.py:287,295, ppo.py:25-36: batch_size 64, repeat 1) on the rows of one
    collect of this job -- 400 gradient steps of 64 rows per agent, 1 200 per update at the default size -- outside the timed region:
    the GPU counterpart of `cpu_baseline.update_reference_default_batch64`.  Device time by HIP events around
    the update (one hipGraph replay after the first, capturing call)."""
    from tianshou_marl_amd.algorithm.ppo import policy_within_training_step

    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    times, steps = [], None
    with policy_within_training_step(algo):
        for k in range(reps + 1):
            col.collect(n_step=a.n_env * a.horizon)
            e0, e1 = ev(), ev()
            e0.record()
            ts = algo.update(buf, 64, 1)
            e1.record()
            torch.cuda.synchronize()
            _resolve(ts)
            col.reset_buffer(keep_statistics=True)
            if k:  # (call 0 captures the graph)
                times.append(e0.elapsed_time(e1))
            steps = getattr(ts, "gradient_steps", None) or sum(s_.gradient_steps for s_ in getattr(ts, "_agent_id_to_stats", {}).values())
    return {"ms": float(np.median(times)), "ms_all": [round(t, 3) for t in times], "gradient_steps": int(steps), "batch_size": 64,
            "repeat": 1, "rows": a.n_env * a.horizon * a.n_agent, "us_per_gradient_step": float(np.median(times)) * 1e3 / max(int(steps), 1),
            "timing": "HIP events around PPO.update (hipGraph replay), outside the timed region"}


def loss_grid_threads(M: int) -> int:
    """Grid of loss_kernel for M samples (csrc/ppo_loss.hip loss_blocks): 256-sample tiles, at most 2048 workgroups, every
    workgroup the same number of tiles."""
    n = -(-M // 256)
    if n > 2048:
        n = -(-n // -(-n // 2048))
    return n * 256


def pmc_traffic(kernel: str, grid_threads: int, expect: float | None = None):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC summary of this same command
    (profiles/*pmc_traffic.json, written by tools/pmc_traffic.py from separate --pmc FETCH_SIZE / WRITE_SIZE passes with
    the guide's gfx950 correction); None when no profile covers that kernel and grid.  Where the summary lists one (kernel,
    grid) at several problem sizes, `expect` (algorithmic bytes) picks the nearest."""
    import glob
    import math

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_traffic.json")))
    if not files:
        return None
    hits = [r["traffic_B"] for r in json.load(open(files[-1]))["kernels"]
            if kernel in r["kernel"] and r["grid"] == grid_threads and r.get("fetch_KiB") is not None]
    if not hits:
        return None
    _source("traffic", files[-1])
    if expect is None or len(hits) == 1:
        return hits[0]
    return min(hits, key=lambda t: abs(math.log(max(t, 1.0) / expect)))


def pmc_issue(kernel: str, grid_threads: int) -> dict:
    """Matrix-pipe busy share and VALU instructions per MFMA of `kernel` from the committed issue-slot accounting
    (profiles/*pmc_issue_*.json, tools/pmc_issue.py: one rocprofv3 --pmc pass of this command).  pipe_busy is clock-independent:
    SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x launch cycles); `frac` (achieved / the 2.4 GHz peak) is pipe_busy x useful / issued flops
    (the clock itself holds 2.40 GHz under sustained f32-MFMA load, profiles/r05_probe_mfma_valu_overlap.txt; see PEAK_NOTE).  {} when no profile covers it."""
    import glob

    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_issue_*.json")), reverse=True):
        for r in json.load(open(f))["kernels"]:
            if kernel in r["kernel"] and r["grid"] == grid_threads:
                _source("mfma_pipe_busy / other_valu_per_mfma", f)
                return {"mfma_pipe_busy": round(r["pipe_busy"], 3), "other_valu_per_mfma": round(r["other_valu_per_mfma"], 2)}
    return {}


def gae_grid_threads(T: int, L: int, ch: int = 4) -> int:
    """Launch shape of tsm_gae_lanes (csrc/gae.hip pick_waves): 64 lanes x W waves per workgroup."""
    blocks = -(-L // 64)
    want, max_by_t, w = -(-2048 // blocks), -(-T // ch), 1
    while w < 16 and w < want and w < max_by_t:
        w <<= 1
    return blocks * 64 * w


def kernel_rooflines(a, algo, buf):
    """Live per-launch device time of the two kernels that dominate the step, on this job's own buffers:
    graph-batched launches bracketed by HIP events on the launch stream (no host gaps inside the bracket)."""
    from tianshou_marl_amd import ops

    dev = buf.device
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def per_launch(fn, n=20, reps=5):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with ops.graph_capture(g):
            for _ in range(n):
                fn()
        g.replay()
        torch.cuda.synchronize()
        tot = 0.0
        for _ in range(reps):
            e0, e1 = ev(), ev()
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1) * 1e-3 / n
        return tot / reps

    T, L, D = a.horizon, a.n_env * a.n_agent, 6 * a.n_agent
    net = algo.net
    # (1) fused PPO gradient step (forward + loss + backward) on one minibatch of the real rollout rows
    n = T * L
    M = min(a.minibatch, n)
    perm = torch.randperm(n, device=dev)[:M].contiguous()
    adv = torch.randn(n, device=dev)
    stats = ops.ppo_adv_stats(adv, torch.tensor([0, M], device=dev), perm=perm)
    nb = ops.ppo_update_grid(M)
    slabs = torch.empty(nb, net.flat.numel(), device=dev)
    partial = torch.empty(nb * 4, dtype=torch.float64, device=dev)
    obs, act = buf.obs_store[:T].reshape(n, D), buf.act_store[:T].reshape(n)
    lp, ret = buf.logp_store[:T].reshape(n), torch.randn(n, device=dev)
    m_, v_ = torch.zeros_like(net.flat.data), torch.zeros_like(net.flat.data)
    p_ = net.flat.data.clone()
    img_ = net.image.clone() if net.image is not None else None

    def grad_step():  # exactly the in-situ kernel sequence of one gradient step (cold image / fresh slabs every time)
        ops.ppo_update_fused(p_, obs, act, lp, adv, ret, algo._cfg, net.n_act, net.hidden, adv_stats=stats[0], perm=perm,
                             M=M, n_blocks=nb, slabs=slabs, partial=partial, want_scalars=False, image=img_)
        ops.adam_step(p_, slabs, m_, v_, 1, lr=0.0, image=img_, image_map=net.image_map)

    step_s = per_launch(grad_step)
    adam_s = per_launch(lambda: ops.adam_step(p_, slabs, m_, v_, 1, lr=0.0, image=img_, image_map=net.image_map))
    upd_s = step_s - adam_s
    # (2) GAE scan over the rows of this job
    # distinct arrays for every operand: aliased inputs would be served from L2 and flatter the HBM fraction
    v, v2, v3 = (torch.randn(T, L, device=dev) for _ in range(3))
    fl, fl2 = (torch.zeros(T, L, dtype=torch.uint8, device=dev) for _ in range(2))
    out = (torch.empty_like(v), torch.empty_like(v))
    gae_s = per_launch(lambda: ops.gae_lanes(v, v2, v3, fl, fl2, out=out))
    # (3) the HBM-bound kernels at the north star's roofline size (n_env=4096, n_agent=8: 32 768 lanes)
    grid = []
    Lg = 4096 * 8

    def gae_entry(Tg, n_sets, label, n, reps):
        """`n` launches per graph over `n_sets` distinct operand sets in rotation: with n_sets x 22 B x Tg x Lg above the
        256 MB Infinity Cache (+ 32 MB of L2) every launch finds its operands in HBM."""
        sets = []
        for _ in range(n_sets):
            sets.append(([torch.randn(Tg, Lg, device=dev) for _ in range(3)],
                         [torch.zeros(Tg, Lg, dtype=torch.uint8, device=dev) for _ in range(2)],
                         (torch.empty(Tg, Lg, device=dev), torch.empty(Tg, Lg, device=dev))))
        k = [0]

        def launch():
            (v_, vn_, r_), (f1, f2), o_ = sets[k[0] % n_sets]
            k[0] += 1
            ops.gae_lanes(v_, vn_, r_, f1, f2, out=o_)

        s_g = per_launch(launch, n=n, reps=reps)
        b = 22 * Tg * Lg
        grid.append({"kernel": "gae_lanes_kernel", "n_env": 4096, "n_agent": 8, "T": Tg, "bound": "hbm", "operands": label,
                     "timing": "back_to_back (graph of %d launches, HIP events)" % n,
                     "in_situ_us_rocprof": in_situ_us("gae_lanes_kernel", "c3ppo", gae_grid_threads(Tg, Lg)) if Tg == 25 else None,
                     "bytes_per_launch": b, "us_per_launch": s_g * 1e6, "achieved": b / s_g / 1e9,
                     "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": b / s_g / HBM_PEAK,
                     "traffic": pmc_traffic("gae_lanes_kernel", gae_grid_threads(Tg, Lg), expect=b)})
        del sets

    # SURVEY 8d roofline grid.  T = 25 (the env's own horizon, 18 MB): once on ONE operand set replayed back to back -- a
    # cache-resident figure, labelled so -- and once cold, rotating 16 sets (288 MB).  T = 2048 (1.48 GB per launch): HBM-bound
    # by size, the figure the 40 % target of the north star is about.  (T = 256 only with --pooled-grid.)
    gae_entry(25, 1, "cache-resident: one 18 MB operand set, back-to-back launches (L2 32 MB / Infinity Cache 256 MB)", 20, 5)
    gae_entry(25, 16, "cold: 16 operand sets in rotation (288 MB > Infinity Cache)", 32, 5)
    gae_entry(2048, 1, "HBM-resident by size: 1.48 GB per launch", 4, 3)
    if getattr(a, "pooled_grid", False):
        gae_entry(256, 2, "2 operand sets of 185 MB in rotation", 8, 3)
    Tg = 25
    Mg, A = Tg * Lg, net.n_act
    lg_ = torch.randn(Mg, A, device=dev)
    vals = [torch.randn(Mg, device=dev) for _ in range(4)]
    actg = torch.randint(0, A, (Mg,), dtype=torch.int32, device=dev)
    stg = ops.ppo_adv_stats(vals[2], torch.tensor([0, Mg], device=dev))
    s_l = per_launch(lambda: ops.ppo_loss_fwd_bwd(lg_, vals[0], actg, vals[1], vals[2], vals[3], algo._cfg,
                                                  adv_stats=stg[0], finalize=False))
    loss_bytes = (8 * A + 24) * Mg  # logits + dlogits, value/act/logp_old/adv/ret read, dvalue written (64 B at A=5)
    grid.append({"kernel": "loss_kernel<5> (PPO clip loss fwd+bwd on given logits/value)", "rows": Mg, "bound": "hbm",
                 "timing": "back_to_back (graph of 20 launches on one 52 MB operand set, HIP events)",
                 "bytes_per_launch": loss_bytes, "us_per_launch": s_l * 1e6, "achieved": loss_bytes / s_l / 1e9,
                 "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": loss_bytes / s_l / HBM_PEAK,
                 "traffic": pmc_traffic("loss_kernel", loss_grid_threads(Mg))})
    del lg_, vals, actg
    # (4) the fused gradient step when the workload hands it more than one 16-row tile per workgroup: pooled minibatch
    # of 65 536 rows (SURVEY 8d grid) out of 819 200 buffer rows of this job's observation width.  Opt-in
    # (--pooled-grid): its launches would otherwise mix into the per-kernel averages of the committed rocprofv3 summary,
    # which has to agree with the live figure of the headline launch.
    if getattr(a, "pooled_grid", False):
        Hn = net.hidden
        (fa_, ba_), (fc_, bc_) = mlp_flops((D, Hn, Hn, net.n_act)), mlp_flops((D, Hn, Hn, 1))
        step_flop_row = fa_ + ba_ + fc_ + bc_  # useful flops of one sample's gradient step, actor + critic
        nG, MG = Tg * Lg, 65536
        obsG = torch.randn(nG, D, device=dev)
        actG = torch.randint(0, net.n_act, (nG,), dtype=torch.int32, device=dev)
        lpG, advG, retG = (torch.randn(nG, device=dev) for _ in range(3))
        permG = torch.randperm(nG, device=dev)[:MG].contiguous()
        stG = ops.ppo_adv_stats(advG, torch.tensor([0, MG], device=dev), perm=permG)
        nbG = ops.ppo_update_grid(MG)
        slabsG = torch.empty(nbG, net.flat.numel(), device=dev)
        partG = torch.empty(nbG * 4, dtype=torch.float64, device=dev)
        s_u = per_launch(lambda: ops.ppo_update_fused(p_, obsG, actG, lpG, advG, retG, algo._cfg, net.n_act, Hn,
                                                      adv_stats=stG[0], perm=permG, M=MG, n_blocks=nbG, slabs=slabsG,
                                                      partial=partG, want_scalars=False, image=img_), n=10)
        grid.append({"kernel": "ppo_update_split_kernel<64> (fused fwd+loss+bwd) at a pooled minibatch", "rows": MG, "bound": "mfma",
                     "timing": "back_to_back (graph of 10 launches, HIP events)",
                     "flop_per_launch": step_flop_row * MG, "us_per_launch": s_u * 1e6,
                     "achieved": step_flop_row * MG / s_u / 1e12, "peak": MFMA_F32_PEAK / 1e12, "unit": "TFLOP/s",
                     "frac": step_flop_row * MG / s_u / MFMA_F32_PEAK, "n_blocks": nbG, "traffic": None})
        del obsG, actG, lpG, advG, retG, permG, slabsG
    H = net.hidden
    (fa, ba), (fc, bc) = mlp_flops((D, H, H, net.n_act)), mlp_flops((D, H, H, 1))
    upd_flop = (fa + ba + fc + bc) * M        # useful flops: forward + backward without layer-1 dX (60 672 per sample at D = 18)
    upd_bytes = (4 * D + 16 + 8) * M                                     # obs + act/logp/adv/ret + perm (88 B)
    gae_bytes = 22 * T * L                                               # 22 B / sample
    return {
        "roofline": {"bound": "mfma", "kernel": "ppo_update_split_kernel<64> (fused fwd+loss+bwd, f32 MFMA; one net per "
                                                "workgroup: grid n_blocks x 2)",
                     "achieved": upd_flop / upd_s / 1e12, "peak": MFMA_F32_PEAK / 1e12, "unit": "TFLOP/s",
                     "frac": upd_flop / upd_s / MFMA_F32_PEAK,
                     "traffic": pmc_traffic("ppo_update_split_kernel", nb * 2 * 256),
                     **pmc_issue("ppo_update_split_kernel", nb * 2 * 256),
                     "peak_note": PEAK_NOTE,
                     "traffic_note": "HBM bytes per launch (PMC): dominated by the per-workgroup gradient slabs "
                                     "(n_blocks x n_param x 4 B written, read back by adam_kernel)",
                     "flop_per_launch": upd_flop, "flop_per_sample": fa + ba + fc + bc,
                     "flop_note": "useful flops (forward + weight gradients + input gradients of layers 2, 3; no layer-1 dX, "
                                  "no padding of the 5 / 1-wide heads to MFMA tiles)",
                     "algorithmic_bytes_per_launch": upd_bytes, "hbm_GBps": upd_bytes / upd_s / 1e9,
                     "hbm_frac": upd_bytes / upd_s / HBM_PEAK,
                     "us_per_launch": upd_s * 1e6, "rows_per_launch": M,
                     "timing": "back_to_back: gap-inclusive (graph of 20 x (update, adam) minus 20 x adam, HIP events)",
                     "in_situ_us_rocprof": in_situ_us("ppo_update_split_kernel", grid=nb * 2 * 256),
                     "how": "graph of 20 x (ppo_update_kernel, adam_kernel) timed with HIP events, minus the same graph "
                            "of adam_kernel alone", "grad_step_us": step_s * 1e6, "adam_us": adam_s * 1e6},
        "roofline_gae": {"bound": "hbm", "kernel": "gae_lanes_kernel", "achieved": gae_bytes / gae_s / 1e9,
                         "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": gae_bytes / gae_s / HBM_PEAK,
                         "traffic": pmc_traffic("gae_lanes_kernel", gae_grid_threads(T, L), expect=gae_bytes),
                         "bytes_per_launch": gae_bytes, "us_per_launch": gae_s * 1e6,
                         "timing": "back_to_back (graph of 20 launches on one operand set: launch latency at this size)",
                         "in_situ_us_rocprof": in_situ_us("gae_lanes_kernel", "bench", gae_grid_threads(T, L))},
        "roofline_grid": grid,
    }


def c3_rooflines(device):
    """roofline_grid entries for the north star's roofline configuration (BASELINE configs[2]: simple_spread N = 8,
    4096 envs, T = 25, shared actor 48-128-128-5 + centralized critic 384-128-128-1, minibatch 65 536 samples of whole
    joint rows): (i) the WHOLE GAE + PPO update as `GenericPPO.update` runs it (one hipGraph replay), priced against the
    f32-MFMA peak with the flops it actually executes; (ii) its dominant kernel, the one-launch actor step."""
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import GenericPPO, policy_within_training_step
    from tianshou_marl_amd.data.batch import split_bounds
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.utils.net import MLPActorCritic

    n_env, N, T, mb, H, A = 4096, 8, 25, 65536, 128, 5
    env = DeviceSimpleSpreadVectorEnv(n_env, N, max_cycles=T, device=device, seed=1626)
    D = env.obs_dim
    net = MLPActorCritic(D, A, (H, H), critic_obs_dim=N * D, device=device, seed=1626)
    algo = GenericPPO(net=net, critic_input="global", n_agent=N, lr=3e-4, shuffle="device", seed=1626, dispatch="pooled")
    buf = DeviceVectorReplayBuffer(n_env * T, n_env, N, D, device=device)
    col = Collector(algo, env, buf, async_stats=True)
    col.reset()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    cols, upds = [], []
    reps, warm = 7, 4  # (the 2nd update captures the graph; the median keeps one-off runtime hiccups out of the figure)
    for i in range(warm + reps):
        e0, e1, e2 = ev(), ev(), ev()
        with policy_within_training_step(algo):
            e0.record()
            cs = col.collect(n_step=n_env * T)
            e1.record()
            ts = algo.update(buf, mb, 1)
            e2.record()
        torch.cuda.synchronize()
        _resolve(cs)
        col.reset_buffer(keep_statistics=True)
        if i >= warm:
            cols.append(e0.elapsed_time(e1))
            upds.append(e1.elapsed_time(e2))
    t_col, t_upd = sorted(cols)[reps // 2], sorted(upds)[reps // 2]
    rows, samples = n_env * T, n_env * T * N
    (f_actor, b_actor), (f_critic, b_critic) = mlp_flops((D, H, H, A)), mlp_flops((N * D, H, H, 1))
    # USEFUL flops as executed: V(obs) for every joint row and V(obs_next) for the last slot's rows (the other slots take it
    # from the next slot's V(obs): GenericPPO._next_values_chained; logp_old comes from the rollout) + one gradient step of
    # every sample through the actor and of every joint row through the critic (forward + weight gradients + input gradients
    # of layers 2 and 3 -- no kernel forms dX of layer 1; actor 126 720 per sample, critic 295 680 per joint row)
    flop = (rows + n_env) * f_critic + samples * (f_actor + b_actor) + rows * (f_critic + b_critic)
    # issued on the matrix pipe beyond that: the A = 5 logits / their two backward products run as 16-wide MFMA tiles
    issued_extra = samples * 6 * H * (16 - A)
    steps = len(split_bounds(rows, mb // N, True))
    out = [{"kernel": "C3 whole GAE + PPO update (GenericPPO.update: V(obs_next), GAE, advantage statistics, %d gradient "
                      "steps of actor-rows kernel + critic-rows kernel + 2 Adam; one hipGraph replay)" % steps,
            "n_env": n_env, "n_agent": N, "T": T, "minibatch": mb, "bound": "mfma", "ms_per_update": t_upd,
            "flop_per_update": flop, "issued_mfma_flop": flop + issued_extra,
            "flop_note": "useful flops (mlp_flops: forward + backward without layer-1 dX, no padding); issued_mfma_flop adds "
                         "the actor head's 5 -> 16 padding",
            "achieved": flop / (t_upd * 1e-3) / 1e12, "peak": MFMA_F32_PEAK / 1e12,
            "unit": "TFLOP/s", "frac": flop / (t_upd * 1e-3) / MFMA_F32_PEAK,
            "hbm_frac": (22 + 4 * D + 24) * samples / (t_upd * 1e-3) / HBM_PEAK, "collect_ms": t_col,
            "ms_per_update_all": [round(x, 3) for x in upds], "ms_per_update_min": min(upds), "ms_per_update_max": max(upds),
            "timing": "median of %d updates after %d warm-up iterations (0: eager, 1: capture + first replay); min / max / all "
                      "listed -- tools/c3_step_times.py has the per-step timeline of 80 steps" % (reps, warm),
            "env_steps_per_s": samples / ((t_col + t_upd) * 1e-3), "gradient_steps": ts.gradient_steps,
            "note": "the critic runs once per joint row (the reference evaluates it once per sample: 8x the flops on identical "
                    "inputs); hbm_frac: SURVEY 8d's algorithmic bytes (GAE 22 B + fused step 4 D + 24 B per sample) against the "
                    "HBM peak -- the update is compute-bound, the MFMA roof is the one that binds"}]
    # (ii) the actor step alone, graph-batched launches on the job's own rows
    n = samples
    obs, act = buf.obs_store[:T].reshape(n, D), buf.act_store[:T].reshape(n)
    lp, adv = buf.logp_store[:T].reshape(n), torch.randn(n, device=device)
    perm = torch.randperm(n, device=device)[:mb].contiguous()
    st = ops.ppo_adv_stats(adv, torch.tensor([0, mb], device=device), perm=perm, max_rows=mb)
    nb = ops.ppo_actor_rows_grid(mb)
    slabs = torch.empty(nb, net.n_actor, device=device)
    part = torch.empty(nb * 4, dtype=torch.float64, device=device)
    fn = lambda: ops.ppo_actor_rows_update(net.actor.flat.data, obs, act, lp, adv, algo._cfg, A, H, adv_stats=st[0],  # noqa: E731
                                           perm=perm, M=mb, n_blocks=nb, slabs=slabs, partial=part)
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        for _ in range(10):
            fn()
    g.replay()
    torch.cuda.synchronize()
    tot = 0.0
    for _ in range(5):
        e0, e1 = ev(), ev()
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        tot += e0.elapsed_time(e1) * 1e-3 / 10 / 5
    a_flop, a_bytes = (f_actor + b_actor) * mb, (4 * D + 4 + 4 + 4 + 8) * mb
    t64 = -(-mb // 64) >= ops.device_info()["n_cu"]  # (tsm_ppo_actor_rows_grid's rule: 64-sample tiles once every CU gets one)
    a_kernel = "actor_rows64_kernel" if t64 else "ppo_actor_rows_kernel"
    out.append({"kernel": a_kernel + "<3> (actor 48-128-128-5: forward + policy loss + backward in one launch; "
                          + ("64-sample tiles, layer-2 weights in registers)" if t64 else "32-sample tiles)"),
                "rows": mb, "bound": "mfma", "flop_per_launch": a_flop, "issued_mfma_flop": a_flop + 6 * H * (16 - A) * mb,
                "timing": "back_to_back (graph of 10 launches, HIP events)",
                "in_situ_us_rocprof": in_situ_us(a_kernel, "c3ppo"), "us_per_launch": tot * 1e6,
                "achieved": a_flop / tot / 1e12, "peak": MFMA_F32_PEAK / 1e12, "unit": "TFLOP/s",
                "frac": a_flop / tot / MFMA_F32_PEAK, "n_blocks": nb, "algorithmic_bytes_per_launch": a_bytes,
                "slab_bytes_per_launch": nb * net.n_actor * 4, "traffic": pmc_traffic(a_kernel, nb * 512),
                **pmc_issue(a_kernel, nb * 512)})
    # (iii) the critic step alone: the same minibatch as whole joint rows (mb / N rows of N * D floats); two launches
    # (csrc/critic_train.hip: forward + value loss + backward to dH1; csrc/critic_dw1.hip: dW1 as a split-K pass)
    mr = mb // N
    joint, ret = buf.obs_store[:T].reshape(rows, N * D), torch.randn(n, device=device)
    rid = torch.randperm(rows, device=device)[:mr].contiguous()
    cws: dict = {}
    fc = lambda: ops.critic_rows_grad_ppo(net.critic.flat.data, joint, ret, algo._cfg, N, H, rows=rid, Mr=mr, ws=cws)  # noqa: E731

    def graph_time(fn_, n_rep=10):
        fn_()
        torch.cuda.synchronize()
        g_ = torch.cuda.CUDAGraph()
        with ops.graph_capture(g_):
            for _ in range(n_rep):
                fn_()
        g_.replay()
        torch.cuda.synchronize()
        tot_ = 0.0
        for _ in range(5):
            e0, e1 = ev(), ev()
            e0.record()
            g_.replay()
            e1.record()
            torch.cuda.synchronize()
            tot_ += e0.elapsed_time(e1) * 1e-3 / n_rep / 5
        return tot_

    tot_gather = graph_time(fc)  # (first step of an update: W1 gathered from the flat vector)
    wc = next(iter(cws.values()))
    c_flop, c_bytes = (f_critic + b_critic) * mr, (4 * N * D + 8 + 4 * N) * mr
    # (as GenericPPO runs every step but the first of an update: first-layer weights from the fragment image the optimizer keeps)
    w1_img = ops.critic_w1_image(net.critic.flat.data, N * D)
    tot = graph_time(lambda: ops.critic_rows_grad_ppo(net.critic.flat.data, joint, ret, algo._cfg, N, H, rows=rid, Mr=mr, ws=cws,
                                                     w1_image=w1_img))
    out.append({"kernel": "critic_rows_train_kernel<24> + critic_dw1_kernel (centralized critic 384-128-128-1 on joint rows: "
                          "forward + value loss of the row's 8 agents + backward, dW1 as a split-K pass; two launches)",
                "us_per_launch_w1_gathered": tot_gather * 1e6,
                "in_situ_note": "in the update the dW1 launch also carries the side reductions (actor + small critic slabs -> one row "
                                "each) that the optimizer launch shed: dW1 14 -> 20 us, adam_segs 14 -> 5 us per step",
                "rows": mr, "samples": mb, "bound": "mfma", "flop_per_launch": c_flop,
                "timing": "back_to_back (graph of 10 launch pairs, HIP events)",
                "in_situ_us_rocprof": (lambda a_, b_: None if a_ is None or b_ is None else round(a_ + b_, 3))(
                    in_situ_us("critic_rows_train_kernel", "c3ppo"), in_situ_us("critic_dw1_kernel", "c3ppo")),
                "us_per_launch": tot * 1e6,
                "achieved": c_flop / tot / 1e12, "peak": MFMA_F32_PEAK / 1e12, "unit": "TFLOP/s",
                "frac": c_flop / tot / MFMA_F32_PEAK, "n_blocks": wc["nb"], "dw1_chunks": wc["nc"],
                "algorithmic_bytes_per_launch": c_bytes,
                "slab_bytes_per_launch": (wc["rest"].numel() + wc["w1"].numel() + wc["dh1"].numel()) * 4,
                "traffic": (lambda a_, b_: None if a_ is None or b_ is None else a_ + b_)(
                    pmc_traffic("critic_rows_train_kernel", wc["nb"] * 512),
                    pmc_traffic("critic_dw1_kernel", -(-N * D // 48) * (-(-wc["nc"] // 8) * 8) * 512)),  # (48-column blocks at this size)
                **pmc_issue("critic_rows_train_kernel", wc["nb"] * 512)})
    # (iv) V(row) of the same critic for every joint row of the buffer (the preprocessing's critic pass), one launch
    vout = torch.empty(rows, device=device)
    tot = graph_time(lambda: ops.critic_rows_forward(net.critic.flat.data, joint, H, out=vout), n_rep=5)
    v_flop = f_critic * rows
    out.append({"kernel": "critic_rows_forward_kernel<24> (V(row) for all %d joint rows: layer-1 weights in registers, layer 3 "
                          "folded into layer 2)" % rows, "rows": rows, "bound": "mfma", "flop_per_launch": v_flop,
                "timing": "back_to_back (graph of 5 launches, HIP events)",
                "in_situ_us_rocprof": in_situ_us("critic_rows_forward_kernel", "c3ppo", near_us=tot * 1e6),
                "us_per_launch": tot * 1e6, "achieved": v_flop / tot / 1e12, "peak": MFMA_F32_PEAK / 1e12, "unit": "TFLOP/s",
                "frac": v_flop / tot / MFMA_F32_PEAK, "algorithmic_bytes_per_launch": (4 * N * D + 4) * rows,
                "traffic": pmc_traffic("critic_rows_forward_kernel", min(256, -(-rows // 32)) * 512, expect=(4 * N * D + 4) * rows),
                **pmc_issue("critic_rows_forward_kernel", min(256, -(-rows // 32)) * 512)})
    return out


def cpu_baseline(a):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cpu_path  # test/benchmark infrastructure: the CPU port of the same step

    # the GPU job's own per-GPU size (n_env = 1024 by default): a handful of ~4 s steps inside the 20 s budget, then the
    # separate legs SURVEY 8(d) lists: the scan alone (serial / all cores) and the reference-default batch-64 update
    out = cpu_path.run_baseline(n_env=a.cpu_envs or a.n_env, n_agent=a.n_agent, horizon=a.horizon, minibatch=a.minibatch,
                                repeat=a.repeat, dispatch=a.dispatch, budget_s=20.0, ref_default_leg=True)
    out.update(cpu_path.gae_legs(shapes=((a.horizon, a.n_env * a.n_agent), (25, 4096 * 8)), budget_s=4.0))
    return out


def run_c3(a, device):
    """BASELINE configs[2] (not the headline line; `--workload c3`): simple_spread N=8 (obs 48), shared decentralized
    actor 48-128-128-5 and centralized critic 384-128-128-8 (CTDEPolicy), num_envs=4096 on one GPU.  A step = collect
    T=25 vector steps (actor GEMMs + categorical sampling + env step + buffer add, one hipGraph) + CTDEPolicy.learn on
    every agent's batch with the concatenated global state (8 TD/policy-gradient steps over 102 400 rows each)."""
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.multiagent import (CentralizedCritic, CTDEPolicy, DecentralizedActor,
                                                        FlexibleMultiAgentPolicyManager, SimultaneousTrainer,
                                                        agent_batches_from_buffer)
    from tianshou_marl_amd.algorithm.ppo import policy_within_training_step
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv

    n_env, N, T, H = 4096, 8, 25, 128
    env = DeviceSimpleSpreadVectorEnv(n_env, N, max_cycles=T, device=device, seed=1626)
    D = env.obs_dim
    # (async_stats: the losses of a learn() are read when the caller looks at them, one step late below)
    pol = CTDEPolicy(actor=DecentralizedActor(D, 5, H, device=device, seed=1),
                     critic=CentralizedCritic(N * D, N, H, device=device, seed=2), seed=1626, async_stats=True)
    mgr = FlexibleMultiAgentPolicyManager(pol, env, mode="shared")
    buf = DeviceVectorReplayBuffer(n_env * T, n_env, N, D, device=device)
    col = Collector(mgr, env, buf, async_stats=True)
    col.reset()
    trainer = SimultaneousTrainer(mgr)

    def step():
        with policy_within_training_step(mgr):
            cs = col.collect(n_step=n_env * T)
            # copies=False: the learners read the time-major stores in place (no env-major copies of the 157 MB joint rows)
            losses = trainer.train_step(agent_batches_from_buffer(buf, env.agents, copies=False))
        _resolve(cs)  # read every step's statistics (see one_step)
        col.reset_buffer(keep_statistics=True)
        return cs, losses

    prev = None
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        cs, losses = step()
        if prev is not None:  # every learner's losses are read, one step late (as a logger would)
            for v in prev.values():
                float(v["critic_loss"])
        prev = losses
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, {**buffer_outputs(buf), "actor_params": pol.actor.flat.data,
                                      "critic_params": pol.critic.flat.data, **episode_outputs(cs), **scalar_outputs("train", losses)})
    R = n_env * T
    out = {
        "metric": "env-steps/sec (n_env x n_agent) incl. CTDE update, simple_spread N=8", "value": n_env * N * T / dt,
        "unit": "env-steps/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "simple_spread_v3 N=8 CTDEPolicy (shared actor 48-128-128-5, centralized critic 384-128-128-8), "
                               "num_envs=4096, T=25", "learn_calls_per_step": N, "rows_per_learn": R,
                               "learn": "fused: rows read in place, critic forward / TD step / dW1 / actor step / two Adam steps"},
        "losses_agent_0": {k: float(v) for k, v in losses["agent_0"].items()},
    }
    if a.full:
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        e0, e1, e2 = ev(), ev(), ev()
        with policy_within_training_step(mgr):
            e0.record()
            col.collect(n_step=n_env * T)
            e1.record()
            trainer.train_step(agent_batches_from_buffer(buf, env.agents, copies=False))
            e2.record()
        torch.cuda.synchronize()
        col.reset_buffer(keep_statistics=True)
        # roofline of one learn() call AS EXECUTED (one hipGraph replay: V(last slot), TD step of the critic with its split-K dW1
        # pass, actor step, finalize, two Adam launches), priced against the f32-MFMA peak: flops per row of the agent batch =
        # critic forward + backward down to dH1 (2 (K1 H + H H + H n) + 4 H H + 4 n H) + dW1 (2 K1 H) + the actor's gradient step
        # (useful flops, mlp_flops: no layer-1 dX)
        K1, A_ = N * D, 5
        flop_row = sum(mlp_flops((K1, H, H, N))) + sum(mlp_flops((D, H, H, A_)))
        learn_flop = R * flop_row + n_env * 2 * (K1 * H + H * H + H * N)
        learn_s = e1.elapsed_time(e2) * 1e-3 / N
        out.update({
            "collect_ms": e0.elapsed_time(e1), "ctde_update_ms": e1.elapsed_time(e2),
            "roofline": {"bound": "mfma", "kernel": "CTDEPolicy.learn as executed (critic_rows_forward + critic_rows_train_kernel<24, true, 1> + "
                                   "critic_dw1_kernel + actor_rows64_kernel<3> + ctde_finalize + 2 x adam_segs; one hipGraph replay)",
                         "achieved": learn_flop / learn_s / 1e12, "peak": MFMA_F32_PEAK / 1e12, "unit": "TFLOP/s",
                         "frac": learn_flop / learn_s / MFMA_F32_PEAK, "traffic": None, "us_per_learn": learn_s * 1e6,
                         "flop_per_learn": learn_flop, "rows_per_learn": R}})
    _ = ops
    _emit(out)


def run_c3ppo(a, device):
    """`--workload c3ppo`: the north star's roofline configuration with PPO -- simple_spread N=8 (obs 48), 4096 envs,
    T=25, shared actor 48-128-128-5 and a CENTRALIZED critic 384-128-128-1 on the concatenated global state
    (GenericPPO on the dense kernels), per-agent dispatch, minibatch 65536 (SURVEY grid), repeat 1.  Reports env-steps/s
    and the split collect / GAE+PPO update."""
    from tianshou_marl_amd.algorithm import GenericPPO, policy_within_training_step
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.utils.net import MLPActorCritic

    n_env, N, T, mb = 4096, 8, 25, 65536
    env = DeviceSimpleSpreadVectorEnv(n_env, N, max_cycles=T, device=device, seed=1626)
    D = env.obs_dim
    net = MLPActorCritic(D, 5, (128, 128), critic_obs_dim=N * D, device=device, seed=1626)
    algo = GenericPPO(net=net, critic_input="global", n_agent=N, lr=3e-4, shuffle="device", seed=1626, dispatch=a.c3_dispatch,
                      async_stats=True)
    buf = DeviceVectorReplayBuffer(n_env * T, n_env, N, D, device=device, ignore_obs_next=a.ignore_obs_next)
    col = Collector(algo, env, buf, async_stats=True)
    col.reset()
    prev = [None]

    def step():
        with policy_within_training_step(algo):
            cs = col.collect(n_step=n_env * T)
            ts = algo.update(buf, mb, 1)
        # every step's statistics are read, as in one_step: the collect statistics while the update runs on the device (the
        # wait is for the rollout only), the training statistics one step late -- the device never idles behind the host
        _resolve(cs)
        _resolve(prev[0])
        prev[0] = ts
        col.reset_buffer(keep_statistics=True)
        return cs, ts

    for _ in range(max(a.warmup, 2)):  # the 2nd update captures the graph
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        cs, ts = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    d = ts.get_loss_stats_dict()
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, {**buffer_outputs(buf), "params": net.flat.data, **episode_outputs(cs),
                                      **scalar_outputs("train", d)})
    out = {
        "metric": "env-steps/sec (n_env x n_agent) incl. PPO update, simple_spread N=8, centralized critic",
        "value": n_env * N * T / dt, "unit": "env-steps/s", "n_gpus": 1, "steps": a.steps, "warmup": max(a.warmup, 2),
        "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "simple_spread_v3 N=8 PPO, shared actor 48-128-128-5 + centralized critic 384-128-128-1, "
                               "num_envs=4096, T=25", "minibatch": mb, "repeat": 1, "dispatch": a.c3_dispatch,
                   **({"buffer": "ignore_obs_next=True"} if a.ignore_obs_next else {})},
        "gradient_steps_per_update": sum(int(v) for k, v in d.items() if k.endswith("gradient_steps")),
        "loss": d.get("agent_0/loss", d.get("loss"))}
    if a.full:
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        e0, e1, e2 = ev(), ev(), ev()
        with policy_within_training_step(algo):
            e0.record()
            col.collect(n_step=n_env * T)
            e1.record()
            algo.update(buf, mb, 1)
            e2.record()
        torch.cuda.synchronize()
        col.reset_buffer(keep_statistics=True)
        out.update({
            "collect_ms": e0.elapsed_time(e1), "gae_ppo_update_ms": e1.elapsed_time(e2),
            # the whole GAE + PPO update as executed (one hipGraph replay), priced against the f32-MFMA peak: V(obs) of every joint
            # row + V(obs_next) of the last slot, then one gradient step (useful flops: mlp_flops) of every sample through the actor
            # and of every joint row through the critic (the default bench line's roofline_grid has the same count, medians and
            # the kernels' own entries)
            "roofline": (lambda fl, s_: {"bound": "mfma", "kernel": "C3 whole GAE + PPO update (GenericPPO.update, one hipGraph replay)",
                                         "achieved": fl / s_ / 1e12, "peak": MFMA_F32_PEAK / 1e12, "unit": "TFLOP/s",
                                         "frac": fl / s_ / MFMA_F32_PEAK, "traffic": None, "flop_per_update": fl,
                                         "peak_note": PEAK_NOTE})(
                (n_env * T + n_env) * mlp_flops((N * D, 128, 128, 1))[0]
                + n_env * T * N * sum(mlp_flops((D, 128, 128, 5))) + n_env * T * sum(mlp_flops((N * D, 128, 128, 1))),
                e1.elapsed_time(e2) * 1e-3)})
    _emit(out)


def run_tag(a, device, rank, world, dist, census=None):
    """`--workload tag` (BASELINE configs[4]): simple_tag (3 adversaries v 1 prey, 2 obstacles), grouped policies (one PPO
    per team), league trainer -- per GPU `--tag-envs` worlds (512: 4096 over 8 GPUs), T = 25.  A step = collect + one
    `LeaguePlayTrainer.train_step` in which both teams learn; with N > 1 the two teams' gradients travel in ONE packed
    all-reduce per gradient step (parallel.learn_lockstep).  Weak scaling; value = env-steps/s over all ranks."""
    from tianshou_marl_amd.algorithm.multiagent import FlexibleMultiAgentPolicyManager, LeaguePlayTrainer, agent_batches_from_buffer
    from tianshou_marl_amd.algorithm.ppo import PPO, policy_within_training_step
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe_tag import DeviceSimpleTagVectorEnv
    from tianshou_marl_amd.utils.net import DiscreteActorCritic

    n_env, T = a.tag_envs, a.horizon
    env = DeviceSimpleTagVectorEnv(n_env, device=device, seed=1626 + rank, max_cycles=T)
    N = env.n_agent
    mk = lambda s: PPO(net=DiscreteActorCritic(env.obs_dim, 5, 64, device=device, seed=s), seed=s + rank, lr=3e-4,  # noqa: E731
                       shuffle="device", async_stats=True)  # learn(): one hipGraph replay per call, statistics resolve when read
    #                                                          (data parallel: the groups' lock-step replays from captured graphs,
    #                                                          parallel.learn_lockstep_graph)
    teams = {"adversaries": mk(1626), "good": mk(1627)}
    mgr = FlexibleMultiAgentPolicyManager(teams, env, mode="grouped", agent_groups=env.agent_groups)
    if dist is not None:
        from tianshou_marl_amd.parallel import attach_data_parallel

        attach_data_parallel(mgr, dist)
    buf = DeviceVectorReplayBuffer(n_env * T, n_env, N, env.obs_dim, device=device)
    col = Collector(mgr, env, buf, async_stats=True)  # statistics resolve lazily, as in the headline job
    col.reset()
    trainer = LeaguePlayTrainer(mgr, matchmaking="random")
    np.random.seed(1626)  # matchmaking draws must agree on every rank

    marks = []

    def step():
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        with policy_within_training_step(mgr):
            e[0].record()
            cs = col.collect(n_step=n_env * T)
            e[1].record()
            # one learner per team; copies=False: PPO.learn gathers its column straight from the stores into its graph buffers
            batch = agent_batches_from_buffer(buf, env.agents, only=["agent_0", "adversary_0"], global_state=False, copies=False)
            # (no joint rows: grouped PPO has no centralized critic -- the reference's job builds per-agent batches only)
            batch["good"], batch["adversaries"] = batch["agent_0"], batch["adversary_0"]
            losses = trainer.train_step(batch)
            e[2].record()
        # Both statistics objects of a step are lazy and are read ONE STEP LATE (the timed loop below): here the GPU work behind the
        # rollout is short (~0.16 ms of learn() graphs), so a host that waited for THIS rollout's statistics before it prepared
        # the next collect left the GPU idle ~60 us per step (gpurun_out/r05: collect_ms 0.32 for a 0.265 ms kernel).  The host
        # still never runs more than one step ahead: it blocks on step k - 1's events while step k executes.
        col.reset_buffer(keep_statistics=True)
        marks.append(e)
        return cs, losses

    for _ in range(a.warmup):
        _resolve(step()[0])
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prev = None
    for _ in range(a.steps):
        cs, losses = step()
        if prev is not None:  # every step's collect AND training statistics are read, one step late (as a logger would)
            _resolve(prev[0])
            for v in prev[1].values():
                float(v["loss"])
        prev = (cs, losses)
    _resolve(prev[0])
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, {**buffer_outputs(buf), **{"params_" + k: p.net.flat.data for k, p in sorted(teams.items())},
                                      **episode_outputs(prev[0]), **scalar_outputs("train", losses)})
    replicas_identical = None
    if dist is not None and a.full:
        diff = torch.zeros(1, device=device)
        for p in teams.values():
            ref = p.net.flat.data.clone()
            dist.broadcast(ref, src=0)
            diff += 0.0 if torch.equal(ref, p.net.flat.data) else 1.0
        dist.all_reduce(diff, op=dist.ReduceOp.MAX)
        replicas_identical = bool(diff.item() == 0.0)
    if rank == 0:
        out = {"metric": "env-steps/sec (n_env x n_agent) incl. league PPO update, simple_tag 3v1",
               "value": n_env * N * T * world / (dt / a.steps), "unit": "env-steps/s", "n_gpus": world, **(census or {}),
               "steps": a.steps,
               "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": "simple_tag_v3 3 adversaries + 1 prey, 2 obstacles, grouped PPO (one policy per team), "
                                      "LeaguePlayTrainer, num_envs=%d per GPU, T=%d" % (n_env, T),
                          "parallelism": "env-shard x%d, one packed gradient all-reduce per step for both teams" % world,
                          **_allreduce_path(getattr(mgr, "_grad_sync", None))},
               "collect_ms": float(np.median([e[0].elapsed_time(e[1]) for e in marks[-a.steps:]])),
               "league_train_step_ms": float(np.median([e[1].elapsed_time(e[2]) for e in marks[-a.steps:]])),
               "losses": {k: float(v["loss"]) for k, v in losses.items()}}
        if replicas_identical is not None:
            out["replicas_identical"] = replicas_identical
        _emit(out)


_OUT: list = []


_ARGS = None


def _emit(line) -> None:
    """The bench's JSON line: held back until fd 1 is the real stdout again (see main).  A dict gets the proof of its own
    configuration first (`config.kernel_options`; a non-default selection is refused or labelled, see guard_configuration) and
    the list of committed profile files its looked-up fields came from."""
    if isinstance(line, dict):
        guard_configuration(_ARGS, line)
        if _SOURCES:
            line["profile_sources"] = dict(_SOURCES, note="these fields are looked up in committed summaries of EARLIER runs of this "
                                           "command under rocprofv3 (tools/r0N_profiles.sh); this run did not measure them")
        line = json.dumps(line)
    _OUT.append(line)


def main():
    # Libraries write to fd 1 behind Python's back (RCCL prints a version banner when a communicator comes up, gloo its
    # connection notes): send fd 1 to stderr for the duration of the run so that stdout carries the ONE JSON line only.
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        _main()
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)
    for line in _OUT:
        print(line, flush=True)


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher around it: start N fresh interpreters, one rank per GPU, with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set (what `torch.distributed.run` would export), relay rank 0's ONE JSON line
    and fail if any rank fails.  This process never touches the GPU (no HIP call happens before this point), and no
    process that has touched one is ever replaced or restarted."""
    import socket
    import subprocess

    with socket.socket() as s:  # a free rendezvous port (the capture probe uses port + 1)
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr.fileno(), stderr=None))
    out0, failed = b"", None
    alive = set(range(n))
    while alive and failed is None:
        for r in sorted(alive):
            try:
                if r == 0:
                    out0 += procs[0].communicate(timeout=0.5)[0] or b""
                else:
                    procs[r].wait(timeout=0.05)
            except subprocess.TimeoutExpired:
                continue
            alive.discard(r)
            if procs[r].returncode != 0:
                failed = r
                break
    if failed is not None:  # stop exactly the ranks this process started
        for r in alive:
            procs[r].terminate()
        for r in alive:
            try:
                procs[r].wait(timeout=20)
            except subprocess.TimeoutExpired:
                procs[r].kill()
        print("bench: rank %d exited with code %s; stopped the other ranks" % (failed, procs[failed].returncode), file=sys.stderr)
        return int(procs[failed].returncode or 1)
    lines = [ln for ln in out0.decode(errors="replace").splitlines() if ln.startswith("{")]
    if not lines:
        print("bench: rank 0 printed no JSON line", file=sys.stderr)
        return 1
    _emit(lines[-1])
    return 0


def _main():
    global _ARGS
    a = _ARGS = parse()
    guard_configuration(a)  # (environment only: before any rank is started and before anything touches the GPU)
    # ---- who runs: nothing below this block may run before it, and nothing in it calls into HIP -----------------------
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        if a.workload in ("c3", "c3ppo"):
            raise SystemExit("bench.py --workload %s is a single-GPU job (BASELINE configs[2]): use --gpus 1" % a.workload)
        code = launch_ranks(a.gpus)
        if code:
            raise SystemExit(code)
        return
    from tianshou_marl_amd.utils.host import limit_host_threads

    limit_host_threads()  # torch's pool sized for the machine, not for the CPU quota, gets the launch thread frozen (utils/host.py)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus != world:
        raise SystemExit("bench.py --gpus %d, but the launcher started WORLD_SIZE=%d ranks: pass --gpus %d" % (a.gpus, world, world))
    if a.workload == "c3ppo":
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
        torch.cuda.set_device(0)
        run_c3ppo(a, torch.device("cuda", 0))
        return
    if a.workload == "c3":
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
        torch.cuda.set_device(0)
        run_c3(a, torch.device("cuda", 0))
        return
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.device_count() == 0:  # (counting devices does not initialise the GPU)
        raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
    # Rehearsal switches for a single-GPU box (never used by the real multi-GPU run):
    #   TSM_FORCE_DIST=1            process group + replica broadcast + captured all-reduce with a world of ONE rank (RCCL)
    #   TSM_SHARE_GPU=1             every rank uses cuda:0 (RCCL refuses two ranks on one device, so combine it with ...)
    #   TSM_DIST_BACKEND=gloo       ... the gloo backend: exercises the multi-process logic (env shards, per-step gradient
    #                               sync, max-over-ranks timing) end to end; its all-reduce cannot be graph-captured, so the
    #                               update falls back to eager launches on every rank alike
    if os.environ.get("TSM_SHARE_GPU") == "1":
        local = 0
    # N > 1 over RCCL: ask a child process whether this box can capture collectives into a hipGraph BEFORE this process
    # touches the GPU (a failed capture cannot be recovered from in-process); if any rank's probe fails, every rank runs
    # eager collectives (slower, but a measured run instead of an aborted one)
    capture_ok = None
    if (world > 1 or os.environ.get("TSM_FORCE_DIST") == "1") and os.environ.get("TSM_DIST_BACKEND", "nccl") == "nccl" \
            and "TSM_GRAPH_COLLECTIVES" not in os.environ:
        from tianshou_marl_amd.parallel import probe_collective_capture

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        capture_ok = probe_collective_capture(rank, world, local)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    dist = None
    ranks_seen, backend = 1, None
    force_dist = os.environ.get("TSM_FORCE_DIST") == "1"
    if world > 1 or force_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        backend = os.environ.get("TSM_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device, rank=rank, world_size=world)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        # who showed up: a sum of ones over the process group -- `n_gpus` of the JSON line is THIS number, not an env var
        ones = torch.ones(1, device=device, dtype=torch.int32)
        dist.all_reduce(ones)
        ranks_seen = int(ones.item())
        if ranks_seen != world:
            raise SystemExit("bench.py: the %s process group counts %d ranks, WORLD_SIZE says %d" % (backend, ranks_seen, world))
        if capture_ok is not None:  # every rank must take the same path
            t = torch.tensor([1 if capture_ok else 0], device=device, dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            capture_ok = bool(t.item())
            if not capture_ok:
                os.environ["TSM_GRAPH_COLLECTIVES"] = "0"
                if rank == 0:
                    print("bench: the collective-capture probe failed on some rank: running eager collectives", file=sys.stderr)
    # `n_gpus` = the ranks the process group itself counted; `ranks_backend` says who counted (nccl == RCCL)
    census = {} if dist is None else {"rccl_ranks" if backend == "nccl" else "group_ranks": ranks_seen, "ranks_backend": backend}
    if dist is not None and os.environ.get("TSM_SHARE_GPU") == "1":
        census["rehearsal"] = "%d ranks share cuda:0 (TSM_SHARE_GPU=1): multi-process logic only, not a scaling figure" % ranks_seen
    if a.workload == "tag":
        run_tag(a, device, rank, ranks_seen, dist, census)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    env, net, algo, buf, col = build_job(a, device, rank)
    if dist is not None:
        from tianshou_marl_amd.parallel import attach_data_parallel

        attach_data_parallel(algo, dist)
    for _ in range(a.warmup):
        one_step(a, algo, buf, col)
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        cs, ts = one_step(a, algo, buf, col)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    ms_per_step = dt / a.steps * 1e3
    agent_steps = a.n_env * a.n_agent * a.horizon * ranks_seen
    value = agent_steps / (dt / a.steps)
    grad_steps = getattr(ts, "gradient_steps", None) or sum(
        s.gradient_steps for s in getattr(ts, "_agent_id_to_stats", {}).values())
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, {**buffer_outputs(buf), "params": net.flat.data, **episode_outputs(cs),
                                      **scalar_outputs("train", ts)})
    if a.full:  # every rank runs the phase split: update() contains the gradient all-reduce when N > 1
        t_col_ms, t_upd_ms = phase_times(a, algo, buf, col)
    replicas_identical = None
    if dist is not None and a.full:  # data-parallel invariant: after any number of synced steps every rank holds the same bits
        mine = net.flat.data.clone()
        ref = mine.clone()
        dist.broadcast(ref, src=0)
        diff = torch.tensor([0.0 if torch.equal(mine, ref) else 1.0], device=device)
        dist.all_reduce(diff, op=dist.ReduceOp.MAX)
        replicas_identical = bool(diff.item() == 0.0)
    if rank == 0:
        out = {
            "metric": "env-steps/sec (n_env x n_agent) incl. PPO update, simple_spread N=%d" % a.n_agent,
            "value": value, "unit": "env-steps/s", "n_gpus": ranks_seen, **census, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "simple_spread_v3 N=%d shared PPO, num_envs=%d per GPU, obs %d, A=5, T=%d, MLP 64-64"
                       % (a.n_agent, a.n_env, 6 * a.n_agent, a.horizon),
                       "minibatch": a.minibatch, "repeat": a.repeat, "dispatch": a.dispatch, "parallelism": "env-shard x%d" % world,
                       **({} if dist is None else {"collectives": "captured in the update hipGraph" if getattr(algo, "graph_collectives", False)
                                                   else "eager, between segmented hipGraphs"}),
                       **_allreduce_path(getattr(algo, "_grad_sync", None))},
            "gradient_steps_per_update": grad_steps,
        }
        if a.full:
            out.update({"collect_ms": t_col_ms, "ppo_update_ms": t_upd_ms,
                        "collect_env_steps_per_s": a.n_env * a.n_agent * a.horizon / (t_col_ms * 1e-3)})
            if replicas_identical is not None:
                out["replicas_identical"] = replicas_identical
            if world == 1 and not a.no_batch64:
                out["update_reference_default_batch64"] = batch64_update(a, algo, buf, col)
            out.update(kernel_rooflines(a, algo, buf))
            if world == 1 and not a.no_c3_grid:
                del algo, buf, col, env  # (free the headline job's graphs before the 4096-env job is built)
                out["roofline_grid"] += c3_rooflines(device)
            if not a.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline(a)
        _emit(out)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
