"""Inputs and float64 yardsticks of the shape sweeps over the off-policy heads, the sum tree and the n-step walk: the case
lists, one deterministic input builder and one `*_reference(case)` per family.  tests/test_gpu_offpolicy_shapes.py runs the
kernels on these inputs; tests/test_host_offpolicy_shapes.py checks on the CPU that every precondition below holds and that
the float32 restatement alone stays inside the bars.  Plain numpy / torch-CPU module.

The yardsticks are the project's restatements (dqn_, distq_, iqn_, dsac_, per_restatement.py), each pinned to the reference's
own runs to 1e-10 by its host test.  A `*_reference` returns per variant
  * the float64 restatement's outputs,
  * `e_ref[array] = max |restatement(float32) - restatement(float64)|`: what float32 costs the reference itself at this shape,
and per case the precondition values:
  * `greedy_margin`: min over the rows of (best - second best candidate of the float64 q_next after the mask offset) divided by
    64 float32 ulp of max |q_next|; it must exceed 1 with and without the mask, so that no float32 evaluation of q_next can
    choose another a*.  A = 1 gives inf; a row with one legal action has its second candidate more than 1 below;
  * `min_abs_pre` (the IQN embedding): min |pre-activation| of the embedding's ReLU over all M x H entries, at least 1e-5: a
    unit nearer the kink may take either side in float32, and the backward gate turns that into a full d_e * f term.
Loss and gradient are continuous at the Huber kinks, at the u <= 0 indicator and at C51's clamps: no condition is needed there.

Every case names its seed.  The seeds are the first of 1000 + 17 k, k = 0, 1, ..., for which the preconditions hold (run this
file to search them again); no row or element is ever dropped from a comparison.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distq_restatement import c51_head, dist_values, qr_head, support_of, tau_hat_of  # noqa: E402
from dqn_restatement import RestatedBuffer, nstep_walk, td_head  # noqa: E402
from dsac_restatement import actor_head, alpha_state, alpha_step, critic_head, target  # noqa: E402
from iqn_restatement import embed, iqn_head, iqn_values  # noqa: E402
from per_restatement import RestatedPrio, RestatedTree  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
MIN_ABS_PRE = 1e-5
V_MIN, V_MAX = -10.0, 10.0
HUBER_DELTA = 0.7


def _seed(k: int) -> int:
    return 1000 + 17 * k


def case_id(c: dict) -> str:
    return "-".join(f"{k}{v}" for k, v in c.items() if k not in ("seed", "family"))


def _err(a32, a64) -> float:
    return float(np.abs(np.asarray(a32, np.float64) - np.asarray(a64, np.float64)).max())


def greedy_margin(q_next64: np.ndarray, mask) -> float:
    """min over rows of (top1 - top2 of q_next + (1 - mask) (min - max - 1)) / (64 ulp32(max |q_next|)), with and without mask."""
    q = np.asarray(q_next64, np.float64)
    if q.shape[1] == 1:
        return float("inf")
    ulp = 64.0 * float(np.spacing(np.float32(np.abs(q).max())))
    out = np.inf
    for m in (None, mask):
        sel = q if m is None else q + (1.0 - np.asarray(m, np.float64)) * (q.min() - q.max() - 1.0)
        top = np.sort(sel, axis=1)
        out = min(out, float((top[:, -1] - top[:, -2]).min()) / ulp)
    return out


def _row_inputs(rs, B: int, A: int) -> dict:
    """What every head takes per row: the taken action, the n-step walk's outputs, IS weights and a next-action mask with 1 to
    A legal actions per row."""
    mask = np.zeros((B, A), bool)
    for b in range(B):
        mask[b, rs.choice(A, 1 + rs.randint(0, A), replace=False)] = True
    vmask = (rs.rand(B) < 0.85).astype(np.uint8)
    return dict(act=rs.randint(0, A, B).astype(np.int64), mc=(2.0 * rs.standard_normal(B)).astype(np.float32),
                gpow=(0.99 ** rs.randint(1, 4, B)).astype(np.float32), vmask=vmask,
                weight=rs.uniform(0.5, 1.5, B).astype(np.float32), mask=mask)


# ---- DQN TD head ----------------------------------------------------------------------------------------------------------
# 256 rows per workgroup, one thread per row: one live wave / a full wave / one lane of the second wave / the last lane of the
# workgroup / a second workgroup with one row / 17 workgroups; the narrowest and the widest rows in two workgroups.
DQN_CASES = [dict(family="dqn", A=5, B=1, seed=_seed(0)), dict(family="dqn", A=5, B=63, seed=_seed(0)),
             dict(family="dqn", A=5, B=64, seed=_seed(0)), dict(family="dqn", A=5, B=65, seed=_seed(0)),
             dict(family="dqn", A=5, B=255, seed=_seed(0)), dict(family="dqn", A=5, B=256, seed=_seed(0)),
             dict(family="dqn", A=5, B=257, seed=_seed(0)), dict(family="dqn", A=5, B=4099, seed=_seed(0)),
             dict(family="dqn", A=1, B=257, seed=_seed(0)), dict(family="dqn", A=64, B=257, seed=_seed(0))]
# (is_double, lagged target, loss, mask_next): the fixture's 24 variants
DQN_VARIANTS = [(d, t, loss, m) for d in (0, 1) for t in (0, 1) for loss in ("mse", "msew", "huber") for m in (0, 1)]


def dqn_inputs(c: dict) -> dict:
    rs = np.random.RandomState(c["seed"])
    B, A = c["B"], c["A"]
    d = _row_inputs(rs, B, A)
    d.update({k: rs.standard_normal((B, A)).astype(np.float32) for k in ("q", "on", "tg")})
    return d


def _dqn_call(d, v, dtype):
    dbl, tgt, loss, msk = v
    return td_head(d["q"], d["on"], d["tg"] if tgt else None, d["mask"] if msk else None, d["act"], d["mc"], d["gpow"], d["vmask"],
                   d["weight"] if loss == "msew" else None, bool(dbl), HUBER_DELTA if loss == "huber" else None, dtype)


@functools.lru_cache(maxsize=None)
def _dqn_reference(key):
    c = dict(key)
    d = dqn_inputs(c)
    rows = np.arange(c["B"])
    qs = d["q"][rows, d["act"]]
    out = dict(greedy_margin=greedy_margin(d["on"], d["mask"]), variants={},
               mean_q=float(qs.astype(np.float64).mean()), mean_q_eref=abs(float(qs.mean(dtype=np.float32)) - float(qs.astype(np.float64).mean())))
    for v in DQN_VARIANTS:
        r64, r32 = _dqn_call(d, v, torch.float64), _dqn_call(d, v, torch.float32)
        r64["e_ref"] = {k: _err(r32[k], r64[k]) for k in ("returns", "td_error", "dq", "loss")}
        out["variants"][v] = r64
    return out


def dqn_reference(c: dict) -> dict:
    return _dqn_reference(tuple(sorted(c.items())))


# ---- C51 / QR-DQN ---------------------------------------------------------------------------------------------------------
# Atom j lives in lane j % 64, register j / 64: the register boundaries; 16 rows per workgroup, 4 per wave: the row edges and
# 257 workgroups; the smallest and the largest (A, N).
DISTQ_N_SWEEP = [dict(family="distq", A=3, N=n, B=33, seed=_seed(0)) for n in (63, 64, 65, 128, 129, 255, 256)]
DISTQ_B_SWEEP = [dict(family="distq", A=3, N=8, B=b, seed=_seed(0)) for b in (1, 15, 16, 17, 4099)]
DISTQ_CORNERS = [dict(family="distq", A=1, N=2, B=17, seed=_seed(0)), dict(family="distq", A=64, N=256, B=17, seed=_seed(0))]
DISTQ_CASES = DISTQ_N_SWEEP + DISTQ_B_SWEEP + DISTQ_CORNERS
HEAD_VARIANTS = [(t, w, m) for t in (0, 1) for w in (0, 1) for m in (0, 1)]   # (lagged target, weight, mask_next)


def distq_inputs(c: dict) -> dict:
    rs = np.random.RandomState(c["seed"])
    B, A, N = c["B"], c["A"], c["N"]
    d = _row_inputs(rs, B, A)
    # a spread over the atoms that keeps the softmax away from one-hot and lets |u| fall on both sides of 1
    d.update({k: (1.5 * rs.standard_normal((B, A * N))).astype(np.float32) for k in ("raw", "on", "tg")})
    d["mc"] = (4.0 * d["mc"]).astype(np.float32)   # some returns leave [v_min, v_max] at each end
    return d


def _distq_call(kind, d, v, A, N, dtype):
    tgt, wgt, msk = v
    args = (d["raw"], d["on"], d["tg"] if tgt else None, d["mask"] if msk else None, d["act"], d["mc"], d["gpow"], d["vmask"],
            d["weight"] if wgt else None)
    if kind == "c5":
        return c51_head(*args, support_of(V_MIN, V_MAX, N), V_MIN, V_MAX, A, N, dtype)
    return qr_head(*args, tau_hat_of(N), A, N, dtype)


@functools.lru_cache(maxsize=None)
def _distq_reference(key):
    c = dict(key)
    d = distq_inputs(c)
    A, N = c["A"], c["N"]
    out = dict(greedy_margin=np.inf, values={}, variants={})
    for kind, sup in (("c5", support_of(V_MIN, V_MAX, N)), ("qr", None)):
        v64 = {m: dist_values(d["on"], A, N, sup, d["mask"] if m else None) for m in (0, 1)}
        v32 = dist_values(d["on"], A, N, sup, None, torch.float32)
        out["greedy_margin"] = min(out["greedy_margin"], greedy_margin(v64[0]["q"], d["mask"]))
        out["values"][kind] = dict(q=v64[0]["q"], probs=v64[0]["probs"], act=v64[0]["act"], act_masked=v64[1]["act"],
                                   e_ref=dict(q=_err(v32["q"], v64[0]["q"]),
                                              probs=0.0 if sup is None else _err(v32["probs"], v64[0]["probs"])))
        for v in HEAD_VARIANTS:
            r64, r32 = _distq_call(kind, d, v, A, N, torch.float64), _distq_call(kind, d, v, A, N, torch.float32)
            r64.pop("u", None)
            r64["mean_q"] = float(r64["q_taken"].mean())
            r64["e_ref"] = {k: _err(r32[k], r64[k]) for k in ("returns", "prio", "d_out", "loss")}
            r64["e_ref"]["mean_q"] = abs(float(r32["q_taken"].astype(np.float32).mean(dtype=np.float32)) - r64["mean_q"])
            out["variants"][kind, v] = r64
    return out


def distq_reference(c: dict) -> dict:
    return _distq_reference(tuple(sorted(c.items())))


# ---- IQN values and head --------------------------------------------------------------------------------------------------
# Lane i holds online sample i (N <= 64), the N' targets sit in LDS: full and nearly full waves, N and N' apart both ways;
# 16 rows per workgroup: the row edges and 257 workgroups; the narrowest and the widest rows at N = N' = 64.
IQN_N_SWEEP = [dict(family="iqn", A=3, N=n, Np=p, B=33, seed=_seed(0)) for n, p in ((64, 64), (63, 64), (64, 2), (2, 64), (33, 31))]
IQN_B_SWEEP = [dict(family="iqn", A=3, N=8, Np=8, B=b, seed=_seed(0)) for b in (1, 15, 16, 17, 4099)]
IQN_CORNERS = [dict(family="iqn", A=a, N=64, Np=64, B=17, seed=_seed(0)) for a in (1, 64)]
IQN_CASES = IQN_N_SWEEP + IQN_B_SWEEP + IQN_CORNERS


def iqn_inputs(c: dict) -> dict:
    """out [B, N, A] under taus [B, N]; on [B, N, A]: the online net on the successor rows (it chooses a*, and is the next
    distribution when there is no lagged net); tg [B, N', A]: the lagged net there."""
    rs = np.random.RandomState(c["seed"])
    B, A, N, Np = c["B"], c["A"], c["N"], c["Np"]
    d = _row_inputs(rs, B, A)
    d["out"] = (1.5 * rs.standard_normal((B, N, A))).astype(np.float32)
    d["on"] = (1.5 * rs.standard_normal((B, N, A))).astype(np.float32)
    d["tg"] = (1.5 * rs.standard_normal((B, Np, A))).astype(np.float32)
    d["taus"] = rs.rand(B, N).astype(np.float32)
    return d


def _iqn_call(d, v, dtype):
    tgt, wgt, msk = v
    return iqn_head(d["out"], d["on"], d["tg"] if tgt else None, d["mask"] if msk else None, d["taus"], d["act"], d["mc"],
                    d["gpow"], d["vmask"], d["weight"] if wgt else None, dtype)


@functools.lru_cache(maxsize=None)
def _iqn_reference(key):
    c = dict(key)
    d = iqn_inputs(c)
    v64 = {m: iqn_values(d["on"], d["mask"] if m else None) for m in (0, 1)}
    v32 = iqn_values(d["on"], None, torch.float32)
    out = dict(greedy_margin=greedy_margin(v64[0]["q"], d["mask"]), variants={},
               values=dict(q=v64[0]["q"], act=v64[0]["act"], act_masked=v64[1]["act"], e_ref=dict(q=_err(v32["q"], v64[0]["q"]))))
    for v in HEAD_VARIANTS:
        r64, r32 = _iqn_call(d, v, torch.float64), _iqn_call(d, v, torch.float32)
        r64.pop("u")
        r64["mean_q"] = float(r64["q_taken"].mean())
        r64["e_ref"] = {k: _err(r32[k], r64[k]) for k in ("returns", "prio", "d_out", "loss")}
        r64["e_ref"]["mean_q"] = abs(float(r32["q_taken"].astype(np.float32).mean(dtype=np.float32)) - r64["mean_q"])
        out["variants"][v] = r64
    return out


def iqn_reference(c: dict) -> dict:
    return _iqn_reference(tuple(sorted(c.items())))


# ---- IQN embedding --------------------------------------------------------------------------------------------------------
# Wave w owns the cosines [16 w, 16 w + 16): C = 20 / 36 / 52 leave the last wave 4 of its 16; workgroups of 64 (forward) or
# 16 (backward) embedding columns: H = 512 is the limit, H = 496 leaves the last forward workgroup one idle wave; S = 64 is
# the limit of the fractions.  (H = 512 comes with M = 15 network rows: the fewer entries, the sooner a seed keeps all of
# them away from the ReLU's kink.)
EMBED_SHAPES = [(3, 5, 20, 16), (3, 5, 36, 32), (3, 5, 52, 48), (3, 5, 64, 512), (2, 8, 8, 496), (1, 64, 4, 16), (5, 64, 64, 64)]
EMBED_SEEDS = {(3, 5, 20, 16): _seed(0), (3, 5, 36, 32): _seed(0), (3, 5, 52, 48): _seed(0), (3, 5, 64, 512): _seed(0),
               (2, 8, 8, 496): _seed(1), (1, 64, 4, 16): _seed(0), (5, 64, 64, 64): _seed(0)}
EMBED_CASES = [dict(family="embed", B=s[0], S=s[1], C=s[2], H=s[3], relu_f=r, seed=EMBED_SEEDS[s]) for s in EMBED_SHAPES for r in (0, 1)]


def embed_inputs(c: dict) -> dict:
    rs = np.random.RandomState(c["seed"])
    B, S, C, H = c["B"], c["S"], c["C"], c["H"]
    bound = 1.0 / np.sqrt(C)
    return dict(f=rs.standard_normal((B, H)).astype(np.float32), We=rs.uniform(-bound, bound, (H, C)).astype(np.float32),
                be=rs.uniform(-bound, bound, H).astype(np.float32), d_e=rs.standard_normal((B * S, H)).astype(np.float32),
                taus=rs.rand(B, S).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _embed_reference(key):
    c = dict(key)
    d = embed_inputs(c)
    r64 = embed(d["f"], d["taus"], d["We"], d["be"], bool(c["relu_f"]), d["d_e"])
    r32 = embed(d["f"], d["taus"], d["We"], d["be"], bool(c["relu_f"]), d["d_e"], dtype=torch.float32)
    r64["e_ref"] = {k: _err(r32[k], r64[k]) for k in ("e", "d_f", "dWe", "dbe")}
    r64["min_abs_pre"] = float(np.abs(r64["pre"]).min())
    r64["same_gate32"] = bool(np.array_equal(r32["pre"] > 0, r64["pre"] > 0))
    return r64


def embed_reference(c: dict) -> dict:
    return _embed_reference(tuple(sorted(c.items())))


# ---- Discrete SAC heads ---------------------------------------------------------------------------------------------------
# 16 rows per workgroup: the row edges and 257 workgroups (the finalize and the alpha step fold several partials per lane).
DSAC_CASES = [dict(family="dsac", A=5, B=b, seed=_seed(0)) for b in (1, 15, 16, 17, 4099)] + [dict(family="dsac", A=1, B=17, seed=_seed(0))]
DSAC_VARIANTS = [(w, a) for w in (0, 1) for a in (0, 1)]       # (weight, auto-tuned alpha): the fixture's four
DSAC_ALPHA = {0: 0.2, 1: float(np.exp(-0.75))}                 # a fixed alpha; exp(log_alpha) of the auto-tuned kind
DSAC_LOG_ALPHA, DSAC_TARGET_ENTROPY, DSAC_LR = -0.75, 0.3, 1e-3


def dsac_inputs(c: dict) -> dict:
    rs = np.random.RandomState(c["seed"])
    B, A = c["B"], c["A"]
    d = _row_inputs(rs, B, A)
    d.update({k: rs.standard_normal((B, A)).astype(np.float32) for k in ("lnext", "q1n", "q2n", "logits", "q1", "q2")})
    return d


@functools.lru_cache(maxsize=None)
def _dsac_reference(key):
    c = dict(key)
    d = dsac_inputs(c)
    out = {}
    for v in DSAC_VARIANTS:
        wgt, auto = v
        alpha = DSAC_ALPHA[auto]
        r, e = {}, {}
        for dt, tag in ((np.float64, 64), (np.float32, 32)):
            ret = target(d["lnext"], d["q1n"], d["q2n"], alpha, d["mc"], d["gpow"], d["vmask"], dtype=dt)
            ch = critic_head(d["q1"], d["q2"], d["act"], ret, d["weight"] if wgt else None, dtype=dt)
            ah = actor_head(d["logits"], d["q1"], d["q2"], alpha, dtype=dt)
            st = alpha_state(DSAC_LOG_ALPHA)
            a_loss = alpha_step(st, ah["mean_entropy"], DSAC_TARGET_ENTROPY, lr=DSAC_LR)
            r[tag] = dict(returns=ret, dq1=ch["dq1"], dq2=ch["dq2"], prio=ch["prio"], critic1_loss=ch["loss1"],
                          critic2_loss=ch["loss2"], d_logits=ah["d_logits"], entropy=ah["entropy"], actor_loss=ah["loss"],
                          mean_entropy=ah["mean_entropy"], alpha_loss=a_loss, log_alpha=st["log_alpha"],
                          alpha=float(np.exp(st["log_alpha"])))
        for k in r[64]:
            e[k] = _err(r[32][k], r[64][k])
        r[64] = {k: np.asarray(x, np.float64) if isinstance(x, np.ndarray) else x for k, x in r[64].items()}
        r[64]["e_ref"] = e
        out[v] = r[64]
    return out


def dsac_reference(c: dict) -> dict:
    return _dsac_reference(tuple(sorted(c.items())))


# ---- n-step walk ----------------------------------------------------------------------------------------------------------
NSTEP_BUFFERS = [(1, 1), (1, 2), (3, 5), (7, 16)]      # (buffer_num, sub_size)
NSTEP_GAMMAS = (0.0, 0.99, 1.0)
NSTEP_COLS = (0, 1)
NSTEP_REW_DIM = 2


def nstep_horizons(sub_size: int) -> list:
    return sorted({1, 2, sub_size, sub_size + 3, 40})


def nstep_script(buffer_num: int, sub_size: int) -> list:
    """The add script of one buffer: a list of (env, rew f32 [2], terminated, truncated), in order.  With three or more
    sub-buffers: 0 is written past its end twice with an episode ending on its last slot in each lap, 1 stays empty, the last
    is partly filled with its newest row unfinished; the others get random lengths, ends and truncations.  A single
    sub-buffer is written past its end twice and ends on an unfinished row."""
    rs = np.random.RandomState(4000 + 31 * buffer_num + sub_size)
    S = sub_size
    rows = []

    def add(env, term=False, trunc=False):
        rows.append((env, rs.standard_normal(NSTEP_REW_DIM).astype(np.float32), bool(term), bool(trunc)))

    if buffer_num == 1:
        for k in range(2 * S + max(1, S // 2)):
            add(0, term=(S > 1 and k % S == S - 1 and k < 2 * S), trunc=(S > 2 and k % 3 == 1))
        if rows[-1][2] or rows[-1][3]:
            rows[-1] = (0, rows[-1][1], False, False)
        return rows
    per_env = {}
    for env in range(buffer_num):
        if env == 0:
            per_env[env] = [(k % S == S - 1, k % 4 == 1) for k in range(2 * S + 2)]          # wraps twice, ends on slot S - 1
        elif env == 1:
            per_env[env] = []                                                                # never written
        elif env == buffer_num - 1:
            per_env[env] = [(k == 1, False) for k in range(max(2, S // 2))]                  # partly filled, newest unfinished
            per_env[env][-1] = (False, False)
        else:
            n = int(rs.randint(S - 1, 3 * S))                                                # around one to three laps
            per_env[env] = [(rs.rand() < 0.15, rs.rand() < 0.1) for _ in range(n)]
    # interleaved as a vector env would add them
    for k in range(max(len(v) for v in per_env.values())):
        for env in range(buffer_num):
            if k < len(per_env[env]):
                add(env, *per_env[env][k])
    return rows


def nstep_restated(buffer_num: int, sub_size: int):
    """-> (RestatedBuffer after the script, the script, indices: every stored index and its negative alias, tiled past 256)."""
    script = nstep_script(buffer_num, sub_size)
    rb = RestatedBuffer(buffer_num, sub_size, NSTEP_REW_DIM)
    for env, rew, term, trunc in script:
        rb.add(env, rew.astype(np.float64), term, trunc)
    stored = rb.sample_indices_all()
    both = np.concatenate([stored, stored - buffer_num * sub_size])
    idx = np.tile(both, -(-258 // len(both)))
    return rb, script, idx.astype(np.int64)


def nstep_reference(rb, idx, n_step: int, gamma: float, col: int) -> dict:
    idx_n, mc, gpow, vmask = nstep_walk(rb, idx, n_step, gamma, col)
    # the reference keeps mc and gamma^m in float64 and rounds once on the way out: that rounding is its float32 cost
    return dict(idx_n=idx_n, mc=mc, gpow=gpow, vmask=vmask,
                e_ref=dict(mc=_err(mc.astype(np.float32), mc), gpow=_err(gpow.astype(np.float32), gpow)))


# ---- sum tree -------------------------------------------------------------------------------------------------------------
# One workgroup of at most 1024 threads walks `for (i = t; i < n; i += nt)`: n = 1024 is the last single pass, 1025 gives one
# thread a second entry, 4099 gives every thread four or five.
TREE_SIZES = [1500, 70000]           # bounds 2048 and 131072
TREE_NS = [1024, 1025, 4099]
PRIO_ALPHAS = [1.0, 0.6]
PRIO_BETA = 0.4


def tree_indices(rs, size: int, n: int) -> np.ndarray:
    """n leaf indices drawn with replacement; where n >= 2 size + 1 every leaf is first listed twice, so that every leaf has
    duplicates whatever the draw."""
    if n >= 2 * size + 1:
        idx = np.concatenate([np.arange(size), np.arange(size), rs.randint(0, size, n - 2 * size)])
        return rs.permutation(idx).astype(np.int64)
    return rs.randint(0, size, n).astype(np.int64)


def tree_set_calls(size: int, lattice: bool = False) -> list:
    """[(index i64 [n], value f64 [n])] for n in TREE_NS.  lattice: multiples of 1/8 in [1/8, 8], whose sums are all exact."""
    rs = np.random.RandomState(5000 + size + int(lattice))
    out = []
    for n in TREE_NS:
        idx = tree_indices(rs, size, n)
        val = rs.randint(1, 65, n) / 8.0 if lattice else rs.uniform(0.1, 2.0, n)
        out.append((idx, val.astype(np.float64)))
    return out


def tree_after(size: int, lattice: bool = False) -> list:
    """The RestatedTree's array after each call of `tree_set_calls`."""
    t = RestatedTree(size)
    out = []
    for idx, val in tree_set_calls(size, lattice):
        t.set(idx, val)
        out.append(t.tree.copy())
    return out


def prefix_tree(size: int = 1500) -> RestatedTree:
    t = RestatedTree(size)
    for idx, val in tree_set_calls(size, lattice=True):
        t.set(idx, val)
    return t


def prefix_values(t: RestatedTree, n: int = 4099, n_edge: int = 64):
    """-> (values f64 [n], edge nodes i64 [n_edge], first leaf right of each edge node's left child i64 [n_edge]).  The last
    n_edge values equal, exactly, the sum of all leaves left of an inner node's right child (RestatedTree.reduce; on the
    lattice tree every addition and subtraction is exact): the descent reaches that node with the left child's sum in hand,
    and the strict `<` must send it left."""
    rs = np.random.RandomState(6000 + t.size)
    total = t.reduce()
    vals = rs.uniform(0.0, total, n - n_edge)
    nodes, firsts = [], []
    level_nodes = [k for k in range(1, t.bound) if t.tree[2 * k + 1] > 0 and t.tree[2 * k] > 0]
    for k in rs.choice(level_nodes, n_edge, replace=False):
        k = int(k)
        right = 2 * k + 1
        while right < t.bound:
            right *= 2                      # the leftmost leaf under the right child
        nodes.append(k)
        firsts.append(right - t.bound)
    edge = np.array([t.reduce(0, f) for f in firsts], np.float64)
    return np.concatenate([vals, edge]), np.array(nodes, np.int64), np.array(firsts, np.int64)


def prio_calls(size: int) -> list:
    """[("update", index, td f32) | ("init", index, None)]: for each n an update_weight and an init_weight of n entries."""
    rs = np.random.RandomState(7000 + size)
    out = []
    for n in TREE_NS:
        out.append(("update", tree_indices(rs, size, n), (3.0 * rs.standard_normal(n)).astype(np.float32)))
        out.append(("init", tree_indices(rs, size, n), None))
    return out


def prio_after(size: int, alpha: float, weight_norm: bool = True):
    """-> (the RestatedPrio after `prio_calls`, [(tree, [max_prio, min_prio])] after each call)."""
    p = RestatedPrio(size, alpha, PRIO_BETA, weight_norm)
    out = []
    for kind, idx, td in prio_calls(size):
        if kind == "update":
            p.update_weight(idx, td)
        else:
            p.init_weight(idx)
        out.append((p.t.tree.copy(), np.array([p.max_prio, p.min_prio])))
    return p, out


# ---- choosing the seeds ---------------------------------------------------------------------------------------------------
def preconditions_hold(c: dict) -> bool:
    fam = c["family"]
    if fam == "embed":
        r = embed_reference(c)
        return r["min_abs_pre"] >= MIN_ABS_PRE
    if fam == "dsac":
        return True
    ref = {"dqn": dqn_reference, "distq": distq_reference, "iqn": iqn_reference}[fam](c)
    return ref["greedy_margin"] > 1.0


ALL_CASES = DQN_CASES + DISTQ_CASES + IQN_CASES + EMBED_CASES + DSAC_CASES


if __name__ == "__main__":   # print, per case, the first seed of the sequence for which the preconditions hold
    for case in ALL_CASES:
        for k in range(200):
            trial = dict(case, seed=_seed(k))
            if preconditions_hold(trial):
                break
        print(case_id(case), case["family"], "seed", trial["seed"], "(k = %d)" % k, "" if trial["seed"] == case["seed"] else "<-- differs")
