"""Inputs and float64 yardsticks of the shape sweeps over the CTDE family's kernels alone: tsm_qmix_mix_td / tsm_qmix_finalize /
tsm_qmix_egreedy (csrc/qmix.hip) and tsm_ctde_td_head / tsm_ctde_finalize / tsm_global_state (csrc/ctde.hip) -- the case lists,
one deterministic input builder and one `*_reference(case)` per family.  tests/test_gpu_ctde_shapes.py runs the kernels on
these inputs; tests/test_host_ctde_shapes.py checks on the CPU that every property promised below holds and that the float32
restatement alone stays inside the bars.  Plain numpy / torch-CPU module.

The yardsticks:
  * mix/TD: `mix` and `td_loss` of tests/qmix_restatement.py (pinned to the reference to 1e-10 by tests/test_host_qmix.py) on
    the kernel's own inputs -- the per-agent Q rows and the eight hypernetwork outputs --, the per-row gradients from autograd;
  * the CTDE head: the autograd expression of CTDEPolicy.learn (ctde.py:149-185) with its (B,) x (B, 1) broadcast;
  * tsm_ctde_finalize: the float64 expression on partials whose sums and quotients are all exact;
  * tsm_global_state: np.concatenate, and a float32 sum in agent order divided by float32(N).
A mix / head reference returns the float64 outputs and `e_ref[array] = max |restatement(float32) - restatement(float64)|`: what
float32 costs the reference itself at this shape.

The mix/TD cases need no precondition on their inputs: ELU's derivative is continuous at 0 (1 from the right, exp(0) from the
left), so a pre-activation that float32 puts on the other side of 0 moves no gradient by more than its own rounding; `abs` and
`max` act on float32 inputs, which the float64 run sees exactly, so the sign of every w1raw / w2raw entry and the greatest
entry of every q_next row are the same in both runs (an exact zero has gradient sgn(0) = 0 in both); and the kernel chooses no
action -- `act` is an input.
The CTDE head has one: |mean advantage| >= 0.1 in float64, so that the bar on actor_loss = -mean(logp) * mean(adv), and on
dlogits, which carries mean(adv) as a factor, does not collapse onto a near-zero product of which float32 keeps few digits.

Every case names its seed.  The head's seeds are the first of 1000 + 17 k, k = 0, 1, ..., for which the precondition holds
(run this file to search them again); no row or element is ever dropped from a comparison.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from offpolicy_cases import _err, _seed, case_id  # noqa: E402,F401
from qmix_restatement import mix, td_loss  # noqa: E402

GAMMA = 0.99
MIN_ABS_MEAN_ADV = 0.1
ZERO_SHARE = 0.03         # of the w1raw / w2raw entries, set to exactly 0.0 where B >= 15
OUTER_MAX = 1 << 25       # the head's (B, B) product is formed up to this many entries (B <= 5792)


def _key(c: dict):
    return tuple(sorted(c.items()))


# ---- QMIX mix / TD ----------------------------------------------------------------------------------------------------------
# A workgroup owns R rows, a wave RW of them (32 / 8 at E = 32, 16 / 4 at E = 64): B = 1, around RW, around R, and 4099 rows
# (129 / 257 workgroups: tsm_qmix_finalize folds more than 64 partials).  The corners: the fewest agents and actions; A = 64
# (the R x 64 limit of the staged segment) with the most agents; N = 8 with nr * A no multiple of 4 in the last workgroup (the
# float4 loop and its tail both run); one agent with A = 64 over 129 / 257 workgroups.  `offset = 1`: the same inputs with
# every agent's q_next and dq starting one float into a larger buffer, so that no workgroup's segment is 16-byte aligned.
def rows_per_block(E: int) -> int:
    return 256 // (E // 4)


def _mix_case(E, N, A, B, term="mixed", offset=0):
    return dict(family="mix", E=E, N=N, A=A, B=B, term=term, offset=offset, seed=_seed(0))


MIX_B_SWEEP = ([_mix_case(32, 3, 5, b, term={1: "all", 8: "none"}.get(b, "mixed")) for b in (1, 7, 8, 9, 31, 32, 33, 4099)]
               + [_mix_case(64, 3, 5, b, term={1: "none", 4: "all"}.get(b, "mixed")) for b in (1, 3, 4, 5, 15, 16, 17, 4099)])
MIX_CORNERS = [_mix_case(E, n, a, b, term=t) for E in (32, 64)
               for n, a, b, t in ((1, 1, 17, "all" if E == 32 else "none"), (8, 64, 33, "mixed"), (8, 3, 33, "mixed"), (1, 64, 4099, "mixed"))]
MIX_UNALIGNED = [_mix_case(E, n, a, 33, offset=1) for E in (32, 64) for n, a in ((3, 5), (8, 3))]
MIX_CASES = MIX_B_SWEEP + MIX_CORNERS + MIX_UNALIGNED
MIX_MONOTONIC = (1, 0)
MIX_KEYS = ("dq", "dw1", "db1", "dw2", "db2", "q_tot", "loss", "mean_q")
GUARD, GUARD_FLOATS = -7.0, 8


def mix_inputs(c: dict) -> dict:
    """The kernel's inputs: q, q_next [N][B, A], act i64 [N][B], rew [N][B], the online hypernetwork outputs w1raw [B, N E],
    b1 [B, E], w2raw [B, E], b2 [B, 1], the target ones (tw1raw, ...), term u8 [B].  The `offset` of a case does not enter."""
    rs = np.random.RandomState(c["seed"] + 101 * c["E"] + 1009 * c["N"] + 10007 * c["A"] + 100003 * c["B"])
    E, N, A, B = c["E"], c["N"], c["A"], c["B"]
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    d = dict(q=f(N, B, A), q_next=f(N, B, A), act=rs.randint(0, A, (N, B)).astype(np.int64), rew=f(N, B))
    rows = np.arange(B)
    sel = {"": np.stack([d["q"][i, rows, d["act"][i]] for i in range(N)], 1), "t": d["q_next"].max(-1).T}       # [B, N]
    for side in ("", "t"):
        w1, w2 = f(B, N * E), f(B, E)
        if B >= 15:
            for w in (w1, w2):
                flat = w.reshape(-1)
                flat[rs.choice(flat.size, max(1, int(round(ZERO_SHARE * flat.size))), replace=False)] = 0.0
        # b1 is shifted by the median of the monotonic mixer's q . |w1|, so that the pre-activations straddle ELU's kink
        dot = np.einsum("bn,bne->be", sel[side].astype(np.float64), np.abs(w1.astype(np.float64)).reshape(B, N, E))
        d[side + "w1raw"], d[side + "w2raw"] = w1, w2
        d[side + "b1"] = (0.5 * rs.standard_normal((B, E)) - np.median(dot)).astype(np.float32)
        d[side + "b2"] = (3.0 + rs.standard_normal((B, 1))).astype(np.float32)   # keeps mean q_tot of the raw-weight mixer off 0
    mixed = rs.rand(B) < 0.3
    mixed[0], mixed[-1] = True, False     # both kinds whatever the draw (a mixed case has B >= 3)
    d["term"] = {"mixed": mixed, "all": np.ones(B, bool), "none": np.zeros(B, bool)}[c["term"]].astype(np.uint8)
    return d


def mix_td(d: dict, monotonic: bool, gamma: float, dtype) -> dict:
    """What tsm_qmix_mix_td computes, in `dtype`: q_sel = gather, q_max = max, `mix` on both sides, `td_loss`, and the autograd
    gradients of the loss with respect to every q_i and to the four online hypernetwork outputs."""
    N, B, A = np.shape(d["q"])
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)  # noqa: E731
    q = [t(d["q"][i]).requires_grad_() for i in range(N)]
    act = torch.as_tensor(np.asarray(d["act"])).to(torch.int64)
    q_sel = torch.cat([q[i].gather(1, act[i].unsqueeze(-1)) for i in range(N)], dim=-1)
    q_max = torch.cat([t(d["q_next"][i]).max(dim=-1, keepdim=True)[0] for i in range(N)], dim=-1)
    E = np.shape(d["b1"])[1]
    shapes = ((B, N, E), (B, 1, E), (B, E, 1), (B, 1, 1))
    on = [t(d[k]).view(s).requires_grad_() for k, s in zip(("w1raw", "b1", "w2raw", "b2"), shapes)]
    tg = [t(d[k]).view(s) for k, s in zip(("tw1raw", "tb1", "tw2raw", "tb2"), shapes)]
    q_tot = mix(q_sel, *on, monotonic)
    with torch.no_grad():
        q_tot_next = mix(q_max, *tg, monotonic)
        pre = torch.bmm(q_sel.view(B, 1, N), torch.abs(on[0]) if monotonic else on[0]) + on[1]
    loss = td_loss(q_tot, q_tot_next, [t(d["rew"][i]) for i in range(N)], torch.as_tensor(np.asarray(d["term"])).to(torch.bool), gamma)
    g = torch.autograd.grad(loss, q + on)
    n = lambda x: x.detach().to(torch.float64).numpy()  # noqa: E731
    return dict(dq=np.stack([n(x) for x in g[:N]]), dw1=n(g[N]).reshape(B, N * E), db1=n(g[N + 1]).reshape(B, E),
                dw2=n(g[N + 2]).reshape(B, E), db2=n(g[N + 3]).reshape(B, 1), q_tot=n(q_tot).reshape(B), loss=float(loss.item()),
                mean_q=float(q_tot.mean().item()), pre=n(pre).reshape(B, E))


@functools.lru_cache(maxsize=None)
def _mix_td_reference(key):
    d = mix_inputs(dict(key))
    z1, z2 = d["w1raw"] == 0.0, d["w2raw"] == 0.0
    out = {}
    for mono in MIX_MONOTONIC:
        r64, r32 = mix_td(d, bool(mono), GAMMA, torch.float64), mix_td(d, bool(mono), GAMMA, torch.float32)
        r64["e_ref"] = {k: _err(r32[k], r64[k]) for k in MIX_KEYS}
        # the entries under an exact zero of w1raw / w2raw on their own: exactly 0 when monotonic, else the unsigned product
        r64["zero"] = dict(dw1=z1, dw2=z2)
        for k, z in (("dw1", z1), ("dw2", z2)):
            r64["e_ref"][k + "@0"] = _err(r32[k][z], r64[k][z]) if z.any() else 0.0
        out[mono] = r64
    return out


def mix_td_reference(c: dict) -> dict:
    """{monotonic: float64 outputs + e_ref + zero masks} of a case; the `offset` of a case does not enter."""
    return _mix_td_reference(_key({k: v for k, v in c.items() if k != "offset"}))


# ---- epsilon-greedy at eps = 0 ------------------------------------------------------------------------------------------------
EGREEDY_CASE = dict(family="egreedy", N=8, A=64, B=17, seed=_seed(0))


def egreedy_inputs(c: dict = EGREEDY_CASE) -> dict:
    """q [N][B, A]; in the rows with (b + i) % 10 == 0 (a tenth) the row's maximum stands at two or three places."""
    rs = np.random.RandomState(c["seed"])
    N, A, B = c["N"], c["A"], c["B"]
    q = rs.standard_normal((N, B, A)).astype(np.float32)
    planted = np.zeros((N, B), bool)
    for i in range(N):
        for b in range(B):
            if (b + i) % 10 == 0:
                at = np.sort(rs.choice(A, 3, replace=False))
                q[i, b, at] = q[i, b].max() + np.float32(0.5)
                planted[i, b] = True
    return dict(q=q, planted=planted, act=q.argmax(-1).T.astype(np.int32))   # np.argmax: the first maximum; act [B, N]


# ---- CTDE TD head -------------------------------------------------------------------------------------------------------------
# One row per thread, 256 per workgroup, a wave's 64: one row / around a wave / around a workgroup / 17 workgroups / 258
# workgroups, whose partials the actor-gradient kernel folds two to a thread (n_part > 256); the narrowest rows, several critic
# outputs, and the widest of both.
HEAD_SEEDS = {}


def _head_case(n_out, A, B):
    return dict(family="head", n_out=n_out, A=A, B=B, seed=HEAD_SEEDS.get((n_out, A, B), _seed(0)))


HEAD_SHAPES = [(1, 5, b) for b in (1, 63, 64, 65, 255, 256, 257, 4099, 65793)] + [(1, 1, 257), (3, 5, 257), (8, 64, 257)]
HEAD_KEYS = ("dq", "dlogits", "actor_loss", "critic_loss")


def head_inputs(c: dict) -> dict:
    rs = np.random.RandomState(c["seed"])
    n_out, A, B = c["n_out"], c["A"], c["B"]
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    return dict(q=f(B, n_out), q_next=f(B, n_out), rew=(0.5 + rs.standard_normal(B)).astype(np.float32),
                term=(rs.rand(B) < 0.2).astype(np.uint8), logits=f(B, A), act=rs.randint(0, A, B).astype(np.int64), gamma=GAMMA)


def ctde_head(d: dict, dtype, outer: bool | None = None) -> dict:
    """CTDEPolicy.learn's losses and their gradients (ctde.py:149-185) in `dtype`.  outer: form the (B, B) product of the
    reference's (B,) x (B, 1) broadcast; by default up to OUTER_MAX entries.  Beyond, its mean is restated as the product of
    the two means, which it equals in real arithmetic (and to 1e-12 in float64: tests/test_host_ctde_shapes.py)."""
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)  # noqa: E731
    q, logits = t(d["q"]).requires_grad_(), t(d["logits"]).requires_grad_()
    B, n_out = q.shape
    values, values_next = q, t(d["q_next"])
    if n_out > 1:
        values, values_next = values.mean(dim=1, keepdim=True), values_next.mean(dim=1, keepdim=True)
    term = torch.as_tensor(np.asarray(d["term"])).to(torch.bool).unsqueeze(-1)
    td_target = t(d["rew"]).unsqueeze(-1) + d["gamma"] * values_next * (~term).to(dtype)
    critic_loss = F.mse_loss(values, td_target.detach())
    advantage = (td_target - values).detach()
    log_probs = -F.cross_entropy(logits, torch.as_tensor(np.asarray(d["act"])).to(torch.int64), reduction="none")
    if B * B <= OUTER_MAX if outer is None else outer:
        actor_loss = -(log_probs * advantage).mean()   # (B,) * (B, 1) -> (B, B)
    else:
        actor_loss = -(log_probs.mean() * advantage.mean())
    dq, = torch.autograd.grad(critic_loss, q)
    dlogits, = torch.autograd.grad(actor_loss, logits)
    n = lambda x: x.detach().to(torch.float64).numpy()  # noqa: E731
    return dict(dq=n(dq), dlogits=n(dlogits), actor_loss=float(actor_loss.item()), critic_loss=float(critic_loss.item()),
                mean_adv=float(advantage.to(torch.float64).mean().item()))


def _head_both(d: dict) -> dict:
    r64, r32 = ctde_head(d, torch.float64), ctde_head(d, torch.float32)
    r64["e_ref"] = {k: _err(r32[k], r64[k]) for k in HEAD_KEYS}
    return r64


@functools.lru_cache(maxsize=None)
def _head_reference(key):
    return _head_both(head_inputs(dict(key)))


def ctde_head_reference(c: dict) -> dict:
    """c: a case of HEAD_CASES, or the inputs themselves (a dict with q, q_next, rew, term, logits, act and gamma; not cached)
    -> the float64 dq, dlogits, actor_loss, critic_loss, mean_adv and e_ref."""
    return _head_both(c) if "q" in c else _head_reference(_key(c))


HEAD_CASES = [_head_case(*s) for s in HEAD_SHAPES]


# ---- tsm_ctde_finalize ----------------------------------------------------------------------------------------------------------
# One wave, lane l takes entries l, l + 64, ...: one entry / around the wave, the two counts apart both ways / more than four
# entries per lane.  B is a power of two and every slot that is read a multiple of 1/8 below 8 in size: each sum is a multiple
# of 1/8 below 2^12, each mean a dyadic fraction, and their product has fewer than 31 significant bits -- all exact in float64.
FINALIZE_CASES = [dict(family="finalize", nb_c=c_, nb_a=a_, B=b_) for c_, a_, b_ in ((1, 1, 1), (63, 65, 64), (64, 64, 4096), (65, 1, 65536),
                                                                                     (257, 130, 1 << 20))]
FINALIZE_POISON = 1e30


def finalize_inputs(c: dict) -> dict:
    """pc [nb_c, 4] = {sum adv, sum sq, poison, poison}, pa [nb_a, 4] = {sum logp, poison, poison, poison}: the layout of the
    one-launch kernels' partials.  The lattice of offpolicy_cases.tree_set_calls(lattice=True), adv of both signs, logp <= 0."""
    rs = np.random.RandomState(5000 + 3 * c["nb_c"] + c["nb_a"])
    lat = lambda n: rs.randint(1, 65, n) / 8.0  # noqa: E731
    pc, pa = np.full((c["nb_c"], 4), FINALIZE_POISON), np.full((c["nb_a"], 4), FINALIZE_POISON)
    pc[:, 0] = lat(c["nb_c"]) * rs.choice([-1.0, 1.0], c["nb_c"])
    pc[:, 1] = lat(c["nb_c"])
    pa[:, 0] = -lat(c["nb_a"])
    return dict(pc=pc, pa=pa)


def finalize_reference(c: dict) -> dict:
    d = finalize_inputs(c)
    B = float(c["B"])
    m_adv, m_logp = d["pc"][:, 0].sum() / B, d["pa"][:, 0].sum() / B
    return dict(scalars=np.array([-m_logp * m_adv, d["pc"][:, 1].sum() / B]).astype(np.float32), mean_adv=np.float32(m_adv))


# ---- tsm_global_state -----------------------------------------------------------------------------------------------------------
# One thread per output element, 256 per workgroup: one element / a ragged middle / the 64-agent limit at D = 1 and at a D
# that divides nothing / one and two rows of a wide D / 255, 256 and 257 elements of the concatenation.
GLOBAL_CASES = [dict(family="global", N=n, D=d_, B=b) for n, d_, b in ((1, 1, 1), (3, 18, 37), (64, 1, 4), (64, 7, 33), (5, 51, 1), (5, 51, 2),
                                                                       (1, 1, 255), (1, 1, 256), (1, 1, 257))]


def global_inputs(c: dict) -> np.ndarray:
    return np.random.RandomState(8000 + 97 * c["N"] + 13 * c["D"] + c["B"]).standard_normal((c["N"], c["B"], c["D"])).astype(np.float32)


def global_reference(c: dict) -> dict:
    obs = global_inputs(c)
    s = np.zeros(obs.shape[1:], np.float32)
    for a in range(c["N"]):
        s = s + obs[a]                       # float32, agents in order
    return dict(concatenate=np.concatenate(list(obs), axis=1), mean=s / np.float32(c["N"]))


# ---- choosing the seeds -------------------------------------------------------------------------------------------------------
def preconditions_hold(c: dict) -> bool:
    return c["family"] != "head" or abs(ctde_head_reference(c)["mean_adv"]) >= MIN_ABS_MEAN_ADV


if __name__ == "__main__":   # print, per head case, the first seed of the sequence for which the precondition holds
    for case in HEAD_CASES:
        for k in range(200):
            trial = dict(case, seed=_seed(k))
            if preconditions_hold(trial):
                break
        print(case_id(case), "seed", trial["seed"], "(k = %d)" % k, "" if trial["seed"] == case["seed"] else "<-- differs")
