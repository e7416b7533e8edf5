"""GPU tests (`-m gpu`) of the CTDE family's kernels alone, at their shape limits: tsm_qmix_mix_td, tsm_qmix_finalize and
tsm_qmix_egreedy (csrc/qmix.hip), tsm_ctde_td_head, tsm_ctde_finalize and tsm_global_state (csrc/ctde.hip) -- the row, wave,
workgroup, action-count and agent-count boundaries, the exact zeros of the monotonic weights, the out-of-range action, and
the branches that only an unaligned per-agent array takes, none of which the learner-level tests (A = 5, N in {3, 8}, torch's
aligned allocations, gradients summed over the batch) reach.  Cases, inputs and float64 yardsticks: tests/ctde_cases.py
(tests/test_host_ctde_shapes.py checks their promises on the CPU).  Bars, all of them the sibling files' own:
  * the per-row mix/TD outputs, q_tot, the loss and mean q (through tsm_qmix_finalize), the head's gradients and scalars:
    test_gpu_distq._bar, max |hip - ref64| <= 1e-5 max |ref64| + e_ref, e_ref = max |restatement(float32) -
    restatement(float64)| at that shape;
  * the zeros of dq off the taken action and under an exact zero of a monotonic weight, the guard floats, dlogits at A = 1,
    tsm_ctde_finalize, tsm_global_state and the greedy actions: exact.
Every launch runs twice and must give the same bits.  Every comparison prints `PARITY name: ...`.

No test passes an out-of-range action to tsm_ctde_td_head: the head indexes `logits` with `act` unchecked."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import ctde_cases as cc  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_gpu_dqn import _d  # noqa: E402
from test_gpu_offpolicy_shapes import _exact, _finalized, _same_bits, _worst  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops

LEAD = cc.GUARD_FLOATS + 1      # floats in front of an unaligned dq: the guard, and the one float that breaks the alignment


def _one_float_in(x):
    """A contiguous view with the values of x [B, A] that starts one float into a buffer of its own: 4 past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _guarded(B, A):
    """(buffer of GUARD, dq [B, A] inside it, one float past a 16-byte boundary, GUARD_FLOATS guard floats on each side)."""
    buf = torch.full((LEAD + B * A + cc.GUARD_FLOATS,), cc.GUARD, dtype=torch.float32, device=DEV)
    v = buf[LEAD:LEAD + B * A].view(B, A)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return buf, v


def _guards_intact(buf, n):
    return bool((buf[:LEAD] == cc.GUARD).all()) and bool((buf[LEAD + n:] == cc.GUARD).all()) and buf.numel() == LEAD + n + cc.GUARD_FLOATS


class _Mix:
    """A mix/TD case's inputs on the device and its launches."""

    def __init__(self, c, act=None):
        self.c, d = c, cc.mix_inputs(c)
        self.d = d
        N, B, A, E = c["N"], c["B"], c["A"], c["E"]
        self.q = [_d(d["q"][i]) for i in range(N)]
        self.q_next = [_d(d["q_next"][i]) for i in range(N)]
        self.act = [_d((d["act"] if act is None else act)[i]) for i in range(N)]
        self.rew = [_d(d["rew"][i]) for i in range(N)]
        self.hyper = tuple(_d(d[k]) for k in ("w1raw", "b1", "w2raw", "b2"))
        self.hyper_next = tuple(_d(d[k]) for k in ("tw1raw", "tb1", "tw2raw", "tb2"))
        self.term = _d(d["term"])
        self.q_next_off = [_one_float_in(x) for x in self.q_next]

    def launch(self, mono, want_qtot=True, unaligned=False, hyper=None, grads=None):
        """-> (outputs by name, the guarded dq buffers of an unaligned launch)."""
        c = self.c
        N, B, A, E = c["N"], c["B"], c["A"], c["E"]
        qtot = torch.full((B,), float("nan"), device=DEV) if want_qtot else None
        out, bufs = None, []
        if unaligned or grads is not None:
            bufs, dq = zip(*[_guarded(B, A) for _ in range(N)]) if unaligned else ((), [torch.empty(B, A, device=DEV) for _ in range(N)])
            if grads is None:
                grads = tuple(torch.empty(B, w, device=DEV) for w in (N * E, E, E, 1))
            out = (list(dq), grads, torch.empty(ops.qmix_partial_elems(B, E), dtype=torch.float64, device=DEV))
        dq, grads, partial = ops.qmix_mix_td(self.q, self.q_next_off if unaligned else self.q_next, self.act, self.rew,
                                             self.hyper if hyper is None else hyper, self.hyper_next, self.term, cc.GAMMA,
                                             monotonic=bool(mono), out=out, qtot_out=qtot)
        h = {f"dq{i}": x for i, x in enumerate(dq)}
        h.update(dw1=grads[0], db1=grads[1], dw2=grads[2], db2=grads[3], partial=partial)
        if want_qtot:
            h["q_tot"] = qtot
        return h, list(bufs)


def _n(t):
    return t.cpu().numpy()


def _check_mix(p, c, d, r, h, slot, worst, mono):
    """One launch's outputs against the float64 yardstick r."""
    N, B, A, E = c["N"], c["B"], c["A"], c["E"]
    assert h["partial"].numel() == 2 * -(-B // cc.rows_per_block(E))
    dq = np.stack([_n(h[f"dq{i}"]) for i in range(N)])
    rows = np.arange(B)
    off = dq.copy()
    for i in range(N):
        off[i, rows, d["act"][i]] = 0.0
    assert not off.any(), p                       # exactly zero off the taken action
    stat = _finalized(h["partial"], B, slot)
    got = dict(dq=dq, dw1=_n(h["dw1"]), db1=_n(h["db1"]), dw2=_n(h["dw2"]), db2=_n(h["db2"]), q_tot=_n(h["q_tot"]),
               loss=[stat[0]], mean_q=[stat[1]])
    for key in cc.MIX_KEYS:
        want = r[key] if isinstance(r[key], np.ndarray) else [r[key]]
        worst[key] = max(worst.get(key, 0.0), _bar(p + key, got[key], want, r["e_ref"][key]))
    for key in ("dw1", "dw2"):                    # under an exact zero of w1raw / w2raw
        z = r["zero"][key]
        if not z.any():
            continue
        if mono:
            assert not got[key][z].any(), (p, key)   # sgn(0) = 0, as the gradient of torch.abs
            print(f"PARITY {p}{key} under {int(z.sum())} exact zeros: all 0")
        else:
            worst[key + "@0"] = max(worst.get(key + "@0", 0.0), _bar(p + key + " under exact zeros", got[key][z], r[key][z], r["e_ref"][key + "@0"]))


# ---- QMIX mix / TD ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono", cc.MIX_MONOTONIC)
@pytest.mark.parametrize("c", cc.MIX_CASES, ids=cc.case_id)
def test_mix_td(c, mono):
    m = _Mix(c)
    r = cc.mix_td_reference(c)[mono]
    N, B, A = c["N"], c["B"], c["A"]
    p = f"mix {cc.case_id(c)} mono{mono} "
    slot, worst = torch.zeros(2, device=DEV), {}
    h = {}
    for want_qtot in (1, 0):                      # q_tot asked for / not: the same bits in everything else
        h[want_qtot], _ = m.launch(mono, want_qtot)
        _same_bits(p + f"qtot{want_qtot}", h[want_qtot], m.launch(mono, want_qtot)[0])
    _same_bits(p + "qtot given / not", h[0], {k: h[1][k] for k in h[0]})
    _check_mix(p, c, m.d, r, h[1], slot, worst, mono)
    if c["offset"]:                               # every agent's q_next and dq one float past a 16-byte boundary
        u, bufs = m.launch(mono, unaligned=True)
        u2, bufs2 = m.launch(mono, unaligned=True)
        _same_bits(p + "unaligned", u, u2)
        for b in bufs + bufs2:
            assert _guards_intact(b, B * A), p
        print(f"PARITY {p}guards: {2 * N} x {2 * cc.GUARD_FLOATS + 1} floats around dq, all {cc.GUARD}")
        _check_mix(p + "unaligned ", c, m.d, r, u, slot, worst, mono)
        _same_bits(p + "unaligned against aligned", u, h[1])
    _worst(p, worst)


@pytest.mark.parametrize("c", cc.MIX_UNALIGNED[::2], ids=cc.case_id)
def test_mix_td_refuses_an_unaligned_hypernetwork_output(c):
    m = _Mix(c)
    N, B, E = c["N"], c["B"], c["E"]
    grads = tuple(torch.full((B, w), cc.GUARD, device=DEV) for w in (N * E, E, E, 1))
    hyper = (_one_float_in(m.hyper[0]),) + m.hyper[1:]
    with pytest.raises(ValueError, match="16-byte aligned"):
        m.launch(1, hyper=hyper, grads=grads)
    torch.cuda.synchronize()
    assert all(bool((g == cc.GUARD).all()) for g in grads)    # refused before any launch: dw1 and the others untouched
    h, _ = m.launch(1, grads=grads)                           # the same buffers, aligned inputs: written
    assert not bool((h["dw1"] == cc.GUARD).any())


@pytest.mark.parametrize("E", (32, 64))
def test_mix_td_out_of_range_actions(E):
    """An action outside [0, A) reads nothing, leaves that row's dq zero and poisons the loss; every other row is as it was."""
    c = next(c for c in cc.MIX_UNALIGNED if (c["E"], c["N"], c["A"], c["B"]) == (E, 3, 5, 33))   # its inputs, aligned here
    N, B, A = c["N"], c["B"], c["A"]
    clean = _Mix(c)
    act = clean.d["act"].copy()
    low, high = 5, B - 1                           # a row of the first workgroup, the only row of the last
    act[:, low], act[:, high] = -1, A
    bad = _Mix(c, act=act)
    slot = torch.zeros(2, device=DEV)
    keep = np.setdiff1d(np.arange(B), [low, high])
    for mono in cc.MIX_MONOTONIC:
        p = f"mix {cc.case_id(c)} mono{mono} out-of-range "
        h0, h1 = clean.launch(mono)[0], bad.launch(mono)[0]
        _same_bits(p, h1, bad.launch(mono)[0])
        assert np.isnan(_finalized(h1["partial"], B, slot)[0]) and np.isfinite(_finalized(h0["partial"], B, slot)).all()
        for i in range(N):
            assert not _n(h1[f"dq{i}"])[[low, high]].any(), (p, i)
        for k in h0:
            if k != "partial":
                x0, x1 = (_n(h[k]).reshape(B, -1)[keep].view(np.int32) for h in (h0, h1))
                _exact(p + k + " of the other rows (bits)", x1.reshape(-1), x0.reshape(-1))


# ---- epsilon-greedy at eps = 0 ------------------------------------------------------------------------------------------------
def test_qmix_egreedy_takes_the_first_maximum_from_unaligned_rows():
    c, d = cc.EGREEDY_CASE, cc.egreedy_inputs()
    N, A, B = c["N"], c["A"], c["B"]
    q = [_d(d["q"][i]) for i in range(N)]
    eps0 = torch.zeros(1, device=DEV)
    outs = []
    for qs in ([_one_float_in(x) for x in q], [_one_float_in(x) for x in q], q):
        out = torch.full((B + 1, N), int(cc.GUARD), dtype=torch.int32, device=DEV)    # a guard row behind row B
        ops.qmix_egreedy(qs, eps0, seed=5, out=out)
        outs.append(out.cpu().numpy())
    for tag, out in zip(("unaligned", "unaligned again", "aligned"), outs):
        _exact(f"egreedy {cc.case_id(c)} {tag}", out[:B].reshape(-1), d["act"].reshape(-1))
        assert (out[B] == int(cc.GUARD)).all(), tag


# ---- CTDE head --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.HEAD_CASES, ids=cc.case_id)
def test_ctde_td_head(c):
    d, r = cc.head_inputs(c), cc.ctde_head_reference(c)
    assert abs(r["mean_adv"]) >= cc.MIN_ABS_MEAN_ADV
    assert d["act"].min() >= 0 and d["act"].max() < c["A"]
    q, qn, rew, term, logits, act = (_d(d[k]) for k in ("q", "q_next", "rew", "term", "logits", "act"))
    run = lambda: ops.ctde_td_head(q, qn, rew, term, d["gamma"], logits, act)  # noqa: E731
    h = run()
    p = f"head {cc.case_id(c)} "
    _same_bits(p, h, run())
    dq, dl, s = (_n(x) for x in h)
    assert dq.shape == (c["B"], c["n_out"]) and dl.shape == (c["B"], c["A"])
    if c["A"] == 1:
        assert not dl.any()                       # 1 - softmax = 0 exactly
    worst = {}
    for key, got, want in (("dq", dq, r["dq"]), ("dlogits", dl, r["dlogits"]), ("actor_loss", [s[0]], [r["actor_loss"]]),
                           ("critic_loss", [s[1]], [r["critic_loss"]])):
        worst[key] = _bar(p + key, got, want, r["e_ref"][key])
    _worst(p, worst)


# ---- tsm_ctde_finalize --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.FINALIZE_CASES, ids=cc.case_id)
def test_ctde_finalize(c):
    d, r = cc.finalize_inputs(c), cc.finalize_reference(c)
    pc, pa = _d(d["pc"]), _d(d["pa"])
    assert pc.dtype == torch.float64 and pc.shape == (c["nb_c"], 4) and pa.shape == (c["nb_a"], 4)
    for kind in ("device", "pinned"):
        for rep in range(2):
            scalars = torch.full((2,), float("nan"), device=DEV) if kind == "device" else torch.full((2,), float("nan")).pin_memory()
            mean_adv = torch.full((1,), float("nan"), device=DEV)
            ops.ctde_finalize(pc, c["nb_c"], pa, c["nb_a"], c["B"], scalars, mean_adv)
            torch.cuda.synchronize()
            p = f"finalize {cc.case_id(c)} {kind} "
            _exact(p + "scalars", _n(scalars), r["scalars"])
            _exact(p + "mean_adv", _n(mean_adv), np.array([r["mean_adv"]]))


# ---- tsm_global_state ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.GLOBAL_CASES, ids=cc.case_id)
def test_global_state(c):
    obs, r = cc.global_inputs(c), cc.global_reference(c)
    N, D, B = c["N"], c["D"], c["B"]
    by_agent = [_d(obs[a]) for a in range(N)]
    for mode in ("concatenate", "mean"):
        out = ops.global_state(by_agent, mode)
        assert torch.equal(out, ops.global_state(by_agent, mode))
        assert out.dtype == torch.float32
        _exact(f"global {cc.case_id(c)} {mode}", _n(out), r[mode])
        empty = ops.global_state([x[:0] for x in by_agent], mode)
        assert tuple(empty.shape) == ((0, N * D) if mode == "concatenate" else (0, D)) and empty.dtype == torch.float32
