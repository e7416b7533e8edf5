"""GPU tests (`-m gpu`) of the three kernels of csrc/bdqn.hip at their shape limits, against the float64 restatement
(tests/bdqn_restatement.py, pinned to the reference's float64 run by tests/test_host_bdqn.py).

Shapes: B in {1, 255, 256, 257} (one row; the last row of the 16th workgroup of 16 rows, a full one, one row more) times
(K, A) in {(1, 1), (1, 64), (3, 5), (64, 2)}, and (64, 64) at B = 65: both limits at once, 16 * 64 (row, branch) pairs per
workgroup -- four trips of its 256 threads -- and a last workgroup of one row.  Every head shape runs both `is_double`, with and
without a lagged input, with and without weights, and `end` all 0, all 1 and mixed.

Bar: test_gpu_distq.py's `_bar` with e_ref = 0 (max |hip - ref64| <= 1e-5 max |ref64|); greedy and random actions bit for bit.
Inputs are drawn so that every argmax gap exceeds 1e-3 (asserted here on the CPU, in the restatement): no row is left out."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import bdqn_restatement as R  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_gpu_sampling import _ctr_dev, _exact  # noqa: E402
from test_host_sampling import COMMON, ROWS  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops

SHAPES = [(B, K, A) for B in (1, 255, 256, 257) for K, A in ((1, 1), (1, 64), (3, 5), (64, 2))] + [(65, 64, 64)]


def _d(x, dt=None):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dt or torch.float32)


def _n(t):
    return t.detach().cpu().numpy().astype(np.float64)


def gapped(rs, B, K, A):
    """f32 [B, K, A]: per (b, k) a shuffled ladder of steps 4e-3 with a jitter below 1e-3 and an offset of its own, so the top two
    entries of every row lie 3e-3 apart at least."""
    x = np.arange(A) * 4e-3 + rs.uniform(0, 1e-3, (B, K, A))
    x = np.take_along_axis(x, rs.random_sample((B, K, A)).argsort(-1), -1) + rs.standard_normal((B, K, 1))
    x = x.astype(np.float32)
    assert R.argmax_gap(x) > 1e-3
    return x


def _final(partial, n):
    out = torch.empty(2, device=DEV)
    ops.qmix_finalize(partial, n, out)
    return _n(out)


@pytest.mark.parametrize("B,K,A", SHAPES)
def test_combine_head_and_egreedy_match_the_restatement(B, K, A):
    rs = np.random.RandomState(1000 * B + 10 * K + A)
    tag = f"B={B} K={K} A={A}"
    adv, v = rs.standard_normal((K, B, A)).astype(np.float32), rs.standard_normal(B).astype(np.float32)
    a64 = adv.astype(np.float64).transpose(1, 0, 2)
    q_hip = ops.bdqn_combine(_d(adv), _d(v))
    assert tuple(q_hip.shape) == (B, K, A)
    _bar(f"combine {tag}", _n(q_hip), v.astype(np.float64)[:, None, None] + (a64 - a64.mean(2, keepdims=True)), 0.0)

    q, on, tg = rs.standard_normal((B, K, A)).astype(np.float32), gapped(rs, B, K, A), gapped(rs, B, K, A)
    act = rs.randint(0, A, (B, K)).astype(np.int32)
    rew, weight = rs.standard_normal(B).astype(np.float32), (0.5 + rs.rand(B)).astype(np.float32)
    ends = [np.zeros(B, bool), np.ones(B, bool), rs.rand(B) < 0.5]
    dq, don, dtg, dact, drew = _d(q), _d(on), _d(tg), _d(act, torch.int32), _d(rew)
    for is_double in (True, False):
        for lag in (True, False):
            for wt in (None, weight):
                for ei, end in enumerate(ends):
                    ref = R.head(q, on, tg if lag else None, act, rew, end, 0.99, wt, is_double)
                    assert ref["gap"] > 1e-3
                    h = ops.bdqn_head(dq, don, dtg if lag else None, dact, drew, _d(end, torch.uint8), 0.99,
                                      weight=None if wt is None else _d(wt), is_double=is_double)
                    t2 = f"{tag} double={is_double} lagged={lag} weight={wt is not None} end={ei}"
                    _bar(f"returns {t2}", _n(h["returns"]), ref["returns"], 0.0)
                    _bar(f"prio {t2}", _n(h["prio"]), ref["prio"], 0.0)
                    _bar(f"d_adv {t2}", _n(h["d_adv"]), ref["d_adv"], 0.0)
                    _bar(f"d_v {t2}", _n(h["d_v"]), ref["d_v"], 0.0)
                    fin = _final(h["partial"], B)
                    _bar(f"loss {t2}", fin[0], ref["loss"], 0.0)
                    _bar(f"mean taken q {t2}", fin[1], ref["q_taken"], 0.0)
    again = ops.bdqn_head(dq, don, dtg, dact, drew, _d(ends[2], torch.uint8), 0.99, weight=_d(weight), is_double=True)
    first = ops.bdqn_head(dq, don, dtg, dact, drew, _d(ends[2], torch.uint8), 0.99, weight=_d(weight), is_double=True)
    for key in ("returns", "prio", "d_adv", "d_v"):
        assert torch.equal(again[key].view(torch.int32), first[key].view(torch.int32)), key   # two runs, the same bits
    assert torch.equal(again["partial"].view(torch.int64), first["partial"].view(torch.int64))

    for eps in (0.0, 0.5, 1.0):
        got = ops.bdqn_egreedy(don, _d(np.array([eps], np.float32)), 0x1234ABCD5678, offset=2**32 - 3)
        ref, _ = R.bdqn_egreedy(on, eps, 0x1234ABCD5678, 2**32 - 3)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, K)
        _exact(f"egreedy {tag} eps {eps}", got.cpu().numpy(), ref["act"])


def test_an_action_outside_its_range_poisons_its_row_and_reads_nothing():
    B, K, A = 20, 3, 5
    rs = np.random.RandomState(3)
    q, on = rs.standard_normal((B, K, A)).astype(np.float32), gapped(rs, B, K, A)
    act = rs.randint(0, A, (B, K)).astype(np.int32)
    rew, end = rs.standard_normal(B).astype(np.float32), np.zeros(B, bool)
    good = ops.bdqn_head(_d(q), _d(on), None, _d(act, torch.int32), _d(rew), _d(end, torch.uint8), 0.99)
    act[4, 1], act[17, 2] = A, -1
    h = ops.bdqn_head(_d(q), _d(on), None, _d(act, torch.int32), _d(rew), _d(end, torch.uint8), 0.99)
    prio = _n(h["prio"])
    assert np.isnan(prio[[4, 17]]).all() and not np.isnan(np.delete(prio, [4, 17])).any()
    assert np.isnan(_final(h["partial"], B)[0]) and torch.equal(h["returns"], good["returns"])
    d_adv, d_v = _n(h["d_adv"]), _n(h["d_v"])
    assert not d_adv[1, 4].any() and not d_adv[2, 17].any() and np.isfinite(d_adv).all() and np.isfinite(d_v).all()
    keep = np.ones((K, B), bool)
    keep[1, 4] = keep[2, 17] = False
    assert np.array_equal(d_adv[keep], _n(good["d_adv"])[keep])
    ok_rows = np.delete(np.arange(B), [4, 17])
    assert np.array_equal(d_v[ok_rows], _n(good["d_v"])[ok_rows])


@pytest.mark.parametrize("K,A", [(1, 1), (5, 25), (9, 64)])
def test_bdqn_egreedy_matches_the_restatement_across_the_carry(K, A):
    rs = np.random.RandomState(K)
    for seed, off, dev in COMMON:
        for Rr in ROWS:
            q = gapped(rs, Rr, K, A)
            for eps in (0.0, 0.5, 1.0):
                got = ops.bdqn_egreedy(_d(q), _d(np.array([eps], np.float32)), seed, offset=off, offset_dev=_ctr_dev(dev))
                ref, _ = R.bdqn_egreedy(q, eps, seed, off, dev)
                _exact(f"bdqn_egreedy K{K} A{A} R{Rr} eps {eps} seed {seed:#x}", got.cpu().numpy(), ref["act"])
                if eps == 0.5 and Rr >= 255:
                    assert 0.35 < ref["random"].mean() < 0.65
