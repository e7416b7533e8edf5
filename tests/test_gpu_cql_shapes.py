"""GPU tests (`-m gpu`) of csrc/cql.hip at the smallest shapes that can break it: one transition, flat-index counts around
the row loops' and the workgroup's edges, the widest and the narrowest action, rows that are no multiple of 16 bytes, values
where a log-sum-exp without the subtracted maximum overflows in float32, the calibration max on either side of every value,
the multiplier on both ends of its clamp, and no multiplier.  Reference: tests/cql_restatement.py in float64; bar:
test_gpu_distq.py's `_bar` with e_ref = 0.  Outputs are filled with a sentinel first: exactly the documented elements are
written."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import cql_restatement as R  # noqa: E402
from test_gpu_cac import _d, _final, _n  # noqa: E402
from test_gpu_cql import head_inputs, run_head  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops

# B R = 1, 15, 16, 17, 33 (the issue's), 3 x 10, and the workgroup's own edge TSM_CQL_ROWS_PER_BLOCK = 256: 255, 256, 257, 514
BR_SHAPES = [(1, 1), (15, 1), (16, 1), (17, 1), (11, 3), (3, 10), (255, 1), (64, 4), (257, 1), (257, 2)]


@pytest.mark.parametrize("B,Rn", BR_SHAPES)
def test_head_at_the_block_edges(B, Rn):
    assert _abi.CQL_ROWS_PER_BLOCK == 256
    d = head_inputs(B, Rn, seed=B * 31 + Rn)
    ch, _, _ = run_head(d, Rn, 3, calib=True, la=0.2, T=0.5, w=0.8, thr=0.3, step=True, tag=f"B={B} R={Rn} ")
    assert ch["partial"].numel() == 6 * -(-B * Rn // 256) and ch["dq1"].numel() == B + 3 * B * Rn


def test_head_log_sum_exp_near_the_float32_overflow():
    """|v / T| near 80: exp(80) overflows nothing in float64 but exp(v / T) without the subtracted maximum would in float32."""
    B, Rn, T = 17, 3, 0.5
    d = head_inputs(B, Rn, seed=2, scale=1.0)
    for k in ("q1", "q2"):
        d[k][B:] = (d[k][B:] * 2.0 + 40.0 * np.sign(d[k][B:])).astype(np.float32)   # v / T within about +-(80 +- 8)
    ch, got, _ = run_head(d, Rn, 3, calib=False, la=None, T=T, tag="near 80 ")
    assert np.isfinite(got[:2]).all() and bool(torch.isfinite(ch["dq1"]).all())


@pytest.mark.parametrize("where", ["above", "below"])
def test_head_calibration_on_either_side_of_every_value(where):
    B, Rn = 5, 3
    d = head_inputs(B, Rn, seed=3)
    d["calib"][:] = 50.0 if where == "above" else -50.0
    ch, _, rh = run_head(d, Rn, 2, calib=True, la=0.1, tag=f"calib {where} ")
    cons = _n(ch["dq1"])[B:]
    assert (cons == 0.0).all() if where == "above" else (cons > 0.0).all()
    if where == "below":   # the same numbers as without calibration
        ch0, _, _ = run_head(d, Rn, 2, calib=False, la=0.1, tag="calib absent ")
        assert torch.equal(ch0["dq1"], ch["dq1"]) and torch.equal(ch0["dq2"], ch["dq2"])


@pytest.mark.parametrize("la,amin,amax", [(-3.0, 0.5, 2.0), (3.0, 0.5, 2.0), (0.0, 1.0, 1.0)])
def test_multiplier_on_both_ends_of_its_clamp(la, amin, amax):
    d = head_inputs(7, 2, seed=4)
    _, got, _ = run_head(d, 2, 3, calib=True, la=la, amin=amin, amax=amax, thr=0.2, step=True, tag=f"clamp la={la} ")
    assert got[2] == (amin if la < 0 else amax)
    if la != 0.0:   # the clamp is active: no gradient, and Adam's step of a zero gradient moves nothing
        assert got[4] == 0.0 and got[5] == np.float32(la)
    else:           # exp(0) = 1 sits on both ends: torch.clamp's backward passes there
        assert got[4] != 0.0 and got[5] != 0.0


@pytest.mark.parametrize("B,Rn,D,Ad", [(1, 1, 1, 1), (3, 10, 5, 2), (2, 3, 3, 64), (17, 2, 6, 3)])
def test_rows_at_odd_widths(B, Rn, D, Ad):
    """D + Ad in {2, 7, 67, 9}: no row starts on a 16-byte boundary but the first."""
    assert Ad in (1, _abi.CAC_MAX_ACT_DIM) or (D + Ad) % 4
    rs = np.random.RandomState(B)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    obs, nxt, act, ra = f(B, D), f(B, D), f(B, Ad), f(B * Rn, Ad)
    n, W = B + 3 * B * Rn, D + Ad
    Xp = torch.full((n * W + 8,), 9.0, device=DEV)
    Ap = torch.full((2 * B * Rn * D + 8,), 9.0, device=DEV)
    X, A = Xp[:n * W].view(n, W), Ap[:2 * B * Rn * D].view(2 * B * Rn, D)
    ops.cql_rows(_d(obs), _d(nxt), _d(act), _d(ra), Rn, out=X, actor_rows=A)
    rx, ra_ = R.rows(obs, nxt, act, ra, Rn)
    hole = np.isnan(rx)
    assert np.array_equal(_n(X)[~hole], rx[~hole]) and (_n(X)[hole] == 9.0).all() and np.array_equal(_n(A), ra_)
    assert bool((Xp[n * W:] == 9.0).all()) and bool((Ap[2 * B * Rn * D:] == 9.0).all())
    # tsm_sac_action then fills exactly the holes
    raw = _d(f(2 * B * Rn, 2 * Ad) * 0.5)
    ops.sac_action(raw, _d(f(2 * B * Rn, Ad)), out=X[B + B * Rn:], col0=D)
    assert not bool((X == 9.0).any())


@pytest.mark.parametrize("B,Ad", [(1, 1), (1, 64), (17, 3), (17, 64), (33, 5)])
def test_td3bc_actor_head_shapes_and_mixed_signs(B, Ad):
    rs = np.random.RandomState(B + Ad)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    D, M = 3, 2.0
    g1, raw, a_data = f(B, Ad), np.clip(f(B, Ad), -3, 3), rs.uniform(-1, 1, (B, Ad)).astype(np.float32)
    q = f(B) if B == 1 else (np.abs(f(B)) * np.where(np.arange(B) % 2, -1.0, 1.0)).astype(np.float32)   # mixed sign
    rows = torch.full((B, D + Ad), 9.0, device=DEV)
    _, omt2 = ops.cac_det_action(_d(raw), M, out=rows, col0=D, want_backward=True)
    pad = torch.full((B * Ad + 8,), 9.0, device=DEV)
    ah = ops.td3bc_actor_head(_d(g1), omt2, _d(q), rows[:, D:], _d(a_data), 2.5, M, out=pad[:B * Ad].view(B, Ad))
    ref = R.td3bc_actor_head(g1, _n(omt2), q, _n(rows[:, D:]), a_data, 2.5, M)
    _bar(f"td3bc d_raw B={B} Ad={Ad}", _n(ah["d_raw"]), ref["d_raw"], 0.0)
    _bar(f"td3bc actor_loss B={B} Ad={Ad}", _final(ah["partial"], B)[0], ref["loss"], 0.0)
    assert bool((pad[B * Ad:] == 9.0).all()) and bool((rows[:, :D] == 9.0).all())
    assert ah["partial"].numel() == 2 * -(-B // _abi.CAC_ROWS_PER_BLOCK)


def test_wrappers_refuse_bad_shapes():
    z = torch.zeros(4, 3, device=DEV)
    with pytest.raises(ValueError, match=r"rand_act \[8, 3\]"):
        ops.cql_rows(torch.zeros(4, 5, device=DEV), torch.zeros(4, 5, device=DEV), z, z, 2)
    with pytest.raises(ValueError, match="q1 must have 28 entries"):
        ops.cql_head(torch.zeros(16, device=DEV), torch.zeros(28, device=DEV), torch.zeros(4, device=DEV), torch.zeros(8, device=DEV),
                     torch.zeros(8, device=DEV), 2, 3)
    with pytest.raises(ValueError, match="six sums"):
        ops.cql_finalize(torch.zeros(5, dtype=torch.float64, device=DEV), 4, 1, torch.zeros(6, device=DEV))
    with pytest.raises(ValueError, match="come together"):
        ops.cql_finalize(torch.zeros(6, dtype=torch.float64, device=DEV), 4, 1, torch.zeros(6, device=DEV), log_alpha=torch.zeros(1, device=DEV),
                         exp_avg=torch.zeros(1, device=DEV))
    with pytest.raises(ValueError, match=r"interval \[2, 1\] is empty"):
        ops.cql_uniform(4, 2.0, 1.0, 0, device=DEV)
