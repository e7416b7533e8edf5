"""GPU tests (`-m gpu`) of the GAIL kernels alone (csrc/gail.hip: tsm_gail_draw, tsm_gail_rows, tsm_gail_reward, tsm_gail_head,
tsm_gail_finalize) at their shape limits, against the float64 restatement (tests/gail_restatement.py, pinned to the reference by
tests/test_gail_restatement.py).

Logits sit on a lattice of eighths, exact in float32.  Bars: values rounded once from float64 (rewards, d_logits, the partial
sums, the loss): max |hip - ref64| <= 1e-5 max |ref64| per array, the project's bar; the rows (copies, zeros and ones), the
untouched bytes, the counts and accuracies' numerators, the drawn ids and a second run of the head: bit for bit."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import gail_restatement as gr  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops

    RPB = _abi.GAIL_ROWS_PER_BLOCK
else:
    RPB = gr.ROWS_PER_BLOCK
SIZES = [1, 63, 64, 65, RPB - 1, RPB, RPB + 1, 3 * RPB + 5]


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _rel(name, got, ref, bar=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), float(np.finfo(np.float32).tiny))
    ratio = float(np.abs(got - ref).max()) / (bar * scale)
    print(f"PARITY {name}: max |hip - ref64| / (1e-5 max |ref64|) = {ratio:.3g}")
    assert ratio <= 1.0, (name, ratio)


def logits_of(n, seed=0):
    rs = np.random.RandomState(100 + n + seed)
    lat = rs.randint(-96, 97, n)
    lat[lat == 0] = 3
    if n > 8:
        lat[[1, 3, 5, 7]] = (320, -320, 720, -720)   # +-40, +-90
    return (lat / 8.0).astype(np.float32)


@pytest.mark.parametrize("R", SIZES)
def test_head_and_finalize_with_the_split_on_either_side_of_a_block_edge(R):
    n = R + 1
    for Rp in sorted({1, R, max(1, min(R, RPB - 1)), max(1, min(R, RPB)), max(1, min(R, RPB + 1)), max(1, n // 2)}):
        Re = n - Rp
        lg = logits_of(n, Rp)
        h = gr.head(lg, Rp)
        o = ops.gail_head(_d(lg), Rp)
        o2 = ops.gail_head(_d(lg), Rp)
        d, part = o["d_logits"].cpu().numpy(), o["partial"].cpu().numpy().reshape(-1, 4)
        assert np.array_equal(d, o2["d_logits"].cpu().numpy()) and np.array_equal(part, o2["partial"].cpu().numpy().reshape(-1, 4))
        assert part.shape == h["partial"].shape == (-(-n // RPB), 4)
        _rel(f"R{R} Rp{Rp} d_logits", d, h["d_logits"])
        assert (d[:Rp] >= 0).all() and (d[Rp:] <= 0).all() and (d[np.abs(lg) <= 40] != 0).all()   # sigmoid(40) - 1 is not 0
        for k in (0, 1):
            if h["partial"][:, k].any():
                _rel(f"R{R} Rp{Rp} partial {k}", part[:, k], h["partial"][:, k])
            assert np.array_equal(part[:, k] == 0, h["partial"][:, k] == 0)
        assert np.array_equal(part[:, 2:], h["partial"][:, 2:])   # counts
        out = ops.gail_finalize(o["partial"], Rp, Re).cpu().numpy()
        _rel("loss", out[:1], [h["loss"]])
        assert out[1] == np.float32(h["acc_pi"]) and out[2] == np.float32(h["acc_exp"])
    assert ops.gail_finalize(_d(h["partial"]), Rp, Re).cpu().numpy()[0] == pytest.approx(h["loss"], rel=1e-6)   # 1 and several blocks


@pytest.mark.parametrize("R", SIZES)
def test_reward_with_and_without_ids(R):
    lg = logits_of(R)
    want = gr.softplus(lg)
    rs = np.random.RandomState(R)
    store0 = (rs.randint(-24, 25, 3 * R + 5) / 8.0).astype(np.float32)
    for name, ids in (("none", None), ("reversed", np.arange(R)[::-1].astype(np.int64)), ("strided", (3 * np.arange(R) + 2).astype(np.int64))):
        store = _d(store0)
        ops.gail_reward(_d(lg), store, None if ids is None else _d(ids))
        got = store.cpu().numpy()
        at = np.arange(R) if ids is None else ids
        _rel(f"R{R} reward {name}", got[at], want)
        keep = np.setdiff1d(np.arange(store0.size), at)
        assert np.array_equal(got[keep], store0[keep]), name    # an overwrite of the named entries, nothing else
    two = torch.zeros(2, device=DEV)
    ops.gail_reward(_d(np.float32([90.0, 0.0])), two)
    assert two.cpu().numpy()[0] == np.float32(90.0) and two.cpu().numpy()[1] == np.float32(np.log(2.0))


@pytest.mark.parametrize("A", [1, 2, 5, 64])
@pytest.mark.parametrize("D", [1, 18, 63, 64, 65, 513])
def test_rows_are_exact_and_leave_the_other_half_untouched(D, A):
    R, P = 67, 90
    rs = np.random.RandomState(10 * D + A)
    obs = rs.standard_normal((P, D)).astype(np.float32)
    act = rs.randint(0, A, P).astype(np.int32)
    act[[2, 11]] = (-1, A)                                       # out of range: an all-zero one-hot
    ids = rs.permutation(P)[:R].astype(np.int64)
    ids[:2] = (2, 11)
    got = ops.gail_rows(_d(obs), _d(act), A).cpu().numpy()
    assert got.shape == (P, D + A) and np.array_equal(got, gr.rows(obs, act, A)) and not got[2, D:].any() and not got[11, D:].any()
    assert np.array_equal(ops.gail_rows(_d(obs), _d(act), A, R=R).cpu().numpy(), gr.rows(obs, act, A, R=R))
    # a two-call matrix: each call writes its half, the bytes beyond stay as they were
    x = torch.full((R + 5 + 3, D + A), -7.0, device=DEV)
    ops.gail_rows(_d(obs), _d(act), A, ids=_d(ids), out=x[:R])
    after_first = x.cpu().numpy()
    assert np.array_equal(after_first[:R], gr.rows(obs, act, A, ids)) and (after_first[R:] == -7.0).all()
    ops.gail_rows(_d(obs), _d(act), A, ids=_d(ids[:5]), out=x[R:R + 5])
    both = x.cpu().numpy()
    assert np.array_equal(both[:R], after_first[:R]) and np.array_equal(both[R:R + 5], gr.rows(obs, act, A, ids[:5]))
    assert (both[R + 5:] == -7.0).all()
    # the stores' own shape [S, B, N, D] / [S, B, N] is read in place
    got4 = ops.gail_rows(_d(obs.reshape(5, 6, 3, D)), _d(act.reshape(5, 6, 3)), A, ids=_d(ids)).cpu().numpy()
    assert np.array_equal(got4, both[:R])


@pytest.mark.parametrize("n_valid,n_agent", [(1, 1), (2, 1), (1, 2), (3, 1), (7, 3), (2 ** 31 + 7, 1)])
def test_draw_matches_the_restatement_exactly(n_valid, n_agent):
    R = 300
    valid = None if n_valid > 1000 else (np.arange(n_valid, dtype=np.int64) * 5 + 2)
    for seed, counter, cdev in ((11, 0, None), (11, 2 ** 32 - 7, None), (2 ** 63 + 5, 2 ** 32 - 100, 90), (11, (3 << 32), None)):
        want, j, _ = gr.draw(valid, n_valid, n_agent, R, seed, counter, None if cdev is None else np.array([cdev], np.uint64))
        cd = None if cdev is None else torch.tensor([cdev], dtype=torch.int64, device=DEV)
        got = ops.gail_draw(None if valid is None else _d(valid), n_valid, n_agent, R, seed, counter=counter, counter_dev=cd,
                            device=DEV).cpu().numpy()
        assert np.array_equal(got, want), (seed, counter, cdev)
        assert ((j >= 0) & (j < n_valid * n_agent)).all()
    if n_valid > 1000:
        assert want.max() > 2 ** 31 - 2 ** 27 and want.max() < n_valid          # the top of the range is reached, not passed
    out = torch.full((R + 1,), -1, dtype=torch.int64, device=DEV)
    ops.gail_draw(None if valid is None else _d(valid), n_valid, n_agent, R, 11, out=out[:R])
    assert int(out[R]) == -1


def test_shapes_are_refused_before_any_launch():
    obs, act = torch.zeros(8, 3, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="n_act = 65"):
        ops.gail_rows(obs, act, 65)
    with pytest.raises(ValueError, match="one action per row"):
        ops.gail_rows(obs, act[:7], 2)
    with pytest.raises(ValueError, match="R = 9 rows asked of 8 pairs"):
        ops.gail_rows(obs, act, 2, R=9)
    with pytest.raises(ValueError, match=r"out must be \[8, 5\]"):
        ops.gail_rows(obs, act, 2, out=torch.zeros(8, 4, device=DEV))
    with pytest.raises(ValueError, match="each at least 1"):
        ops.gail_head(torch.zeros(4, device=DEV), 4)
    with pytest.raises(ValueError, match="at least 4 entries"):
        ops.gail_reward(torch.zeros(4, device=DEV), torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="ids must have 4 entries"):
        ops.gail_reward(torch.zeros(4, device=DEV), torch.zeros(9, device=DEV), ids=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gail_rows(torch.zeros(8, 3), torch.zeros(8, dtype=torch.int32), 2)
