"""GPU tests (`-m gpu`) of the four kernels of csrc/gstate.hip alone, against the float64 restatement
(tests/gstate_restatement.py): tsm_attn_pool_forward / _backward and tsm_agent_pool_forward / _backward at N in {1, 2, 3, 8},
D in {4, 8, 48, 256} and B in {1, 2, R - 1, R, R + 1, 3 R + 5} with R = TSM_GSTATE_ROWS_PER_BLOCK, on inputs of a lattice that
float32 holds exactly.  The bar is the project's: max |hip - ref64| <= 1e-5 max |ref64| per array.  Every output lies between
guard floats that must stay untouched, every launch runs twice and must give the same bits.  Two softmax cases pin the
subtracted maximum: scores hundreds apart (no NaN, the zeros of float64 rounded to float32) and all-equal scores (P = 1 / N)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import gstate_restatement as R  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops

GUARD, NG = 12345.0, 64


def _rows():
    r = _abi.GSTATE_ROWS_PER_BLOCK
    return sorted({1, 2, max(r - 1, 1), r, r + 1, 3 * r + 5})


def _lattice(rs, shape, span=8, step=8.0):
    return (rs.randint(-span, span + 1, shape) / step).astype(np.float32)


def _guarded(*shape):
    """(buffer, the output inside it): NG guard floats on each side; the output starts 16-byte aligned."""
    n = int(np.prod(shape))
    buf = torch.full((NG + n + NG,), GUARD, dtype=torch.float32, device=DEV)
    return buf, buf[NG:NG + n].view(*shape)


def _intact(buf, n):
    return bool((buf[:NG] == GUARD).all()) and bool((buf[NG + n:] == GUARD).all())


def _bar(name, got, ref, tol=1e-5):
    got, ref = got.double().cpu().numpy(), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, name
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"PARITY {name}: err {err:.3g} of max |ref| {scale:.3g}")
    assert np.isfinite(got).all(), name
    assert err <= tol * scale, (name, err, scale)


def _attn(qkv, d_ctx):
    """Both attention launches through the C ABI into guarded buffers, twice -> (ctx, P, d_qkv)."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    q, dc = torch.as_tensor(qkv).to(DEV), torch.as_tensor(d_ctx).to(DEV)
    runs = []
    for _ in range(2):
        (bc, ctx), (bp, P), (bd, d_qkv) = _guarded(B, D), _guarded(B, 4, N, N), _guarded(B, N, 3 * D)
        ops.call("tsm_attn_pool_forward", ops.ptr(q), B, N, D, ctx.data_ptr(), P.data_ptr(), ops.stream_ptr())
        ops.call("tsm_attn_pool_backward", ops.ptr(dc), ops.ptr(q), P.data_ptr(), B, N, D, d_qkv.data_ptr(), ops.stream_ptr())
        torch.cuda.synchronize()
        assert _intact(bc, B * D) and _intact(bp, B * 4 * N * N) and _intact(bd, B * N * 3 * D), (B, N, D)
        assert not bool((ctx == GUARD).any()) and not bool((P == GUARD).any()) and not bool((d_qkv == GUARD).any())
        runs.append((ctx.clone(), P.clone(), d_qkv.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "a second run must give the same bits"
    # the wrappers give the same bits as the raw entry points
    ctx2, P2 = ops.attn_pool_forward(q, N)
    assert torch.equal(ctx2, runs[0][0]) and torch.equal(P2, runs[0][1])
    assert torch.equal(ops.attn_pool_backward(dc, q, P2), runs[0][2])
    return runs[0]


@pytest.mark.parametrize("D", [4, 8, 48, 256])
@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_attention_core_against_the_restatement(N, D):
    rs = np.random.RandomState(1000 * N + D)
    for B in _rows():
        qkv, d_ctx = _lattice(rs, (B, N, 3 * D)), _lattice(rs, (B, D))
        ctx, P, d_qkv = _attn(qkv, d_ctx)
        ctx_r, P_r = R.attn_core(qkv)
        _bar(f"ctx N={N} D={D} B={B}", ctx, ctx_r)
        _bar(f"P N={N} D={D} B={B}", P, P_r)
        # the backward under test reads the forward's own P; its yardstick is float64 throughout
        _bar(f"d_qkv N={N} D={D} B={B}", d_qkv, R.attn_core_backward(d_ctx, qkv, P_r))


def test_softmax_saturates_without_nan_and_with_float64s_zeros():
    """Keys whose scores lie 128 and 1024 apart: exp underflows below float32, the row maximum keeps its one."""
    N, D, B = 3, 8, 5
    rs = np.random.RandomState(7)
    qkv = _lattice(rs, (B, N, 3 * D))
    qkv[:, :, :D] = 16.0                                  # Q: every score is 16 * sum(K_h) / sqrt(2)
    qkv[:, 0, D:2 * D], qkv[:, 1, D:2 * D], qkv[:, 2, D:2 * D] = 32.0, 26.0, -16.0
    S = R.attn_scores(qkv)
    assert (S.max(-1) - S.min(-1)).min() > 90 and np.sort(S, -1)[..., -1].min() - np.sort(S, -1)[..., -2].max() > 90
    d_ctx = _lattice(rs, (B, D))
    ctx, P, d_qkv = _attn(qkv, d_ctx)
    P_r = R.attn_core(qkv)[1]
    P32 = P_r.astype(np.float32)
    assert (P32[..., 1:] == 0).all() and (P32[..., 0] == 1).all()
    np.testing.assert_array_equal(P.cpu().numpy(), P32)   # no NaN, the same zeros and ones
    np.testing.assert_array_equal(ctx.cpu().numpy(), qkv[:, 0, 2 * D:])   # the mean of N copies of V[0], exactly
    got = d_qkv.cpu().numpy()
    assert np.isfinite(got).all() and (got[:, :, :2 * D] == 0).all()   # a saturated softmax passes nothing to Q and K
    _bar("d_qkv saturated", d_qkv, R.attn_core_backward(d_ctx, qkv, P_r))


@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_equal_scores_give_the_uniform_softmax(N):
    D, B = 8, 3
    rs = np.random.RandomState(N)
    qkv = _lattice(rs, (B, N, 3 * D))
    qkv[:, :, D:2 * D] = qkv[:, :1, D:2 * D]              # every agent holds the same key
    ctx, P, _ = _attn(qkv, _lattice(rs, (B, D)))
    np.testing.assert_array_equal(P.cpu().numpy(), np.full((B, 4, N, N), np.float32(1.0) / np.float32(N)))
    _bar(f"ctx uniform N={N}", ctx, qkv[:, :, 2 * D:].astype(np.float64).mean(axis=1))


@pytest.mark.parametrize("H", [1, 5, 64, 257])
@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_agent_pool_against_the_restatement(N, H):
    rs = np.random.RandomState(100 * N + H)
    c = (rs.randint(1, 17, N) / 16.0).astype(np.float32)
    c_d = torch.as_tensor(c).to(DEV)
    for B in _rows():
        h, d = _lattice(rs, (B, N, H)), _lattice(rs, (B, H))
        h_d, d_d = torch.as_tensor(h).to(DEV), torch.as_tensor(d).to(DEV)
        for relu in (False, True):
            runs = []
            for _ in range(2):
                (bo, out), (bh, d_h) = _guarded(B, H), _guarded(B, N, H)
                ops.call("tsm_agent_pool_forward", ops.ptr(h_d), ops.ptr(c_d), B, N, H, int(relu), out.data_ptr(), ops.stream_ptr())
                ops.call("tsm_agent_pool_backward", ops.ptr(d_d), ops.ptr(c_d), ops.ptr(h_d) if relu else None, B, N, H,
                         d_h.data_ptr(), ops.stream_ptr())
                torch.cuda.synchronize()
                assert _intact(bo, B * H) and _intact(bh, B * N * H), (B, N, H)
                runs.append((out.clone(), d_h.clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
            assert torch.equal(ops.agent_pool_forward(h_d, c_d, relu=relu), runs[0][0])
            assert torch.equal(ops.agent_pool_backward(d_d, c_d, N, h_relu=h_d if relu else None), runs[0][1])
            _bar(f"pool N={N} H={H} B={B} relu={relu}", runs[0][0], R.agent_pool(h, c, relu=relu))
            # a product of two float32 lattice values: exact
            want = R.agent_pool_backward(d, c, h_relu=h if relu else None)
            np.testing.assert_array_equal(runs[0][1].cpu().numpy(), want.astype(np.float32))


def test_entry_points_name_the_limit():
    x = torch.zeros(4 * 9 * 3 * 256 + 64, device=DEV)
    p = x.data_ptr()
    for args, word in (((p, 1, 9, 8, p, p), "agents"), ((p, 1, 3, 6, p, p), "obs_dim"), ((p, 1, 3, 260, p, p), "obs_dim"),
                       ((p, 0, 3, 8, p, p), "rows"), ((None, 1, 3, 8, p, p), "null"), ((p + 4, 1, 3, 8, p, p), "aligned")):
        with pytest.raises(ValueError, match=word):
            ops.call("tsm_attn_pool_forward", *args, ops.stream_ptr())
    with pytest.raises(ValueError, match="at least 1"):
        ops.call("tsm_agent_pool_forward", p, p, 1, 3, 0, 0, p, ops.stream_ptr())
    with pytest.raises(ValueError, match="agents"):
        ops.call("tsm_agent_pool_backward", p, p, None, 1, 9, 4, p, ops.stream_ptr())
