"""GPU tests (`-m gpu`) of csrc/bcq.hip at the smallest shapes that can break it: one transition, one sample, row counts
around the wave's, the workgroup's and the grid-stride loop's edges, the widest and the narrowest action and latent, rows that
are no multiple of 16 bytes, no second group in the decode, one and a hundred candidates per observation, exact ties in q, and
every clamp exactly on and just beyond its bound.  Reference: tests/bcq_restatement.py in float64; bar: test_gpu_distq.py's
`_bar` with e_ref = 0.  Outputs are filled with a sentinel first: exactly the documented elements are written."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import bcq_restatement as R  # noqa: E402
from test_gpu_cac import _d, _final, _n  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops

# (B, K): B K = 1, 15, 16, 17, 255, 256, 257 with B = 1 and K = 1 among them
BK_SHAPES = [(1, 1), (1, 15), (15, 1), (16, 1), (17, 1), (51, 5), (1, 256), (257, 1)]
# (D, Ad, L): Ad 1 and 64, L 1 and 128, D + L and D + Ad no multiple of 4
WIDTHS = [(1, 1, 1), (3, 64, 2), (5, 2, 128), (6, 3, 5), (2, 64, 128)]


def padded(n, w, fill=9.0):
    """A sentinel-filled [n, w] view with 8 sentinels behind it -> (view, the whole buffer)."""
    buf = torch.full((n * w + 8,), fill, device=DEV)
    return buf[:n * w].view(n, w), buf


def tail_kept(buf, n, fill=9.0) -> bool:
    return bool((buf[n:] == fill).all())


@pytest.mark.parametrize("B,K", BK_SHAPES)
def test_decode_action_rows_and_target_at_the_row_edges(B, K):
    D, Ad, L, M = 5, 2, 2, 1.5
    assert (D + L) % 4 and (D + Ad) % 4
    rs = np.random.RandomState(B * 31 + K)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    obs, nxt, z = f(B, D), f(B, D), f(B * K + B, L)
    n = B * K + B
    xd, xd_buf = padded(n, D + L)
    ops.bcq_decode_rows(_d(nxt), K, _d(obs), _d(z), out=xd)
    rxd = R.decode_rows(nxt, K, obs, z)
    assert np.array_equal(_n(xd), rxd) and tail_kept(xd_buf, n * (D + L))
    raw = np.clip(f(n, Ad), -3, 3)
    X, X_buf = padded(n, D + Ad)
    ops.bcq_action_rows(_d(raw), xd, D, M, out=X)
    _bar(f"action rows B={B} K={K}", _n(X), R.action_rows(raw, rxd, D, M), 0.0)
    assert tail_kept(X_buf, n * (D + Ad))
    q1, q2, rew, done = f(B * K), f(B * K), f(B), rs.rand(B) < 0.4
    t_buf = torch.full((B + 8,), 9.0, device=DEV)
    ops.bcq_target(_d(q1), _d(q2), _d(rew), _d(~done, torch.bool), K, 0.99, 0.75, out=t_buf[:B])
    _bar(f"target B={B} K={K}", _n(t_buf[:B]), R.target(q1, q2, rew, ~done, K, 0.99, 0.75), 0.0)
    assert tail_kept(t_buf, B)


@pytest.mark.parametrize("D,Ad,L", WIDTHS)
@pytest.mark.parametrize("B", [1, 17])
def test_every_row_kernel_at_the_width_limits(B, D, Ad, L):
    assert Ad in (1, _abi.CAC_MAX_ACT_DIM) or L in (1, 2 * _abi.CAC_MAX_ACT_DIM) or ((D + L) % 4 and (D + Ad) % 4)
    rs = np.random.RandomState(B + D + Ad + L)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    M, phi = 2.0, 0.3
    head, eps, obs, act = f(B, 2 * L), f(B, L), f(B, D), rs.uniform(-M, M, (B, Ad)).astype(np.float32)
    head[:, L:] = 2.0 * head[:, L:] - 3.0
    x, x_buf = padded(B, D + L)
    _, std = ops.bcq_latent(_d(head), _d(eps), _d(obs), out=x)
    rx, rstd = R.latent(head, eps, obs)
    _bar(f"latent rows {B, D, Ad, L}", _n(x), rx, 0.0)
    _bar(f"latent std {B, D, Ad, L}", _n(std), rstd, 0.0)
    assert tail_kept(x_buf, B * (D + L))
    raw = np.clip(f(B, Ad), -3, 3)
    d_raw, d_buf = padded(B, Ad)
    vh = ops.bcq_vae_head(_d(raw), _d(act), _d(head), M, out=d_raw)
    rv = R.vae_head(raw, act, head, M)
    _bar(f"vae d_raw {B, D, Ad, L}", _n(d_raw), rv["d_raw"], 0.0)
    _bar(f"vae_loss {B, D, Ad, L}", _final(vh["partial"], B)[0], rv["vae_loss"], 0.0)
    _bar(f"KL_loss {B, D, Ad, L}", _final(vh["partial"], B)[1], rv["kl_loss"], 0.0)
    assert tail_kept(d_buf, B * Ad) and vh["partial"].numel() == 2 * -(-B // _abi.CAC_ROWS_PER_BLOCK)
    dz = f(B, L)
    dh, dh_buf = padded(B, 2 * L)
    ops.bcq_latent_grad(_d(dz), _d(head), _d(eps), out=dh)
    _bar(f"latent d_head {B, D, Ad, L}", _n(dh), R.latent_grad(dz, head, eps), 0.0)
    assert tail_kept(dh_buf, B * 2 * L)
    x_in = np.concatenate([obs, act], 1)
    raw_p = f(B, Ad)
    xo, xo_buf = padded(B, D + Ad)
    _, factor = ops.bcq_perturb(_d(raw_p), _d(x_in), phi, M, out=xo)
    rxo, rf, _ = R.perturb(raw_p, x_in, D, phi, M)
    _bar(f"perturbed rows {B, D, Ad, L}", _n(xo), rxo, 0.0)
    _bar(f"perturb factor {B, D, Ad, L}", _n(factor), rf, 0.0)
    assert tail_kept(xo_buf, B * (D + Ad))
    assert ops.bcq_perturb(_d(raw_p), _d(x_in), phi, M, want_factor=False)[1] is None


@pytest.mark.parametrize("n,S", [(1, 1), (3, 1), (1, 100), (10, 100), (5, 64), (5, 65), (9, 3)])
def test_decode_without_a_second_group_and_select(n, S):
    D, Ad, L = 5, 2, 3
    rs = np.random.RandomState(n * 7 + S)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    obs, z = f(n, D), f(n * S, L)
    xd, xd_buf = padded(n * S, D + L)
    ops.bcq_decode_rows(_d(obs), S, None, _d(z), out=xd)   # n_b = 0: the acting path
    assert np.array_equal(_n(xd), R.decode_rows(obs, S, None, z)) and tail_kept(xd_buf, n * S * (D + L))
    rows, q = f(n * S, D + Ad), f(n * S)
    if S > 2:   # exact ties of the maximum: the first index wins, across the lanes' strides as well
        qv = q.reshape(n, S)
        qv[:, S - 1] = qv[:, S // 2] = qv.max(1) + 1.0
    act, a_buf = padded(n, Ad)
    _, index = ops.bcq_select(_d(q), _d(rows), S, D, Ad, out=act)
    ra, ri = R.select(q, rows, S, D, Ad)
    assert np.array_equal(index.cpu().numpy(), ri) and np.array_equal(_n(act), ra.astype(np.float64)) and tail_kept(a_buf, n * Ad)
    if S > 2:
        assert (ri == S // 2).all()


def test_every_clamp_on_and_just_beyond_its_bound():
    up, dn = lambda v: np.nextafter(np.float32(v), np.float32(np.inf)), lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))  # noqa: E731
    # raw log_std at exactly -4 and 15 (the gradient passes) and just beyond (zero)
    ls = np.array([[-4.0, dn(-4.0), 15.0, up(15.0), 0.0]], np.float32)
    L = ls.shape[1]
    head = np.concatenate([np.full((1, L), 0.3, np.float32), ls], 1)
    eps, dz = np.full((1, L), 0.7, np.float32), np.full((1, L), 1e-3, np.float32)
    dh = _n(ops.bcq_latent_grad(_d(dz), _d(head), _d(eps)))
    _bar("clamp d_head", dh, R.latent_grad(dz, head, eps), 0.0)
    assert (dh[0, L:] != 0.0).tolist() == [True, False, True, False, True]
    _, std = ops.bcq_latent(_d(head), _d(eps), _d(np.zeros((1, 2), np.float32)))
    assert _n(std)[0, 0] == _n(std)[0, 1] == np.float32(np.exp(-4.0)) and _n(std)[0, 2] == _n(std)[0, 3] == np.float32(np.exp(15.0))
    # normals at exactly +-0.5 and just beyond
    z = np.array([[0.5, -0.5, up(0.5), dn(-0.5), dn(0.5), 7.0]], np.float32)
    xd = _n(ops.bcq_decode_rows(_d(np.zeros((1, 1), np.float32)), 1, None, _d(z)))
    assert xd[0, 1:].tolist() == [0.5, -0.5, 0.5, -0.5, float(dn(0.5)), 0.5]
    # a perturbed action at exactly +-max_action (the factor is kept) and beyond (zero); |raw| of 20 under the tanh
    M, phi = 1.0, 0.5
    a = np.array([[0.5, -0.5, 0.75, -0.75, 0.0, 0.0]], np.float32)
    raw_p = np.array([[20.0, -20.0, 20.0, -20.0, 20.0, 0.0]], np.float32)   # tanh(20) = 1 in float64: u = +-1, +-1.25, 0.5, 0
    x_in = np.concatenate([np.zeros((1, 1), np.float32), a], 1)
    x_out, factor = ops.bcq_perturb(_d(raw_p), _d(x_in), phi, M)
    assert _n(x_out)[0, 1:].tolist() == [1.0, -1.0, 1.0, -1.0, 0.5, 0.0]
    assert bool(torch.isfinite(factor).all()) and _n(factor)[0].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, phi]   # 1 - tanh^2(20) = 0
    raw_p2 = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    x_in2 = np.concatenate([np.zeros((1, 1), np.float32), np.array([[1.0, -1.0, up(1.0), dn(-1.0), 0.0, 0.0]], np.float32)], 1)
    _, f2 = ops.bcq_perturb(_d(raw_p2), _d(x_in2), phi, M)
    assert _n(f2)[0].tolist() == [phi, phi, 0.0, 0.0, phi, phi]   # bounds included, as torch.clamp's backward
    raw = np.array([[20.0, -20.0, 0.0]], np.float32)
    X = _n(ops.bcq_action_rows(_d(raw), _d(np.zeros((1, 2), np.float32)), 1, 2.0))
    assert X[0, 1:].tolist() == [2.0, -2.0, 0.0]
    vh = ops.bcq_vae_head(_d(raw), _d(np.zeros((1, 3), np.float32)), _d(np.zeros((1, 2), np.float32)), 2.0)
    assert _n(vh["d_raw"])[0].tolist() == [0.0, 0.0, 0.0] and np.isfinite(_final(vh["partial"], 1)).all()


def test_wrappers_refuse_bad_shapes():
    z = torch.zeros(4, 3, device=DEV)
    with pytest.raises(ValueError, match=r"head must be \[4, 6\]"):
        ops.bcq_latent(torch.zeros(4, 5, device=DEV), z, torch.zeros(4, 2, device=DEV))
    with pytest.raises(ValueError, match=r"z must be \[12, 'width'\]"):
        ops.bcq_decode_rows(torch.zeros(4, 5, device=DEV), 2, torch.zeros(4, 5, device=DEV), torch.zeros(8, 3, device=DEV))
    with pytest.raises(ValueError, match="q1 must have 8 entries"):
        ops.bcq_target(torch.zeros(4, device=DEV), torch.zeros(8, device=DEV), torch.zeros(4, device=DEV),
                       torch.zeros(4, dtype=torch.bool, device=DEV), 2, 0.99, 0.75)
    with pytest.raises(ValueError, match="must not be x_in"):
        x = torch.zeros(4, 8, device=DEV)
        ops.bcq_perturb(z, x, 0.05, 1.0, out=x)
    with pytest.raises(ValueError, match="groups of 3"):
        ops.bcq_select(torch.zeros(4, device=DEV), torch.zeros(4, 8, device=DEV), 3, 5, 3)
    with pytest.raises(ValueError, match=r"latent_dim = 129 outside \[1, 128\]"):
        ops.bcq_latent(torch.zeros(2, 258, device=DEV), torch.zeros(2, 129, device=DEV), torch.zeros(2, 3, device=DEV))
