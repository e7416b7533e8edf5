"""GPU tests (`-m gpu`) of the two LSTM kernels alone (csrc/lstm.hip: tsm_lstm_forward, tsm_lstm_backward) and of the
dense-engine launches around them (tsm_dense_linear / _dgrad / _wgrad), against the float64 restatement of
tests/recurrent_restatement.py.

Cases: the row tile is T = 16 (TSM_LSTM_ROWS_PER_BLOCK).  B in {1, T-1, T, T+1, 2T+3} x L in {1, 2, 5}: every pair; H in
{16, 64, 128} and layers in {1, 2} and h0 / c0 absent / given: every value at least once, rotated over the pairs.  One case with
pre-activations past +-40; one where d_h is non-zero at every step (every case of `test_layer_*` is: the lower-layer
path); slab sums for n_split in {1, 2}.

Bar: max |hip - ref64| <= 1e-5 max |ref64| per block (each output tensor, each parameter's gradient); the worst ratio is
printed per test."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import recurrent_restatement as rr  # noqa: E402
from test_gpu_dense_shapes import _bars  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops
    from tianshou_marl_amd.utils.net import Recurrent

T = 16
BS, LS, HS = (1, T - 1, T, T + 1, 2 * T + 3), (1, 2, 5), (16, 64, 128)
# every (B, L); H, the initial state and the slab count rotate over them
CASES = [(B, L, HS[(i + j) % 3], (i + j) % 2 == 0, 1 + (i + 2 * j) % 2) for i, B in enumerate(BS) for j, L in enumerate(LS)]


def _d(x):
    return torch.as_tensor(np.array(x, np.float32)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _layer_inputs(B, L, H, given, seed):
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    k = 1.0 / np.sqrt(H)
    d = dict(x=f(B, L, H), w_ih=k * f(4 * H, H), w_hh=k * f(4 * H, H), b_ih=k * f(4 * H), b_hh=k * f(4 * H), d_h=f(B, L, H),
             d_hn=f(B, H), d_cn=f(B, H))
    d["h0"], d["c0"] = (0.5 * f(B, H), f(B, H)) if given else (None, None)
    return {k_: (None if v is None else v.astype(np.float32)) for k_, v in d.items()}


def _run_layer(d, n_split):
    """One layer through the kernels: projection, recurrence, backward through time, the three gradient GEMMs."""
    B, L, H = d["x"].shape
    g = {k: (None if v is None else _d(v)) for k, v in d.items()}
    proj = ops.dense_linear(g["x"].view(B * L, H), g["w_ih"], g["b_ih"]).view(B, L, 4 * H)
    fw = ops.lstm_forward(proj, g["w_hh"], g["b_hh"], g["h0"], g["c0"])
    bw = ops.lstm_backward(g["d_h"], g["w_hh"], fw["gates"], fw["c"], g["c0"], g["d_hn"], g["d_cn"], want_state_grad=True)
    P = 2 * 4 * H * H + 2 * 4 * H
    slabs = torch.full((n_split, P), float("nan"), device=DEV)
    dg = bw["d_gates"].view(B * L, 4 * H)
    ops.dense_wgrad(dg, g["x"].view(B * L, H), slabs, n_split, 0, 8 * H * H)
    ops.dense_wgrad(dg, fw["h_prev"].view(B * L, H), slabs, n_split, 4 * H * H, 8 * H * H + 4 * H)
    d_x = ops.dense_dgrad(dg, g["w_ih"]).view(B, L, H)
    return fw, bw, slabs, d_x


def _ref_layer(d):
    fw = rr.lstm_layer_forward(d["x"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"], d["h0"], d["c0"])
    bw = rr.lstm_layer_backward(fw, d["w_hh"], d["d_h"], d["d_hn"], d["d_cn"])
    return fw, bw, rr.lstm_layer_grads(fw, d["x"], bw["d_gates"], d["w_ih"])


def _layer_pairs(d, n_split):
    B, L, H = d["x"].shape
    fw, bw, slabs, d_x = _run_layer(d, n_split)
    rfw, rbw, (dwi, dwh, db, rdx) = _ref_layer(d)
    g = _n(slabs).sum(0)
    assert np.isfinite(g).all()   # every slab entry was written
    o = 4 * H * H
    pairs = [(_n(fw[k]), rfw[k]) for k in ("h", "h_prev", "c", "gates", "h_n", "c_n")]
    pairs += [(_n(bw[k]), rbw[k]) for k in ("d_gates", "d_h0", "d_c0")]
    pairs += [(g[:o].reshape(4 * H, H), dwi), (g[o:2 * o].reshape(4 * H, H), dwh), (g[2 * o:2 * o + 4 * H], db),
              (g[2 * o + 4 * H:], db), (_n(d_x), rdx)]
    for got, _ in pairs:
        assert np.isfinite(got).all()
    return pairs


@pytest.mark.parametrize("B,L,H,given,n_split", CASES, ids=[f"B{c[0]}-L{c[1]}-H{c[2]}-{'s' if c[3] else 'z'}-n{c[4]}" for c in CASES])
def test_layer_forward_backward(B, L, H, given, n_split):
    _bars(f"lstm layer B={B} L={L} H={H} state={given} n_split={n_split}", _layer_pairs(_layer_inputs(B, L, H, given, 7 + B + L), n_split))


def test_every_axis_value_is_covered():
    assert {c[0] for c in CASES} == set(BS) and {c[1] for c in CASES} == set(LS) and {c[2] for c in CASES} == set(HS)
    assert {(c[0], c[1]) for c in CASES} == {(b, l) for b in BS for l in LS}
    assert {c[3] for c in CASES} == {True, False} and {c[4] for c in CASES} == {1, 2}


def test_saturated_gates_stay_finite():
    """Pre-activations past +-40: every third gate unit carries a bias of +-45 (b_ih) and +-15 (b_hh), so its sigmoid / tanh
    saturates to 0 / +-1 in float32 at every step, next to units in the ordinary range.  Everything stays finite and within
    the bar.  (The large values sit in the biases, not the weights: a pre-activation of magnitude 40 carries an absolute
    float32 rounding of 2e-6 per addition, which a saturated unit does not pass on and an unsaturated one would.)"""
    d = _layer_inputs(T + 1, 5, 64, True, 3)
    sign = np.where(np.arange(0, 256, 3) % 2 == 0, 1.0, -1.0).astype(np.float32)
    d["b_ih"][::3], d["b_hh"][::3] = 45.0 * sign, 15.0 * sign
    d["b_ih"][1::12] = 100.0 * sign[:len(d["b_ih"][1::12])]    # past expf's range (88.7): exp(-|x|) underflows, nothing overflows
    rfw = _ref_layer(d)[0]
    pre = d["x"].astype(np.float64) @ d["w_ih"].T.astype(np.float64) + d["b_ih"] + d["b_hh"]
    assert (pre > 40.0).any() and (pre < -40.0).any() and (rfw["gates"] == 1.0).any() and (rfw["gates"] < 1e-17).any()
    _bars("lstm saturated", _layer_pairs(d, 2))


@pytest.mark.parametrize("layers,H,L,B,given", [(1, 128, 5, T + 1, False), (2, 64, 2, 2 * T + 3, True), (2, 16, 1, T - 1, False)])
@pytest.mark.parametrize("n_split", [1, 2])
def test_recurrent_net_against_restatement(layers, H, L, B, given, n_split):
    """The whole net (fc1 -> layers -> fc2): with two layers the lower one receives d_h at every step."""
    D, A = 6, 5
    net = Recurrent(layer_num=layers, state_shape=D, action_shape=A, hidden_layer_size=H, device=DEV, seed=5)
    rs = np.random.RandomState(17)
    obs, r = rs.standard_normal((B, L, D)).astype(np.float32), rs.standard_normal((B, A)).astype(np.float32)
    state = (0.5 * rs.standard_normal((B, layers, H)).astype(np.float32), rs.standard_normal((B, layers, H)).astype(np.float32)) \
        if given else None
    out, (hid, cell) = net(_d(obs), None if state is None else tuple(_d(s) for s in state))
    slabs = net.backward(_d(r), n_split=n_split)
    assert tuple(slabs.shape) == (n_split, net.flat.numel())
    params = {k: _n(v) for k, v in net.reference_named_views()}
    rout, (rh, rc), saved = rr.recurrent_forward(params, obs, layers, state)
    rg = rr.recurrent_backward(params, saved, r, layers)
    got = dict(net.reference_named_views(slabs.sum(0)))
    pairs = [(_n(out), rout), (_n(hid), rh), (_n(cell), rc)] + [(_n(got[k]), rg[k]) for k in rg]
    _bars(f"Recurrent layers={layers} H={H} L={L} B={B} state={given} n_split={n_split}", pairs)


def test_lstm_check_rejects_unsupported_widths():
    for H in (136, 8):
        with pytest.raises(ValueError, match="lstm"):
            ops.lstm_check(H)
        with pytest.raises(ValueError, match="lstm"):
            ops.lstm_forward(torch.zeros(2, 1, 4 * H, device=DEV), torch.zeros(4 * H, H, device=DEV))
        z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731  (real tensors of the sizes H asks for: nothing may run on them)
        with pytest.raises(ValueError, match="lstm"):
            ops.lstm_backward(z(2, 1, H), z(4 * H, H), z(2, 1, 4 * H), z(2, 1, H))
        d_h, w, gates, c, dg = z(2, 1, H), z(4 * H, H), z(2, 1, 4 * H), z(2, 1, H), z(2, 1, 4 * H)
        with pytest.raises(ValueError, match="lstm"):   # the C entry itself, behind the wrapper's own check
            _abi.call("tsm_lstm_backward", d_h.data_ptr(), None, None, w.data_ptr(), gates.data_ptr(), c.data_ptr(), None, 0, 2,
                      1, H, dg.data_ptr(), None, None, None)


def test_state_reset_zeroes_finished_envs_only():
    E, R, layers, H = 5, 2, 2, 16
    h, c = torch.randn(E * R, layers, H, device=DEV), torch.randn(E * R, layers, H, device=DEV)
    h0, c0 = h.clone(), c.clone()
    done = torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8, device=DEV)
    ops.lstm_state_reset(h, c, done, rows_per_env=R)
    keep = (done == 0).repeat_interleave(R)
    assert torch.equal(h[keep], h0[keep]) and torch.equal(c[keep], c0[keep])
    assert not h[~keep].any() and not c[~keep].any() and (~keep).sum() == 4
