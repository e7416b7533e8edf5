"""GPU tests (`-m gpu`) of the GRU kernels (csrc/gru.hip), the dense-engine launches around them and `Recurrent(cell="gru")`
against torch's nn.GRU / nn.Linear in float64 on the CPU with autograd.  Row tile T = 16: B in {1, T-1, T, T+1, 2T+3} x L in
{1, 2, 5}; H, h0 and n_split rotate.  Bar: max |hip - ref64| <= 1e-5 max |ref64| per tensor (the LSTM tests' `_bars`)."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

from test_gpu_dense_shapes import _bars, _d, _n  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.utils.net import Recurrent

T = 16
BS, LS, HS = (1, T - 1, T, T + 1, 2 * T + 3), (1, 2, 5), (16, 64, 128)
CASES = [(B, L, HS[(i + j) % 3], (i + j) % 2 == 0, 1 + (i + 2 * j) % 2) for i, B in enumerate(BS) for j, L in enumerate(LS)]
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
_t64 = functools.partial(torch.tensor, dtype=torch.float64)


def _layer_inputs(B, L, H, given, seed):
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    k = np.float32(1.0 / np.sqrt(H))
    return dict(x=f(B, L, H), weight_ih=k * f(3 * H, H), weight_hh=k * f(3 * H, H), bias_ih=k * f(3 * H), bias_hh=k * f(3 * H),
                d_h=f(B, L, H), d_hn=f(B, H), h0=0.5 * f(B, H) if given else None)


def _layer_pairs(d, n_split):
    B, L, H = d["x"].shape
    g = {k: (None if v is None else _d(v)) for k, v in d.items()}
    proj = ops.dense_linear(g["x"].view(B * L, H), g["weight_ih"], g["bias_ih"]).view(B, L, 3 * H)
    fw = ops.gru_forward(proj, g["weight_hh"], g["bias_hh"], g["h0"])
    bw = ops.gru_backward(g["d_h"], g["weight_hh"], fw["gates"], fw["q"], fw["h_prev"], g["d_hn"], want_state_grad=True)
    o = 3 * H * H
    slabs = torch.full((n_split, 2 * o + 6 * H), float("nan"), device=DEV)   # an unwritten entry stays NaN
    dgx, dgh = bw["d_gates_x"].view(B * L, 3 * H), bw["d_gates_h"].view(B * L, 3 * H)
    ops.dense_wgrad(dgx, g["x"].view(B * L, H), slabs, n_split, 0, 2 * o)
    ops.dense_wgrad(dgh, fw["h_prev"].view(B * L, H), slabs, n_split, o, 2 * o + 3 * H)
    got = dict(h=fw["h"], h_n=fw["h_n"], d_x=ops.dense_dgrad(dgx, g["weight_ih"]).view(B, L, H), d_h0=bw["d_h0"])
    got.update(zip(NAMES, torch.split(slabs.sum(0), [o, o, 3 * H, 3 * H])))
    gru = torch.nn.GRU(H, H, 1, batch_first=True).double()
    gru.load_state_dict({f"{k}_l0": _t64(d[k]) for k in NAMES})
    x, h0 = _t64(d["x"], requires_grad=True), _t64(np.zeros((B, H)) if d["h0"] is None else d["h0"], requires_grad=True)
    h, hn = gru(x, h0[None])
    ((h * _t64(d["d_h"])).sum() + (hn[0] * _t64(d["d_hn"])).sum()).backward()
    ref = dict(h=h, h_n=hn[0], d_x=x.grad, d_h0=h0.grad, **{k: getattr(gru, f"{k}_l0").grad for k in NAMES})
    return [(_n(got[k]).reshape(ref[k].shape), ref[k].detach().numpy()) for k in ref]


@pytest.mark.parametrize("B,L,H,given,n_split", CASES, ids=[f"B{c[0]}-L{c[1]}-H{c[2]}-{'s' if c[3] else 'z'}-n{c[4]}" for c in CASES])
def test_layer_forward_backward(B, L, H, given, n_split):
    _bars(f"gru layer B={B} L={L} H={H} state={given} n_split={n_split}", _layer_pairs(_layer_inputs(B, L, H, given, 7 + B + L), n_split))


def test_saturated_gates_stay_finite():
    """Every third gate unit carries a bias of +-45 (b_ih) and +-15 (b_hh), a few +-100 (past expf's range), beside ordinary ones."""
    d = _layer_inputs(T + 1, 5, 64, True, 3)
    sign = np.where(np.arange(0, 192, 3) % 2 == 0, 1.0, -1.0).astype(np.float32)
    d["bias_ih"][::3], d["bias_hh"][::3] = 45.0 * sign, 15.0 * sign
    d["bias_ih"][1::12] = 100.0 * sign[:16]
    pre = (d["x"].astype(np.float64) @ d["weight_ih"].T.astype(np.float64) + d["bias_ih"])[..., :128] + d["bias_hh"][:128]
    assert (pre > 40.0).any() and (pre < -40.0).any()   # r and z, before the recurrent product of at most 8 / sqrt(64) in size
    _bars("gru saturated", _layer_pairs(d, 2))


class _RefNet(torch.nn.Module):
    def __init__(self, D, H, A, layers):
        super().__init__()
        self.nn, self.fc1, self.fc2 = torch.nn.GRU(H, H, layers, batch_first=True), torch.nn.Linear(D, H), torch.nn.Linear(H, A)

    def forward(self, obs, h0=None):
        y, hn = self.nn(self.fc1(obs), None if h0 is None else h0.transpose(0, 1).contiguous())
        return self.fc2(y[:, -1]), hn.transpose(0, 1)


def ref_net(net):
    sd = net.to_reference_state_dict()
    ref = _RefNet(net.obs_dim, net.hidden, net.n_out, net.layer_num).double()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    ref.load_state_dict(sd)
    return ref


@pytest.mark.parametrize("layers,H,L,B,given", [(1, 128, 5, T + 1, False), (2, 64, 2, 2 * T + 3, True), (2, 16, 1, T - 1, False)])
@pytest.mark.parametrize("n_split", [1, 2])
def test_recurrent_gru_net(layers, H, L, B, given, n_split):
    kw = dict(layer_num=layers, state_shape=6, action_shape=5, hidden_layer_size=H, device=DEV, cell="gru")
    net = Recurrent(seed=5, **kw)
    rs = np.random.RandomState(17)
    obs, r = rs.standard_normal((B, L, 6)).astype(np.float32), rs.standard_normal((B, 5)).astype(np.float32)
    h0 = 0.5 * rs.standard_normal((B, layers, H)).astype(np.float32) if given else None
    out, state = net(_d(obs), None if h0 is None else dict(hidden=_d(h0)))
    slabs = net.backward(_d(r), n_split=n_split, slabs=torch.full((n_split, net.flat.numel()), float("nan"), device=DEV))
    ref = ref_net(net)
    rout, rh = ref(_t64(obs), None if h0 is None else _t64(h0))
    (rout * _t64(r)).sum().backward()
    assert len(state) == 1 and tuple(state[0].shape) == (B, layers, H)
    pairs = [(_n(out), rout.detach().numpy()), (_n(state[0]), rh.detach().numpy())]
    pairs += [(_n(v), dict(ref.named_parameters())[k].grad.numpy()) for k, v in net.reference_named_views(slabs.sum(0))]
    _bars(f"Recurrent gru layers={layers} H={H} L={L} B={B} state={given} n_split={n_split}", pairs)
    other = Recurrent(seed=9, **kw)
    other.load_reference_state_dict(ref.state_dict())
    assert torch.equal(other.flat.data, net.flat.data)


@pytest.mark.parametrize("args,limit", [((8,), "multiple of 16"), ((24,), "multiple of 16"), ((144,), "128"), ((64, 0), "layer_num"),
                                        ((64, 1, 0), "sequence length")])
def test_gru_check_and_cell_argument_name_their_limits(args, limit):
    with pytest.raises(ValueError, match=f"gru.*{limit}"):
        ops.gru_check(*args)
    kw = dict(layer_num=2, state_shape=6, action_shape=5, hidden_layer_size=32, device=DEV, seed=4)
    with pytest.raises(ValueError, match="'lstm' or 'gru'"):
        Recurrent(cell="rnn", **kw)
    assert torch.equal(Recurrent(cell="lstm", **kw).flat.data, Recurrent(**kw).flat.data)
    assert Recurrent(cell="gru", **kw).flat.numel() == Recurrent(**kw).flat.numel() - 2 * 2 * (32 * 32 + 32)
