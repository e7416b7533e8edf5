"""GPU tests (`-m gpu`) of the kernels of csrc/rainbow.hip on their own, at the shapes where they can go wrong: tsm_noisy_compose
and tsm_noisy_grad at layers (6, 32), (32, 255), (1, 1), (33, 7); tsm_noisy_sample on a net of 4096+ slots (moments, keys,
counters, and the normals against a float64 restatement of Philox + Box-Muller); tsm_dueling_combine and its backward at
(A, N) = (1, 2), (3, 51), (5, 51), (2, 200); tsm_dueling_features and its backward.

Bars: bit-for-bit where the kernel only copies, adds zero or repeats itself; otherwise test_gpu_distq.py's `_bar`,
max |hip - ref64| <= 1e-5 max |ref64| + e_ref, with e_ref the float32-against-float64 difference of the restatement itself where
it has a float32 form (the draw) and 0 elsewhere; the moment bounds of the draw are 7 standard errors of each sample mean."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

from rainbow_restatement import (compose, dueling_combine, dueling_combine_backward, noise_of, noisy_grad,  # noqa: E402
                                 philox_normals, split_flat)
from test_gpu_distq import _bar  # noqa: E402
from test_gpu_dqn import _d  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.utils.net import FlatAdam, RainbowNet

LAYERS = [(6, 32), (32, 255), (1, 1), (33, 7)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _flat(rs, layers):
    """A flat vector for `layers` = [(in, out, noisy)] with every block filled, the noise as the reference forms it."""
    P = sum(2 * i * o + 3 * o + i if z else i * o + o for i, o, z in layers)
    flat = rs.standard_normal(P)
    for v in split_flat(flat, layers):
        for k in ("eps_p", "eps_q"):
            if k in v:
                v[k][...] = np.sign(v[k]) * np.sqrt(np.abs(v[k]))
    return flat.astype(np.float32)


# ---- compose and the gradient map ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_split", [1, 3])
def test_compose_and_gradient_map_match_the_restatement(n_split):
    rs = np.random.RandomState(31)
    # each shape as a noisy layer on its own (one layer, several workgroups or a ragged single one), then all in one table with a
    # plain layer between them (blockIdx.y picks the layer; the widest sets the grid)
    tables = [[(i, o, 1)] for i, o in LAYERS] + [[(6, 32, 1), (32, 255, 1), (1, 1, 1), (33, 7, 0), (33, 7, 1)]]
    for layers in tables:
        layers_b = [(i, o, bool(z)) for i, o, z in layers]
        t = ops.noisy_net_table(layers)
        flat = _flat(rs, layers_b)
        eg = rs.standard_normal((n_split, t.P_eff)).astype(np.float32)
        fd, egd = _d(flat), _d(eg)
        for training in (True, False):
            eff = ops.noisy_compose(t, fd, training)
            _bar(f"compose {layers} train={training}", eff.cpu().numpy(), compose(flat, layers_b, training), 0.0)
            slabs = ops.noisy_grad(t, fd, egd, training)
            assert slabs.shape == (n_split, t.P)
            for s in range(n_split):
                ref = noisy_grad(flat, layers_b, eg[s].astype(np.float64), training)
                _bar(f"grad map {layers} train={training} slab {s}", slabs[s].cpu().numpy(), ref, 0.0)
                got = slabs[s].cpu().numpy()
                for v in split_flat(got, layers_b):
                    if "mu_W" in v:    # the mu blocks are the effective slab bit for bit, the noise slots +0.0 bit for bit
                        assert not v["eps_p"].view(np.int32).any() and not v["eps_q"].view(np.int32).any()
                        assert training or not (v["sigma_W"].view(np.int32).any() or v["sigma_bias"].view(np.int32).any())
                mu_of_slab = compose(got.astype(np.float64), layers_b, False).astype(np.float32)
                assert np.array_equal(mu_of_slab.view(np.int32), eg[s].view(np.int32))
            if not training:     # eval mode: mu bit for bit
                assert np.array_equal(eff.cpu().numpy().view(np.int32), compose(flat, layers_b, False).astype(np.float32).view(np.int32))
        # all eps = 0: the composed vector is mu bit for bit, the sigma slabs are exactly 0
        z = flat.copy()
        for v in split_flat(z, layers_b):
            for k in ("eps_p", "eps_q"):
                if k in v:
                    v[k][...] = 0.0
        eff0 = ops.noisy_compose(t, _d(z), True).cpu().numpy()
        assert np.array_equal(eff0.view(np.int32), compose(z, layers_b, False).astype(np.float32).view(np.int32))
        s0 = ops.noisy_grad(t, _d(z), egd, True).cpu().numpy()
        for s in range(n_split):
            for v in split_flat(s0[s], layers_b):
                if "sigma_W" in v:
                    assert not v["sigma_W"].any() and not v["sigma_bias"].any()
            assert np.array_equal(compose(s0[s].astype(np.float64), layers_b, False).astype(np.float32).view(np.int32), eg[s].view(np.int32))
        a, b = ops.noisy_grad(t, fd, egd, True), ops.noisy_grad(t, fd, egd, True)
        assert torch.equal(_bits(a), _bits(b))


def test_adam_step_leaves_the_noise_bits_alone():
    net = RainbowNet(6, (32,), 3, 7, q_hidden=(33,), device=DEV, seed=2)
    net.sample(5)
    x = _d(np.random.RandomState(0).standard_normal((37, 6)).astype(np.float32))
    slabs = net.backward(net.forward(x) * 0 + 1.0, 3)
    before, w_before = net.noise().clone(), net.flat.data.clone()
    FlatAdam(net, lr=1e-2).step(slabs)
    assert torch.equal(_bits(net.noise()), _bits(before)) and bool(before.any())
    moved = net.flat.data != w_before
    assert bool(moved.any()) and int(moved.sum()) <= net.flat.numel() - net.n_slots


# ---- the draw -------------------------------------------------------------------------------------------------------------
def test_draw_has_the_reference_distribution_and_follows_its_key():
    net = RainbowNet(64, (1024,), 4, 8, q_hidden=(1024,), v_hidden=(999,), device=DEV, seed=0)
    n = net.n_slots
    assert n >= 4096 and n % 4 != 0          # the last Philox block is ragged
    layers = [(int(i), int(o), bool(z)) for i, o, z in net._layers]
    seed = 0x1234ABCD5678
    net.flat.data.zero_()
    net.sample(seed, offset=11)
    g = net.noise().double().cpu().numpy()
    assert np.isfinite(g).all()
    m1, m2, m4 = abs(g.mean()), abs((g ** 2).mean() - 0.79788), abs((g ** 4).mean() - 1.0)
    print(f"PARITY draw moments over {n} slots: |mean| {m1:.3g} / {7 * np.sqrt(0.79788 / n):.3g}, |mean g^2 - E|x|| {m2:.3g} / "
          f"{7 * np.sqrt(0.36338 / n):.3g}, |mean g^4 - 1| {m4:.3g} / {7 * np.sqrt(2 / n):.3g}")
    assert m1 <= 7 * np.sqrt(0.79788 / n) and m2 <= 7 * np.sqrt(0.36338 / n) and m4 <= 7 * np.sqrt(2.0 / n)
    assert (g > 0).any() and (g < 0).any()
    # only the noise slots were written
    rest = net.flat.data.double().cpu().numpy().copy()
    assert np.count_nonzero(rest) == np.count_nonzero(noise_of(rest, layers)) == np.count_nonzero(g)
    first = net.noise().clone()
    net.sample(seed, offset=11)
    assert torch.equal(_bits(net.noise()), _bits(first))                   # the same key gives the same bits
    net.sample(seed + 1, offset=11)
    assert not torch.equal(net.noise(), first)                             # another seed ...
    net.sample(seed, offset=12)
    assert not torch.equal(net.noise(), first)                             # ... or counter gives other numbers
    net.sample(seed, offset=4, offset_dev=torch.tensor([7], dtype=torch.int64, device=DEV))
    assert torch.equal(_bits(net.noise()), _bits(first))                   # host offset + device counter = the summed offset
    # the recovered normals against the float64 restatement of Philox + Box-Muller
    z64 = philox_normals(seed, 11, n)
    e_ref = float(np.abs(z64 - philox_normals(seed, 11, n, np.float32)).max())
    gf = first.double().cpu().numpy()
    _bar("draw: sign(g) g^2 against Philox + Box-Muller in float64", np.sign(gf) * gf ** 2, z64, e_ref)


# ---- the dueling streams ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N", [(1, 2), (3, 51), (5, 51), (2, 200)])
def test_dueling_combine_and_backward_match_the_restatement(A, N):
    rs = np.random.RandomState(A * 1000 + N)
    R = 37
    q, v, d = (rs.standard_normal(s).astype(np.float32) for s in ((R, A * N), (R, N), (R, A * N)))
    out = ops.dueling_combine(_d(q), _d(v), A, N)
    d_q, d_v = ops.dueling_combine_backward(_d(d), A, N)
    assert out.shape == (R, A * N) and d_q.shape == (R, A * N) and d_v.shape == (R, N)
    _bar(f"combine A{A} N{N}", out.cpu().numpy(), dueling_combine(q, v, A, N), 0.0)
    rq, rv = dueling_combine_backward(d, A, N)
    _bar(f"combine backward d_q A{A} N{N}", d_q.cpu().numpy(), rq, 0.0)
    _bar(f"combine backward d_v A{A} N{N}", d_v.cpu().numpy(), rv, 0.0)
    if A == 1:
        assert torch.equal(_bits(out), _bits(_d(v))) and not d_q.any() and torch.equal(_bits(d_v), _bits(_d(d)))
    out2 = ops.dueling_combine(_d(q), _d(v), A, N)
    q2, v2 = ops.dueling_combine_backward(_d(d), A, N)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(d_q), _bits(q2)) and torch.equal(_bits(d_v), _bits(v2))


def test_dueling_features_and_backward():
    rs = np.random.RandomState(3)
    z = rs.standard_normal((37, 33)).astype(np.float32)
    z[0, :4] = [0.0, -0.0, 1e-30, -1e-30]
    a, b = rs.standard_normal((37, 33)).astype(np.float32), rs.standard_normal((37, 33)).astype(np.float32)
    f = ops.dueling_features(_d(z)).cpu().numpy()
    assert np.array_equal(f, np.maximum(z, 0.0))
    dz = ops.dueling_features_backward(_d(z), _d(a), _d(b)).cpu().numpy()
    assert np.array_equal(dz, np.where(z > 0, a + b, np.float32(0.0))) and not dz[0, :2].any()
    assert not dz[z <= 0].view(np.int32).any()           # structural zeros are +0.0
