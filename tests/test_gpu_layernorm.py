"""GPU tests (`-m gpu`) of the LayerNorm MLPs (csrc/layernorm.hip behind `FlatMLP(norm="layer")`): forward, gradient slabs and
input gradient against torch float64 autograd on the CPU over a hand-built nn.Sequential (Linear, LayerNorm(eps), activation,
..., Linear) that holds the float32 parameters.

Bar: max |hip - ref64| <= 1e-5 max |ref64| (test_gpu_distq.py's `_bar`, e_ref = 0) per block: each layer's activations, each
dW_l, db_l, dgamma_l, dbeta_l of the summed slabs, the input gradient and a column window of it.  The inputs are conditioned on
the float64 side only: every pre-norm row has |mu| / sigma <= 4 and, outside the eps case, var >= 100 eps, so that the GEMM's
f32 rounding is not amplified by the normalisation; ReLU cases take the first seed whose pre-activations stay 1e-4 off the kink.

Measured on an MI355X with f32 row statistics (worst ratio to the bar over the cases): activations 0.075 (cap), slabs summed
0.044 (aligned), input gradient 0.073 (cap), its window 0.098 (cap); the file takes under 2 s."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DEV, NAN = "cuda", float("nan")

from dense_cases import slab_rows  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_host_dqn import _Discrete  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops
    from tianshou_marl_amd.algorithm.dqn import DQN, DiscreteQLearningPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data import Batch
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.utils.net import (ContinuousActorProbabilistic, ContinuousCritic, FlatMLP, IntrinsicCuriosityModule, lagged_copy,
                                             ref_layer_keys)

    CAP = _abi.LN_MAX_WIDTH
else:
    CAP = 512

# (dims, act, B, n_split, eps, scale of W and b): each the smallest case that reaches its branch
CASES = {
    "one_row": ([3, 5, 2], "tanh", 1, 1, 1e-5, 1.0),             # width below one MFMA tile, one row
    "tile_edges": ([20, 17, 65, 4], "relu", 17, 3, 1e-5, 1.0),   # fast-then-guarded k, a one-row slab and an empty slab
    "aligned": ([16, 64, 64, 1], "relu", 65, 1, 1e-5, 1.0),      # all-aligned interior, ragged row tile
    "ragged": ([9, 130, 2], "tanh", 15, 2, 1e-5, 1.0),           # ragged widths and rows
    "cap": ([8, CAP, 3], "tanh", 16, 2, 1e-5, 1.0),              # the width cap
    "no_act": ([7, 5, 3], "none", 17, 1, 1e-5, 1.0),
    "eps": ([16, 64, 4], "tanh", 33, 1, 1e-2, 0.17),             # row variances of eps's order
}
ACT = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh}


def _sequential(dims, act, eps):
    mods = []
    for k, o in zip(dims[:-2], dims[1:-1]):
        mods += [torch.nn.Linear(k, o), torch.nn.LayerNorm(o, eps=eps)] + ([ACT[act]()] if act != "none" else [])
    return torch.nn.Sequential(*mods, torch.nn.Linear(dims[-2], dims[-1]))


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    """f32 parameters and inputs of a case and their float64 reference: the first seed that meets the module docstring's conditions."""
    dims, act, B, _, eps, scale = CASES[cid]
    for seed in range(64):
        g = torch.Generator().manual_seed(seed)
        seq = _sequential(dims, act, eps)
        for m in seq:
            if isinstance(m, torch.nn.Linear):
                m.weight.data = (torch.rand(m.weight.shape, generator=g) * 2 - 1) * scale / m.in_features**0.5
                m.bias.data = (torch.rand(m.bias.shape, generator=g) * 2 - 1) * scale / m.in_features**0.5
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.data = 1 + 0.3 * torch.randn(m.weight.shape, generator=g)
                m.bias.data = 0.3 * torch.randn(m.bias.shape, generator=g)
        x, d_out = torch.randn(B, dims[0], generator=g), torch.randn(B, dims[-1], generator=g)
        flat = torch.cat([p.data.reshape(-1) for p in seq.parameters()])
        seq = seq.double()
        x64 = x.double().requires_grad_()
        h, acts, ok = x64, [], True
        for m in seq:
            norm = isinstance(m, torch.nn.LayerNorm)
            if norm:   # h is the pre-norm row y
                mu, var = h.mean(1), h.var(1, unbiased=False)
                lo, hi = (0.1 * eps, 10 * eps) if cid == "eps" else (100 * eps, float("inf"))
                ok &= bool((mu.abs() <= 4 * var.sqrt()).all()) and bool((var >= lo).all()) and bool((var <= hi).all())
            h = m(h)
            if norm and act == "relu":
                ok &= bool((h.abs() >= 1e-4).all())
            if isinstance(m, tuple(ACT.values())) or (norm and act == "none"):
                acts.append(h.detach().numpy())
        if not ok:
            continue
        (h * d_out.double()).sum().backward()
        return dict(flat=flat, x=x, d_out=d_out, acts=acts + [h.detach().numpy()], dx=x64.grad.numpy(),
                    grads=[(k, p.grad.numpy()) for k, p in seq.named_parameters()])
    raise AssertionError(f"{cid}: no seed in 64 meets the conditions on the inputs")


def _run(cid, B=None):
    """Forward, slabs, input gradient and a window of it through ops; every output buffer starts as NaN."""
    dims, act, _, n_split, eps, _ = CASES[cid]
    r = _inputs(cid)
    B = CASES[cid][2] if B is None else B
    desc, params, x, d_out = ops.mlp_desc(dims, act), r["flat"].to(DEV), r["x"][:B].to(DEV), r["d_out"][:B].to(DEV)
    assert ops.mlp_ln_param_count(desc) == params.numel()
    acts = torch.full((B * sum(dims[1:]),), NAN, device=DEV)
    saved = torch.full((ops.mlp_ln_save_elems(desc, B),), NAN, device=DEV)
    out, acts, saved = ops.mlp_ln_forward(desc, eps, params, x, acts=acts, saved=saved)
    slabs = ops.mlp_ln_backward(desc, params, x, acts, saved, d_out, n_split, slabs=torch.full((n_split, params.numel()), NAN, device=DEV))
    dx = ops.mlp_ln_input_grad(desc, params, x, acts, saved, d_out, 0, dims[0], out=torch.full((B, dims[0]), NAN, device=DEV))
    c0, nc = 1, max(1, dims[0] // 2)
    win = ops.mlp_ln_input_grad(desc, params, x, acts, saved, d_out, c0, nc, out=torch.full((B, nc), NAN, device=DEV))
    return dict(out=out, acts=acts, saved=saved, slabs=slabs, dx=dx, win=win, c0=c0)


_first = functools.lru_cache(maxsize=None)(_run)


@pytest.mark.parametrize("cid", CASES)
def test_forward_slabs_and_input_gradient_meet_float64_block_by_block(cid):
    dims, _, B, n_split, _, _ = CASES[cid]
    r, g = _inputs(cid), _first(cid)
    o = 0
    for l, ref in enumerate(r["acts"]):
        _bar(f"{cid} activations {l}", g["acts"][o:o + ref.size].view(ref.shape).cpu().numpy(), ref, 0.0)
        o += ref.size
    assert o == g["acts"].numel() and bool(torch.isfinite(g["saved"]).all())
    assert bool(torch.isfinite(g["slabs"]).all()), "an entry of a slab was not written"
    for s, (r0, r1) in enumerate(slab_rows(B, n_split)):
        if r0 == r1:   # a slab without rows is written all the same, as +0.0
            assert not bool(g["slabs"][s].view(torch.int32).any()), (cid, s)
    total, o = g["slabs"].double().sum(0).cpu().numpy(), 0
    for name, ref in r["grads"]:
        _bar(f"{cid} slabs summed {name}", total[o:o + ref.size].reshape(ref.shape), ref, 0.0)
        o += ref.size
    dx = r["dx"]
    _bar(f"{cid} input gradient", g["dx"].cpu().numpy(), dx, 0.0)
    _bar(f"{cid} input gradient window", g["win"].cpu().numpy(), dx[:, g["c0"]:g["c0"] + g["win"].shape[1]], 0.0)


@pytest.mark.parametrize("cid", ["tile_edges", "cap"])
def test_two_runs_give_the_same_bits_and_rows_do_not_depend_on_the_batch(cid):
    a, b = _first(cid), _run(cid)
    for k in ("acts", "saved", "slabs", "dx", "win"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (cid, k)
    dims, B = CASES[cid][0], CASES[cid][2]
    fewer, o, o1 = _run(cid, B - 1), 0, 0
    for w in dims[1:]:   # the first B - 1 rows of every layer's block keep their bits without the last row
        full = a["acts"][o:o + B * w].view(B, w)[:B - 1]
        assert torch.equal(full.view(torch.int32), fewer["acts"][o1:o1 + (B - 1) * w].view(B - 1, w).view(torch.int32)), (cid, w)
        o, o1 = o + B * w, o1 + (B - 1) * w


def test_boundaries_refuse_by_name_before_any_launch_and_no_norm_is_the_dense_path():
    with pytest.raises(ValueError, match=f"{CAP + 1} wide.*up to {CAP}"):
        FlatMLP([4, CAP + 1, 2], device=DEV, norm="layer")
    with pytest.raises(ValueError, match="norm='batch' is not supported"):
        FlatMLP([4, 8, 2], device=DEV, norm="batch")
    with pytest.raises(NotImplementedError, match="no plain tsm_mlp_desc"):
        FlatMLP([4, 8, 2], device=DEV, norm="layer").desc
    net = FlatMLP([20, 17, 65, 4], "relu", device=DEV, seed=3, norm=None)
    x, d_out = torch.randn(17, 20, device=DEV), torch.randn(17, 4, device=DEV)
    out, acts = ops.mlp_forward(net.desc, net.flat.data, x)
    slabs = ops.mlp_backward(net.desc, net.flat.data, x, acts, d_out, 3)
    assert torch.equal(net(x).view(torch.int32), out.view(torch.int32))
    assert torch.equal(net.backward(d_out, 3).view(torch.int32), slabs.view(torch.int32))


def _reference_module(kind, dims, act, eps):
    """The torch module whose `state_dict()` a net of `kind` must fill: a bare Sequential, or the reference's nesting of it under a
    critic (`preprocess.model.model` + `last.model`) or a probabilistic actor (`sigma_param`, then the trunk, then `mu.model`)."""
    seq = _sequential(dims, act, eps)
    if kind == "seq":
        return seq
    m, m.preprocess, last = torch.nn.Module(), torch.nn.Module(), torch.nn.Module()
    if kind == "prob":
        m.sigma_param = torch.nn.Parameter(torch.zeros(dims[-1], 1))
    m.preprocess.model = torch.nn.Module()
    m.preprocess.model.model, last.model = seq[:-1], torch.nn.Sequential(seq[-1])
    setattr(m, "mu" if kind == "prob" else "last", last)
    return m


@pytest.mark.parametrize("kind,act", [("seq", "relu"), ("seq", "none"), ("head", "tanh"), ("prob", "relu")])
def test_checkpoint_round_trips_under_the_reference_keys(kind, act):
    class Seq(FlatMLP):
        ref_scheme = "seq"

    eps, kw = 1e-3, dict(act=act, device=DEV, norm="layer", norm_eps=1e-3)
    make = {"seq": lambda seed: Seq([20, 17, 65, 4], seed=seed, **kw), "head": lambda seed: ContinuousCritic(15, 5, (17, 65), seed=seed, **kw),
            "prob": lambda seed: ContinuousActorProbabilistic(20, 4, (17, 65), seed=seed, **kw)}[kind]
    net = make(5)
    assert all(bool((g == 1).all()) and not bool(b.any()) for g, b in net.norm_views())
    net.flat.data.copy_(torch.randn(net.flat.numel(), generator=torch.Generator().manual_seed(1)))
    sd, ref = net.to_reference_state_dict(), _reference_module(kind, net.dims, act, eps)
    assert list(sd) == list(ref.state_dict()) and len(sd) == len(list(ref.parameters())) == len(net.param_views())
    ref.load_state_dict(sd, strict=True)
    assert sum(v.numel() for v in net.param_views()) == net.flat.numel()   # gamma and beta are in the optimizer's split too
    other = make(6)
    other.load_reference_state_dict(sd)
    assert torch.equal(other.flat.data.view(torch.int32), net.flat.data.view(torch.int32))
    twin = lagged_copy(net)
    assert twin.norm == "layer" and twin.norm_eps == eps and len(twin.norm_views()) == 2
    for (g, b), (tg, tb) in zip(net.norm_views(), twin.norm_views()):
        assert tg.data_ptr() - twin.flat.data_ptr() == g.data_ptr() - net.flat.data_ptr() and torch.equal(tg, g) and torch.equal(tb, b)


def test_no_checkpoint_path_drops_gamma_and_beta():
    """A caller that names the layers itself must name the LayerNorms too; the nets that wrap a user's FlatMLP list them."""
    feat = FlatMLP([6, 8, 4], device=DEV, seed=0, norm="layer")
    for f in (lambda: feat.named_layers(ref_layer_keys(2, "fc")), lambda: feat.export_layers(ref_layer_keys(2, "fc")),
              lambda: feat.import_layers({}, ref_layer_keys(2, "fc"))):
        with pytest.raises(ValueError, match="needs norm_keys for its 1 LayerNorms"):
            f()
    assert [k for k, _ in feat.named_reference_layers("fc", "actors.0.")][2:4] == ["actors.0.norm1.weight", "actors.0.norm1.bias"]
    icm = IntrinsicCuriosityModule(feature_net=feat, feature_dim=4, action_dim=3, hidden_sizes=(8,))
    views = icm.reference_named_views()
    assert [k for k, _ in views][:6] == [f"feature_net.model.{i}.{p}" for i in (0, 1, 3) for p in ("weight", "bias")]
    assert len(views) == 14 and sum(v.numel() for v in icm.param_views()) == icm.flat.numel()


def test_dqn_learns_a_normalised_q_network_and_syncs_its_lagged_copy():
    rs = np.random.RandomState(0)
    buf = DeviceVectorReplayBuffer(32, 2, n_agent=1, obs_dim=6, device=DEV)
    for _ in range(10):
        buf.add(Batch(obs=rs.randn(2, 1, 6).astype(np.float32), act=rs.randint(0, 5, (2, 1)), rew=rs.randn(2, 1).astype(np.float32),
                      terminated=rs.rand(2) < 0.2, truncated=np.zeros(2, bool), obs_next=rs.randn(2, 1, 6).astype(np.float32)))
    net = FlatMLP([6, 16, 16, 5], "relu", device=DEV, seed=0, norm="layer")
    algo = DQN(policy=DiscreteQLearningPolicy(model=net, action_space=_Discrete(5)), optim=AdamOptimizerFactory(lr=1e-3),
               n_step_return_horizon=2, target_update_freq=1)
    algo.is_within_training_step = True
    w0 = net.flat.data.clone()
    assert np.isfinite(algo.update(buf, 16).loss)
    w1 = net.flat.data.clone()
    assert np.isfinite(algo.update(buf, 16).loss)   # its sync copies the weights the first update left
    for (g0, b0), (g1, b1), (tg, tb) in zip(net.norm_views(w0), net.norm_views(w1), algo.model_old.norm_views()):
        assert not torch.equal(g0, g1) and not torch.equal(b0, b1) and torch.equal(tg, g1) and torch.equal(tb, b1)
