"""GPU tests (`-m gpu`) of csrc/fisher.hip against torch on the CPU in float64 with the same weights and inputs: the tangent
forward pass against forward-mode autograd, the Fisher head and the composed F v + 0.1 v against the reference's double backward
(npg.py:162-166, 195-200), and the KL / surrogate head against torch.distributions.  Bar: 1e-5 of max |reference| per output."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.utils.net import FlatMLP

DEV = "cuda"


def _forward(theta, dims, act, x):
    h, o = x, 0
    for i in range(len(dims) - 1):
        k, n = dims[i], dims[i + 1]
        h = h @ theta[o:o + n * k].view(n, k).T + theta[o + n * k:o + n * k + n]
        o += n * k + n
        if i + 2 < len(dims):
            h = torch.tanh(h) if act == "tanh" else torch.relu(h)
    return h


def _close(got, ref, what):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    err = (got.detach().double().cpu() - ref).abs().max().item()
    bar = 1e-5 * max(ref.abs().max().item(), 1e-300)
    print(f"{what}: max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar, what


# tile edges in every dimension, a k seam off the tile grid and unaligned leading dimensions: 33-130-70-6, B 129
@pytest.mark.parametrize("dims,B,act", [((7, 24, 3), 50, "relu"), ((18, 64, 64, 5), 256, "tanh"),
                                        ((33, 130, 70, 6), 129, "relu"), ((3, 2), 1, "relu")])
def test_tangent_head_and_fisher_product_match_float64_autograd(dims, B, act):
    g = torch.Generator().manual_seed(11)
    net = FlatMLP(dims, act, device=DEV, seed=4)
    x, v = torch.randn(B, dims[0], generator=g), torch.randn(net.flat.numel(), generator=g)
    theta = net.flat.data.cpu().double().requires_grad_(True)
    x64, v64 = x.double(), v.double()
    logits_ref, jv_ref = torch.autograd.functional.jvp(lambda th: _forward(th, dims, act, x64), theta.detach(), v64)
    p = torch.softmax(logits_ref, -1)
    pt = (p * jv_ref).sum(-1, keepdim=True)
    # the reference's own second derivative: KL(old || new) with old the same forward, differentiated twice
    dist = torch.distributions.Categorical(logits=_forward(theta, dims, act, x64))
    kl = torch.distributions.kl_divergence(torch.distributions.Categorical(logits=dist.logits.detach()), dist).mean()
    kg = torch.autograd.grad(kl, theta, create_graph=True)[0]
    Fv = torch.autograd.grad((kg * v64).sum(), theta)[0]

    xd, vd = x.to(DEV), v.to(DEV)
    logits = net.forward(xd, save=True)
    jv, _ = ops.mlp_tangent_forward(net.desc, net.flat.data, vd, *net._saved)
    _close(jv, jv_ref, "J v")
    u, part = ops.fisher_head(logits, jv)
    _close(u, p * (jv_ref - pt) / B, "u")
    _close(part.sum(), (v64 * Fv).sum(), "v F v")
    slabs, part2 = ops.fisher_vector_product(net, vd)
    _close(slabs.sum(0) + 0.1 * vd, Fv + 0.1 * v64, "F v + 0.1 v")
    _close(part2.sum(), (v64 * Fv).sum(), "v F v (composed)")


@pytest.mark.parametrize("A,B", [(2, 1), (2, 50), (5, 1), (5, 50)])
@pytest.mark.parametrize("kind", ["ratio", "logp"])
def test_kl_surrogate_head_matches_float64(A, B, kind):
    g = torch.Generator().manual_seed(5)
    lo, ln = torch.randn(B, A, generator=g), torch.randn(B, A, generator=g)
    act = torch.randint(0, A, (B,), generator=g).to(torch.int32)
    logp_old, adv = -torch.rand(B, generator=g) - 0.5, torch.randn(B, generator=g)
    ln64 = ln.double().requires_grad_(True)
    new = torch.distributions.Categorical(logits=ln64)
    logp = new.log_prob(act.long())
    loss = -((logp - logp_old.double()).exp() * adv.double()).mean() if kind == "ratio" else -(logp * adv.double()).mean()
    kl = torch.distributions.kl_divergence(torch.distributions.Categorical(logits=lo.double()), new).mean()
    part, d_logits = ops.categorical_kl_surrogate(lo.to(DEV), ln.to(DEV), act.to(DEV), logp_old.to(DEV), adv.to(DEV), kind,
                                                  want_grad=True)
    sums = part.view(-1, 2).sum(0) / B
    _close(sums[0], kl.detach(), "kl")
    _close(sums[1], loss.detach(), "loss")
    _close(d_logits, torch.autograd.grad(loss, ln64)[0], "d_logits")
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)   # run_if = 0: the launch leaves the partials alone
    kept = part.clone()
    ops.categorical_kl_surrogate(ln.to(DEV), lo.to(DEV), act.to(DEV), logp_old.to(DEV), adv.to(DEV), kind, partial=part, run_if=flag)
    assert torch.equal(part, kept)


def test_flat_axpy_dev_is_predicated_and_scaled_on_the_device():
    g = torch.Generator().manual_seed(9)
    base, d = torch.randn(1500, generator=g), torch.randn(1500, generator=g)
    s = torch.tensor([0.37], dtype=torch.float64, device=DEV)
    on, off = (torch.tensor([f], dtype=torch.int32, device=DEV) for f in (1, 0))
    out = ops.flat_axpy_dev(base.to(DEV), d.to(DEV), -2.0, scale_dev=s, run_if=on)
    _close(out, base.double() - 2.0 * 0.37 * d.double(), "base + s d")
    kept = out.clone()
    ops.flat_axpy_dev(d.to(DEV), base.to(DEV), 3.0, run_if=off, out=out)
    assert torch.equal(out, kept)
