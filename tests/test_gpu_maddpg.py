"""GPU tests (`-m gpu`) of MADDPG (csrc/maddpg.hip, tsm_mlp_input_grad, the dense actors and critics under two HIP Adams).

Learn replays are compared with the float64 restatement (tests/maddpg_restatement.py, pinned to the reference's float64 run
by tests/test_host_maddpg.py) within  |hip - ref64| <= 4 max(e_ref, 8 ulp(max |ref64|)),  e_ref = the reference's own
float32 error on that array (tests/golden/maddpg.npz, maddpg_n8.npz); weights after an Adam step also get the `adamcond`
allowance of the CTDE replays (tests/test_gpu_dense.py), targets tau times it, and then more than 99.9 % of the entries
must meet the plain bar alone.  Each test prints the largest |hip - ref64| / tol per array."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

from maddpg_restatement import MaddpgRestatement  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.multiagent.ctde import DecentralizedActor, MADDPGPolicy
    from tianshou_marl_amd.data import Batch
    from tianshou_marl_amd.utils.net import FlatMLP


class _Box:
    def __init__(self, n, low=-1.0, high=1.0):
        self.shape, self.low, self.high = (n,), np.full(n, low, np.float32), np.full(n, high, np.float32)


def _g(name: str = "small"):
    return np.load(os.path.join(HERE, "golden", "maddpg_n8.npz" if name == "n8" else "maddpg.npz"))


def _ulp_floor(ref):
    m = float(np.abs(ref).max()) if np.size(ref) else 0.0
    return 8.0 * float(np.spacing(np.float32(m))) if m > 0 else 8.0 * float(np.finfo(np.float32).tiny)


def _check(name, got, ref, e_ref, extra=0.0):
    """|got - ref| <= plain + extra everywhere, plain = 4 max(e_ref, 8 ulp(max |ref|)).  With an allowance `extra` (Adam
    steps on ill-conditioned parameters, test_gpu_dense.py:488-497) all but 0.1 % must also meet the plain bar alone."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    plain = 4.0 * max(float(e_ref), _ulp_floor(ref))
    tol = plain + extra
    err = np.abs(got - ref)
    ratio = float((err / tol).max())
    msg = f"PARITY {name}: max |hip - ref64| / tol = {ratio:.3g}"
    if np.ndim(extra) > 0:
        share = float((err <= plain).mean())
        msg += f", share within the plain bar {share:.6f}, max |hip - ref64| / plain = {float((err / plain).max()):.3g}"
        assert share > 0.999, (name, share)
    print(msg)
    assert np.all(err <= tol), (name, ratio)
    return ratio


def _policy(init, N, D, Ad, H, gamma=0.99, tau=0.01, **kw):
    actors = [DecentralizedActor(D, Ad, H, device=DEV, seed=i) for i in range(N)]
    critics = [FlatMLP([N * (D + Ad), H, H, 1], device=DEV, seed=50 + i) for i in range(N)]
    pol = MADDPGPolicy(actors, critics, None, _Box(Ad), N, discount_factor=gamma, tau=tau, **kw)
    if init is not None:
        t = torch.as_tensor(np.asarray(init, np.float32), device=DEV)
        pol.flat.copy_(t)
        pol.target_flat.copy_(t)
    return pol


def _batch(rows, N, device=False):
    conv = (lambda x: torch.as_tensor(np.ascontiguousarray(x), device=DEV)) if device else (lambda x: x)
    b = Batch()
    for i in range(N):
        b[f"agent_{i}"] = Batch(obs=conv(rows["obs"][i]), act=conv(rows["act"][i]), rew=conv(rows["rew"][i]),
                                obs_next=conv(rows["obs_next"][i]), terminated=conv(rows["term"][i]))
    return b


def _args(rows):
    return [rows[f] for f in ("obs", "act", "rew", "obs_next", "term")]


def _grad_of(pol, B):
    w = pol._ws[B]
    return torch.cat([w["slabs_actor"].double().sum(0), w["slabs_critic"].double().sum(0)]).cpu().numpy()


@pytest.mark.parametrize("name", ["small", "n8", "odd"])
def test_learn_matches_reference(name):
    g = _g(name)
    N, D, Ad, H, B, rounds = (int(x) for x in g[f"{name}_dims"])
    gamma, tau, lr = float(g["gamma"]), float(g["tau"]), 1e-3
    pol = _policy(g[f"{name}_init"], N, D, Ad, H, gamma, tau)
    R = MaddpgRestatement(g[f"{name}_init"], N, [D, H, H, Ad], [N * (D + Ad), H, H, 1], gamma=gamma, tau=tau)
    keys = [str(k) for k in g[f"{name}_loss_keys"]]
    cond = np.zeros(pol.flat.numel())
    extra_t = np.zeros(pol.flat.numel())
    grad_tol = None
    for k in range(rounds):
        rows = {f: g[f"{name}_r{k}_{f}"] for f in ("obs", "act", "rew", "obs_next", "term")}
        out = pol.learn(_batch(rows, N))
        r = R.learn(*_args(rows))
        cond += R.adam_cond()
        assert list(out.keys()) == keys
        ref64, ref32 = g[f"{name}_r{k}_losses"]
        for j, key in enumerate(keys):
            _check(f"{name} r{k} {key}", [out[key]], [r[key]], abs(float(ref32[j]) - float(ref64[j])))
        if k == 0:
            e = float(g[f"{name}_r0_grad_eref"])
            _check(f"{name} r0 grad", _grad_of(pol, B), r["grads"], e)
            grad_tol = 4.0 * max(e, _ulp_floor(r["grads"]))
        extra = np.minimum(cond * grad_tol, 2 * lr * (k + 1))
        _check(f"{name} r{k} weights", pol.flat.double().cpu().numpy(), R.weights(), float(g[f"{name}_r{k}_weights_eref"]), extra)
        pol.update_target_networks()
        R.update_targets()
        # a target takes tau x the weight's error per update: t_k = tau w_k + (1 - tau) t_{k-1}
        extra_t = tau * extra + (1 - tau) * extra_t
        _check(f"{name} r{k} targets", pol.target_flat.double().cpu().numpy(), R.targets(),
               float(g[f"{name}_r{k}_targets_eref"]), extra_t)


def test_learn_on_device_leaves_is_bitwise_the_numpy_learn_and_async_stats():
    g = _g("odd")
    N, D, Ad, H, B, _ = (int(x) for x in g["odd_dims"])
    rows = {f: g[f"odd_r0_{f}"] for f in ("obs", "act", "rew", "obs_next", "term")}
    pa, pb = _policy(g["odd_init"], N, D, Ad, H), _policy(g["odd_init"], N, D, Ad, H, async_stats=True)
    ra = [pa.learn(_batch(rows, N)) for _ in range(2)]
    rb = [pb.learn(_batch(rows, N, device=True)) for _ in range(2)]
    assert isinstance(ra[0], dict) and type(rb[0]).__name__ == "MADDPGScalars"
    assert np.array_equal(pa.flat.cpu().numpy().view(np.uint32), pb.flat.cpu().numpy().view(np.uint32))
    assert ra[0] == rb[0] and ra[1] == rb[1] and ra[0] != ra[1]
    assert ra[0]["actor_loss"] == float(np.mean([ra[0][f"agent_{i}_actor_loss"] for i in range(N)]))


@pytest.mark.parametrize("replace", [False, True])
@pytest.mark.parametrize("D,Ad", [(18, 2), (17, 3), (4, 1), (8, 4)])
def test_joint_rows_exact(D, Ad, replace):
    """(8, 4) adds the all-16-byte path to the issue's three shapes; (4, 1) at N = 8 moves the observations 16 bytes at a
    time and the actions one float at a time."""
    rs = np.random.RandomState(D * 10 + Ad)
    for N in (1, 3, 8):
        for B in (1, 63, 257):
            obs = rs.standard_normal((N, B, D)).astype(np.float32)
            act = rs.standard_normal((N, B, Ad)).astype(np.float32)
            rep = rs.standard_normal((N, B, Ad)).astype(np.float32)
            dev = lambda a: [torch.as_tensor(a[i], device=DEV) for i in range(N)]  # noqa: E731
            W = N * (D + Ad)
            shape = (N, B, W) if replace else (B, W)
            out = torch.full((int(np.prod(shape)) + 8,), -7.0, device=DEV)  # a guard behind the rows
            got = ops.maddpg_joint_rows(dev(obs), dev(act), dev(rep) if replace else None,
                                        out=out[:int(np.prod(shape))].view(shape))
            base = np.concatenate([obs.transpose(1, 0, 2).reshape(B, N * D), act.transpose(1, 0, 2).reshape(B, N * Ad)], 1)
            if replace:
                want = np.stack([base] * N)
                for m in range(N):
                    want[m][:, N * D + m * Ad:N * D + (m + 1) * Ad] = rep[m]
            else:
                want = base
            assert np.array_equal(got.cpu().numpy(), want), (N, B)
            assert (out[-8:] == -7.0).all()


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_td_head_and_finalize_against_float64(B):
    N, gamma = 3, 0.99
    rs = np.random.RandomState(B)
    q, qn, rew, q_pi = (rs.standard_normal((N, B)).astype(np.float32) for _ in range(4))
    term = rs.rand(N, B) < 0.3
    term[0], term[1] = True, False  # an all-terminated and a none-terminated agent
    dev = lambda a, **kw: [torch.as_tensor(a[i], device=DEV, **kw) for i in range(N)]  # noqa: E731
    dq, partial = ops.maddpg_td(dev(q), dev(qn), dev(rew), dev(term), gamma)
    assert partial.numel() == N * -(-B // 256) == ops.maddpg_partial_elems(B, N)
    y = rew.astype(np.float64) + gamma * qn.astype(np.float64) * (1.0 - term)
    d = q.astype(np.float64) - y
    want = (2.0 * d / B).astype(np.float32)
    got = np.stack([x.cpu().numpy() for x in dq])
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want))
    print(f"PARITY td B{B}: max |dq - f64| = {float(ulps.max()):.3g} ulp")
    assert ulps.max() <= 2
    out = torch.zeros(2 * N, device=DEV)
    ops.maddpg_finalize(partial, dev(q_pi), B, out)
    got = out.cpu().numpy().astype(np.float64).reshape(N, 2)
    want = np.stack([-q_pi.astype(np.float64).mean(1), (d * d).mean(1)], 1)
    rel = np.abs(got - want) / np.abs(want)
    print(f"PARITY finalize B{B}: max relative error {float(rel.max()):.3g}")
    assert rel.max() <= 1e-6
    pinned = torch.zeros(2 * N, pin_memory=True)
    ops.maddpg_finalize(partial, dev(q_pi), B, pinned)
    torch.cuda.synchronize()
    assert np.array_equal(pinned.numpy(), out.cpu().numpy())


def _close(got, want, tol=1e-5):
    """The dgrad bar of tests/test_gpu_dense.py: 1e-5 of the tensor's scale."""
    want = want.detach().cpu().to(torch.float64)
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got.cpu().to(torch.float64) - want).abs().max())
    print(f"PARITY input_grad: max abs err / (1e-5 scale) = {err / (tol * scale):.3g}")
    assert err <= tol * scale, f"max abs err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("dims,windows", [((60, 64, 64, 1), ((0, 60), (54, 2), (59, 1))), ((23, 32, 1), ((20, 3),))])
def test_mlp_input_grad_matches_float64_autograd(dims, windows, B):
    torch.manual_seed(sum(dims) + B)
    net = FlatMLP(list(dims), device=DEV, seed=4)
    x = torch.randn(B, dims[0], device=DEV)
    d_out = torch.randn(B, 1, device=DEV)
    net(x)
    slabs = net.backward(d_out)
    before = slabs.clone()
    ws = [net.weight(i).double().cpu() for i in range(net.n_layers)]
    bs = [net.bias(i).double().cpu() for i in range(net.n_layers)]
    xr = x.double().cpu().requires_grad_(True)
    h = xr
    for i in range(net.n_layers):
        h = torch.nn.functional.linear(h, ws[i], bs[i])
        if i + 1 < net.n_layers:
            h = torch.relu(h)
    (ref,) = torch.autograd.grad((h * d_out.double().cpu()).sum(), xr)
    for col0, n_col in windows:
        got = net.input_grad(d_out, col0, n_col)
        assert tuple(got.shape) == (B, n_col)
        _close(got, ref[:, col0:col0 + n_col])
    assert torch.equal(slabs, before)  # no weight gradient was written
    with pytest.raises(ValueError, match="leave the input width"):
        net.input_grad(d_out, dims[0] - 1, 2)


@pytest.mark.parametrize("tau", [0.01, 0.005, 1.0])
def test_polyak_bitwise_equals_the_torch_expression(tau):
    for n in (1, 1023, 40905):
        buf_p, buf_t = torch.randn(n + 1, device=DEV), torch.randn(n + 1, device=DEV)
        for off in (0, 1):  # 16-byte aligned and not
            p = buf_p[off:off + n]
            t = buf_t[off:off + n].clone() if off == 0 else buf_t[off:off + n]
            want = tau * p + (1 - tau) * t
            guard = buf_t[0].clone()
            ops.polyak(t, p, tau)
            assert torch.equal(t.view(torch.int32), want.view(torch.int32)), (n, off)
            if off == 1:
                assert torch.equal(buf_t[0], guard)


def test_update_target_networks_is_the_torch_expression_on_the_joint_vector():
    pol = _policy(None, 3, 18, 2, 64, tau=0.01)
    assert pol.flat.numel() == 40905
    pol.flat.copy_(torch.randn_like(pol.flat))
    want = pol.tau * pol.flat + (1 - pol.tau) * pol.target_flat
    pol.update_target_networks()
    assert torch.equal(pol.target_flat.view(torch.int32), want.view(torch.int32))
    assert torch.equal(pol.target_actors[1].weight(0), pol.target_flat[pol._offs[1]:pol._offs[1] + 64 * 18].view(64, 18))


def test_act_device_bits_counter_noise_moments_and_clip():
    N, D, Ad, H, E = 3, 18, 2, 64, 8
    pol = _policy(_g()["small_init"], N, D, Ad, H, seed=17)
    obs = torch.randn(E, N, D, device=DEV)
    mu = torch.stack([FlatMLP.forward(pol.actors[i], obs[:, i].contiguous(), save=False) for i in range(N)], 1)  # [E, N, Ad]
    # sigma = 0, no clip: the actors' bits in [E * N] agent-interleaved order
    r = pol.act_device(obs)
    assert tuple(r["act"].shape) == (E * N, Ad) and torch.equal(r["act"], mu.reshape(E * N, Ad))
    assert not r["logp"].any() and not r["value"].any()
    # the same seed and offset give the same bits, another offset does not
    pol.noise_std = 0.5
    c1, c2 = (torch.tensor([v], dtype=torch.int64, device=DEV) for v in (123456, 123457))  # (read as u64)
    a1, a2, a3 = (pol.act_device(obs, offset_dev=c)["act"].clone() for c in (c1, c1, c2))
    assert torch.equal(a1, a2) and not torch.equal(a1, a3)
    own1, own2 = pol.act_device(obs)["act"].clone(), pol.act_device(obs)["act"].clone()  # the policy's own counter moves
    assert not torch.equal(own1, own2)
    # moments of (a - mu) / sigma over E N Ad = 8 * 3 * 2 * 4096 samples
    big = obs.repeat(4096, 1, 1)
    z = ((pol.act_device(big)["act"].view(4096, E * N * Ad) - mu.reshape(1, -1)) / 0.5).double()
    n = z.numel()
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print(f"noise: n = {n}, mean {mean:.3g} (bar {5 / np.sqrt(n):.3g}), var - 1 = {var - 1:.3g} (bar {5 * np.sqrt(2 / n):.3g})")
    assert n == 8 * 3 * 2 * 4096 and abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n)
    # clip: nothing leaves the bounds, values strictly inside are untouched; an `out` dict is written in place
    pc = _policy(_g()["small_init"], N, D, Ad, H, seed=17, noise_std=0.5, clip_actions=True)
    pc._low.fill_(-0.05)
    pc._high.fill_(0.1)
    pf = _policy(_g()["small_init"], N, D, Ad, H, seed=17, noise_std=0.5)  # (fresh, as pc: a policy's own counter adds to offset_dev)
    free = pf.act_device(obs, offset_dev=c1)["act"]
    buf = dict(act=torch.empty(E * N, Ad, device=DEV), logp=torch.ones(E * N, device=DEV), value=torch.ones(E * N, device=DEV))
    clipped = pc.act_device(obs, out=buf, offset_dev=c1)["act"]
    assert clipped is buf["act"] and not buf["logp"].any()
    assert ((clipped >= -0.05) & (clipped <= 0.1)).all() and (clipped == 0.1).any() and (clipped == -0.05).any()
    inside = (free > -0.05) & (free < 0.1)
    assert inside.any() and torch.equal(clipped[inside], free[inside])
    assert torch.equal(clipped, free.clamp(-0.05, 0.1))


def test_host_forward_returns_the_reference_actions():
    g = _g()
    N, D, Ad, H, _, _ = (int(x) for x in g["small_dims"])
    pol = _policy(g["small_init"], N, D, Ad, H)
    obs = g["fwd_obs"]
    out = pol.forward(Batch(**{f"agent_{i}": Batch(obs=obs[i]) for i in range(N)}))
    R = MaddpgRestatement(g["small_init"], N, [D, H, H, Ad], [N * (D + Ad), H, H, 1])
    ref64 = np.stack(R.forward(obs))
    got = np.stack([out[f"agent_{i}"].act.numpy() for i in range(N)])
    assert not out["agent_0"].act.is_cuda and got.dtype == np.float32 and got.shape == g["fwd_act"].shape
    _check("host forward", got, ref64, np.abs(g["fwd_act"].astype(np.float64) - ref64).max())


_WIDE: dict = {}


def _wide_reference():
    """N 8, D 48, Ad 5, H 128, B 4096: one learn of the f64 and of the f32 restatement on the CPU (computed once).  Rows are
    drawn under the delta rule for the passes on the weights the call starts with (actors, target actors, critics and
    target critics).  The stepped critics' pass on X_i cannot be cleared by redrawing rows at this size: the critic's Adam
    step depends on every row (a redrawn row flips the sign of some near-zero gradient entries, each moving a weight by
    2 lr), so every redraw moves that pass's pre-activations for ALL rows and about 6 % of 4096 rows land in the band
    again (measured on the CPU: 893 rows in the first pass, then a plateau of ~240 for 60 passes).  The bar's e_ref comes
    from the float32 restatement, which meets those rows too."""
    if not _WIDE:
        N, D, Ad, H, B = 8, 48, 5, 128, 4096
        pol = _policy(None, N, D, Ad, H)
        init = pol.flat.double().cpu().numpy()
        mk = lambda dt: MaddpgRestatement(init, N, [D, H, H, Ad], [N * (D + Ad), H, H, 1], dtype=dt)  # noqa: E731
        R64, R32 = mk(torch.float64), mk(torch.float32)
        rs = np.random.RandomState(8)

        def draw():
            return dict(obs=rs.standard_normal((N, B, D)).astype(np.float32),
                        obs_next=rs.standard_normal((N, B, D)).astype(np.float32),
                        act=rs.uniform(-1, 1, (N, B, Ad)).astype(np.float32), rew=rs.standard_normal((N, B)).astype(np.float32),
                        term=rs.rand(N, B) < 0.1)

        rows, share = draw(), None
        for _ in range(50):
            bad = R64.kink_rows(*_args(rows), 1e-5, stepped=False)
            share = float(bad.mean()) if share is None else share
            if not bad.any():
                break
            fresh = draw()
            for k in rows:
                rows[k][:, bad] = fresh[k][:, bad]
        assert not bad.any()
        _WIDE.update(pol=pol, rows=rows, share=share, r64=R64.learn(*_args(rows)), r32=R32.learn(*_args(rows)),
                     w64=R64.weights(), w32=R32.weights(), cond=R64.adam_cond(), dims=(N, D, Ad, H, B))
    return _WIDE


def test_learn_wide_against_f64_restatement():
    w = _wide_reference()
    N, D, Ad, H, B = w["dims"]
    print(f"wide: redraw share {w['share']:.4f}")
    assert w["share"] <= 0.25
    pol, r64, r32 = w["pol"], w["r64"], w["r32"]
    out = pol.learn(_batch(w["rows"], N))
    e = np.abs(r32["grads"] - r64["grads"]).max()
    _check("wide grad", _grad_of(pol, B), r64["grads"], e)
    grad_tol = 4.0 * max(e, _ulp_floor(r64["grads"]))
    _check("wide weights", pol.flat.double().cpu().numpy(), w["w64"], np.abs(w["w32"] - w["w64"]).max(),
           np.minimum(w["cond"] * grad_tol, 2e-3))
    # the per-agent losses as the arrays they are: e_ref = max |ref32 - ref64| over the N agents, as for every other array
    # (one float32 run's error on ONE scalar is no bar: it can be near zero by chance).
    # The actor losses are means over the STEPPED critics' outputs: a one-sided error of the Adam step (every parameter moved
    # a touch too far along its gradient's sign) does not average out in them, which is how this check found one.
    for kind in ("critic_loss", "actor_loss"):
        keys = [f"agent_{i}_{kind}" for i in range(N)]
        for key in keys:
            print(f"wide {key}: hip {out[key]:.9g} ref64 {r64[key]:.9g} ref32 {r32[key]:.9g}")
        _check(f"wide {kind}", [out[kind]], [r64[kind]], abs(r32[kind] - r64[kind]))
        _check(f"wide agent_*_{kind}", [out[k] for k in keys], [r64[k] for k in keys],
               max(abs(r32[k] - r64[k]) for k in keys))


def test_adam_step_coef64_is_within_rounding_of_float64_adam():
    """One step on well-conditioned entries (|g| >= 0.1): with 1 - beta rounded once the new weight is the float64 Adam's
    within 0.75 ulp (half an ulp is the rounding of the weight itself); the f32 differences of tsm_adam_step lengthen the
    step by 6.4e-6 of lr = 6.4e-9, which is printed beside it."""
    from tianshou_marl_amd.utils.net import FlatAdam

    rs = np.random.RandomState(5)
    n, lr = 40905, 1e-3
    w0 = rs.uniform(0.03, 0.06, n).astype(np.float32)
    g = (rs.choice([-1.0, 1.0], n) * rs.uniform(0.1, 1.0, n)).astype(np.float32)
    g64 = g.astype(np.float64)
    m, v = 0.1 * g64, 0.001 * g64 * g64
    want = w0.astype(np.float64) - lr * (m / 0.1) / (np.sqrt(v) / np.sqrt(0.001) + 1e-8)
    err = {}
    for coef64 in (True, False):
        p = torch.as_tensor(w0.copy(), device=DEV)
        FlatAdam(p, lr=lr, coef64=coef64).step(torch.as_tensor(g, device=DEV).view(1, n))
        err[coef64] = np.abs(p.double().cpu().numpy() - want) / np.spacing(np.abs(want).astype(np.float32))
    print(f"PARITY adam step: max |hip - f64| = {err[True].max():.3g} ulp with coef64, {err[False].max():.3g} ulp without")
    assert err[True].max() <= 0.75
