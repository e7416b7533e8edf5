"""GPU tests (`-m gpu`) of the device-side conjugate gradients and of one NPG / TRPO `_update_with_batch` against the reference's
own loops (npg.py:149-224, trpo.py:123-191) written inline with torch autograd on the CPU in float64, same weights and inputs.

Bar, as errors relative to max |reference|: max(1e-5, 4 e32), e32 being the distance of the SAME reference function run in
float32 on the CPU from its float64 run; the factor 4 covers summation orders that differ from torch's (slab splits, tiled k
loops, the quadratic form in place of p.z).  Inputs are conditioned, on the float64 reference, so that no decision is marginal:
every new_rdotr lies outside [1e-12, 1e-8] around residual_tol (CG test); in the update tests, whose normalised advantages put the
tenth r.r near 5e-10, outside [5e-11, 2e-10], twice the tolerance either way -- the float32 run's r.r is asserted to lie within 1 %
of the float64 run's, so a factor 2 leaves room; every line-search trial's kl is 0.1 % away from max_kl and its loss 0.01 % away
from the old loss.  (`breaks_at` counts iterations from 1: the issue's "iteration 2" of the 2-2 case, counted from 0, is 3 here.)"""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import NPG, TRPO
    from tianshou_marl_amd.utils.net import FlatMLP, MLPActorCritic

DEV = "cuda"
Cat, kl_div = torch.distributions.Categorical, torch.distributions.kl_divergence


def _forward(theta, dims, act, x):
    h, o = x, 0
    for i in range(len(dims) - 1):
        k, n = dims[i], dims[i + 1]
        h = h @ theta[o:o + n * k].view(n, k).T + theta[o + n * k:o + n * k + n]
        o += n * k + n
        if i + 2 < len(dims):
            h = torch.tanh(h) if act == "tanh" else torch.relu(h)
    return h


def _ref_actor(kind, dims, act, theta, obs, a, logp_old, adv, dt, hp):
    """The actor half of npg.py:149-177 / trpo.py:133-191 in dtype dt -> dict(x, rr, theta, actor_loss, kl[, step_size, trials])."""
    th = theta.to(dt).clone().requires_grad_(True)
    obs, logp_old, adv = obs.to(dt), logp_old.to(dt), adv.to(dt)
    dist = Cat(logits=_forward(th, dims, act, obs))
    loss_of = lambda d: -((d.log_prob(a) - logp_old).exp() * adv).mean() if kind == "trpo" else -(d.log_prob(a) * adv).mean()  # noqa: E731
    actor_loss = loss_of(dist)
    g = torch.autograd.grad(actor_loss, th, retain_graph=True)[0].detach()
    old = Cat(logits=dist.logits.detach())
    kg = torch.autograd.grad(kl_div(old, dist).mean(), th, create_graph=True)[0]
    mvp = lambda v: torch.autograd.grad((kg * v).sum(), th, retain_graph=True)[0].detach() + v * 0.1  # noqa: E731
    x, r, p, rr_all = torch.zeros_like(g), g.clone(), g.clone(), []   # npg.py:202-224
    rdotr = r.dot(r)
    for _ in range(10):
        z = mvp(p)
        alpha = rdotr / p.dot(z)
        x += alpha * p
        r -= alpha * z
        new_rdotr = r.dot(r)
        rr_all.append(float(new_rdotr))
        if new_rdotr < 1e-10:
            break
        p = r + new_rdotr / rdotr * p
        rdotr = new_rdotr
    # (a mean of terms of either sign has the scale of its terms: with normalised advantages TRPO's old surrogate is 0 up to rounding)
    out = dict(x=x.clone(), rr=rr_all, actor_loss=actor_loss.item(), actor_loss_scale=adv.abs().max().item())
    sd = -x
    step = torch.sqrt(2 * hp.get("max_kl", 0.0) / (sd * mvp(sd)).sum())   # trpo.py:153-160
    with torch.no_grad():
        if kind == "npg":
            new = th + hp["trust_region_size"] * sd
            out["kl"] = float(kl_div(old, Cat(logits=_forward(new, dims, act, obs))).mean())
        else:
            out["trials"] = []
            for i in range(hp["max_backtracks"]):
                new = th + step * sd
                nd = Cat(logits=_forward(new, dims, act, obs))
                new_loss, kl = loss_of(nd), kl_div(old, nd).mean()
                out["trials"].append((float(kl), float(new_loss)))
                if kl < hp["max_kl"] and new_loss < actor_loss:
                    break
                if i < hp["max_backtracks"] - 1:
                    step = step * hp["backtrack_coeff"]
                else:
                    step = torch.zeros(())
            out.update(kl=float(kl), step_size=float(step))
        out["theta"] = new.detach().clone()
    return out


def _ref_critic(dims, act, th, opt, obs, ret, iters):
    """npg.py:180-183: `iters` steps of the torch Adam `opt` over the leaf `th` on mse(returns, V) -> (theta, the last vf_loss)."""
    dt = th.dtype
    for _ in range(iters):
        vf = torch.nn.functional.mse_loss(ret.to(dt), _forward(th, dims, act, obs.to(dt)).flatten())
        opt.zero_grad()
        vf.backward()
        opt.step()
    return th.detach().clone(), vf.item()


def _check(case, got: dict, r64: dict, r32: dict, bar=None):
    """Every entry of `got` against r64 within max(1e-5, 4 e32) -- or within `bar` -- of max |r64|, or of r64's own scale for the
    entry where it states one (`actor_loss_scale`).  Each figure is printed (pytest -s: profiles/npg_parity.txt)."""
    for k, g in got.items():
        a64 = torch.as_tensor(r64[k], dtype=torch.float64).reshape(-1)
        scale = r64.get(k + "_scale") or max(a64.abs().max().item(), 1e-300)
        e32 = (torch.as_tensor(r32[k], dtype=torch.float64).reshape(-1) - a64).abs().max().item() / scale
        err = (torch.as_tensor(g).detach().double().cpu().reshape(-1) - a64).abs().max().item() / scale
        lim = max(1e-5, 4 * e32) if bar is None else bar
        line = f"{case:34s} {k:12s} err {err:.3e}  e32 {e32:.3e}  bar {lim:.3e}"
        print(line)
        assert err <= lim, line


def _data(dims, B, adv_scale, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(B, dims[0], generator=g)
    a = torch.randint(0, dims[-1], (B,), generator=g)
    adv, ret = adv_scale * torch.randn(B, generator=g), torch.randn(B, generator=g)
    return obs, a, adv, ret


@pytest.mark.parametrize("dims,act,B,adv_scale,breaks_at", [((18, 64, 64, 5), "tanh", 256, 10.0, None), ((2, 2), "relu", 33, 1.0, 3)])
def test_device_cg_matches_float64_loop(dims, act, B, adv_scale, breaks_at):
    obs, a, adv, _ = _data(dims, B, adv_scale, 21)
    net = FlatMLP(dims, act, device=DEV, seed=2)
    theta = net.flat.data.cpu()
    logits = net.forward(obs.to(DEV), save=True)
    logp_old, _ = ops.categorical_logp_entropy(logits, a.to(DEV, torch.int32))
    r64, r32 = (_ref_actor("npg", dims, act, theta, obs, a, logp_old.cpu(), adv, dt, dict(trust_region_size=0.5))
                for dt in (torch.float64, torch.float32))
    assert all(not 1e-12 <= v <= 1e-8 for v in r64["rr"]), r64["rr"]
    assert len(r64["rr"]) == (breaks_at or 10)
    _, d_logits = ops.categorical_kl_surrogate(logits, logits, a.to(DEV, torch.int32), logp_old, adv.to(DEV), "logp", want_grad=True)
    n_split = 2   # (two slabs: the slab sums of the gradient and of every product are exercised)
    g_slabs = net.backward(d_logits, n_split)
    st = ops.cg_state(net.flat.numel(), DEV)
    ops.cg_init(st, g_slabs)
    for _ in range(10):
        z_slabs, head = ops.fisher_vector_product(net, st["p"], n_split)
        ops.cg_update(st, z_slabs, head, 0.1)
        ops.cg_direction(st, 1e-10)
    assert int(st["done"].item()) == (breaks_at is not None)
    _check(f"cg {'-'.join(map(str, dims))} B {B}", dict(x=st["x"]), r64, r32)


def _run_update(cls, kind, hp, n_agent=1, seed=31, act="tanh"):
    """One `_update_with_batch` per agent (one minibatch, repeat 1, optim_critic_iters 2) on 18-64-64-5, B 256 per agent, and
    the reference applied to the same rows in the same shuffled order -> (per agent: got, r64, r32), the warnings raised."""
    dims_a, dims_c, B, lr = (18, 64, 64, 5), (18, 64, 64, 1), 256, 1e-3
    norm = hp.get("advantage_normalization", True)
    net = MLPActorCritic(18, 5, (64, 64), act=act, device=DEV, seed=7, init="default")
    algo = cls(net=net, lr=lr, optim_critic_iters=2, dispatch="per_agent" if n_agent > 1 else "pooled", shuffle="numpy", **hp)
    obs, a, adv, ret = _data(dims_a, B * n_agent, 1.0, seed)
    th_a, th_c = net.actor.flat.data.cpu().clone(), net.critic.flat.data.cpu().clone()
    logp_old, _ = ops.categorical_logp_entropy(net.actor.forward(obs.to(DEV), save=False), a.to(DEV, torch.int32))
    pb = dict(T=B, rows=None, obs=obs.to(DEV), act=a.to(DEV, torch.int32), adv=adv.to(DEV), ret=ret.to(DEV), logp_old=logp_old,
              v_s=torch.zeros(B * n_agent, device=DEV), n_env=1, n_agent=n_agent, joint=None)
    np.random.seed(seed)
    algo._preprocess_batch = lambda buffer: pb
    with warnings.catch_warnings(record=True) as warned:
        warnings.simplefilter("always")
        stats = algo._update(SimpleNamespace(n_agent=n_agent), None, 1, 0.0)
    flat = stats.get_loss_stats_dict()
    np.random.seed(seed)
    refs, full = [], {**dict(max_kl=0.01, backtrack_coeff=0.8, max_backtracks=10, trust_region_size=0.5), **hp}
    crit = {dt: th_c.to(dt).clone().requires_grad_(True) for dt in (torch.float64, torch.float32)}
    opts = {dt: torch.optim.Adam([th], lr=lr) for dt, th in crit.items()}   # ONE optimizer: its moments outlive an agent's update
    for k in range(n_agent):   # MARLDispatcher: the shared algorithm updates on agent k's rows, agent after agent
        rows = (torch.arange(B) * n_agent + k)[torch.as_tensor(np.random.permutation(B))]
        lp = logp_old.cpu()[rows]
        both = []
        for dt in (torch.float64, torch.float32):
            ad = adv.to(dt)[rows]
            if norm:
                ad = (ad - ad.mean()) / ad.std()   # npg.py:136-137 on the batch the update is handed
            ra = _ref_actor(kind, dims_a, act, th_a, obs[rows], a[rows], lp, ad, dt, full)
            ra["theta_critic"], ra["vf_loss"] = _ref_critic(dims_c, act, crit[dt], opts[dt], obs[rows], ret[rows], 2)
            both.append(ra)
        # no marginal break: the float64 r.r stay a factor 2 off the tolerance, the float32 run's within 1 % of them
        assert all(not 5e-11 <= v <= 2e-10 for v in both[0]["rr"]), both[0]["rr"]
        assert len(both[1]["rr"]) == len(both[0]["rr"]) and all(abs(u / v - 1) < 1e-2 for u, v in zip(both[1]["rr"], both[0]["rr"]))
        th_a = both[0]["theta"].float()   # the actor that agent k + 1 starts from
        refs.append(both)
    names = ("actor_loss", "vf_loss", "kl") + (("step_size",) if kind == "trpo" else ())
    pre = (lambda k, s: f"agent_{k}/{s}") if n_agent > 1 else (lambda k, s: s)
    got = [{s: flat[pre(k, s)] for s in names} for k in range(n_agent)]
    got[-1].update(theta=net.actor.flat.data, theta_critic=net.critic.flat.data)   # the parameters after the last agent
    return got, refs, [str(w.message) for w in warned]


def test_npg_update_matches_float64_reference():
    got, refs, _ = _run_update(NPG, "npg", {})
    _check("npg update", got[0], *refs[0])


# TRPO with its defaults (normalised advantages: the old surrogate is 0 up to rounding and is compared on the scale of its terms),
# where float64 accepts trial 0; and a case that backtracks.  The true KL stays below its quadratic model on these nets for every
# max_kl tried (0.5 .. 1e4), so that case is a relu actor, without normalisation, whose first trial puts float64 probabilities at
# 0: kl = inf, as torch's.  The float32 reference takes other trials there, so that case is held to 1e-5 of the float64 run flat,
# and the number of backtracks the device reports must be the float64 run's.  Every branch of the accept rule on finite numbers
# is in test_trpo_accept_follows_the_reference_rule.
@pytest.mark.parametrize("hp,act,bar", [(dict(max_kl=0.01), "tanh", None),
                                        (dict(max_kl=200.0, advantage_normalization=False), "relu", 1e-5)])
def test_trpo_update_matches_float64_reference(hp, act, bar):
    got, refs, warned = _run_update(TRPO, "trpo", hp, act=act)
    r64, n_back = refs[0][0], len(refs[0][0]["trials"]) - 1
    assert n_back == (0 if bar is None else 1) and r64["step_size"] > 0
    assert warned == ([f"Backtracking to step {n_back}."] if n_back else []), warned
    for kl, loss in r64["trials"]:
        assert abs(kl - hp["max_kl"]) >= 1e-3 * hp["max_kl"] and abs(loss - r64["actor_loss"]) >= 1e-4 * abs(r64["actor_loss"])
    _check(f"trpo update max_kl {hp['max_kl']} {act}", got[0], *refs[0], bar=bar)


# (kl, new_loss) per trial, the old loss 1.0, max_kl 0.5, three trials at most: accepted at once; rejected on a finite kl, then on
# the loss, then accepted; rejected on kl == max_kl and on new_loss == loss (both comparisons are strict), then failed
@pytest.mark.parametrize("trials", [[(0.1, 0.5)], [(0.7, 0.5), (0.4, 1.5), (0.3, 0.9)], [(0.5, 0.5), (0.1, 1.0), (0.9, 2.0)]])
def test_trpo_accept_follows_the_reference_rule(trials):
    B, max_kl, coeff, n = 4, 0.5, 0.8, 3
    step, kl, at = 2.0, None, -1.0   # trpo.py:167-191; at: the trial that was accepted, -1 for a failed search
    for i, (kl, new_loss) in enumerate(trials):
        if kl < max_kl and new_loss < 1.0:
            at = float(i)
            break
        step = step * coeff if i < n - 1 else 0.0
    pair = lambda k, l: torch.tensor([k * B, l * B], dtype=torch.float64, device=DEV)  # noqa: E731  one workgroup's {sum kl, sum loss}
    head = torch.tensor([0.25], dtype=torch.float64, device=DEV)   # x F x = 0.25, no damping: step size sqrt(2 max_kl / 0.25) = 2
    ls, run = ops.trpo_step_size(head, torch.ones(4, device=DEV), pair(0.0, 1.0), B, 0.0, max_kl)
    out = torch.zeros(4, device=DEV)
    for i in range(n):
        k, l = trials[min(i, len(trials) - 1)]
        ops.trpo_accept(pair(k, l), B, i, n, max_kl, coeff, ls, run, out)
    want = [1.0, kl, step, at]
    assert out.cpu().tolist() == pytest.approx(want, rel=1e-6), (out, want)


def test_npg_per_agent_dispatch_matches_reference_applied_per_agent():
    got, refs, _ = _run_update(NPG, "npg", {}, n_agent=2, seed=33)
    for k in range(2):
        _check(f"npg per_agent agent_{k}", got[k], *refs[k])


def test_checkpoint_round_trip_covers_the_critic_only_optimizer():
    """`_optimizers[0]` lists the critic's six parameters alone (optim_include_actor=False) and a fresh object resumes from it."""
    mk = lambda seed: NPG(net=MLPActorCritic(7, 3, (24, 24), device=DEV, seed=seed), lr=1e-3)  # noqa: E731
    a, b = mk(1), mk(2)
    a.optim.step(torch.randn(1, a.net.n_critic, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)))
    sd = a.state_dict()
    assert sorted(sd["_optimizers"][0]["state"]) == list(range(6)) and len(sd["_optimizers"][0]["param_groups"][0]["params"]) == 6
    b.load_state_dict(sd)
    assert torch.equal(b.net.flat.data, a.net.flat.data) and b.opt_step == 1
    assert torch.equal(b.optim.exp_avg, a.optim.exp_avg) and torch.equal(b.optim.exp_avg_sq, a.optim.exp_avg_sq)
    assert b.optim.exp_avg.numel() == b.net.n_critic
