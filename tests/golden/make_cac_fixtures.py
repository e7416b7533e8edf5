"""Generate tests/golden/cac.npz by RUNNING THE REFERENCE's DDPG, TD3 and SAC (ddpg.py, td3.py, sac.py, imported through
oracle/ref_shim.py) in float64 and float32: per case two consecutive `_preprocess_batch` + `_update_with_batch`
(+ `_postprocess_batch`) calls on a small hand-filled buffer.  The Gaussian draws (TD3's torch.randn, Normal.rsample's
_standard_normal) are replaced by arrays drawn here and recorded as data, so both runs and every test see the same noise.  The
network modules are defined here (`DetActor`, `ProbActor`, `Critic`: the reference's Net casts observations to float32, which
a float64 run cannot use); they compute what ContinuousActorDeterministic / ContinuousActorProbabilistic(conditioned_sigma=True)
/ ContinuousCritic compute.

Sizes: obs 6, act 3, hidden 16-16, B 12, buffer 4 x 16.  Cases (`cases`): kind, n_step, prioritized, and for SAC alpha kind,
unbounded, critic2=None, conditioned sigma (0: the state-independent sigma_param, the reference's default).  Per case `c{i}_`:
  init_*                      the initial flat vectors (float32 values)
  s{k}_indices, z_target, z_actor, weight_in
  s{k}_returns, prio, stats (float64 run), stats32, and `*_eref` = max |ref32 - ref64|
  s{k}_grad_{net}             every gradient of the float64 run, with `_eref`
  s1_w_{net}                  every network after the second call, with `_eref`;  s{k}_log_alpha
  leaves                      the sum tree's leaves after the second call (prioritized cases)
  sd_* / sig_*                reference state_dict keys and shapes (Net + ContinuousActor* / ContinuousCritic), signatures
The generator asserts that actor pre-tanh values stay within +-3, that no ReLU pre-activation and no q1-versus-q2 gap of a
real twin lies within DELTA of zero, and that the restatement (tests/cac_restatement.py) follows the float64 run to 1e-10.  It
prints the float32 run's distance from the float64 run per quantity.
"""
from __future__ import annotations

import copy
import inspect
import os

import numpy as np

from make_dqn_fixtures import DELTA, GAMMA  # noqa: E402  (installs the shim)

import torch  # noqa: E402
from torch import nn  # noqa: E402
import torch.distributions.normal as tdn  # noqa: E402
from tianshou.algorithm.modelfree.ddpg import DDPG, ContinuousDeterministicPolicy  # noqa: E402
from tianshou.algorithm.modelfree.sac import SAC, AutoAlpha, SACPolicy  # noqa: E402
from tianshou.algorithm.modelfree.td3 import TD3  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import Net  # noqa: E402
from tianshou.utils.net.continuous import (ContinuousActorDeterministic, ContinuousActorProbabilistic,  # noqa: E402
                                           ContinuousCritic)
import gymnasium as gym  # noqa: E402  (the shim's fake)

from dqn_restatement import RestatedBuffer, nstep_walk  # noqa: E402
from cac_restatement import CacRestatement, alpha_state  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
D, AD, HID, B, N_ENV, S, T = 6, 3, [16, 16], 12, 4, 16, 13
TAU, LR, MAX_ACTION = 0.05, 1e-3, 1.0
PER_ALPHA, PER_BETA = 0.6, 0.4
POLICY_NOISE, NOISE_CLIP, FREQ = 0.2, 0.5, 2
SAC_FIXED, SAC_LOG_ALPHA, SAC_TARGET_ENTROPY = 0.2, -1.0, -float(AD)
SIGMA_PARAM_INIT = [-0.5, -1.0, 0.25]
STAT_KEYS = ("actor_loss", "critic_loss", "critic1_loss", "critic2_loss", "alpha", "alpha_loss")
#        kind   n_step prio  alpha  unbounded  critic2=None
CASES = [("ddpg", 1, 0, "", 0, 0), ("ddpg", 3, 1, "", 0, 0),
         ("td3", 1, 1, "", 0, 0), ("td3", 3, 0, "", 0, 0), ("td3", 1, 0, "", 0, 1),
         ("sac", 1, 0, "fix", 0, 0), ("sac", 3, 1, "auto", 0, 0), ("sac", 1, 0, "auto", 1, 0), ("sac", 3, 0, "fix", 0, 1),
         ("sac", 3, 1, "auto", 0, 0, 0), ("sac", 1, 0, "fix", 1, 0, 0)]


def _t(x, like):
    return torch.as_tensor(np.asarray(x)).to(like.dtype)


class _MLP(nn.Module):
    def __init__(self, dims) -> None:
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])

    def trunk(self, x, n):
        for l in self.layers[:n]:
            x = torch.relu(l(x))
        return x


class DetActor(_MLP):
    max_action = MAX_ACTION

    def forward(self, obs, state=None, info=None):
        w = self.layers[0].weight
        raw = self.layers[-1](self.trunk(_t(obs, w), len(self.layers) - 1))
        self.last_raw = raw.detach()
        return self.max_action * torch.tanh(raw), state


class Critic(_MLP):
    def forward(self, obs, act=None, info=None):
        w = self.layers[0].weight
        x = torch.cat([_t(obs, w).flatten(1), act.to(w.dtype).flatten(1) if isinstance(act, torch.Tensor) else _t(act, w).flatten(1)], 1)
        return self.layers[-1](self.trunk(x, len(self.layers) - 1))


class ProbActor(_MLP):
    """As ContinuousActorProbabilistic with hidden_sizes=(): conditioned sigma -- the last layer is [mu | sigma], two Linear
    heads on one trunk; else the last layer is mu and `sigma_param` [act, 1] starts at SIGMA_PARAM_INIT (the reference's zeros
    would make both checks of the clamp's pass-through trivial)."""
    max_action = MAX_ACTION

    def __init__(self, dims, unbounded, cond=True) -> None:
        super().__init__(dims)
        self.unbounded, self.cond = unbounded, cond
        if not cond:
            self.sigma_param = nn.Parameter(torch.as_tensor(SIGMA_PARAM_INIT, dtype=torch.float32).reshape(AD, 1).clone())

    def forward(self, obs, state=None, info=None):
        w = self.layers[0].weight
        raw = self.layers[-1](self.trunk(_t(obs, w), len(self.layers) - 1))
        self.last_raw = raw.detach()
        mu = raw[:, :AD]
        if not self.unbounded:
            mu = self.max_action * torch.tanh(mu)
        if self.cond:
            return (mu, torch.clamp(raw[:, AD:], min=-20, max=2).exp()), state
        return (mu, (self.sigma_param.view(1, -1) + torch.zeros_like(mu)).exp()), state   # continuous.py:244-246


def params_of(m):
    """The module's parameters in the flat vectors' order: the layers, then sigma_param."""
    return list(m.layers.parameters()) + ([m.sigma_param] if hasattr(m, "sigma_param") else [])


def flat(m) -> np.ndarray:
    return np.concatenate([p.detach().double().reshape(-1).numpy() for p in params_of(m)])


class Noise:
    """Stands where torch.randn (td3.py:196) and Normal.rsample's _standard_normal stand: hands out the queued arrays."""

    def __init__(self) -> None:
        self.queue, self.used, self.dtype = [], [], torch.float32   # dtype: the running algorithm's (torch.randn has none)

    def randn(self, size=None, *a, device=None, dtype=None, **kw):
        z = self.queue.pop(0)
        assert tuple(z.shape) == tuple(size), (z.shape, size)
        self.used.append(z)
        return torch.as_tensor(z).to(self.dtype if dtype is None else dtype)

    def standard_normal(self, shape, dtype, device):
        return self.randn(tuple(shape), dtype=dtype)


def fill(rs, cls, dt, **kw):
    buf = cls(N_ENV * S, N_ENV, **kw)
    RB = RestatedBuffer(N_ENV, S, 1)
    for t in range(T):
        term, trunc = rs.rand(N_ENV) < 0.12, rs.rand(N_ENV) < 0.08
        rew = rs.standard_normal(N_ENV).astype(np.float32)
        b = Batch(obs=rs.standard_normal((N_ENV, D)).astype(np.float32).astype(dt),
                  act=rs.uniform(-1, 1, (N_ENV, AD)).astype(np.float32).astype(dt), rew=rew.astype(np.float64), terminated=term,
                  truncated=trunc, obs_next=rs.standard_normal((N_ENV, D)).astype(np.float32).astype(dt), info=Batch())
        buf.add(b, buffer_ids=np.arange(N_ENV))
        for e in range(N_ENV):
            RB.add(e, rew[e], bool(term[e]), bool(trunc[e]))
    return buf, RB


def make_algo(kind, nets, dbl, n_step, alpha_kind, no_c2):
    cp = lambda n: copy.deepcopy(n).double() if dbl else copy.deepcopy(n)  # noqa: E731
    actor, c1, c2 = cp(nets[0]), cp(nets[1]), (None if no_c2 else cp(nets[2]))
    space = gym.spaces.Box(low=-1.0, high=1.0, shape=(AD,), dtype=np.float32)
    opt = lambda: AdamOptimizerFactory(lr=LR)  # noqa: E731
    if kind == "sac":
        alpha = SAC_FIXED
        if alpha_kind == "auto":
            alpha = AutoAlpha(SAC_TARGET_ENTROPY, SAC_LOG_ALPHA, opt())
            alpha = alpha.double() if dbl else alpha
        return SAC(policy=SACPolicy(actor=actor, action_space=space), policy_optim=opt(), critic=c1, critic_optim=opt(), critic2=c2,
                   tau=TAU, gamma=GAMMA, alpha=alpha, n_step_return_horizon=n_step)
    pol = ContinuousDeterministicPolicy(actor=actor, action_space=space)
    if kind == "ddpg":
        return DDPG(policy=pol, policy_optim=opt(), critic=c1, critic_optim=opt(), tau=TAU, gamma=GAMMA, n_step_return_horizon=n_step)
    return TD3(policy=pol, policy_optim=opt(), critic=c1, critic_optim=opt(), critic2=c2, tau=TAU, gamma=GAMMA,
               policy_noise=POLICY_NOISE, update_actor_freq=FREQ, noise_clip=NOISE_CLIP, n_step_return_horizon=n_step)


def net_names(kind):
    return {"ddpg": ["actor", "critic", "critic_old", "actor_old"],
            "td3": ["actor", "critic", "critic_old", "critic2", "critic2_old", "actor_old"],
            "sac": ["actor", "critic", "critic_old", "critic2", "critic2_old"]}[kind]


def ref_net(algo, name):
    m = {"actor": lambda: algo.policy.actor, "critic": lambda: algo.critic, "critic2": lambda: algo.critic2,
         "critic_old": lambda: algo.critic_old.module, "critic2_old": lambda: algo.critic2_old.module,
         "actor_old": lambda: algo.actor_old.module}[name]()
    return m


def ref_grad(net):
    return np.concatenate([(torch.zeros_like(q) if q.grad is None else q.grad).detach().double().reshape(-1).numpy() for q in params_of(net)])


def record_grads(algo, kind):
    """The gradient each optimizer steps with, caught at its step (the actor loss's backward later adds to the critics' .grad).
    -> dict filled per call: net name -> flat float64 gradient."""
    got = {}
    pairs = [("actor", algo.policy_optim, algo.policy.actor), ("critic", algo.critic_optim, algo.critic)]
    if kind != "ddpg":
        pairs.append(("critic2", algo.critic2_optim, algo.critic2))
    for name, opt, net in pairs:
        inner = opt._optim.step

        def step(*a, _inner=inner, _name=name, _net=net, **kw):
            got[_name] = ref_grad(_net)
            return _inner(*a, **kw)

        opt._optim.step = step
    return got


def stats_of(st):
    return np.array([np.nan if getattr(st, k, None) is None else float(getattr(st, k)) for k in STAT_KEYS])


def emax(a, b):
    return np.float64(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


class Kink(Exception):
    """The restatement came within DELTA of a non-smooth point: the seed is not used."""


class OutOfRange(Exception):
    """A pre-tanh value left about +-3, where log(1 - a^2 + eps) is dominated by eps and the comparison says nothing: the seed
    is not used.  (Every case finds a seed within its first few; a case that finds none fails the run.)"""


def run_case(ci, case, seed, noise):
    kind, n_step, prio, alpha_kind, unbounded, no_c2 = case[:6]
    cond = bool(case[6]) if len(case) > 6 else True
    rs = np.random.RandomState(seed)
    torch.manual_seed(seed)
    a_dims = [D, *HID, 2 * AD if kind == "sac" and cond else AD]
    c_dims = [D + AD, *HID, 1]
    nets = (ProbActor(a_dims, bool(unbounded), cond) if kind == "sac" else DetActor(a_dims), Critic(c_dims), Critic(c_dims))
    with torch.no_grad():   # keep pre-tanh values small: the last layer's weights shrink
        for p in nets[0].layers[-1].parameters():
            p.mul_(0.6)
    init = {n: flat(m).astype(np.float32) for n, m in zip(("actor", "critic", "critic2"), nets)}
    for m, n in zip(nets, ("actor", "critic", "critic2")):   # the float32 values are the weights of both runs
        o = 0
        with torch.no_grad():
            for q in params_of(m):
                q.copy_(torch.as_tensor(init[n][o:o + q.numel()]).reshape(q.shape))
                o += q.numel()
    if no_c2:
        init.pop("critic2")
    cls, kw = (PrioritizedVectorReplayBuffer, dict(alpha=PER_ALPHA, beta=PER_BETA)) if prio else (VectorReplayBuffer, {})
    bufs, algos = {}, {}
    for dbl in (True, False):
        bufs[dbl], RB = fill(np.random.RandomState(seed + 1000), cls, np.float64 if dbl else np.float32, **kw)
        algos[dbl] = make_algo(kind, nets, dbl, n_step, alpha_kind, no_c2)
        algos[dbl].policy.is_within_training_step = True   # SACPolicy samples (deterministic_eval acts outside of it only)
    caught = {dbl: record_grads(a, kind) for dbl, a in algos.items()}
    alpha = alpha_state(SAC_LOG_ALPHA) if alpha_kind == "auto" else SAC_FIXED
    R = CacRestatement(kind, init, a_dims, c_dims, TAU, lr=LR, max_action=MAX_ACTION, unbounded=bool(unbounded),
                       policy_noise=POLICY_NOISE, noise_clip=NOISE_CLIP, update_actor_freq=FREQ, alpha=alpha,
                       target_entropy=SAC_TARGET_ENTROPY, alpha_lr=LR)
    allidx = bufs[True].sample_indices(0)
    pk = f"c{ci}_"
    new = {pk + "init_" + n: v for n, v in init.items()}
    dist = {}
    for k in range(2):
        indices = rs.choice(allidx, B, replace=True).astype(np.int64)
        zt = rs.standard_normal((B, AD)).astype(np.float32) if kind != "ddpg" else None
        za = rs.standard_normal((B, AD)).astype(np.float32) if kind == "sac" else None
        out = {}
        for dbl, algo in algos.items():
            buf = bufs[dbl]
            noise.queue = [z for z in (zt, za) if z is not None]
            caught[dbl].clear()
            noise.dtype = torch.float64 if dbl else torch.float32
            batch = buf[indices]
            w_in = np.asarray(batch.weight, np.float64).copy() if prio else None
            batch = algo._preprocess_batch(batch, buf, indices)
            raw_t = (algo.policy.actor if kind == "sac" else algo.actor_old.module).last_raw
            st = algo._update_with_batch(batch)
            assert not noise.queue, "a draw was not consumed"
            algo._postprocess_batch(batch, buf, indices)
            raws = [raw_t, algo.policy.actor.last_raw]
            for r in raws:   # pre-tanh values (of mu for SAC) within about +-3
                if float(r[:, :AD].abs().max()) >= 3.0:
                    raise OutOfRange
            if kind == "sac":
                x = raws[1][:, :AD] if unbounded else MAX_ACTION * torch.tanh(raws[1][:, :AD])
                sg = raws[1][:, AD:] if cond else algo.policy.actor.sigma_param.detach().view(1, -1)
                pre = x + torch.clamp(sg, -20, 2).exp() * torch.as_tensor(za).to(x.dtype)
                if float(pre.abs().max()) >= 3.5:
                    raise OutOfRange
            out[dbl] = dict(stats=stats_of(st), ret=batch.returns.detach().double().numpy().reshape(-1),
                            prio=batch.weight.detach().double().numpy().reshape(-1), w_in=w_in,
                            g=dict(caught[dbl]),
                            w={n: flat(ref_net(algo, n)) for n in net_names(kind)},
                            la=float(algo.alpha._log_alpha.detach().double()) if alpha_kind == "auto" else np.nan,
                            leaves=(buf.weight._value[buf.weight._bound:buf.weight._bound + N_ENV * S].copy() if prio else None))
        r64, r32 = out[True], out[False]
        b32 = bufs[False]
        idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
        r = R.update(b32[indices].obs, b32[indices].act, b32[idx_n].obs_next, mc, gpow, vmask, weight=r64["w_in"], z_target=zt,
                     z_actor=za)
        if R.kink <= DELTA:
            raise Kink
        stepped = kind != "td3" or k % FREQ == 0
        mine = np.array([r["actor_loss"], r["critic1_loss"] if kind == "ddpg" else np.nan, np.nan if kind == "ddpg" else r["critic1_loss"],
                         np.nan if kind == "ddpg" else r["critic2_loss"], r.get("alpha", np.nan) if kind == "sac" else np.nan,
                         np.nan if r["alpha_loss"] is None else r["alpha_loss"]])
        assert np.allclose(mine, r64["stats"], rtol=1e-10, atol=0, equal_nan=True), (case, k, mine, r64["stats"])
        assert np.allclose(r["returns"], r64["ret"], rtol=1e-12, atol=1e-13) and np.allclose(r["prio"], r64["prio"], rtol=1e-10, atol=1e-13)
        for n in net_names(kind):
            assert np.allclose(R.weights(n), r64["w"][n], rtol=1e-10, atol=1e-13), (case, k, n)
        for n, gv in r["grads"].items():
            assert np.allclose(gv, r64["g"][n], rtol=1e-10, atol=1e-15), (case, k, n, np.abs(gv - r64["g"][n]).max())
        sk = f"{pk}s{k}_"
        new.update({sk + "indices": indices, sk + "stats": r64["stats"], sk + "stats32": r32["stats"], sk + "returns": r64["ret"],
                    sk + "returns_eref": emax(r64["ret"], r32["ret"]), sk + "prio": r64["prio"],
                    sk + "prio_eref": emax(r64["prio"], r32["prio"]), sk + "log_alpha": np.array([r64["la"], r32["la"]]),
                    sk + "actor_stepped": np.bool_(stepped)})
        if zt is not None:
            new[sk + "z_target"] = zt
        if za is not None:
            new[sk + "z_actor"] = za
        if prio:
            new.update({sk + "weight_in": r64["w_in"], sk + "weight_in_eref": emax(r64["w_in"], r32["w_in"])})
        assert set(r["grads"]) == set(r64["g"]) and ("actor" in r64["g"]) == stepped
        for n, gv in r64["g"].items():
            new.update({f"{sk}grad_{n}": gv, f"{sk}grad_{n}_eref": emax(gv, r32["g"][n])})
            dist[f"grad_{n}"] = max(dist.get(f"grad_{n}", 0.0), emax(gv, r32["g"][n]) / max(np.abs(gv).max(), 1e-300))
        for q in ("ret", "prio"):
            dist[q] = max(dist.get(q, 0.0), emax(r64[q], r32[q]) / np.abs(r64[q]).max())
        dist["stats"] = max(dist.get("stats", 0.0), float(np.nanmax(np.abs(r64["stats"] - r32["stats"]) / np.abs(r64["stats"]))))
        if k == 1:
            for n in net_names(kind):
                new.update({f"{sk}w_{n}": r64["w"][n], f"{sk}w_{n}_eref": emax(r64["w"][n], r32["w"][n])})
            if prio:
                new.update({pk + "leaves": r64["leaves"], pk + "leaves_eref": emax(r64["leaves"], r32["leaves"])})
    return new, dist


def statedict_and_signatures(res):
    torch.manual_seed(0)
    space = gym.spaces.Box(low=-1.0, high=1.0, shape=(AD,), dtype=np.float32)
    net = lambda **kw: Net(state_shape=(D,), hidden_sizes=HID, **kw)  # noqa: E731
    crit = lambda: ContinuousCritic(preprocess_net=net(action_shape=(AD,), concat=True))  # noqa: E731
    opt = lambda: AdamOptimizerFactory(lr=LR)  # noqa: E731
    det = lambda: ContinuousDeterministicPolicy(actor=ContinuousActorDeterministic(preprocess_net=net(), action_shape=(AD,)),  # noqa: E731
                                                action_space=space)
    prob = SACPolicy(actor=ContinuousActorProbabilistic(preprocess_net=net(), action_shape=(AD,), conditioned_sigma=True),
                     action_space=space)
    algos = dict(ddpg=DDPG(policy=det(), policy_optim=opt(), critic=crit(), critic_optim=opt()),
                 td3=TD3(policy=det(), policy_optim=opt(), critic=crit(), critic_optim=opt(), critic2=crit()),
                 sac=SAC(policy=prob, policy_optim=opt(), critic=crit(), critic_optim=opt(), critic2=crit(),
                         alpha=AutoAlpha(SAC_TARGET_ENTROPY, SAC_LOG_ALPHA, opt())))
    probp = SACPolicy(actor=ContinuousActorProbabilistic(preprocess_net=net(), action_shape=(AD,)), action_space=space)
    algos["sacp"] = SAC(policy=probp, policy_optim=opt(), critic=crit(), critic_optim=opt(), critic2=crit())   # sigma_param
    for kind, algo in algos.items():
        sd = {k: v for k, v in algo.state_dict().items() if isinstance(v, torch.Tensor)}
        res[f"sd_{kind}_keys"] = np.array(list(sd.keys()))
        res[f"sd_{kind}_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    ps = inspect.signature(ContinuousActorProbabilistic.__init__).parameters
    res["default_conditioned_sigma"] = np.bool_(ps["conditioned_sigma"].default)
    for cls in (ContinuousDeterministicPolicy, SACPolicy, DDPG, TD3, SAC):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    noise = Noise()
    torch.randn = noise.randn
    tdn._standard_normal = noise.standard_normal
    res = dict(delta=np.float64(DELTA), gamma=np.float64(GAMMA), tau=np.float64(TAU), lr=np.float64(LR),
               dims=np.array([D, AD, *HID, B, N_ENV, S, T], np.int64), max_action=np.float64(MAX_ACTION),
               per=np.array([PER_ALPHA, PER_BETA]), td3=np.array([POLICY_NOISE, NOISE_CLIP, FREQ]),
               sac=np.array([SAC_FIXED, SAC_LOG_ALPHA, SAC_TARGET_ENTROPY]), stat_keys=np.array(STAT_KEYS),
               cases=np.array(["|".join(str(v) for v in c) for c in CASES]))
    worst = {}
    for ci, case in enumerate(CASES):
        for seed in range(101 + 7 * ci, 201 + 7 * ci):   # the first seed whose two updates keep DELTA away from every kink and pre-tanh values in range
            try:
                new, dist = run_case(ci, case, seed, noise)
            except (Kink, OutOfRange):
                continue
            res.update(new)
            res[f"c{ci}_seed"] = np.int64(seed)
            for q, v in dist.items():
                worst[q] = max(worst.get(q, 0.0), float(v))
            print("case", case, "seed", seed, "stats", res[f"c{ci}_s1_stats"].round(6).tolist())
            break
        else:
            raise AssertionError(f"no seed for {case}")
    print("float32 reference's relative distance from the float64 reference (max over cases):",
          {k: f"{v:.2e}" for k, v in sorted(worst.items())})
    res["ref32_distance_keys"] = np.array(sorted(worst))
    res["ref32_distance"] = np.array([worst[k] for k in sorted(worst)])
    statedict_and_signatures(res)
    path = os.path.join(HERE, "cac.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
