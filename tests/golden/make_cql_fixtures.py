"""Generate tests/golden/cql.npz by RUNNING THE REFERENCE's CQL and TD3BC (imitation/cql.py, imitation/td3_bc.py, imported
through oracle/ref_shim.py) in float64 and float32: per case two consecutive `_update_with_batch` calls (TD3BC: with TD3's
`_preprocess_batch` / `_postprocess_batch` around them) on a small hand-filled buffer.  The Gaussian draws (Normal.rsample's
_standard_normal, TD3's torch.randn) and CQL's uniform actions (Tensor.uniform_) are replaced by arrays drawn here and recorded
as data, so both runs and every test see the same draws.  The network modules are make_cac_fixtures.py's.  In the float64 run
`Tensor.float()` keeps float64: cql.py:291 rounds the target to float32 in any run, which a float64 yardstick must not.

Sizes: obs 6, act 3, hidden 16-16, B 12, R 3, buffer 4 x 16 (CQL: 16 steps, exactly full -- the reference's
`calibration_returns` has one entry per sampled row and is indexed by flat buffer row, which agree only then; TD3BC: 13 steps;
a seed is kept only if every sub-buffer holds a finished episode and ends in an unfinished tail).  CQL cases (`cql_cases`): with_lagrange, calibrated,
temperature, critic2=None, entropy alpha kind, min_action, max_action, alpha_max; TD3BC cases (`td3bc_cases`): n_step,
prioritized.  Per case `q{i}_` (CQL) / `t{i}_` (TD3BC):
  init_*                                     the initial flat vectors (float32 values)
  s{k}_indices, z_actor, z_target, z_cur, z_next, u (CQL); z_target, weight_in (TD3BC)
  s{k}_stats (float64 run), stats32; s{k}_target / returns, prio; s{k}_cql_log_alpha; `*_eref` = max |ref32 - ref64|
  s{k}_grad_{net}                            every gradient of the float64 run (the critics': before the clip), with `_eref`
  s1_w_{net}                                 every network after the second call, with `_eref`
  calib                                      `buffer.calibration_returns` by flat row (calibrated cases); leaves (prioritized)
The generator asserts that no ReLU pre-activation, no q1-versus-q2 gap of a real twin and no value-versus-calibration-return
gap lies within DELTA of zero, that pre-tanh values stay in range, and that the restatement (tests/cql_restatement.py) follows
the float64 run to 1e-10.  It prints the float32 run's distance from the float64 run per quantity.
"""
from __future__ import annotations

import inspect
import os

import numpy as np

import make_cac_fixtures as M  # noqa: E402  (installs the shim, through make_dqn_fixtures)
from make_cac_fixtures import (AD, B, D, FREQ, HID, LR, MAX_ACTION, N_ENV, NOISE_CLIP, PER_ALPHA, PER_BETA, POLICY_NOISE, S,  # noqa: E402
                               SAC_FIXED, SAC_LOG_ALPHA, SAC_TARGET_ENTROPY, T, TAU, Critic, DetActor, Kink, Noise, OutOfRange,
                               ProbActor, emax, fill, flat, params_of, ref_grad)
from make_dqn_fixtures import DELTA, GAMMA  # noqa: E402

import torch  # noqa: E402
import torch.distributions.normal as tdn  # noqa: E402
from tianshou.algorithm.imitation.cql import CQL  # noqa: E402
from tianshou.algorithm.imitation.td3_bc import TD3BC  # noqa: E402
from tianshou.algorithm.modelfree.ddpg import ContinuousDeterministicPolicy  # noqa: E402
from tianshou.algorithm.modelfree.sac import AutoAlpha, SACPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from cql_restatement import CqlRestatement, Td3bcRestatement, calibration_returns  # noqa: E402
from dqn_restatement import RestatedBuffer, nstep_walk  # noqa: E402
from dsac_restatement import alpha_state  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
R = 3
T_CQL = S   # CQL's buffer is exactly full: the reference indexes `calibration_returns` (one entry per SAMPLED row, in
#             sample(0) order) by flat buffer row, which agree only for a full buffer that has not wrapped
CQL_ALPHA_LR, CQL_WEIGHT, THRESHOLD, MAX_GRAD_NORM, BC_ALPHA = 3e-3, 1.0, 1.0, 1.0, 2.5
CQL_STAT_KEYS = ("actor_loss", "critic1_loss", "critic2_loss", "alpha", "alpha_loss", "cql_alpha", "cql_alpha_loss")
TD3_STAT_KEYS = ("actor_loss", "critic1_loss", "critic2_loss")
#            lagrange calibrated T  critic2=None alpha  min_action max_action alpha_max
CQL_CASES = [(1, 1, 1.0, 0, "fix", -1.0, 1.0, 1e6), (0, 0, 0.5, 0, "auto", -1.0, 1.0, 1e6), (1, 0, 0.5, 1, "fix", -1.0, 1.0, 1e6),
             (1, 1, 1.0, 0, "auto", -1.0, 2.0, 1e6), (1, 1, 1.0, 0, "fix", -1.0, 1.0, 0.5), (0, 1, 1.0, 0, "fix", -1.0, 1.0, 1e6)]
#              n_step prio
TD3BC_CASES = [(1, 0), (3, 1)]


class Draws(Noise):
    """make_cac_fixtures.Noise, and where Tensor.uniform_ stands while a queue of uniform actions is set."""

    def __init__(self) -> None:
        super().__init__()
        self.uniforms = []
        self._uniform_ = torch.Tensor.uniform_

    def uniform_(self, t, *a, **kw):
        if not self.uniforms:
            return self._uniform_(t, *a, **kw)
        u = self.uniforms.pop(0)
        assert tuple(u.shape) == tuple(t.shape), (u.shape, t.shape)
        return t.copy_(torch.as_tensor(u))


def fill_steps(rs, cls, dt, steps, **kw):
    """make_cac_fixtures.fill with the number of steps as an argument: the same draws per step, in the same order."""
    buf = cls(N_ENV * S, N_ENV, **kw)
    RB = RestatedBuffer(N_ENV, S, 1)
    for _ in range(steps):
        term, trunc = rs.rand(N_ENV) < 0.12, rs.rand(N_ENV) < 0.08
        rew = rs.standard_normal(N_ENV).astype(np.float32)
        b = Batch(obs=rs.standard_normal((N_ENV, D)).astype(np.float32).astype(dt),
                  act=rs.uniform(-1, 1, (N_ENV, AD)).astype(np.float32).astype(dt), rew=rew.astype(np.float64), terminated=term,
                  truncated=trunc, obs_next=rs.standard_normal((N_ENV, D)).astype(np.float32).astype(dt), info=Batch())
        buf.add(b, buffer_ids=np.arange(N_ENV))
        for e in range(N_ENV):
            RB.add(e, rew[e], bool(term[e]), bool(trunc[e]))
    return buf, RB


def stats_of(st, keys):
    return np.array([np.nan if getattr(st, k, None) is None else float(getattr(st, k)) for k in keys])


def catch_grads(algo) -> dict:
    """The gradient each optimizer steps with: the actor's at its torch step, the critics' where the reference clips them
    (before the clip: what the backward gives).  -> dict filled per call: net name -> flat float64 gradient."""
    got = {}
    inner = algo.policy_optim._optim.step

    def step(*a, **kw):
        got["actor"] = ref_grad(algo.policy.actor)
        return inner(*a, **kw)

    algo.policy_optim._optim.step = step
    return got


def sub_orders(buf) -> list:
    """Per sub-buffer the flat indices in time order, oldest first (nothing wraps: at most S steps)."""
    idx = buf.sample_indices(0)
    return [idx[(idx >= e * S) & (idx < (e + 1) * S)] for e in range(N_ENV)]


def prepare_nets(kind, seed):
    torch.manual_seed(seed)
    a_dims, c_dims = [D, *HID, 2 * AD if kind == "cql" else AD], [D + AD, *HID, 1]
    nets = (ProbActor(a_dims, False, True) if kind == "cql" else DetActor(a_dims), Critic(c_dims), Critic(c_dims))
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
    return nets, init, a_dims, c_dims


def copies(nets, dbl, no_c2):
    import copy

    cp = lambda n: copy.deepcopy(n).double() if dbl else copy.deepcopy(n)  # noqa: E731
    return cp(nets[0]), cp(nets[1]), (None if no_c2 else cp(nets[2]))


def check_buffer(buf) -> None:
    done = np.logical_or(buf.terminated, buf.truncated)
    for order in sub_orders(buf):
        if not done[order[:-1]].any() or done[order[-1]]:
            raise Kink   # every sub-buffer: a finished episode and an unfinished tail


def run_cql(ci, case, seed, draws):
    lag, cal, temp, no_c2, alpha_kind, amin_act, amax_act, alpha_max = case
    rs = np.random.RandomState(seed)
    nets, init, a_dims, c_dims = prepare_nets("cql", seed)
    if no_c2:
        init.pop("critic2")
    space = gym.spaces.Box(low=-1.0, high=1.0, shape=(AD,), dtype=np.float32)
    opt = lambda: AdamOptimizerFactory(lr=LR)  # noqa: E731
    bufs, algos, caught, clipped = {}, {}, {}, {}
    for dbl in (True, False):
        bufs[dbl], _ = fill_steps(np.random.RandomState(seed + 1000), VectorReplayBuffer, np.float64 if dbl else np.float32, T_CQL)
        check_buffer(bufs[dbl])
        actor, c1, c2 = copies(nets, dbl, no_c2)
        alpha = SAC_FIXED
        if alpha_kind == "auto":
            alpha = AutoAlpha(SAC_TARGET_ENTROPY, SAC_LOG_ALPHA, opt())
            alpha = alpha.double() if dbl else alpha
        algo = CQL(policy=SACPolicy(actor=actor, action_space=space), policy_optim=opt(), critic=c1, critic_optim=opt(), critic2=c2,
                   cql_alpha_lr=CQL_ALPHA_LR, cql_weight=CQL_WEIGHT, tau=TAU, gamma=GAMMA, alpha=alpha, temperature=temp,
                   with_lagrange=bool(lag), lagrange_threshold=THRESHOLD, min_action=amin_act, max_action=amax_act,
                   num_repeat_actions=R, alpha_min=0.0, alpha_max=alpha_max, max_grad_norm=MAX_GRAD_NORM, calibrated=bool(cal))
        if dbl:
            algo.cql_log_alpha.data = algo.cql_log_alpha.data.double()   # (the optimizer holds the same tensor)
        algo.policy.is_within_training_step = True
        algo.process_buffer(bufs[dbl])
        algos[dbl], caught[dbl] = algo, catch_grads(algo)
    buf64 = bufs[True]
    done_all = np.logical_or(buf64.terminated, buf64.truncated)
    calib_ref = np.asarray(buf64._meta.calibration_returns, np.float64) if cal else None
    if cal:
        mine = calibration_returns(buf64.rew, done_all, sub_orders(buf64), GAMMA)
        valid = buf64.sample_indices(0)
        assert np.allclose(mine[valid], calib_ref[valid], rtol=1e-12, atol=0)
    alpha = alpha_state(SAC_LOG_ALPHA) if alpha_kind == "auto" else SAC_FIXED
    Rst = CqlRestatement(init, a_dims, c_dims, TAU, GAMMA, lr=LR, max_action=MAX_ACTION, alpha=alpha, target_entropy=SAC_TARGET_ENTROPY,
                         alpha_lr=LR, cql_alpha_lr=CQL_ALPHA_LR, cql_weight=CQL_WEIGHT, temperature=temp, with_lagrange=bool(lag),
                         lagrange_threshold=THRESHOLD, num_repeat_actions=R, alpha_min=0.0, alpha_max=alpha_max,
                         max_grad_norm=MAX_GRAD_NORM, calibrated=bool(cal))
    allidx = buf64.sample_indices(0)
    pk = f"q{ci}_"
    new = {pk + "init_" + n: v for n, v in init.items()}
    if cal:
        new[pk + "calib"] = calib_ref
    dist = {}
    names = ["actor", "critic", "critic_old", "critic2", "critic2_old"]
    ref_net = lambda algo, n: {"actor": algo.policy.actor, "critic": algo.critic, "critic2": algo.critic2,  # noqa: E731
                               "critic_old": algo.critic_old.module, "critic2_old": algo.critic2_old.module}[n]
    for k in range(2):
        indices = rs.choice(allidx, B, replace=True).astype(np.int64)
        zs = [rs.standard_normal(shape).astype(np.float32) for shape in ((B, AD), (B, AD), (B * R, AD), (B * R, AD))]
        lo, hi = np.float32(-amin_act), np.float32(amax_act)
        u = (rs.rand(B * R, AD).astype(np.float32) * (hi - lo) + lo).astype(np.float32)
        out = {}
        for dbl, algo in algos.items():
            draws.queue, draws.uniforms = list(zs), [u]
            draws.dtype = torch.float64 if dbl else torch.float32
            caught[dbl].clear()
            clip_seen = []
            real_clip = torch.nn.utils.clip_grad_norm_

            def clip(params, max_norm, *a, _seen=clip_seen, **kw):
                params = list(params)
                _seen.append(np.concatenate([p.grad.detach().double().reshape(-1).numpy() for p in params]))
                return real_clip(params, max_norm, *a, **kw)

            torch.nn.utils.clip_grad_norm_ = clip
            real_float = torch.Tensor.float
            if dbl:
                torch.Tensor.float = lambda t: t.double()
            try:
                st = algo._update_with_batch(bufs[dbl][indices])
            finally:
                torch.nn.utils.clip_grad_norm_, torch.Tensor.float = real_clip, real_float
            assert not draws.queue and not draws.uniforms, "a draw was not consumed"
            assert len(clip_seen) == 2
            raw = algo.policy.actor.last_raw
            if float(raw[:, :AD].abs().max()) >= 3.0:
                raise OutOfRange
            out[dbl] = dict(stats=stats_of(st, CQL_STAT_KEYS), g=dict(caught[dbl], critic=clip_seen[0], critic2=clip_seen[1]),
                            w={n: flat(ref_net(algo, n)) for n in names}, la=float(algo.cql_log_alpha.detach().double()),
                            ela=float(algo.alpha._log_alpha.detach().double()) if alpha_kind == "auto" else np.nan)
        r64, r32 = out[True], out[False]
        b32 = bufs[False][indices]
        calib = calib_ref[indices] if cal else None   # (Batch.to_torch_ keeps a numpy array's dtype: float64 in both runs)
        r = Rst.update(b32.obs, b32.act, b32.rew, b32.done, b32.obs_next, calib, zs[0], zs[1], zs[2], zs[3], u)
        if Rst.kink <= DELTA or Rst.calib_gap <= DELTA:
            raise Kink
        mine = np.array([r["actor_loss"], r["critic1_loss"], r["critic2_loss"], r["alpha"],
                         np.nan if r["alpha_loss"] is None else r["alpha_loss"], np.nan if r["cql_alpha"] is None else r["cql_alpha"],
                         np.nan if r["cql_alpha_loss"] is None else r["cql_alpha_loss"]])
        assert np.allclose(mine, r64["stats"], rtol=1e-10, atol=1e-13, equal_nan=True), (case, k, mine, r64["stats"])
        assert np.isclose(r["cql_log_alpha"], r64["la"], rtol=1e-10, atol=1e-14), (case, k, r["cql_log_alpha"], r64["la"])
        for n in names:
            assert np.allclose(Rst.weights(n), r64["w"][n], rtol=1e-10, atol=1e-13), (case, k, n)
        for n, gv in r["grads"].items():
            assert np.allclose(gv, r64["g"][n], rtol=1e-10, atol=1e-15), (case, k, n, np.abs(gv - r64["g"][n]).max())
        sk = f"{pk}s{k}_"
        new.update({sk + "indices": indices, sk + "stats": r64["stats"], sk + "stats32": r32["stats"], sk + "z_actor": zs[0],
                    sk + "z_target": zs[1], sk + "z_cur": zs[2], sk + "z_next": zs[3], sk + "u": u,
                    sk + "target": r["target"], sk + "cql_log_alpha": np.array([r64["la"], r32["la"]]),
                    sk + "log_alpha": np.array([r64["ela"], r32["ela"]])})
        for n, gv in r64["g"].items():
            new.update({f"{sk}grad_{n}": gv, f"{sk}grad_{n}_eref": emax(gv, r32["g"][n])})
            dist[f"grad_{n}"] = max(dist.get(f"grad_{n}", 0.0), emax(gv, r32["g"][n]) / max(np.abs(gv).max(), 1e-300))
        dist["stats"] = max(dist.get("stats", 0.0), float(np.nanmax(np.abs(r64["stats"] - r32["stats"]) / np.abs(r64["stats"]))))
        dist["cql_log_alpha"] = max(dist.get("cql_log_alpha", 0.0), abs(r64["la"] - r32["la"]) / max(abs(r64["la"]), 1e-300))
        if k == 1:
            for n in names:
                new.update({f"{sk}w_{n}": r64["w"][n], f"{sk}w_{n}_eref": emax(r64["w"][n], r32["w"][n])})
                dist[f"w_{n}"] = max(dist.get(f"w_{n}", 0.0), emax(r64["w"][n], r32["w"][n]) / np.abs(r64["w"][n]).max())
    return new, dist


def run_td3bc(ci, case, seed, draws):
    n_step, prio = case
    rs = np.random.RandomState(seed)
    nets, init, a_dims, c_dims = prepare_nets("td3bc", seed)
    space = gym.spaces.Box(low=-1.0, high=1.0, shape=(AD,), dtype=np.float32)
    opt = lambda: AdamOptimizerFactory(lr=LR)  # noqa: E731
    cls, kw = (PrioritizedVectorReplayBuffer, dict(alpha=PER_ALPHA, beta=PER_BETA)) if prio else (VectorReplayBuffer, {})
    bufs, algos = {}, {}
    for dbl in (True, False):
        bufs[dbl], RB = fill(np.random.RandomState(seed + 1000), cls, np.float64 if dbl else np.float32, **kw)
        actor, c1, c2 = copies(nets, dbl, False)
        algos[dbl] = TD3BC(policy=ContinuousDeterministicPolicy(actor=actor, action_space=space), policy_optim=opt(), critic=c1,
                           critic_optim=opt(), critic2=c2, tau=TAU, gamma=GAMMA, policy_noise=POLICY_NOISE, update_actor_freq=FREQ,
                           noise_clip=NOISE_CLIP, alpha=BC_ALPHA, n_step_return_horizon=n_step)
    caught = {dbl: M.record_grads(a, "td3") for dbl, a in algos.items()}
    Rst = Td3bcRestatement(init, a_dims, c_dims, TAU, lr=LR, max_action=MAX_ACTION, policy_noise=POLICY_NOISE, noise_clip=NOISE_CLIP,
                           update_actor_freq=FREQ, bc_alpha=BC_ALPHA)
    allidx = bufs[True].sample_indices(0)
    pk = f"t{ci}_"
    new = {pk + "init_" + n: v for n, v in init.items()}
    dist = {}
    names = M.net_names("td3")
    for k in range(2):
        indices = rs.choice(allidx, B, replace=True).astype(np.int64)
        zt = rs.standard_normal((B, AD)).astype(np.float32)
        out = {}
        for dbl, algo in algos.items():
            buf = bufs[dbl]
            draws.queue, draws.dtype = [zt], torch.float64 if dbl else torch.float32
            caught[dbl].clear()
            batch = buf[indices]
            w_in = np.asarray(batch.weight, np.float64).copy() if prio else None
            batch = algo._preprocess_batch(batch, buf, indices)
            raw_t = algo.actor_old.module.last_raw
            st = algo._update_with_batch(batch)
            assert not draws.queue, "a draw was not consumed"
            algo._postprocess_batch(batch, buf, indices)
            for r_ in (raw_t, algo.policy.actor.last_raw):
                if float(r_.abs().max()) >= 3.0:
                    raise OutOfRange
            out[dbl] = dict(stats=stats_of(st, TD3_STAT_KEYS), ret=batch.returns.detach().double().numpy().reshape(-1),
                            prio=batch.weight.detach().double().numpy().reshape(-1), w_in=w_in, g=dict(caught[dbl]),
                            w={n: flat(M.ref_net(algo, n)) for n in names},
                            leaves=(buf.weight._value[buf.weight._bound:buf.weight._bound + N_ENV * S].copy() if prio else None))
        r64, r32 = out[True], out[False]
        b32 = bufs[False]
        idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
        r = Rst.update(b32[indices].obs, b32[indices].act, b32[idx_n].obs_next, mc, gpow, vmask, weight=r64["w_in"], z_target=zt)
        if Rst.kink <= DELTA:
            raise Kink
        stepped = k % FREQ == 0
        mine = np.array([r["actor_loss"], r["critic1_loss"], r["critic2_loss"]])
        assert np.allclose(mine, r64["stats"], rtol=1e-10, atol=0), (case, k, mine, r64["stats"])
        assert np.allclose(r["returns"], r64["ret"], rtol=1e-12, atol=1e-13) and np.allclose(r["prio"], r64["prio"], rtol=1e-10, atol=1e-13)
        for n in names:
            assert np.allclose(Rst.weights(n), r64["w"][n], rtol=1e-10, atol=1e-13), (case, k, n)
        assert set(r["grads"]) == set(r64["g"]) and ("actor" in r64["g"]) == stepped
        for n, gv in r["grads"].items():
            assert np.allclose(gv, r64["g"][n], rtol=1e-10, atol=1e-15), (case, k, n)
        sk = f"{pk}s{k}_"
        new.update({sk + "indices": indices, sk + "stats": r64["stats"], sk + "stats32": r32["stats"], sk + "z_target": zt,
                    sk + "returns": r64["ret"], sk + "returns_eref": emax(r64["ret"], r32["ret"]), sk + "prio": r64["prio"],
                    sk + "prio_eref": emax(r64["prio"], r32["prio"]), sk + "actor_stepped": np.bool_(stepped)})
        if prio:
            new.update({sk + "weight_in": r64["w_in"], sk + "weight_in_eref": emax(r64["w_in"], r32["w_in"])})
        for n, gv in r64["g"].items():
            new.update({f"{sk}grad_{n}": gv, f"{sk}grad_{n}_eref": emax(gv, r32["g"][n])})
            dist[f"grad_{n}"] = max(dist.get(f"grad_{n}", 0.0), emax(gv, r32["g"][n]) / max(np.abs(gv).max(), 1e-300))
        for q in ("ret", "prio"):
            dist[q] = max(dist.get(q, 0.0), emax(r64[q], r32[q]) / np.abs(r64[q]).max())
        dist["stats"] = max(dist.get("stats", 0.0), float(np.max(np.abs(r64["stats"] - r32["stats"]) / np.abs(r64["stats"]))))
        if k == 1:
            for n in names:
                new.update({f"{sk}w_{n}": r64["w"][n], f"{sk}w_{n}_eref": emax(r64["w"][n], r32["w"][n])})
            if prio:
                new.update({pk + "leaves": r64["leaves"], pk + "leaves_eref": emax(r64["leaves"], r32["leaves"])})
    return new, dist


def signatures(res):
    for cls in (CQL, TD3BC):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    draws = Draws()
    torch.randn = draws.randn
    tdn._standard_normal = draws.standard_normal
    torch.Tensor.uniform_ = lambda t, *a, **kw: draws.uniform_(t, *a, **kw)
    res = dict(delta=np.float64(DELTA), gamma=np.float64(GAMMA), tau=np.float64(TAU), lr=np.float64(LR),
               dims=np.array([D, AD, *HID, B, N_ENV, S, T, R, T_CQL], np.int64), max_action=np.float64(MAX_ACTION),
               per=np.array([PER_ALPHA, PER_BETA]), td3=np.array([POLICY_NOISE, NOISE_CLIP, FREQ, BC_ALPHA]),
               sac=np.array([SAC_FIXED, SAC_LOG_ALPHA, SAC_TARGET_ENTROPY]),
               cql=np.array([CQL_ALPHA_LR, CQL_WEIGHT, THRESHOLD, MAX_GRAD_NORM]), cql_stat_keys=np.array(CQL_STAT_KEYS),
               td3_stat_keys=np.array(TD3_STAT_KEYS), cql_cases=np.array(["|".join(str(v) for v in c) for c in CQL_CASES]),
               td3bc_cases=np.array(["|".join(str(v) for v in c) for c in TD3BC_CASES]))
    worst = {}
    for tag, cases, run in (("q", CQL_CASES, run_cql), ("t", TD3BC_CASES, run_td3bc)):
        for ci, case in enumerate(cases):
            base = 301 + 7 * ci + (100 if tag == "t" else 0)
            for seed in range(base, base + 200):   # the first seed that keeps DELTA away from every kink, values in range
                try:
                    new, dist = run(ci, case, seed, draws)
                except (Kink, OutOfRange):
                    continue
                res.update(new)
                res[f"{tag}{ci}_seed"] = np.int64(seed)
                for q, v in dist.items():
                    worst[f"{tag}_{q}"] = max(worst.get(f"{tag}_{q}", 0.0), float(v))
                print("case", tag, case, "seed", seed, "stats", res[f"{tag}{ci}_s1_stats"].round(6).tolist())
                break
            else:
                raise AssertionError(f"no seed for {case}")
    print("float32 reference's relative distance from the float64 reference (max over cases):",
          {k: f"{v:.2e}" for k, v in sorted(worst.items())})
    res["ref32_distance_keys"] = np.array(sorted(worst))
    res["ref32_distance"] = np.array([worst[k] for k in sorted(worst)])
    signatures(res)
    path = os.path.join(HERE, "cql.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
