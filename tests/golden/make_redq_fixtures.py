"""Generate tests/golden/redq.npz by RUNNING THE REFERENCE's REDQ (redq.py, imported through oracle/ref_shim.py) in float64 and
float32: per case three consecutive `_preprocess_batch` + `_update_with_batch` (+ `_postprocess_batch`) calls with
actor_delay = 2 on a small hand-filled buffer, so a call that does not step the actor, one that does and the call after it are
all there.  The Gaussian draws (Normal.rsample's _standard_normal) and the subset indices (np.random.choice) are replaced by
arrays drawn here and recorded as data, so both runs and every test see the same noise and the same subsets.  The network
modules are defined here: `ProbActor` is make_cac_fixtures' (conditioned sigma), `EnsCritic` stacks the reference's own
`EnsembleLinear` (utils/net/common.py:522-554) the way ContinuousCritic(Net(linear_layer=EnsembleLinear)) does -- the
reference's Net casts observations to float32, which a float64 run cannot use.

Sizes: obs 6, act 3, hidden 16-16, B 12, buffer 4 x 16.  Cases (`cases`): E | M | mode | n_step | prioritized | alpha kind.
Per case `c{i}_`:
  init_actor, init_critic     the initial flat vectors (float32 values; the critic in the ensemble layout, per layer
                              weight [E, in, out] then bias_weights [E, 1, out])
  s{k}_indices, subset, z_target, z_actor (stepping calls), weight_in (prioritized)
  s{k}_returns, prio, stats (float64 run), stats32, and `*_eref` = max |ref32 - ref64|
  s{k}_grad_{net}             every gradient of the float64 run, with `_eref`;  s{k}_log_alpha;  s{k}_actor_stepped
  s2_w_{net}                  every network after the last call, with `_eref`
  leaves                      the sum tree's leaves after the last call (prioritized cases)
  sd_* / sig_*                reference state_dict keys and shapes (Net + ContinuousActorProbabilistic / ContinuousCritic over
                              EnsembleLinear), signatures, the statistics' fields
The generator asserts that actor pre-tanh values stay within +-3, that no ReLU pre-activation lies within DELTA of zero, and
that the restatement (tests/redq_restatement.py) follows the float64 run to 1e-10.  It prints the float32 run's distance from
the float64 run per quantity.
"""
from __future__ import annotations

import copy
import dataclasses
import inspect
import os

import numpy as np

from make_cac_fixtures import (AD, B, D, HID, LR, MAX_ACTION, N_ENV, PER_ALPHA, PER_BETA, S, SAC_FIXED, SAC_LOG_ALPHA,  # noqa: E402
                               SAC_TARGET_ENTROPY, T, TAU, Kink, Noise, OutOfRange, ProbActor, emax, fill, flat, params_of,
                               record_grads, ref_grad)   # (installs the shim)
from make_dqn_fixtures import DELTA, GAMMA  # noqa: E402

import torch  # noqa: E402
from torch import nn  # noqa: E402
import torch.distributions.normal as tdn  # noqa: E402
from tianshou.algorithm.modelfree.redq import REDQ, REDQPolicy, REDQTrainingStats  # noqa: E402
from tianshou.algorithm.modelfree.sac import AutoAlpha  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import EnsembleLinear, Net  # noqa: E402
from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from dqn_restatement import nstep_walk  # noqa: E402
from redq_restatement import RedqRestatement, alpha_state  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ACTOR_DELAY, N_CALLS = 2, 3
STAT_KEYS = ("actor_loss", "critic_loss", "alpha", "alpha_loss")
NETS = ("actor", "critic", "critic_old")
#         E  M  mode   n_step prio alpha
CASES = [(4, 2, "min", 1, 0, "fix"), (4, 2, "mean", 3, 1, "auto"), (3, 3, "min", 1, 0, "fix"), (1, 1, "min", 1, 0, "auto")]


class EnsCritic(nn.Module):
    def __init__(self, dims, E) -> None:
        super().__init__()
        self.layers = nn.ModuleList([EnsembleLinear(E, dims[i], dims[i + 1]) for i in range(len(dims) - 1)])

    def forward(self, obs, act=None, info=None):
        w = self.layers[0].weight
        as_t = lambda v: (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(w.dtype).flatten(1)  # noqa: E731
        x = torch.cat([as_t(obs), as_t(act)], 1)
        for i, l in enumerate(self.layers):
            x = l(x)
            if i < len(self.layers) - 1:
                x = torch.relu(x)
        return x   # [E, B, 1]


def make_algo(nets, dbl, E, M, mode, n_step, alpha_kind):
    cp = lambda n: copy.deepcopy(n).double() if dbl else copy.deepcopy(n)  # noqa: E731
    space = gym.spaces.Box(low=-1.0, high=1.0, shape=(AD,), dtype=np.float32)
    opt = lambda: AdamOptimizerFactory(lr=LR)  # noqa: E731
    alpha = SAC_FIXED
    if alpha_kind == "auto":
        alpha = AutoAlpha(SAC_TARGET_ENTROPY, SAC_LOG_ALPHA, opt())
        alpha = alpha.double() if dbl else alpha
    return REDQ(policy=REDQPolicy(actor=cp(nets[0]), action_space=space), policy_optim=opt(), critic=cp(nets[1]),
                critic_optim=opt(), ensemble_size=E, subset_size=M, tau=TAU, gamma=GAMMA, alpha=alpha,
                n_step_return_horizon=n_step, actor_delay=ACTOR_DELAY, target_mode=mode)


def ref_net(algo, name):
    return {"actor": lambda: algo.policy.actor, "critic": lambda: algo.critic, "critic_old": lambda: algo.critic_old.module}[name]()


def stats_of(st):
    return np.array([np.nan if getattr(st, k, None) is None else float(getattr(st, k)) for k in STAT_KEYS])


def run_case(ci, case, seed, noise):
    E, M, mode, n_step, prio, alpha_kind = case
    rs = np.random.RandomState(seed)
    torch.manual_seed(seed)
    a_dims, c_dims = [D, *HID, 2 * AD], [D + AD, *HID, 1]
    nets = (ProbActor(a_dims, False, True), EnsCritic(c_dims, E))
    with torch.no_grad():   # keep pre-tanh values small: the last layer's weights shrink
        for p in nets[0].layers[-1].parameters():
            p.mul_(0.6)
    init = {n: flat(m).astype(np.float32) for n, m in zip(("actor", "critic"), nets)}
    for m, n in zip(nets, ("actor", "critic")):   # the float32 values are the weights of both runs
        o = 0
        with torch.no_grad():
            for q in params_of(m):
                q.copy_(torch.as_tensor(init[n][o:o + q.numel()]).reshape(q.shape))
                o += q.numel()
    cls, kw = (PrioritizedVectorReplayBuffer, dict(alpha=PER_ALPHA, beta=PER_BETA)) if prio else (VectorReplayBuffer, {})
    bufs, algos = {}, {}
    for dbl in (True, False):
        bufs[dbl], RB = fill(np.random.RandomState(seed + 1000), cls, np.float64 if dbl else np.float32, **kw)
        algos[dbl] = make_algo(nets, dbl, E, M, mode, n_step, alpha_kind)
        algos[dbl].policy.is_within_training_step = True   # the policy samples (deterministic_eval acts outside of it only)
    caught = {dbl: record_grads(a, "ddpg") for dbl, a in algos.items()}
    alpha = alpha_state(SAC_LOG_ALPHA) if alpha_kind == "auto" else SAC_FIXED
    R = RedqRestatement(init, a_dims, c_dims, E, M, mode, TAU, lr=LR, actor_delay=ACTOR_DELAY, max_action=MAX_ACTION,
                        alpha=alpha, target_entropy=SAC_TARGET_ENTROPY, alpha_lr=LR)
    allidx = bufs[True].sample_indices(0)
    pk = f"c{ci}_"
    new = {pk + "init_" + n: v for n, v in init.items()}
    dist = {}
    for k in range(N_CALLS):
        stepped = (k + 1) % ACTOR_DELAY == 0
        indices = rs.choice(allidx, B, replace=True).astype(np.int64)
        subset = rs.choice(E, M, replace=False).astype(np.int64)
        zt = rs.standard_normal((B, AD)).astype(np.float32)
        za = rs.standard_normal((B, AD)).astype(np.float32) if stepped else None
        out = {}
        for dbl, algo in algos.items():
            buf = bufs[dbl]
            noise.queue = [z for z in (zt, za) if z is not None]
            subsets = [subset]
            caught[dbl].clear()
            noise.dtype = torch.float64 if dbl else torch.float32
            batch = buf[indices]
            w_in = np.asarray(batch.weight, np.float64).copy() if prio else None
            keep = np.random.choice

            def choice(a, size=None, replace=True, p=None):   # stands where redq.py:258 draws
                assert (a, size, replace) == (E, M, False)
                return subsets.pop(0)

            np.random.choice = choice
            try:
                batch = algo._preprocess_batch(batch, buf, indices)
            finally:
                np.random.choice = keep
            assert not subsets, "the subset was not drawn"
            raw_t = algo.policy.actor.last_raw
            st = algo._update_with_batch(batch)
            assert not noise.queue, "a draw was not consumed"
            algo._postprocess_batch(batch, buf, indices)
            raws = [raw_t] + ([algo.policy.actor.last_raw] if stepped else [])
            for r, z in zip(raws, (zt, za)):   # pre-tanh values of mu within +-3, of the sampled action within +-3.5
                if float(r[:, :AD].abs().max()) >= 3.0:
                    raise OutOfRange
                pre = MAX_ACTION * torch.tanh(r[:, :AD]) + torch.clamp(r[:, AD:], -20, 2).exp() * torch.as_tensor(z).to(r.dtype)
                if float(pre.abs().max()) >= 3.5:
                    raise OutOfRange
            out[dbl] = dict(stats=stats_of(st), ret=batch.returns.detach().double().numpy().reshape(-1),
                            prio=batch.weight.detach().double().numpy().reshape(-1), w_in=w_in, g=dict(caught[dbl]),
                            w={n: flat(ref_net(algo, n)) for n in NETS},
                            la=float(algo.alpha._log_alpha.detach().double()) if alpha_kind == "auto" else np.nan,
                            leaves=(buf.weight._value[buf.weight._bound:buf.weight._bound + N_ENV * S].copy() if prio else None))
        r64, r32 = out[True], out[False]
        b32 = bufs[False]
        idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
        r = R.update(b32[indices].obs, b32[indices].act, b32[idx_n].obs_next, mc, gpow, vmask, subset, weight=r64["w_in"],
                     z_target=zt, z_actor=za)
        if R.kink <= DELTA:
            raise Kink
        mine = np.array([r["actor_loss"], r["critic_loss"], r["alpha"], np.nan if r["alpha_loss"] is None else r["alpha_loss"]])
        assert np.allclose(mine, r64["stats"], rtol=1e-10, atol=0, equal_nan=True), (case, k, mine, r64["stats"])
        assert np.allclose(r["returns"], r64["ret"], rtol=1e-12, atol=1e-13) and np.allclose(r["prio"], r64["prio"], rtol=1e-10, atol=1e-13)
        for n in NETS:
            assert np.allclose(R.weights(n), r64["w"][n], rtol=1e-10, atol=1e-13), (case, k, n)
        assert set(r["grads"]) == set(r64["g"]) and ("actor" in r64["g"]) == stepped
        for n, gv in r["grads"].items():
            assert np.allclose(gv, r64["g"][n], rtol=1e-10, atol=1e-15), (case, k, n, np.abs(gv - r64["g"][n]).max())
        sk = f"{pk}s{k}_"
        new.update({sk + "indices": indices, sk + "subset": subset, sk + "z_target": zt, sk + "stats": r64["stats"],
                    sk + "stats32": r32["stats"], sk + "returns": r64["ret"], sk + "returns_eref": emax(r64["ret"], r32["ret"]),
                    sk + "prio": r64["prio"], sk + "prio_eref": emax(r64["prio"], r32["prio"]),
                    sk + "log_alpha": np.array([r64["la"], r32["la"]]), sk + "actor_stepped": np.bool_(stepped)})
        if za is not None:
            new[sk + "z_actor"] = za
        if prio:
            new.update({sk + "weight_in": r64["w_in"], sk + "weight_in_eref": emax(r64["w_in"], r32["w_in"])})
        for n, gv in r64["g"].items():
            new.update({f"{sk}grad_{n}": gv, f"{sk}grad_{n}_eref": emax(gv, r32["g"][n])})
            dist[f"grad_{n}"] = max(dist.get(f"grad_{n}", 0.0), emax(gv, r32["g"][n]) / max(np.abs(gv).max(), 1e-300))
        for q in ("ret", "prio"):
            dist[q] = max(dist.get(q, 0.0), emax(r64[q], r32[q]) / np.abs(r64[q]).max())
        ok = ~np.isnan(r64["stats"]) & (r64["stats"] != 0)
        dist["stats"] = max(dist.get("stats", 0.0), float(np.max(np.abs(r64["stats"] - r32["stats"])[ok] / np.abs(r64["stats"][ok]))))
        if k == N_CALLS - 1:
            for n in NETS:
                new.update({f"{sk}w_{n}": r64["w"][n], f"{sk}w_{n}_eref": emax(r64["w"][n], r32["w"][n])})
            if prio:
                new.update({pk + "leaves": r64["leaves"], pk + "leaves_eref": emax(r64["leaves"], r32["leaves"])})
    return new, dist


def statedict_and_signatures(res):
    torch.manual_seed(0)
    E = 4
    space = gym.spaces.Box(low=-1.0, high=1.0, shape=(AD,), dtype=np.float32)
    lin = lambda x, y: EnsembleLinear(E, x, y)  # noqa: E731
    crit = ContinuousCritic(preprocess_net=Net(state_shape=(D,), action_shape=(AD,), hidden_sizes=HID, concat=True, linear_layer=lin),
                            linear_layer=lin, flatten_input=False)
    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(D,), hidden_sizes=HID), action_shape=(AD,),
                                         conditioned_sigma=True)
    opt = lambda: AdamOptimizerFactory(lr=LR)  # noqa: E731
    algo = REDQ(policy=REDQPolicy(actor=actor, action_space=space), policy_optim=opt(), critic=crit, critic_optim=opt(),
                ensemble_size=E, alpha=AutoAlpha(SAC_TARGET_ENTROPY, SAC_LOG_ALPHA, opt()))
    sd = {k: v for k, v in algo.state_dict().items() if isinstance(v, torch.Tensor)}
    res["sd_redq_keys"] = np.array(list(sd.keys()))
    res["sd_redq_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    res["sd_ensemble_size"] = np.int64(E)
    for cls in (REDQPolicy, REDQ):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])
    res["stats_fields"] = np.array([f.name for f in dataclasses.fields(REDQTrainingStats)])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    noise = Noise()
    tdn._standard_normal = noise.standard_normal
    res = dict(delta=np.float64(DELTA), gamma=np.float64(GAMMA), tau=np.float64(TAU), lr=np.float64(LR),
               dims=np.array([D, AD, *HID, B, N_ENV, S, T], np.int64), max_action=np.float64(MAX_ACTION),
               per=np.array([PER_ALPHA, PER_BETA]), sac=np.array([SAC_FIXED, SAC_LOG_ALPHA, SAC_TARGET_ENTROPY]),
               actor_delay=np.int64(ACTOR_DELAY), n_calls=np.int64(N_CALLS), stat_keys=np.array(STAT_KEYS),
               cases=np.array(["|".join(str(v) for v in c) for c in CASES]))
    worst = {}
    for ci, case in enumerate(CASES):
        for seed in range(301 + 7 * ci, 401 + 7 * ci):   # the first seed whose calls keep DELTA away from every kink and pre-tanh values in range
            try:
                new, dist = run_case(ci, case, seed, noise)
            except (Kink, OutOfRange):
                continue
            res.update(new)
            res[f"c{ci}_seed"] = np.int64(seed)
            for q, v in dist.items():
                worst[q] = max(worst.get(q, 0.0), float(v))
            print("case", case, "seed", seed, "stats", res[f"c{ci}_s{N_CALLS - 1}_stats"].round(6).tolist())
            break
        else:
            raise AssertionError(f"no seed for {case}")
    print("float32 reference's relative distance from the float64 reference (max over cases):",
          {k: f"{v:.2e}" for k, v in sorted(worst.items())})
    res["ref32_distance_keys"] = np.array(sorted(worst))
    res["ref32_distance"] = np.array([worst[k] for k in sorted(worst)])
    statedict_and_signatures(res)
    path = os.path.join(HERE, "redq.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
