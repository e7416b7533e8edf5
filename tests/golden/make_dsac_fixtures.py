"""Generate tests/golden/dsac.npz by RUNNING THE REFERENCE's DiscreteSAC, DiscreteSACPolicy, FixedAlpha and AutoAlpha
(discrete_sac.py, sac.py, imported through oracle/ref_shim.py) in float64 and float32, with e_ref = max |ref32 - ref64| per
array.  The network modules are defined here (`ActorNet`, `CriticNet`, `ActorTable`, `CriticTable`: the reference's Net casts
observations to float32, which a float64 run cannot use).  In a float64 run `AutoAlpha` is `.double()`d as the nets are.

The reference samples an action in `policy(batch)` -- once for the target (ddpg.py:312) and once in the update
(discrete_sac.py:177) -- that neither the target nor the loss reads: it only advances torch's RNG, so nothing recorded here
depends on it.

Sections (every array is data: inputs, indices, initial weights, expected outputs; large float64 arrays as digests):
  hd_*   head inputs per A in {2, 5, 64}, B = 37: logits / lnext / q1 / q2 / q1n / q2n as i16 = 8 x the value (a lattice of
         eighths, exact in float32), act, mc, gpow, vmask, weight.  Row 3 of logits and lnext has two equal top logits; row 7
         has one logit 40 below the rest (p tiny but positive); row 5 has vmask = 0.  q2 - q1 is never zero.
  tg_*   DiscreteSAC._target_q + the n-step line, for fixed alpha 0.25 and AutoAlpha(log_alpha = -1).
  hc_*   DiscreteSAC._update_with_batch around table "networks" whose gradients ARE d loss / d output, over the grid
         {weight, none} x {fixed alpha, AutoAlpha}; the critics' optimisers have lr = 0 so that the actor loss reads the
         critics the fixture holds.
  up_*   three consecutive updates on dqn.npz's buffer script (nets 6-32-32-5, B = 37, n_step 3, tau 0.05, lr 1e-3), for
         alpha = 0.2 (`fix`) and AutoAlpha(0.98 log 5, 0, lr 1e-3) (`auto`): losses, returns, weight digests of all five
         nets, log_alpha, and the mean entropy of the restatement (which the generator pins to the reference).
  pr_*   two updates in front of the reference's PrioritizedVectorReplayBuffer: indices, IS weights, losses, leaves.
  ma_*   MultiAgentOffPolicyAlgorithm with a fixed-alpha and an auto-alpha agent on dqn.npz's AEC rows WITHOUT masks.
  sd_*   reference state_dict keys and shapes (DiscreteActor / DiscreteCritic around Net);  sig_*  constructor signatures.
The generator asserts, in the hd / up / pr / ma sections alike, that no ReLU pre-activation and no q1-versus-q2 gap it uses
lies within DELTA of zero (the `min` is the only other non-smooth point) and that the restatement (tests/dsac_restatement.py)
follows the reference's float64 run to 1e-10.
"""
from __future__ import annotations

import copy
import inspect
import os

import numpy as np

from make_dqn_fixtures import DELTA, GAMMA, FakeEnv, QNet, _Rows, digest, flat  # noqa: E402  (installs the shim)
from make_distq_fixtures import emax, up_buffers  # noqa: E402

import torch  # noqa: E402
from torch import nn  # noqa: E402
from tianshou.algorithm.modelfree.discrete_sac import DiscreteSAC, DiscreteSACPolicy  # noqa: E402
from tianshou.algorithm.modelfree.sac import Alpha, AutoAlpha, FixedAlpha  # noqa: E402
from tianshou.algorithm.multiagent.marl import MultiAgentOffPolicyAlgorithm  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import Net  # noqa: E402
from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from dqn_restatement import RestatedBuffer, nstep_walk  # noqa: E402
from dsac_restatement import DsacRestatement, actor_head, critic_head, target  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ACTS = (2, 5, 64)
B_HEAD = 37
HEAD_FIXED, HEAD_LOG_ALPHA, HEAD_TARGET_ENTROPY = 0.25, -1.0, 0.7
UP_FIXED, TAU, LR = 0.2, 0.05, 1e-3
UP_TARGET_ENTROPY = 0.98 * float(np.log(5.0))
STAT_KEYS = ("actor_loss", "critic1_loss", "critic2_loss", "alpha", "alpha_loss")


def _rows(obs):
    return np.asarray(obs.obs if isinstance(obs, Batch) else obs)


class ActorNet(QNet):
    def forward(self, obs, state=None, info=None):
        return super().forward(_rows(obs), state, info)


class CriticNet(QNet):
    def forward(self, obs, state=None, info=None):
        return super().forward(_rows(obs), state, info)[0]


class ActorTable(nn.Module):
    """obs[:, 0] is a row number into a table of logits."""

    def __init__(self, table) -> None:
        super().__init__()
        self.table = nn.Parameter(torch.as_tensor(table))

    def forward(self, obs, state=None, info=None):
        return self.table[torch.as_tensor(_rows(obs)[:, 0]).long()], state


class CriticTable(ActorTable):
    def forward(self, obs, state=None, info=None):
        return super().forward(obs)[0]


def make_alpha(kind, dbl, log_alpha=0.0, target_entropy=UP_TARGET_ENTROPY, fixed=UP_FIXED):
    if kind == "fix":
        return fixed
    a = AutoAlpha(target_entropy, log_alpha, AdamOptimizerFactory(lr=LR))
    return a.double() if dbl else a


def make_algo(actor, critic, critic2, A, alpha, critic_lr=LR, **kw):
    pol = DiscreteSACPolicy(actor=actor, action_space=gym.spaces.Discrete(A))
    return DiscreteSAC(policy=pol, policy_optim=AdamOptimizerFactory(lr=LR), critic=critic,
                       critic_optim=AdamOptimizerFactory(lr=critic_lr), critic2=critic2, tau=TAU, gamma=GAMMA, alpha=alpha, **kw)


def stats_of(stats):
    return np.array([np.nan if getattr(stats, k) is None else float(getattr(stats, k)) for k in STAT_KEYS])


def log_alpha_of(algo):
    return float(algo.alpha._log_alpha.detach().double()) if isinstance(algo.alpha, AutoAlpha) else np.nan


# ---- hd / tg / hc -------------------------------------------------------------------------------------------------------
def head_inputs(rs, A):
    B = B_HEAD
    lat = lambda lo=-24, hi=25: rs.randint(lo, hi, (B, A)).astype(np.int16)  # noqa: E731
    d = dict(logits=lat(), lnext=lat(), q1=lat(-40, 41), q1n=lat(-40, 41))
    for k in ("logits", "lnext"):
        x = d[k]
        x[3] = np.minimum(x[3], 10)
        x[3, 0] = x[3, A - 1] = 16                      # two equal top logits
        x[7, 1] = x[7].min() - 8 * 40                   # one logit 40 below the rest
    for k in ("q1", "q1n"):                             # q2 = q1 + a non-zero lattice offset: min(q1, q2) has no tie
        off = rs.randint(1, 17, (B, A)) * rs.choice([-1, 1], (B, A))
        d[k.replace("1", "2")] = (d[k] + off).astype(np.int16)
    d["act"] = rs.randint(0, A, B).astype(np.int64)
    d["mc"] = (2.0 * rs.standard_normal(B)).astype(np.float32).astype(np.float64)
    d["gpow"] = (GAMMA ** rs.randint(1, 4, B)).astype(np.float32).astype(np.float64)
    d["vmask"] = rs.rand(B) > 0.2
    d["vmask"][5] = False
    d["weight"] = (0.5 + rs.rand(B)).astype(np.float32)
    return d


def head_sections(res):
    rs = np.random.RandomState(17)
    res["hc_cases"] = np.array([f"w{w}a{a}" for w in (0, 1) for a in (0, 1)])
    res.update(hd_fixed=np.float64(HEAD_FIXED), hd_log_alpha=np.float64(HEAD_LOG_ALPHA), hd_target_entropy=np.float64(HEAD_TARGET_ENTROPY))
    for A in ACTS:
        inp = head_inputs(rs, A)
        p = f"A{A}_"
        res.update({"hd_" + p + k: v for k, v in inp.items()})
        B = B_HEAD
        f = {k: inp[k].astype(np.float64) / 8.0 for k in ("logits", "lnext", "q1", "q2", "q1n", "q2n")}
        act, mc, gpow, vmask, weight = (inp[k] for k in ("act", "mc", "gpow", "vmask", "weight"))
        assert np.abs(f["q1"] - f["q2"]).min() > DELTA and np.abs(f["q1n"] - f["q2n"]).min() > DELTA
        rows = np.arange(B, dtype=np.float32).reshape(B, 1)

        def algo_of(dbl, auto, lr_c=0.0):
            ndt = np.float64 if dbl else np.float32
            stack = lambda a, b: np.concatenate([f[a], f[b]]).astype(ndt)  # noqa: E731
            actor, c1, c2 = ActorTable(stack("logits", "lnext")), CriticTable(stack("q1", "q1n")), CriticTable(stack("q2", "q2n"))
            alpha = make_alpha("auto" if auto else "fix", dbl, HEAD_LOG_ALPHA, HEAD_TARGET_ENTROPY, HEAD_FIXED)
            return make_algo(actor, c1, c2, A, alpha, critic_lr=lr_c), actor, c1, c2

        # -- tg: the soft target through the reference's own _target_q, then the n-step line
        for auto in (0, 1):
            out = {}
            for dbl in (True, False):
                algo, *_ = algo_of(dbl, auto)
                tq = algo._target_q(_Rows(rows + B), np.arange(B)).detach().numpy().reshape(B, 1).copy()
                assert tq.dtype == (np.float64 if dbl else np.float32)
                tq *= vmask.reshape(-1, 1)                                        # algorithm_base.py:796
                out[dbl] = (tq * gpow.reshape(B, 1) + mc.reshape(B, 1)).reshape(B).astype(np.float64)   # :1213-1215
                if dbl:
                    alpha_value = algo.alpha.value
            mine = target(f["lnext"], f["q1n"], f["q2n"], alpha_value if auto else HEAD_FIXED, mc, gpow, vmask)
            assert np.allclose(mine, out[True], rtol=1e-12, atol=1e-13), (A, auto)
            res.update({f"tg_{p}a{auto}_returns": out[True], f"tg_{p}a{auto}_returns_eref": emax(out[True], out[False])})
        # -- hc: the update around tables
        keep = {k: [] for k in ("stats", "stats32", "prio", "prio_eref", "dq_eref", "dl_eref", "ent_eref", "log_alpha")}
        for c, (wgt, auto) in enumerate((w, a) for w in (0, 1) for a in (0, 1)):
            out = {}
            for dbl in (True, False):
                dt = torch.float64 if dbl else torch.float32
                algo, actor, c1, c2 = algo_of(dbl, auto)
                ret = target(f["lnext"], f["q1n"], f["q2n"], algo.alpha.value, mc, gpow, vmask)
                batch = Batch(obs=rows, act=act, returns=torch.as_tensor(ret).to(dt), info=Batch())
                if wgt:
                    batch.weight = torch.as_tensor(weight).to(dt)
                alpha_before = algo.alpha.value
                stats = algo._update_with_batch(batch)
                assert torch.equal(c1.table.detach()[:B], torch.as_tensor(f["q1"]).to(dt))   # lr = 0: the critics stay
                out[dbl] = dict(stats=stats_of(stats), prio=batch.weight.detach().double().numpy(), alpha=alpha_before,
                                dq1=c1.table.grad[:B].double().numpy(), dq2=c2.table.grad[:B].double().numpy(),
                                dl=actor.table.grad[:B].double().numpy(), la=log_alpha_of(algo), ret=ret)
                assert not actor.table.grad[B:].any() and not c1.table.grad[B:].any()
            r64, r32 = out[True], out[False]
            ch = critic_head(f["q1"], f["q2"], act, r64["ret"], weight if wgt else None)
            ah = actor_head(f["logits"], f["q1"], f["q2"], r64["alpha"])
            assert np.allclose(ch["dq1"], r64["dq1"], rtol=1e-12, atol=1e-16) and np.allclose(ch["dq2"], r64["dq2"], rtol=1e-12, atol=1e-16)
            assert np.allclose(ch["prio"], r64["prio"], rtol=1e-12, atol=1e-14)
            assert np.allclose(ah["d_logits"], r64["dl"], rtol=1e-10, atol=1e-15), np.abs(ah["d_logits"] - r64["dl"]).max()
            assert np.allclose([ah["loss"], ch["loss1"], ch["loss2"]], r64["stats"][:3], rtol=1e-12, atol=0)
            assert np.count_nonzero(r64["dq1"]) <= B and (ah["entropy"] > 0).all() and ah["entropy"][7] > 0
            ent32 = actor_head(f["logits"].astype(np.float32), f["q1"], f["q2"], r64["alpha"])["entropy"]
            for k, v in (("stats", r64["stats"]), ("stats32", r32["stats"]), ("prio", r64["prio"]), ("prio_eref", emax(r64["prio"], r32["prio"])),
                         ("dq_eref", max(emax(r64["dq1"], r32["dq1"]), emax(r64["dq2"], r32["dq2"]))),
                         ("dl_eref", emax(r64["dl"], r32["dl"])), ("ent_eref", emax(ah["entropy"], ent32)),
                         ("log_alpha", [r64["la"], r32["la"]])):
                keep[k].append(np.asarray(v, np.float64))
            digest(res, f"hc_{p}c{c}_dl", r64["dl"].reshape(-1))
        res.update({f"hc_{p}{k}": np.stack(v) for k, v in keep.items()})
        print("heads", A, "stats", res[f"hc_{p}stats"][1])


# ---- up / pr ------------------------------------------------------------------------------------------------------------
DIMS = [6, 32, 32, 5]
NETS = ("actor", "critic", "critic2", "critic_old", "critic2_old")


def ref_flat(algo, name):
    return flat({"actor": algo.policy.actor, "critic": algo.critic, "critic2": algo.critic2, "critic_old": algo.critic_old.module,
                 "critic2_old": algo.critic2_old.module}[name])


def ref_grad(net):
    return np.concatenate([q.grad.detach().double().reshape(-1).numpy() for q in net.parameters()])


def fresh_nets(seed):
    torch.manual_seed(seed)
    return ActorNet(DIMS), CriticNet(DIMS), CriticNet(DIMS)


def algos_of(nets, kind, **kw):
    cp = lambda n, dbl: copy.deepcopy(n).double() if dbl else copy.deepcopy(n)  # noqa: E731
    return {dbl: make_algo(cp(nets[0], dbl), cp(nets[1], dbl), cp(nets[2], dbl), DIMS[-1], make_alpha(kind, dbl), **kw)
            for dbl in (True, False)}


def restatement_of(init, kind):
    return DsacRestatement(init[0], init[1], init[2], DIMS, UP_FIXED if kind == "fix" else dict(log_alpha=0.0, m=0.0, v=0.0, t=0),
                           TAU, lr=LR, target_entropy=UP_TARGET_ENTROPY, alpha_lr=LR)


class Kink(Exception):
    pass


def mine_of(r):
    return np.array([r["actor_loss"], r["critic1_loss"], r["critic2_loss"], r["alpha"], np.nan if r["alpha_loss"] is None else r["alpha_loss"]])


def follow(R, r, ref_stats, what):
    """The restatement's update `r` against the reference's float64 statistics; Kink if it came within DELTA of one."""
    if R.kink <= DELTA:
        raise Kink
    assert np.allclose(mine_of(r), ref_stats, rtol=1e-10, atol=0, equal_nan=True), (what, mine_of(r), ref_stats)


def update_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step, _, steps = d[4:10]

    def attempt(kind, seed):
        rs = np.random.RandomState(seed)
        nets = fresh_nets(seed)
        init = np.stack([flat(n).astype(np.float32) for n in nets])
        algos = algos_of(nets, kind, n_step_return_horizon=n_step)
        bufs, RB = up_buffers(gd, VectorReplayBuffer)
        R = restatement_of(init, kind)
        allidx = bufs[True].sample_indices(0)
        new = {f"up_{kind}_init": init}
        for k in range(steps):
            indices = rs.choice(allidx, B, replace=True).astype(np.int64)
            out = {}
            for dbl, algo in algos.items():
                buf = bufs[dbl]
                batch = algo._preprocess_batch(buf[indices], buf, indices)
                stats = algo._update_with_batch(batch)
                out[dbl] = dict(stats=stats_of(stats), w={n: ref_flat(algo, n) for n in NETS}, la=log_alpha_of(algo),
                                ret=batch.returns.double().numpy().reshape(-1),
                                g={n: ref_grad(m) for n, m in (("actor", algo.policy.actor), ("critic", algo.critic), ("critic2", algo.critic2))})
            idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
            r = R.update(bufs[False][indices].obs, bufs[False][indices].act, bufs[False][idx_n].obs_next, mc, gpow, vmask)
            r64, r32 = out[True], out[False]
            follow(R, r, r64["stats"], (kind, k))
            assert np.allclose(r["returns"], r64["ret"], rtol=1e-12, atol=1e-13)
            for n in NETS:
                assert np.allclose(R.weights(n), r64["w"][n], rtol=1e-10, atol=1e-13), (kind, k, n)
            for n in ("actor", "critic", "critic2"):
                assert np.allclose(r["grads"][n], r64["g"][n], rtol=1e-10, atol=1e-15), (kind, k, n)
            pk = f"up_{kind}_s{k}_"
            for n in NETS:
                digest(new, pk + n, r64["w"][n])
                new[pk + n + "_eref"] = emax(r64["w"][n], r32["w"][n])
            digest(new, pk + "returns", r64["ret"])
            new.update({pk + "indices": indices, pk + "stats": np.stack([r64["stats"], r32["stats"]]),
                        pk + "returns_eref": emax(r64["ret"], r32["ret"]), pk + "log_alpha": np.array([r64["la"], r32["la"]]),
                        pk + "mean_entropy": np.float64(r["mean_entropy"]),
                        **{pk + n + "_grad_eref": emax(r64["g"][n], r32["g"][n]) for n in ("actor", "critic", "critic2")}})
        res.update(new)
        print("update stats", kind, [res[f"up_{kind}_s{k}_stats"][0].round(6).tolist() for k in range(steps)])

    for kind in ("fix", "auto"):   # the first seed whose three updates keep DELTA away from every kink
        for seed in range(41, 141):
            try:
                attempt(kind, seed)
                res[f"up_{kind}_seed"] = np.int64(seed)
                break
            except Kink:
                continue
        else:
            raise AssertionError("no seed without a kink")


def set_flat(net, vec):
    with torch.no_grad():
        o = 0
        for q in net.parameters():
            q.copy_(torch.as_tensor(vec[o:o + q.numel()]).reshape(q.shape))
            o += q.numel()


def prio_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step = d[4:8]
    alpha, beta = 0.6, 0.4

    def attempt(seed):
        nets = fresh_nets(0)
        for n, v in zip(nets, res["up_fix_init"]):
            set_flat(n, v)
        algos = algos_of(nets, "fix", n_step_return_horizon=n_step)
        bufs, RB = up_buffers(gd, PrioritizedVectorReplayBuffer, alpha=alpha, beta=beta)
        R = restatement_of(res["up_fix_init"], "fix")
        bound = bufs[True].weight._bound
        np.random.seed(seed)
        new = {}
        for k in range(2):
            indices = bufs[True].sample_indices(B).astype(np.int64)
            out = {}
            for dbl, algo in algos.items():
                buf = bufs[dbl]
                batch = buf[indices]
                w_in = np.asarray(batch.weight, np.float64).copy()
                batch = algo._preprocess_batch(batch, buf, indices)
                stats = algo._update_with_batch(batch)
                algo._postprocess_batch(batch, buf, indices)
                out[dbl] = (stats_of(stats), w_in, buf.weight._value[bound:bound + n_env * S].copy(),
                            np.array([float(buf._max_prio), float(buf._min_prio)]))
            idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
            r = R.update(bufs[False][indices].obs, bufs[False][indices].act, bufs[False][idx_n].obs_next, mc, gpow, vmask,
                         weight=out[True][1])
            follow(R, r, out[True][0], ("pr", k))
            pk = f"pr_s{k}_"
            new.update({pk + "indices": indices, pk + "stats": np.stack([out[True][0], out[False][0]]), pk + "weight": out[True][1],
                        pk + "weight_eref": emax(out[True][1], out[False][1]), pk + "leaves": out[True][2],
                        pk + "leaves_eref": emax(out[True][2], out[False][2]), pk + "prio": out[True][3],
                        pk + "prio_eref": emax(out[True][3], out[False][3])})
        res.update(new)

    res.update(pr_alpha=np.float64(alpha), pr_beta=np.float64(beta))
    for seed in range(47, 147):   # the first numpy seed whose two draws keep DELTA away from every kink
        try:
            attempt(seed)
            res["pr_seed"] = np.int64(seed)
            break
        except Kink:
            continue
    else:
        raise AssertionError("no seed without a kink")
    print("prioritized stats", [res[f"pr_s{k}_stats"][0].round(6).tolist() for k in range(2)])


# ---- ma / sd / sig ------------------------------------------------------------------------------------------------------
def marl_section(res, gd):
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    dims = [D, 16, A]
    env = FakeEnv(N_AG)
    kinds = ["fix", "auto"]
    tgt_ent = 0.98 * float(np.log(A))
    RB = RestatedBuffer(n_env, S, N_AG)
    for t in range(T):
        for e in range(n_env):
            RB.add(e, gd["ma_rew"][t, e], bool(gd["ma_term"][t, e]), bool(gd["ma_trunc"][t, e]))

    def attempt(seed):
        torch.manual_seed(seed)
        nets = [(ActorNet(dims), CriticNet(dims), CriticNet(dims)) for _ in kinds]
        init = np.stack([np.stack([flat(n).astype(np.float32) for n in trio]) for trio in nets])
        out = {}
        for dbl in (True, False):
            dt = np.float64 if dbl else np.float32
            buf = VectorReplayBuffer(n_env * S, n_env)
            for t in range(T):   # dqn.npz's AEC rows, the masks left out
                ids = np.array([env.agents[a] for a in gd["ma_turn"][t]], dtype=object)
                nxt = np.array([env.agents[(a + 1) % N_AG] for a in gd["ma_turn"][t]], dtype=object)
                buf.add(Batch(obs=Batch(agent_id=ids, obs=gd["ma_obs"][t].astype(dt)), act=gd["ma_act"][t],
                              rew=gd["ma_rew"][t].astype(np.float64), terminated=gd["ma_term"][t], truncated=gd["ma_trunc"][t],
                              obs_next=Batch(agent_id=nxt, obs=gd["ma_obs_next"][t].astype(dt))), buffer_ids=np.arange(n_env))
            cp = lambda n: copy.deepcopy(n).double() if dbl else copy.deepcopy(n)  # noqa: E731
            algos = [make_algo(cp(trio[0]), cp(trio[1]), cp(trio[2]), A, make_alpha(k, dbl, target_entropy=tgt_ent),
                               n_step_return_horizon=n_step) for k, trio in zip(kinds, nets)]
            ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=env)
            batch, indices = buf.sample(0)
            stats = ma._update_with_batch(ma._preprocess_batch(batch, buf, indices))
            out[dbl] = np.stack([stats_of(stats._agent_id_to_stats[a]) for a in env.agents])
            if not dbl:
                continue
            for k, agent in enumerate(env.agents):   # the restatement on the agent's rows, its reward column in the walk
                rows = indices[np.nonzero(batch.obs.agent_id == agent)[0]]
                idx_n, mc, gpow, vmask = nstep_walk(RB, rows, n_step, GAMMA, k)
                R = DsacRestatement(init[k][0], init[k][1], init[k][2], dims, UP_FIXED if kinds[k] == "fix" else
                                    dict(log_alpha=0.0, m=0.0, v=0.0, t=0), TAU, lr=LR, target_entropy=tgt_ent, alpha_lr=LR)
                r = R.update(buf[rows].obs.obs, buf[rows].act, buf[idx_n].obs_next.obs, mc, gpow, vmask)
                follow(R, r, out[True][k], ("ma", agent))
        res.update(ma_dims=np.array(dims, np.int64), ma_init=init, ma_kinds=np.array(kinds), ma_stats=np.stack([out[True], out[False]]),
                   ma_target_entropy=np.float64(tgt_ent))
        print("marl stats", out[True].round(6).tolist())

    for seed in range(29, 129):   # the first torch seed whose nets keep DELTA away from every kink
        try:
            attempt(seed)
            res["ma_seed"] = np.int64(seed)
            break
        except Kink:
            continue
    else:
        raise AssertionError("no seed without a kink")


def statedict_and_signatures(res):
    torch.manual_seed(0)
    actor = DiscreteActor(preprocess_net=Net(state_shape=(6,), hidden_sizes=[32, 32]), action_shape=5, softmax_output=False)
    crit = lambda: DiscreteCritic(preprocess_net=Net(state_shape=(6,), hidden_sizes=[32, 32]), last_size=5)  # noqa: E731
    for kind in ("fix", "auto"):
        algo = make_algo(actor, crit(), crit(), 5, make_alpha(kind, False))
        sd = {k: v for k, v in algo.state_dict().items() if isinstance(v, torch.Tensor)}
        res[f"sd_{kind}_keys"] = np.array(list(sd.keys()))
        res[f"sd_{kind}_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    for cls in (DiscreteSACPolicy, DiscreteSAC, AutoAlpha, FixedAlpha):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])
        res[f"sigkind_{cls.__name__}"] = np.array([q.kind.name for q in ps])
    assert isinstance(Alpha.from_float_or_instance(0.2), FixedAlpha)


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    gd = dict(np.load(os.path.join(HERE, "dqn.npz")))
    res = {"delta": np.float64(DELTA), "gamma": np.float64(GAMMA), "tau": np.float64(TAU), "lr": np.float64(LR),
           "up_fixed": np.float64(UP_FIXED), "up_target_entropy": np.float64(UP_TARGET_ENTROPY)}
    head_sections(res)
    update_section(res, gd)
    prio_section(res, gd)
    marl_section(res, gd)
    statedict_and_signatures(res)
    path = os.path.join(HERE, "dsac.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
