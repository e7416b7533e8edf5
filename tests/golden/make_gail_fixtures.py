"""Generate tests/golden/gail.npz by RUNNING THE REFERENCE's GAIL (algorithm/imitation/gail.py, imported through
oracle/ref_shim.py) on top of its PPO, in float64 and float32, with e_ref = max |ref32 - ref64| per array.  The reference's `MLP`
casts its input to float32, which a float64 run cannot use: the discriminator is a `Seq` module (make_icm_fixtures.py) with the
`MLP`'s layer structure and key names, the actor and the critic are `QNet`s.

The ONE line of departure: `OneHotGAIL.disc` one-hots `batch.act` before the concatenation (the reference concatenates the
action as it is, which serves Box actions only).  np.random is seeded before every update, and the permutation of
`batch.split(bsz, merge_last=True)` and the indices of `expert_buffer.sample(bsz)` are recorded as they are drawn.

Sections (every array is data: inputs, indices, initial weights, expected outputs; large float64 arrays as digests):
  hd_*   head inputs on a lattice of eighths in [-12, 12] plus +-40 and +-90, as i16 = 8 x the logit, per (Rp, Re) in HEAD_CASES:
         the loss, both accuracies and d_logits of a table "discriminator" whose gradient IS d loss / d logits.
  rw_*   the rewards -logsigmoid(-l) of the same logits, over a reward array, with and without ids.
  up_*   three consecutive updates of the reference's PPO (nets 6-32-32, whole batch, repeat 2) + GAIL (disc_update_num 4,
         discriminator [6 + 5, 32, 1]) on a rollout script of 3 x 8 rows with episode ends (R = 24) against an expert script of
         2 envs;  um_*: two such updates on 3 x 9 rows (R = 27: bsz 6, the merged last chunk has 9 rows).  Stored: PPO statistics,
         GAIL statistics per step, weight digests of both nets, the rewards GAE read, the permutation and the expert indices.
  sig_*  the constructor's signature;  sd_*  state_dict keys and shapes of a reference `MLP` discriminator.
The generator asserts that the restatement (tests/gail_restatement.py) follows the reference's float64 run to 1e-10, that no
discriminator logit and no ReLU pre-activation lies within DELTA of zero, and that the buffer's rewards are unchanged after an
update.
"""
from __future__ import annotations

import copy
import inspect
import os

import numpy as np

from make_dqn_fixtures import DELTA, GAMMA, digest, flat  # noqa: E402  (installs the shim)
from make_distq_fixtures import emax  # noqa: E402
from make_icm_fixtures import ActorNet, CriticNet, PPO_KEYS, Rows, Seq, StepNothing, relu_gap  # noqa: E402

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)
import tianshou.algorithm.imitation.gail as gail_mod  # noqa: E402
from tianshou.algorithm.imitation.gail import GAIL, GailTrainingStats  # noqa: E402
from tianshou.algorithm.modelfree.a2c import A2CTrainingStats  # noqa: E402
from tianshou.algorithm.modelfree.ppo import PPO as RefPPO  # noqa: E402
from tianshou.algorithm.modelfree.reinforce import DiscreteActorPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, SequenceSummaryStats, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import MLP, ModuleWithVectorOutput  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from gail_restatement import GailRestatement, chunks, head, softplus  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD_CASES = ((1, 1), (37, 37), (3, 2), (16, 17), (100, 33))
LR, N_ACT, DISC_NUM = 1e-3, 5, 4
ON_DIMS, ON_ENV, ON_REPEAT, EXP_ENV, EXP_T = [6, 32, 32], 3, 2, 2, 8
DISC_DIMS = [ON_DIMS[0] + N_ACT, 32, 1]
GAIL_KEYS = ("disc_loss", "acc_pi", "acc_exp")


class OneHotGAIL(GAIL):
    n_act = N_ACT

    def disc(self, batch):
        dt = next(self.disc_net.parameters()).dtype
        obs = torch.as_tensor(np.asarray(batch.obs)).to(dt)
        act = F.one_hot(torch.as_tensor(np.asarray(batch.act)).long().reshape(-1), self.n_act).to(dt)   # the departure
        return self.disc_net(torch.cat([obs, act], dim=1))


class RecordingStats:
    """Stands where gail.py names SequenceSummaryStats: keeps the per-step sequences it is handed."""

    seqs: list = []

    @classmethod
    def from_sequence(cls, seq):
        cls.seqs.append(np.asarray(seq, np.float64).copy())
        return SequenceSummaryStats.from_sequence(seq)


gail_mod.SequenceSummaryStats = RecordingStats


class Recorder:
    """Records np.random.permutation and a buffer's sample_indices while active."""

    def __init__(self, buf) -> None:
        self.buf, self.perms, self.samples = buf, [], []

    def __enter__(self):
        self._perm, self._si = np.random.permutation, self.buf.sample_indices

        def perm(n):
            out = self._perm(n)
            self.perms.append(np.asarray(out).copy())
            return out

        def si(n):
            out = self._si(n)
            self.samples.append(np.asarray(out).copy())
            return out

        np.random.permutation, self.buf.sample_indices = perm, si
        return self

    def __exit__(self, *exc):
        np.random.permutation = self._perm
        del self.buf.sample_indices


def make_gail(actor, critic, disc, expert, dbl, cls=OneHotGAIL, disc_optim=None, n_act=N_ACT):
    cp = lambda n: copy.deepcopy(n).double() if dbl else copy.deepcopy(n)  # noqa: E731
    a, c, d = cp(actor), cp(critic), cp(disc)
    pol = DiscreteActorPolicy(actor=ModuleWithVectorOutput.from_module(a, n_act), action_space=gym.spaces.Discrete(n_act))
    algo = cls(policy=pol, critic=c, optim=AdamOptimizerFactory(lr=LR), expert_buffer=expert, disc_net=d,
               disc_optim=AdamOptimizerFactory(lr=LR), disc_update_num=DISC_NUM)
    if disc_optim is not None:
        algo.disc_optim = disc_optim
    return algo, a, c, d


# ---- hd / rw ------------------------------------------------------------------------------------------------------------
def head_logits(rs, n):
    lat = rs.randint(-96, 97, n).astype(np.int16)
    lat[lat == 0] = 1
    for i, v in enumerate((320, -320, 720, -720)):   # +-40, +-90
        if n > 4:
            lat[(7 * i + 3) % n] = v
    return lat


def head_section(res):
    rs = np.random.RandomState(29)
    for Rp, Re in HEAD_CASES:
        p = f"hd_{Rp}_{Re}_"
        lat = head_logits(rs, Rp + Re)
        if (Rp, Re) == (1, 1):
            lat[:] = (320, -720)
        res[p + "logits"] = lat
        lg = lat.astype(np.float64) / 8.0
        out = {}
        for dbl in (True, False):
            ndt = np.float64 if dbl else np.float32
            table = Rows(lg.astype(ndt).reshape(-1, 1), index=True)

            class TableGAIL(GAIL):
                def disc(self, batch, table=table):
                    return table(torch.as_tensor(np.asarray(batch.obs)))

            expert = VectorReplayBuffer(Re, 1)
            for i in range(Re):
                expert.add(Batch(obs=np.array([[Rp + i]], ndt), act=np.array([0]), rew=np.array([0.0]), terminated=np.array([False]),
                                 truncated=np.array([False]), obs_next=np.array([[0]], ndt)), buffer_ids=[0])
            expert.sample = lambda n, expert=expert, Re=Re: (expert[np.arange(Re)], np.arange(Re))
            algo, *_ = make_gail(ActorNet([1, 4, N_ACT]), CriticNet([1, 4, 1]), table, expert, dbl, cls=TableGAIL)
            algo.disc_net, algo.disc_optim, algo.disc_update_num = table, StepNothing(), 1
            RecordingStats.seqs.clear()
            batch = Batch(obs=np.arange(Rp, dtype=ndt).reshape(Rp, 1), act=np.zeros(Rp, int))
            # the reference's own _update_with_batch (gail.py:214-248) on one chunk, its PPO part stubbed out: this section has
            # no rollout
            zero = SequenceSummaryStats.from_single_value(0.0)
            ppo_update = RefPPO._update_with_batch
            RefPPO._update_with_batch = lambda self, b, bs, rep: A2CTrainingStats(loss=zero, actor_loss=zero, vf_loss=zero,
                                                                                 ent_loss=zero, gradient_steps=0)
            try:
                got = algo._update_with_batch(batch, None, 1)
            finally:
                RefPPO._update_with_batch = ppo_update
            assert isinstance(got, GailTrainingStats) and all(len(q) == 1 for q in RecordingStats.seqs)
            stats = [q[0] for q in RecordingStats.seqs]
            out[dbl] = dict(stats=np.array(stats, np.float64), d_logits=table.table.grad.double().numpy().reshape(-1))
        r64, r32 = out[True], out[False]
        h = head(lg, Rp)
        # the reference forms both accuracies with `.float().mean()`: float32 in its float64 run too
        assert np.isclose(h["loss"], r64["stats"][0], rtol=1e-10, atol=0), (Rp, Re)
        assert np.allclose([h["acc_pi"], h["acc_exp"]], r64["stats"][1:], rtol=1e-6, atol=0), (Rp, Re)
        assert np.allclose(h["d_logits"], r64["d_logits"], rtol=1e-10, atol=1e-300), (Rp, Re)
        res.update({p + "stats": np.stack([r64["stats"], r32["stats"]]), p + "d_logits": r64["d_logits"],
                    p + "d_logits_eref": emax(r64["d_logits"], r32["d_logits"])})
        # rw: the reward of the same logits, written over a reward array
        ids = rs.permutation(2 * (Rp + Re) + 3)[:Rp + Re].astype(np.int64)
        rew0 = (rs.randint(-16, 17, 2 * (Rp + Re) + 3) / 8.0).astype(np.float32)
        r = {dbl: (-F.logsigmoid(-torch.as_tensor(lg.astype(np.float64 if dbl else np.float32)))).double().numpy() for dbl in (True, False)}
        assert np.allclose(softplus(lg), r[True], rtol=1e-10, atol=1e-300)
        p = f"rw_{Rp}_{Re}_"
        res.update({p + "ids": ids, p + "rew0": rew0, p + "rew": r[True], p + "rew_eref": emax(r[True], r[False])})
    print("heads", res["hd_37_37_stats"][0])


# ---- up -----------------------------------------------------------------------------------------------------------------
def script(rs, T, n_env, D, A):
    rows = dict(obs=rs.standard_normal((T, n_env, D)).astype(np.float32), obs_next=rs.standard_normal((T, n_env, D)).astype(np.float32),
                act=rs.randint(0, A, (T, n_env)), rew=rs.standard_normal((T, n_env)).astype(np.float32),
                term=rs.rand(T, n_env) < 0.1, trunc=rs.rand(T, n_env) < 0.05)
    rows["trunc"][-1] = True
    return rows


def fill(rows, dt):
    T, n_env = rows["act"].shape
    buf = VectorReplayBuffer(n_env * T, n_env)
    for t in range(T):
        buf.add(Batch(obs=rows["obs"][t].astype(dt), act=rows["act"][t], rew=rows["rew"][t].astype(np.float64), terminated=rows["term"][t],
                      truncated=rows["trunc"][t], obs_next=rows["obs_next"][t].astype(dt)), buffer_ids=np.arange(n_env))
    return buf


def update_section(res, prefix, T, n_updates, seed0):
    D, A = ON_DIMS[0], N_ACT

    def attempt(seed):
        rs = np.random.RandomState(seed)
        torch.manual_seed(seed)
        rows, erows = script(rs, T, ON_ENV, D, A), script(rs, EXP_T, EXP_ENV, D, A)
        actor, critic, disc = ActorNet(ON_DIMS + [A]), CriticNet(ON_DIMS + [1]), Seq(DISC_DIMS)
        init_ppo = np.concatenate([flat(actor), flat(critic)]).astype(np.float32)
        init_disc = flat(disc).astype(np.float32)
        Rst = GailRestatement(init_disc, DISC_DIMS, A, lr=LR)
        runs = {}
        for dbl in (True, False):
            dt = np.float64 if dbl else np.float32
            buf, expert = fill(rows, dt), fill(erows, dt)
            runs[dbl] = (buf, expert, *make_gail(actor, critic, disc, expert, dbl))
        new = {prefix + "init_ppo": init_ppo, prefix + "init_disc": init_disc, **{f"{prefix}rows_{k}": v for k, v in rows.items()},
               **{f"{prefix}exp_{k}": v for k, v in erows.items()},
               prefix + "dims": np.array(ON_DIMS + [A, ON_ENV, T, ON_REPEAT, n_updates, EXP_ENV, EXP_T, DISC_NUM], np.int64)}
        for k in range(n_updates):
            out = {}
            for dbl, (buf, expert, algo, a, c, d) in runs.items():
                if min(relu_gap(a, rows["obs"]), relu_gap(c, rows["obs"]), relu_gap(c, rows["obs_next"])) <= DELTA:
                    return None
                rew_before = buf.rew.copy()
                np.random.seed(1000 * seed + k)
                batch, indices = buf.sample(0)
                RecordingStats.seqs.clear()
                with policy_within_training_step(algo.policy), torch.enable_grad(), Recorder(expert) as rec:
                    algo.train()
                    batch = algo._preprocess_batch(batch, buf, indices)
                    rew = np.asarray(batch.rew, np.float64).copy()
                    stats = algo._update_with_batch(batch, None, ON_REPEAT)
                assert np.array_equal(buf.rew, rew_before) and isinstance(stats, GailTrainingStats) and stats.gradient_steps == ON_REPEAT
                steps = len(rec.samples)
                assert steps == len(batch) // (len(batch) // DISC_NUM) and len(RecordingStats.seqs) == 3
                out[dbl] = dict(gail=np.stack(RecordingStats.seqs, 1), ppo=np.array([getattr(stats, s).mean for s in PPO_KEYS]),
                                summary=np.array([[getattr(getattr(stats, s), f) for f in ("mean", "std", "max", "min")] for s in GAIL_KEYS]),
                                w_ppo=np.concatenate([flat(a), flat(c)]), w_disc=flat(d), rew=rew, indices=indices,
                                perm=rec.perms[0], exp_idx=np.stack(rec.samples))
            r64, r32 = out[True], out[False]
            assert np.array_equal(r64["perm"], r32["perm"]) and np.array_equal(r64["exp_idx"], r32["exp_idx"])
            buf, expert = runs[False][0], runs[False][1]
            idx, perm, eidx = r64["indices"], r64["perm"], r64["exp_idx"]
            assert sorted(perm) == list(range(len(idx))) and eidx.shape == (len(idx) // (len(idx) // DISC_NUM), len(idx) // DISC_NUM)
            mine = Rst.update(buf[idx].obs, buf[idx].act, perm, np.stack([expert[e].obs for e in eidx]), np.stack([expert[e].act for e in eidx]),
                              DISC_NUM)
            if Rst.kink <= DELTA:
                return None
            # Q64: the reward GAE read is -logsigmoid(-D) of the discriminator from BEFORE this update's steps
            assert np.allclose(mine["rew"], r64["rew"], rtol=1e-10, atol=1e-14), k
            assert np.allclose(mine["loss"], r64["gail"][:, 0], rtol=1e-10, atol=0), k
            assert np.allclose(np.stack([mine["acc_pi"], mine["acc_exp"]], 1), r64["gail"][:, 1:], rtol=1e-6, atol=0), k   # float32 means
            assert np.allclose(Rst.weights(), r64["w_disc"], rtol=1e-10, atol=1e-13)
            assert [len(range(lo, hi)) for lo, hi in chunks(len(idx), DISC_NUM)][-1] == len(idx) - (eidx.shape[0] - 1) * eidx.shape[1]
            pk = f"{prefix}s{k}_"
            digest(new, pk + "ppo", r64["w_ppo"])
            digest(new, pk + "disc", r64["w_disc"])
            new.update({pk + "gail": np.stack([r64["gail"], r32["gail"]]), pk + "summary": np.stack([r64["summary"], r32["summary"]]),
                        pk + "ppo_stats": np.stack([r64["ppo"], r32["ppo"]]), pk + "ppo_eref": emax(r64["w_ppo"], r32["w_ppo"]),
                        pk + "disc_eref": emax(r64["w_disc"], r32["w_disc"]), pk + "rew": r64["rew"], pk + "rew_eref": emax(r64["rew"], r32["rew"]),
                        pk + "indices": idx.astype(np.int64), pk + "perm": perm.astype(np.int64), pk + "exp_idx": eidx.astype(np.int64)})
        return new

    for seed in range(seed0, seed0 + 100):
        new = attempt(seed)
        if new is not None:
            res.update(new)
            res[prefix + "seed"] = np.int64(seed)
            print(prefix, "ppo stats", [res[f"{prefix}s{k}_ppo_stats"][0].round(6).tolist() for k in range(n_updates)])
            print(prefix, "gail stats", [res[f"{prefix}s{k}_summary"][0][:, 0].round(6).tolist() for k in range(n_updates)])
            return
    raise AssertionError("no seed without a kink")


# ---- sd / sig -----------------------------------------------------------------------------------------------------------
def statedict_and_signatures(res):
    torch.manual_seed(0)
    sd = MLP(input_dim=DISC_DIMS[0], output_dim=1, hidden_sizes=DISC_DIMS[1:-1]).state_dict()
    res["sd_keys"] = np.array(list(sd.keys()))
    res["sd_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    for cls in (GAIL, GailTrainingStats):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])
        res[f"sigkind_{cls.__name__}"] = np.array([q.kind.name for q in ps])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    res = {"delta": np.float64(DELTA), "gamma": np.float64(GAMMA), "lr": np.float64(LR), "n_act": np.int64(N_ACT),
           "disc_dims": np.array(DISC_DIMS, np.int64), "head_cases": np.array(HEAD_CASES, np.int64)}
    head_section(res)
    update_section(res, "up_", 8, 3, 81)
    update_section(res, "um_", 9, 2, 91)
    statedict_and_signatures(res)
    path = os.path.join(HERE, "gail.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
