"""Generate tests/golden/icm.npz by RUNNING THE REFERENCE's IntrinsicCuriosityModule.forward, _ICMMixin and
ICMOffPolicyWrapper around DQN (utils/net/discrete.py:378-429, algorithm/modelbased/icm.py, imported through
oracle/ref_shim.py) in float64 and float32, with e_ref = max |ref32 - ref64| per array.  The reference's `MLP` casts its input
to float32, which a float64 run cannot use: the three networks are `Seq` modules defined here, with the `MLP`'s layer
structure and key names (`model.{2 i}`), put in the reference module's places.

Sections (every array is data: inputs, indices, initial weights, expected outputs; large float64 arrays as digests):
  hd_*   head inputs per F in {1, 7, 16, 512} x A in {1, 2, 5, 64}, R = 37: phi2_hat / phi2 / act_hat as i8 = 8 x the value (a
         lattice of eighths, exact in float32), act, rew.  The reference's forward and _icm_preprocess_batch /
         _icm_update run around table "networks" whose gradients ARE d loss / d output: mse, shaped rewards, the three losses
         and the three gradients.
  md_*   the module 6-32-16, hidden (32,), A = 5 on R = 37 rows: outputs, losses and the gradient of the whole vector.
  off_*  three updates of the reference's DQN + ICMOffPolicyWrapper on dqn.npz's buffer script and indices (n_step 3), beside a
         bare DQN from the same weights: the wrapped DQN's weights and losses are asserted EQUAL to the bare run's, bit for bit,
         in float64 and in float32 (compute_nstep_return reads buffer.rew: the intrinsic reward never reaches the TD target).
  on_*   three consecutive updates of the reference's PPO (nets 6-32-32, whole batch, repeat 2) + ICMOnPolicyWrapper (F 16) on a
         buffer script of 3 x 8 rows with episode ends: PPO statistics, ICM statistics, weight digests of both.  The generator
         asserts that the reward GAE read is rew + mse * reward_scale with the mse of the ICM weights from BEFORE the update
         (preprocess, wrapped update, ICM step), and that the buffer's rewards are unchanged afterwards.
  sd_*   state_dict keys and shapes of the reference module around `MLP`s;  sig_*  constructor signatures.
The generator asserts that no ReLU pre-activation it uses lies within DELTA of zero and that the restatement
(tests/icm_restatement.py) follows the reference's float64 run to 1e-10.
"""
from __future__ import annotations

import copy
import inspect
import os

import numpy as np

from make_dqn_fixtures import DELTA, GAMMA, QNet, digest, flat, make_dqn  # noqa: E402  (installs the shim)
from make_distq_fixtures import emax, up_buffers  # noqa: E402

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402
from tianshou.algorithm.modelbased.icm import ICMOffPolicyWrapper, ICMOnPolicyWrapper, ICMTrainingStats, _ICMMixin  # noqa: E402
from tianshou.algorithm.algorithm_base import TrainingStats  # noqa: E402
from tianshou.algorithm.modelfree.ppo import PPO  # noqa: E402
from tianshou.algorithm.modelfree.reinforce import DiscreteActorPolicy  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import MLP  # noqa: E402
from tianshou.utils.net.discrete import IntrinsicCuriosityModule  # noqa: E402

from icm_restatement import IcmRestatement, head  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
R_HEAD = 37
FEATS, ACTS = (1, 7, 16, 512), (1, 2, 5, 64)
LR_SCALE, REWARD_SCALE, W_FWD, LR = 0.7, 0.125, 0.2, 1e-3
FEAT_DIMS, HIDDEN, N_ACT = [6, 32, 16], (32,), 5
STAT_KEYS = ("icm_loss", "icm_forward_loss", "icm_inverse_loss")


class Seq(nn.Module):
    """The reference `MLP`'s layers and key names, taking the dtype of its weights."""

    def __init__(self, dims) -> None:
        super().__init__()
        mods = []
        for i in range(len(dims) - 1):
            mods.append(nn.Linear(dims[i], dims[i + 1]))
            if i < len(dims) - 2:
                mods.append(nn.ReLU())
        self.model = nn.Sequential(*mods)

    def forward(self, x):
        return self.model(torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(self.model[0].weight.dtype))


class Rows(nn.Module):
    """A table "network": the rows of a table, whatever the input (its first column a row number where `index` is set)."""

    def __init__(self, table, index: bool = False) -> None:
        super().__init__()
        self.table, self.index = nn.Parameter(torch.as_tensor(table)), index

    def forward(self, x):
        return self.table[x[:, 0].long()] if self.index else self.table


class StepNothing:
    """An optimizer whose step only takes the gradient."""

    def step(self, loss):
        loss.backward()


def stats_of(stats):
    return np.array([float(getattr(stats, k)) for k in STAT_KEYS])


def make_icm(dbl):
    icm = IntrinsicCuriosityModule(feature_net=Seq(FEAT_DIMS), feature_dim=FEAT_DIMS[-1], action_dim=N_ACT, hidden_sizes=HIDDEN)
    icm.forward_model = Seq([FEAT_DIMS[-1] + N_ACT, *HIDDEN, FEAT_DIMS[-1]])
    icm.inverse_model = Seq([2 * FEAT_DIMS[-1], *HIDDEN, N_ACT])
    return icm.double() if dbl else icm


# ---- hd -----------------------------------------------------------------------------------------------------------------
def head_section(res):
    rs = np.random.RandomState(23)
    R = R_HEAD
    res.update(hd_lr_scale=np.float64(LR_SCALE), hd_reward_scale=np.float64(REWARD_SCALE), hd_w=np.float64(W_FWD))
    for Fd in FEATS:
        for A in ACTS:
            p = f"hd_F{Fd}_A{A}_"
            lat = lambda n: rs.randint(-24, 25, (R, n)).astype(np.int8)  # noqa: E731
            inp = dict(phi2_hat=lat(Fd), phi2=lat(Fd), act_hat=lat(A), act=rs.randint(0, A, R).astype(np.int64),
                       rew=(rs.randint(-16, 17, R) / 8.0).astype(np.float32))
            res.update({p + k: v for k, v in inp.items()})
            f = {k: inp[k].astype(np.float64) / 8.0 for k in ("phi2_hat", "phi2", "act_hat")}
            out = {}
            for dbl in (True, False):
                ndt = np.float64 if dbl else np.float32
                icm = IntrinsicCuriosityModule(feature_net=Rows(np.concatenate([np.zeros((R, Fd)), f["phi2"]]).astype(ndt), True),
                                               feature_dim=Fd, action_dim=A)
                icm.forward_model, icm.inverse_model = Rows(f["phi2_hat"].astype(ndt)), Rows(f["act_hat"].astype(ndt))
                mix = _ICMMixin(model=icm, optim=StepNothing(), lr_scale=LR_SCALE, reward_scale=REWARD_SCALE, forward_loss_weight=W_FWD)
                rows = np.arange(R, dtype=np.float32).reshape(R, 1)
                batch = Batch(obs=rows, obs_next=rows + R, act=inp["act"], rew=inp["rew"].astype(ndt).copy())
                mix._icm_preprocess_batch(batch)
                shaped = np.asarray(batch.rew, np.float64).copy()
                stats = mix._icm_update(batch, TrainingStats())
                mix._icm_postprocess_batch(batch)
                # `orig_rew` is the array that `batch.rew +=` then changes in place: the reference's restore puts the shaped
                # reward back.  The batch is a copy of the buffer's rows, so nothing outside it sees that.
                assert np.array_equal(np.asarray(batch.rew, np.float64), shaped)
                g = lambda m: m.table.grad.double().numpy()  # noqa: E731
                out[dbl] = dict(mse=batch.policy.mse_loss.detach().double().numpy(), shaped=shaped, stats=stats_of(stats),
                                d_phi2_hat=g(icm.forward_model), d_phi2_fwd=g(icm.feature_net)[R:], d_act_hat=g(icm.inverse_model))
                assert not g(icm.feature_net)[:R].any()
            r64, r32 = out[True], out[False]
            h = head(f["phi2_hat"], f["phi2"], f["act_hat"], inp["act"], W_FWD, LR_SCALE)
            for k in ("mse", "d_phi2_hat", "d_phi2_fwd", "d_act_hat"):
                assert np.allclose(h[k], r64[k], rtol=1e-10, atol=1e-16), (Fd, A, k)
            assert np.allclose([h["loss"], h["forward_loss"], h["inverse_loss"]], r64["stats"], rtol=1e-10, atol=1e-14)
            assert np.allclose(inp["rew"] + h["mse"] * REWARD_SCALE, r64["shaped"], rtol=1e-12, atol=0)
            res.update({p + "stats": np.stack([r64["stats"], r32["stats"]]), p + "mse": r64["mse"], p + "shaped": r64["shaped"],
                        p + "d_act_hat": r64["d_act_hat"]})
            digest(res, p + "d_phi2_hat", r64["d_phi2_hat"].reshape(-1))
            res.update({p + k + "_eref": emax(r64[k], r32[k]) for k in ("mse", "shaped", "d_phi2_hat", "d_phi2_fwd", "d_act_hat")})
    print("heads", res[f"hd_F16_A5_stats"][0])


# ---- md -----------------------------------------------------------------------------------------------------------------
def ref_module_run(icm, s1, act, s2):
    mix = _ICMMixin(model=icm, optim=StepNothing(), lr_scale=LR_SCALE, reward_scale=REWARD_SCALE, forward_loss_weight=W_FWD)
    batch = Batch(obs=s1, obs_next=s2, act=act, rew=np.zeros(len(act)))
    mix._icm_preprocess_batch(batch)
    stats = mix._icm_update(batch, TrainingStats())
    grads = np.concatenate([q.grad.detach().double().reshape(-1).numpy() for q in icm.parameters()])
    return dict(mse=batch.policy.mse_loss.detach().double().numpy(), act_hat=batch.policy.act_hat.detach().double().numpy(),
                stats=stats_of(stats), grads=grads)


def module_section(res):
    R = R_HEAD
    for seed in range(31, 131):   # the first seed whose rows keep DELTA away from every kink
        rs = np.random.RandomState(seed)
        torch.manual_seed(seed)
        base = make_icm(False)
        init = flat(base).astype(np.float32)
        s1, s2 = rs.standard_normal((R, FEAT_DIMS[0])).astype(np.float32), rs.standard_normal((R, FEAT_DIMS[0])).astype(np.float32)
        act = rs.randint(0, N_ACT, R).astype(np.int64)
        Rst = IcmRestatement(init, FEAT_DIMS, N_ACT, HIDDEN)
        mine = Rst.loss_grads(s1, act, s2, W_FWD, LR_SCALE)
        if Rst.kink <= DELTA:
            continue
        out = {dbl: ref_module_run(copy.deepcopy(base).double() if dbl else copy.deepcopy(base), s1, act, s2) for dbl in (True, False)}
        r64, r32 = out[True], out[False]
        for k in ("mse", "act_hat", "grads"):
            assert np.allclose(mine[k], r64[k], rtol=1e-10, atol=1e-15), k
        assert np.allclose([mine[k] for k in STAT_KEYS], r64["stats"], rtol=1e-10, atol=0)
        res.update(md_seed=np.int64(seed), md_init=init, md_s1=s1, md_s2=s2, md_act=act, md_mse=r64["mse"], md_act_hat=r64["act_hat"],
                   md_stats=np.stack([r64["stats"], r32["stats"]]), md_grads=r64["grads"],
                   **{f"md_{k}_eref": emax(r64[k], r32[k]) for k in ("mse", "act_hat", "grads")})
        print("module stats", r64["stats"])
        return
    raise AssertionError("no seed without a kink")


# ---- off ----------------------------------------------------------------------------------------------------------------
def offpolicy_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    dims, (B, n_env, S, n_step, freq, steps) = d[:4], d[4:10]
    qnet = QNet(dims)
    with torch.no_grad():
        o = 0
        for q in qnet.parameters():
            q.copy_(torch.as_tensor(gd["up_init"][o:o + q.numel()]).reshape(q.shape))
            o += q.numel()

    def attempt(seed):
        torch.manual_seed(seed)
        base = make_icm(False)
        init = flat(base).astype(np.float32)
        bufs, _ = up_buffers(gd, VectorReplayBuffer)
        Rst = IcmRestatement(init, FEAT_DIMS, N_ACT, HIDDEN, lr=LR)
        algos = {}
        for dbl in (True, False):
            kw = dict(n_step_return_horizon=n_step, target_update_freq=freq)
            icm = copy.deepcopy(base).double() if dbl else copy.deepcopy(base)
            wrapped = ICMOffPolicyWrapper(wrapped_algorithm=make_dqn(qnet, dims[-1], dbl, **kw), model=icm,
                                          optim=AdamOptimizerFactory(lr=LR), lr_scale=LR_SCALE, reward_scale=REWARD_SCALE,
                                          forward_loss_weight=W_FWD)
            algos[dbl] = (wrapped, make_dqn(qnet, dims[-1], dbl, **kw), icm)
        new = {"off_init": init}
        for k in range(steps):
            indices = gd[f"up_s{k}_indices"]
            out = {}
            for dbl, (wrapped, bare, icm) in algos.items():
                buf = bufs[dbl]
                rew_before = buf.rew.copy()
                batch = wrapped._preprocess_batch(buf[indices], buf, indices)
                shaped = np.asarray(batch.rew, np.float64).copy()
                stats = wrapped._update_with_batch(batch)
                wrapped._postprocess_batch(batch, buf, indices)
                b2 = bare._preprocess_batch(buf[indices], buf, indices)
                bare_loss = bare._update_with_batch(b2).loss
                w_dqn, w_bare = flat(wrapped.wrapped_algorithm.policy.model), flat(bare.policy.model)
                # the off-policy quirk, in the running reference: the TD target never sees the intrinsic reward
                assert np.array_equal(w_dqn, w_bare) and stats.loss == bare_loss, "the wrapped DQN left the bare DQN's path"
                assert np.array_equal(batch.returns.numpy(), b2.returns.numpy()) and np.array_equal(buf.rew, rew_before)
                assert np.array_equal(np.asarray(batch.rew, np.float64), shaped)   # the restore is a no-op (see hd), on a copy
                assert isinstance(stats, ICMTrainingStats)
                out[dbl] = dict(stats=stats_of(stats), w=flat(icm), loss=float(stats.loss), shaped=shaped)
            o_rows, a_rows, n_rows = bufs[False][indices].obs, bufs[False][indices].act, bufs[False][indices].obs_next
            mine = Rst.update(o_rows, a_rows, n_rows, W_FWD, LR_SCALE)
            if Rst.kink <= DELTA:
                return None
            r64, r32 = out[True], out[False]
            assert np.allclose([mine[s] for s in STAT_KEYS], r64["stats"], rtol=1e-10, atol=0), (k, r64["stats"])
            assert np.allclose(Rst.weights(), r64["w"], rtol=1e-10, atol=1e-13)
            assert np.allclose(np.asarray(bufs[False][indices].rew) + mine["mse"] * REWARD_SCALE, r64["shaped"], rtol=1e-10, atol=1e-13)
            pk = f"off_s{k}_"
            digest(new, pk + "icm", r64["w"])
            new.update({pk + "stats": np.stack([r64["stats"], r32["stats"]]), pk + "icm_eref": emax(r64["w"], r32["w"]),
                        pk + "dqn_loss": np.array([r64["loss"], r32["loss"]]), pk + "shaped": r64["shaped"],
                        pk + "shaped_eref": emax(r64["shaped"], r32["shaped"])})
            assert abs(r64["loss"] - float(gd[f"up_s{k}_loss"][0])) <= 1e-12 * abs(r64["loss"])   # dqn.npz's own bare run
        return new

    for seed in range(61, 161):
        new = attempt(seed)
        if new is not None:
            res.update(new, off_seed=np.int64(seed))
            print("off-policy icm stats", [res[f"off_s{k}_stats"][0].round(6).tolist() for k in range(steps)])
            return
    raise AssertionError("no seed without a kink")


# ---- on -----------------------------------------------------------------------------------------------------------------
ON_DIMS, ON_ENV, ON_T, ON_REPEAT = [6, 32, 32], 3, 8, 2
PPO_KEYS = ("loss", "actor_loss", "vf_loss", "ent_loss")


class ActorNet(QNet):
    pass


class CriticNet(QNet):
    def forward(self, obs, state=None, info=None):
        return super().forward(obs, state, info)[0]


def relu_gap(net, x) -> float:
    """The smallest |ReLU pre-activation| of a QNet over the rows x."""
    gap, x = np.inf, torch.as_tensor(np.asarray(x)).to(net.layers[0].weight.dtype)
    with torch.no_grad():
        for l in list(net.layers)[:-1]:
            x = l(x)
            gap = min(gap, float(x.abs().min()))
            x = F.relu(x)
    return gap


def onpolicy_section(res):
    """Three consecutive updates of the reference's PPO + ICMOnPolicyWrapper (whole batch, repeat 2: no permutation enters a
    mean) on a buffer of ON_ENV x ON_T rows with episode ends: PPO and ICM statistics, weight digests of both."""
    D, A = ON_DIMS[0], N_ACT

    def attempt(seed):
        rs = np.random.RandomState(seed)
        torch.manual_seed(seed)
        rows = dict(obs=rs.standard_normal((ON_T, ON_ENV, D)).astype(np.float32), obs_next=rs.standard_normal((ON_T, ON_ENV, D)).astype(np.float32),
                    act=rs.randint(0, A, (ON_T, ON_ENV)), rew=rs.standard_normal((ON_T, ON_ENV)).astype(np.float32),
                    term=rs.rand(ON_T, ON_ENV) < 0.1, trunc=rs.rand(ON_T, ON_ENV) < 0.05)
        rows["trunc"][-1] = True
        actor, critic, base = ActorNet(ON_DIMS + [A]), CriticNet(ON_DIMS + [1]), make_icm(False)
        init_ppo = np.concatenate([flat(actor), flat(critic)]).astype(np.float32)
        init_icm = flat(base).astype(np.float32)
        Rst = IcmRestatement(init_icm, FEAT_DIMS, N_ACT, HIDDEN, lr=LR)
        runs = {}
        for dbl in (True, False):
            dt = np.float64 if dbl else np.float32
            buf = VectorReplayBuffer(ON_ENV * ON_T, ON_ENV)
            for t in range(ON_T):
                buf.add(Batch(obs=rows["obs"][t].astype(dt), act=rows["act"][t], rew=rows["rew"][t].astype(np.float64),
                              terminated=rows["term"][t], truncated=rows["trunc"][t], obs_next=rows["obs_next"][t].astype(dt)),
                        buffer_ids=np.arange(ON_ENV))
            cp = lambda n: copy.deepcopy(n).double() if dbl else copy.deepcopy(n)  # noqa: E731
            a, c, icm = cp(actor), cp(critic), cp(base)
            ppo = PPO(policy=DiscreteActorPolicy(actor=a, action_space=gym.spaces.Discrete(A)), critic=c, optim=AdamOptimizerFactory(lr=LR))
            wrapped = ICMOnPolicyWrapper(wrapped_algorithm=ppo, model=icm, optim=AdamOptimizerFactory(lr=LR), lr_scale=LR_SCALE,
                                         reward_scale=REWARD_SCALE, forward_loss_weight=W_FWD)
            runs[dbl] = (buf, wrapped, a, c, icm)
        new = {"on_init_ppo": init_ppo, "on_init_icm": init_icm, **{f"on_rows_{k}": v for k, v in rows.items()},
               "on_dims": np.array(ON_DIMS + [A, ON_ENV, ON_T, ON_REPEAT, 3], np.int64)}
        for k in range(3):
            out = {}
            for dbl, (buf, wrapped, a, c, icm) in runs.items():
                if min(relu_gap(a, rows["obs"]), relu_gap(c, rows["obs"]), relu_gap(c, rows["obs_next"])) <= DELTA:
                    return None
                rew_before = buf.rew.copy()
                batch, indices = buf.sample(0)
                with policy_within_training_step(wrapped.policy), torch.enable_grad():
                    wrapped.train()
                    batch = wrapped._preprocess_batch(batch, buf, indices)
                    shaped = np.asarray(batch.rew, np.float64).copy()
                    stats = wrapped._update_with_batch(batch, None, ON_REPEAT)
                    wrapped._postprocess_batch(batch, buf, indices)
                assert np.array_equal(buf.rew, rew_before) and isinstance(stats, ICMTrainingStats) and stats.gradient_steps == ON_REPEAT
                out[dbl] = dict(icm_stats=stats_of(stats), ppo_stats=np.array([getattr(stats, s).mean for s in PPO_KEYS]),
                                w_ppo=np.concatenate([flat(a), flat(c)]), w_icm=flat(icm), shaped=shaped, indices=indices)
            r64, r32 = out[True], out[False]
            buf = runs[False][0]
            idx = r64["indices"]
            mine = Rst.update(buf[idx].obs, buf[idx].act, buf[idx].obs_next, W_FWD, LR_SCALE)
            if Rst.kink <= DELTA:
                return None
            assert np.allclose([mine[s] for s in STAT_KEYS], r64["icm_stats"], rtol=1e-10, atol=0), (k, r64["icm_stats"])
            assert np.allclose(Rst.weights(), r64["w_icm"], rtol=1e-10, atol=1e-13)
            # Q62: what GAE read IS rew + mse * reward_scale, with the mse of the ICM weights from before this update
            assert np.allclose(np.asarray(buf[idx].rew, np.float64) + mine["mse"] * REWARD_SCALE, r64["shaped"], rtol=1e-10, atol=1e-13)
            pk = f"on_s{k}_"
            digest(new, pk + "ppo", r64["w_ppo"])
            digest(new, pk + "icm", r64["w_icm"])
            new.update({pk + "icm_stats": np.stack([r64["icm_stats"], r32["icm_stats"]]), pk + "ppo_stats": np.stack([r64["ppo_stats"], r32["ppo_stats"]]),
                        pk + "ppo_eref": emax(r64["w_ppo"], r32["w_ppo"]), pk + "icm_eref": emax(r64["w_icm"], r32["w_icm"])})
        return new

    for seed in range(71, 171):
        new = attempt(seed)
        if new is not None:
            res.update(new, on_seed=np.int64(seed))
            print("on-policy ppo stats", [res[f"on_s{k}_ppo_stats"][0].round(6).tolist() for k in range(3)])
            print("on-policy icm stats", [res[f"on_s{k}_icm_stats"][0].round(6).tolist() for k in range(3)])
            return
    raise AssertionError("no seed without a kink")


# ---- sd / sig -----------------------------------------------------------------------------------------------------------
def statedict_and_signatures(res):
    torch.manual_seed(0)
    icm = IntrinsicCuriosityModule(feature_net=MLP(input_dim=FEAT_DIMS[0], output_dim=FEAT_DIMS[-1], hidden_sizes=FEAT_DIMS[1:-1]),
                                   feature_dim=FEAT_DIMS[-1], action_dim=N_ACT, hidden_sizes=HIDDEN)
    sd = icm.state_dict()
    res["sd_keys"] = np.array(list(sd.keys()))
    res["sd_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    for cls in (IntrinsicCuriosityModule, ICMOnPolicyWrapper, ICMOffPolicyWrapper, ICMTrainingStats):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])
        res[f"sigkind_{cls.__name__}"] = np.array([q.kind.name for q in ps])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    gd = dict(np.load(os.path.join(HERE, "dqn.npz")))
    res = {"delta": np.float64(DELTA), "gamma": np.float64(GAMMA), "lr": np.float64(LR), "lr_scale": np.float64(LR_SCALE),
           "reward_scale": np.float64(REWARD_SCALE), "w": np.float64(W_FWD), "feat_dims": np.array(FEAT_DIMS, np.int64),
           "hidden": np.array(HIDDEN, np.int64), "n_act": np.int64(N_ACT)}
    head_section(res)
    module_section(res)
    offpolicy_section(res, gd)
    onpolicy_section(res)
    statedict_and_signatures(res)
    path = os.path.join(HERE, "icm.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
