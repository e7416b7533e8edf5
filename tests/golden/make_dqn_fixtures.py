"""Generate tests/golden/dqn.npz by RUNNING THE REFERENCE's DQN, DiscreteQLearningPolicy, compute_nstep_return and
MultiAgentOffPolicyAlgorithm (dqn.py, algorithm_base.py:720-815, marl.py:208-311, imported through oracle/ref_shim.py), in
float32 and -- where a network is involved -- in float64 (`.double()` modules, a fresh Adam, float64 observations).

Sections (every array is data: inputs, add scripts, indices, initial weights, expected outputs):
  ns_*     the n-step walk: VectorReplayBuffer(24, 3) with two reward columns under a script of adds (sub-buffer 0 wraps
           around, episode ends inside n-step windows, a terminated and a truncated end, an unfinished tail and a finished
           one); n_step in {1, 3, 5}, both columns swapped in for `buffer.rew` as MARLDispatcher does (marl.py:231,240);
           indices = sample_indices(0) plus a shuffled subset with repeats.  idx_n, mc, gamma^m, value mask, and `returns`
           of compute_nstep_return with a table as target_q_fn.
  hd_*     the TD head, B = 37, A in {2, 5, 9}: DQN._target_q and DQN._update_with_batch around a Q-"network" that is a
           table of logits (its gradient IS d loss / d q), all of is_double x target net x {mse, mse + weight, huber} x
           {mask, no mask}; row 3 of q_next_online carries an exact tie.
  up_*     three consecutive DQN updates (net 6-32-32-5, B = 37, n_step 3, target_update_freq 2, lr 1e-3) on a buffer of
           3 x 16 slots: losses, returns, and digests (sum, sum of squares, 128 fixed entries) of the float64 weights and target weights
           after every step, e_ref = |ref32 - ref64| per array.
  ma_*     MultiAgentOffPolicyAlgorithm over a hand-filled AEC buffer (2 agents, 3 sub-buffers of 8, masks, n_step 2):
           per-agent losses.  Every row's obs_next carries the mask of its obs: the device AEC buffer keeps
           one mask per row.
  ex_*     add_exploration_noise under a numpy seed, with and without a mask.
  sd_*     the state_dict keys and shapes of a reference DQN around `Net(hidden_sizes=[32, 32])` with a target network.
The Q-network module `QNet` is defined here: the reference's `Net` casts observations to float32 (common.py), which a
float64 run cannot use.  The generator asserts that no ReLU pre-activation or greedy top-2 gap of the rows it uses lies within
DELTA of its kink, and that the restatement (tests/dqn_restatement.py) follows the reference's float64 run.
"""
from __future__ import annotations

import copy
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import ref_shim  # noqa: E402

ref_shim.install()

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402
from tianshou.algorithm.algorithm_base import Algorithm, _nstep_return  # noqa: E402
from tianshou.algorithm.modelfree.dqn import DQN, DiscreteQLearningPolicy  # noqa: E402
from tianshou.algorithm.multiagent.marl import MultiAgentOffPolicyAlgorithm  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import Net  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from dqn_restatement import DqnRestatement, RestatedBuffer, nstep_walk, td_head  # noqa: E402

DELTA = 1e-5
GAMMA = 0.99


class QNet(nn.Module):
    def __init__(self, dims) -> None:
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])

    def forward(self, obs, state=None, info=None):
        x = torch.as_tensor(np.asarray(obs), dtype=self.layers[0].weight.dtype)
        for i, l in enumerate(self.layers):
            x = l(x)
            if i < len(self.layers) - 1:
                x = F.relu(x)
        return x, state


class TableNet(nn.Module):
    """obs[:, 0] is a row number into a table of logits."""

    def __init__(self, table) -> None:
        super().__init__()
        self.table = nn.Parameter(torch.as_tensor(table))

    def forward(self, obs, state=None, info=None):
        return self.table[torch.as_tensor(np.asarray(obs)[:, 0]).long()], state


class FakeEnv:
    def __init__(self, n):
        self.agents = [f"agent_{i}" for i in range(n)]
        self.agent_idx = {a: i for i, a in enumerate(self.agents)}


N_DIGEST = 128


def digest(res: dict, key: str, x: np.ndarray) -> None:
    """What pins a float64 parameter array: its sum, its sum of squares and N_DIGEST fixed entries."""
    idx = np.sort(np.random.RandomState(12345).choice(x.size, min(N_DIGEST, x.size), replace=False))
    res.update({f"{key}_dsum": np.float64(x.sum()), f"{key}_dsq": np.float64((x * x).sum()), f"{key}_didx": idx.astype(np.int32),
                f"{key}_dval": x[idx]})


def flat(net) -> np.ndarray:
    return np.concatenate([p.detach().double().reshape(-1).numpy() for p in net.parameters()])


def f32(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


# ---- ns ------------------------------------------------------------------------------------------------------------
def nstep_section(res):
    rs = np.random.RandomState(3)
    B, S, D = 3, 8, 2
    plan = {0: [(i, i == 2 or i == 9, i == 6) for i in range(11)],   # wraps; terminated, truncated, terminated; tail open
            1: [(i, i == 7, i == 3) for i in range(8)],               # truncated, then its last row terminates
            2: [(i, False, False) for i in range(5)]}                 # one open episode
    script = [(e, t, tr) for step in itertools.zip_longest(*[[(e, *x[1:]) for x in plan[e]] for e in range(B)]) for (e, t, tr)
              in [s for s in step if s is not None]]
    env = np.array([s[0] for s in script], np.int64)
    term = np.array([s[1] for s in script], bool)
    trunc = np.array([s[2] for s in script], bool)
    rew = f32(rs, len(script), D)
    buf, R = VectorReplayBuffer(B * S, B), RestatedBuffer(B, S, D)
    for k in range(len(script)):
        o = Batch(obs=np.zeros((1, 1), np.float32), act=np.zeros(1, int), rew=rew[k:k + 1].astype(np.float64),
                  terminated=term[k:k + 1], truncated=trunc[k:k + 1], obs_next=np.zeros((1, 1), np.float32))
        buf.add(o, buffer_ids=[int(env[k])])
        R.add(int(env[k]), rew[k], bool(term[k]), bool(trunc[k]))
    allidx = buf.sample_indices(0)
    assert np.array_equal(allidx, R.sample_indices_all()) and np.array_equal(buf.unfinished_index(), R.unfinished_index())
    indices = np.concatenate([allidx, rs.choice(allidx, 13, replace=True)]).astype(np.int64)
    tq = f32(rs, B * S)
    res.update(ns_dims=np.array([B, S, D], np.int64), ns_env=env, ns_term=term, ns_trunc=trunc, ns_rew=rew,
               ns_indices=indices, ns_tq=tq, ns_all=allidx, ns_unfinished=buf.unfinished_index(), gamma=np.float64(GAMMA))
    save_rew = buf.rew
    for n, col in itertools.product((1, 3, 5), (0, 1)):
        buf._meta.rew = save_rew[:, col]
        seen = {}

        def target_q_fn(b, idx):
            seen["idx"] = idx.copy()
            return torch.as_tensor(tq[idx])

        batch = Algorithm.compute_nstep_return(buf[indices], buf, indices, target_q_fn, GAMMA, n)
        stack = [indices]
        for _ in range(n - 1):
            stack.append(buf.next(stack[-1]))
        stack = np.stack(stack)
        end = buf.done.copy()
        end[buf.unfinished_index()] = True
        I = len(indices)
        mc = _nstep_return(buf.rew, end, np.zeros((I, 1)), stack, GAMMA, n).reshape(I)
        gp = _nstep_return(buf.rew, end, np.ones((I, 1)), stack, GAMMA, n).reshape(I) - mc
        vm = Algorithm.value_mask(buf, seen["idx"])
        p = f"ns_n{n}_c{col}_"
        res.update({p + "idxn": seen["idx"].astype(np.int64), p + "mc": mc, p + "gpow": gp, p + "vmask": vm,
                    p + "returns": batch.returns.numpy().reshape(I)})
        r_idx, r_mc, r_gp, r_vm = nstep_walk(R, indices, n, GAMMA, col)
        assert np.array_equal(r_idx, seen["idx"]) and np.array_equal(r_vm, vm)
        assert np.allclose(r_mc, mc, rtol=1e-14, atol=1e-15) and np.allclose(r_gp, gp, rtol=1e-12, atol=0), (n, col)
    buf._meta.rew = save_rew


# ---- hd ------------------------------------------------------------------------------------------------------------
class _Rows:
    """buffer[indices].obs_next of DQN._target_q."""

    def __init__(self, obs_next):
        self.obs_next = obs_next

    def __getitem__(self, idx):
        return Batch(obs_next=self.obs_next[idx])


HEAD_CASES = [(dbl, tgt, loss, msk) for dbl in (0, 1) for tgt in (0, 1) for loss in ("mse", "msew", "huber") for msk in (0, 1)]


def head_section(res):
    rs = np.random.RandomState(5)
    B = 37
    res["hd_cases"] = np.array([f"d{d}t{t}_{l}_m{m}" for d, t, l, m in HEAD_CASES])
    res["hd_huber_delta"] = np.float64(0.7)
    for A in (2, 5, 9):
        q, on, tg = f32(rs, B, A), f32(rs, B, A), f32(rs, B, A)
        on[3, 1] = on[3].max() + 0.5
        on[3, min(A - 1, 3)] = on[3, 1]          # an exact tie at the row maximum: the first one wins
        if A == 2:
            on[3, 0] = on[3, 1]
        act = rs.randint(0, A, B).astype(np.int64)
        mc, gpow = f32(rs, B).astype(np.float64), (GAMMA ** rs.randint(1, 6, B)).astype(np.float32).astype(np.float64)
        vmask = rs.rand(B) > 0.2
        weight = (0.5 + rs.rand(B)).astype(np.float32)
        mask = np.zeros((B, A), bool)
        for b in range(B):
            mask[b, rs.choice(A, rs.randint(1, A), replace=False) if A > 1 else 0] = True
        p = f"hd_A{A}_"
        res.update({p + "q": q, p + "on": on, p + "tg": tg, p + "act": act, p + "mc": mc, p + "gpow": gpow, p + "vmask": vmask,
                    p + "weight": weight, p + "mask": mask})
        rows = np.arange(B, dtype=np.float32).reshape(B, 1)
        stacked = {k: [] for k in ("loss", "dqsel")}
        td_of = {}    # td_error does not depend on the loss: one row per (is_double, target net, mask), index 4 d + 2 t + m
        for dbl, tgt, loss, msk in HEAD_CASES:
            out = {}
            for dt in (torch.float64, torch.float32):
                model = TableNet(np.concatenate([q, on]).astype(np.float64 if dt == torch.float64 else np.float32))
                pol = DiscreteQLearningPolicy(model=model, action_space=gym.spaces.Discrete(A))
                algo = DQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), gamma=GAMMA, target_update_freq=5 if tgt else 0,
                           is_double=bool(dbl), huber_loss_delta=0.7 if loss == "huber" else None)
                if tgt:
                    with torch.no_grad():
                        algo.model_old.module.table[B:] = torch.as_tensor(tg).to(dt)
                nxt = rows + B
                obs_next = Batch(obs=nxt, mask=mask) if msk else nxt
                target = algo._target_q(_Rows(obs_next), np.arange(B))
                tq = target.detach().numpy().reshape(B, 1).copy()
                tq *= vmask.reshape(-1, 1)                                        # algorithm_base.py:796
                ret = (tq * gpow.reshape(B, 1) + mc.reshape(B, 1)).reshape(B)     # :1213-1215
                batch = Batch(obs=rows, act=act, returns=torch.as_tensor(ret).to(dt), info=Batch())
                if loss == "msew":
                    batch.weight = torch.as_tensor(weight).to(dt)
                stats = algo._update_with_batch(batch)
                out[dt] = dict(loss=stats.loss, td=batch.weight.detach().double().numpy(), ret=ret.astype(np.float64),
                               dq=model.table.grad[:B].double().numpy())
                assert not model.table.grad[B:].any()
            r64, r32 = out[torch.float64], out[torch.float32]
            dq = r64["dq"]
            assert np.count_nonzero(dq) <= B and all(np.count_nonzero(np.delete(dq[b], act[b])) == 0 for b in range(B))
            for k, v in (("loss", [r64["loss"], r32["loss"]]), ("dqsel", dq[np.arange(B), act])):
                stacked[k].append(np.asarray(v, np.float64))
            assert np.array_equal(td_of.setdefault(4 * dbl + 2 * tgt + msk, r64["td"]), r64["td"])
            h = td_head(q, on, tg if tgt else None, mask if msk else None, act, mc, gpow, vmask, weight if loss == "msew" else None,
                        bool(dbl), 0.7 if loss == "huber" else None)
            assert abs(h["loss"] - r64["loss"]) <= 1e-12 * abs(r64["loss"]) and np.allclose(h["dq"], dq, rtol=1e-12, atol=1e-15)
            assert np.allclose(h["td_error"], r64["td"], rtol=1e-12, atol=1e-14)
            if loss == "huber":
                a = np.abs(r64["td"])
                assert (a > 0.7).any() and (a < 0.7).any()
        res.update({p + k: np.stack(v) for k, v in stacked.items()})   # one row per entry of HEAD_CASES, in its order
        res[p + "td"] = np.stack([td_of[i] for i in range(8)])


# ---- up ------------------------------------------------------------------------------------------------------------
def fill_rows(rs, n_rows, n_env, D, A, p_end=0.15):
    return dict(obs=f32(rs, n_rows, n_env, D), obs_next=f32(rs, n_rows, n_env, D), act=rs.randint(0, A, (n_rows, n_env)),
                rew=f32(rs, n_rows, n_env), term=rs.rand(n_rows, n_env) < p_end / 2, trunc=rs.rand(n_rows, n_env) < p_end / 2)


def make_dqn(net, A, double, **kw):
    net = copy.deepcopy(net).double() if double else copy.deepcopy(net)
    pol = DiscreteQLearningPolicy(model=net, action_space=gym.spaces.Discrete(A))
    return DQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), gamma=GAMMA, **kw)


def update_section(res):
    rs = np.random.RandomState(9)
    torch.manual_seed(9)
    dims, B, n_env, S, n_step, freq, steps = [6, 32, 32, 5], 37, 3, 16, 3, 2, 3
    D, A = dims[0], dims[-1]
    rows = fill_rows(rs, 20, n_env, D, A)   # 20 rows per sub-buffer of 16: every one wraps around
    bufs = {}
    for dbl in (True, False):
        buf = VectorReplayBuffer(n_env * S, n_env)
        for t in range(20):
            dt = np.float64 if dbl else np.float32
            buf.add(Batch(obs=rows["obs"][t].astype(dt), act=rows["act"][t], rew=rows["rew"][t].astype(np.float64),
                          terminated=rows["term"][t], truncated=rows["trunc"][t], obs_next=rows["obs_next"][t].astype(dt)),
                    buffer_ids=np.arange(n_env))
        bufs[dbl] = buf
    net = QNet(dims)
    init = flat(net).astype(np.float32)
    res.update(up_dims=np.array(dims + [B, n_env, S, n_step, freq, steps, 20], np.int64), up_init=init,
               **{f"up_rows_{k}": v for k, v in rows.items()})
    a64 = make_dqn(net, A, True, n_step_return_horizon=n_step, target_update_freq=freq)
    a32 = make_dqn(net, A, False, n_step_return_horizon=n_step, target_update_freq=freq)
    R = DqnRestatement(init, dims, target_update_freq=freq)
    RB = RestatedBuffer(n_env, S, 1)
    for t in range(20):
        for e in range(n_env):
            RB.add(e, rows["rew"][t, e], bool(rows["term"][t, e]), bool(rows["trunc"][t, e]))
    allidx = bufs[True].sample_indices(0)
    for k in range(steps):
        indices = rs.choice(allidx, B, replace=True).astype(np.int64)
        res[f"up_s{k}_indices"] = indices
        out = {}
        for dbl, algo in ((True, a64), (False, a32)):
            buf = bufs[dbl]
            batch = algo._preprocess_batch(buf[indices], buf, indices)
            stats = algo._update_with_batch(batch)
            grad = np.concatenate([p.grad.detach().double().reshape(-1).numpy() for p in algo.policy.model.parameters()])
            out[dbl] = (stats.loss, flat(algo.policy.model), flat(algo.model_old.module), batch.returns.double().numpy().reshape(-1),
                        grad)
        idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
        o, on = bufs[False][indices].obs, bufs[False][idx_n].obs_next
        assert R.min_kink_gap(np.concatenate([o, on])) > DELTA, "a kink within DELTA: change the seed"
        r = R.update(o, bufs[False][indices].act, on, None, mc, gpow, vmask)
        assert abs(r["loss"] - out[True][0]) <= 1e-11 * abs(out[True][0]), (k, r["loss"], out[True][0])
        assert np.allclose(R.weights(), out[True][1], rtol=1e-10, atol=1e-13) and np.allclose(R.targets(), out[True][2], rtol=1e-10, atol=1e-13)
        assert np.allclose(r["grads"], out[True][4], rtol=1e-10, atol=1e-14)
        digest(res, f"up_s{k}_weights", out[True][1])
        digest(res, f"up_s{k}_targets", out[True][2])
        res.update({f"up_s{k}_loss": np.array([out[True][0], out[False][0]]),
                    f"up_s{k}_grad_eref": np.float64(np.abs(out[True][4] - out[False][4]).max()),
                    f"up_s{k}_weights_eref": np.float64(np.abs(out[True][1] - out[False][1]).max()),
                    f"up_s{k}_returns": out[True][3],
                    f"up_s{k}_returns_eref": np.float64(np.abs(out[True][3] - out[False][3]).max())})
    print("update losses", [float(res[f"up_s{k}_loss"][0]) for k in range(steps)])


# ---- ma ------------------------------------------------------------------------------------------------------------
def marl_section(res):
    rs = np.random.RandomState(21)
    torch.manual_seed(21)
    N, n_env, S, D, A, n_step, T = 2, 3, 8, 4, 3, 2, 7
    dims = [D, 16, A]
    env = FakeEnv(N)
    obs, obs_next = f32(rs, T, n_env, D), f32(rs, T, n_env, D)
    act = rs.randint(0, A, (T, n_env))
    rew = f32(rs, T, n_env, N)
    term, trunc = rs.rand(T, n_env) < 0.1, rs.rand(T, n_env) < 0.1
    mask = np.zeros((T, n_env, A), bool)
    for t in range(T):
        for e in range(n_env):
            mask[t, e, rs.choice(A, rs.randint(1, A + 1), replace=False)] = True
    turn = (np.arange(T)[:, None] + np.arange(n_env)[None, :]) % N       # whose turn a row is
    res.update(ma_dims=np.array([N, n_env, S, D, A, n_step, T] + dims, np.int64), ma_obs=obs, ma_obs_next=obs_next, ma_act=act,
               ma_rew=rew, ma_term=term, ma_trunc=trunc, ma_mask=mask, ma_turn=turn)
    nets = [QNet(dims) for _ in range(N)]
    res["ma_init"] = np.stack([flat(n).astype(np.float32) for n in nets])
    out = {}
    for dbl in (True, False):
        dt = np.float64 if dbl else np.float32
        buf = VectorReplayBuffer(n_env * S, n_env)
        for t in range(T):
            ids = np.array([env.agents[a] for a in turn[t]], dtype=object)
            nxt = np.array([env.agents[(a + 1) % N] for a in turn[t]], dtype=object)
            buf.add(Batch(obs=Batch(agent_id=ids, obs=obs[t].astype(dt), mask=mask[t]), act=act[t], rew=rew[t].astype(np.float64),
                          terminated=term[t], truncated=trunc[t],
                          obs_next=Batch(agent_id=nxt, obs=obs_next[t].astype(dt), mask=mask[t])), buffer_ids=np.arange(n_env))
        algos = [make_dqn(n, A, dbl, n_step_return_horizon=n_step, target_update_freq=3) for n in nets]
        ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=env)
        batch, indices = buf.sample(0)
        stats = ma._update_with_batch(ma._preprocess_batch(batch, buf, indices))
        out[dbl] = [stats._agent_id_to_stats[a].loss for a in env.agents]
    res["ma_loss"] = np.array([out[True], out[False]])
    print("marl losses", out[True])


# ---- ex / sd --------------------------------------------------------------------------------------------------------
def noise_section(res):
    rs = np.random.RandomState(2)
    B, A = 64, 5
    pol = DiscreteQLearningPolicy(model=QNet([3, A]), action_space=gym.spaces.Discrete(A), eps_training=0.3, eps_inference=0.0)
    pol.is_within_training_step = True
    act = rs.randint(0, A, B).astype(np.int64)
    mask = np.zeros((B, A), bool)
    for b in range(B):
        mask[b, rs.choice(A, rs.randint(1, A), replace=False)] = True
    res.update(ex_act=act, ex_mask=mask, ex_seed=np.int64(77), ex_eps=np.float64(0.3))
    np.random.seed(77)
    res["ex_out_nomask"] = pol.add_exploration_noise(act.copy(), Batch(obs=np.zeros((B, 3), np.float32)))
    np.random.seed(77)
    res["ex_out_mask"] = pol.add_exploration_noise(act.copy(), Batch(obs=Batch(obs=np.zeros((B, 3), np.float32), mask=mask)))


def statedict_section(res):
    torch.manual_seed(0)
    net = Net(state_shape=(6,), action_shape=5, hidden_sizes=[32, 32])
    pol = DiscreteQLearningPolicy(model=net, action_space=gym.spaces.Discrete(5))
    algo = DQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), target_update_freq=2)
    sd = {k: v for k, v in algo.state_dict().items() if isinstance(v, torch.Tensor) and v.dim() > 0}
    res["sd_keys"] = np.array(list(sd.keys()))
    res["sd_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])


def main():
    import logging

    logging.disable(logging.WARNING)   # the reference warns once per add about vector-valued episode returns
    torch.set_num_threads(4)
    res = {"delta": np.float64(DELTA)}
    nstep_section(res)
    head_section(res)
    update_section(res)
    marl_section(res)
    noise_section(res)
    statedict_section(res)
    path = os.path.join(HERE, "dqn.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
