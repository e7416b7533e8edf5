"""Generate tests/golden/distq.npz by RUNNING THE REFERENCE's C51, C51Policy, QRDQN and QRDQNPolicy (c51.py, qrdqn.py,
imported through oracle/ref_shim.py) in float64 and float32, with e_ref = max |ref32 - ref64| per array.  In the float64
runs the support and the quantile midpoints keep the reference's float32 values (torch.linspace in float32), carried in
float64; the Q-network modules are defined here (`DistNet`, `DistTable`: the reference's Net casts observations to float32).

Sections (every array is data: inputs, indices, initial weights, expected outputs; large float64 arrays as digests):
  hd_*   shared head inputs per (A, N), A in {2, 5}, N in {2, 51, 200}, B = 37: raw / on / tg i8 = 8 x the logits (a lattice
         of eighths, exact in float32), act, mc, gpow, vmask, weight, mask.  Row 3 of `on` ties actions 0 and 1 at the top;
         row 5 has vmask = 0 and mc on an interior atom; act of no row is out of range.
  dv_*   values and greedy actions of both policies on `on`, with and without the mask.
  c5_*   C51._target_dist + C51._update_with_batch around a table "network", {target net, none} x {weight, none} x
         {mask, none}: losses, priorities, a*, digests of returns and of d loss / d raw.
  qr_*   the same grid for QRDQN._target_q + QRDQN._update_with_batch.
  up_*   three consecutive updates of each learner on dqn.npz's buffer script (net 6-32-32-(5 N), N = 51 / 32, B = 37,
         n_step 3, target_update_freq 2, lr 1e-3): losses, returns digests, weight digests.
  pr_*   two updates of each learner in front of the reference's PrioritizedVectorReplayBuffer: indices, IS weights, losses,
         leaves, max / min priority.
  ma_*   MultiAgentOffPolicyAlgorithm with a C51 agent and a QR-DQN agent on dqn.npz's hand-filled AEC buffer.
  sd_*   reference state_dict keys and shapes;  sig_*  constructor signatures.
The generator asserts that nothing it uses lies within DELTA of a point of non-smoothness (ReLU pre-activations, greedy
top-2 gaps but for the intended tie, |u| against 1, u against 0, unclamped returns against v_min / v_max) and that the
restatement (tests/distq_restatement.py) follows the reference's float64 run.
"""
from __future__ import annotations

import copy
import inspect
import os

import numpy as np

from make_dqn_fixtures import DELTA, GAMMA, FakeEnv, QNet, _Rows, digest, flat  # noqa: E402  (installs the shim)

import torch  # noqa: E402
from torch import nn  # noqa: E402
from tianshou.algorithm.modelfree.c51 import C51, C51Policy  # noqa: E402
from tianshou.algorithm.modelfree.qrdqn import QRDQN, QRDQNPolicy  # noqa: E402
from tianshou.algorithm.multiagent.marl import MultiAgentOffPolicyAlgorithm  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import Net  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from distq_restatement import DistqRestatement, c51_head, dist_values, qr_head, support_of, tau_hat_of  # noqa: E402
from dqn_restatement import RestatedBuffer, nstep_walk  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
V_MIN, V_MAX = -10.0, 10.0
GRID = [(A, N) for A in (2, 5) for N in (2, 51, 200)]
VARIANTS = [(t, w, m) for t in (0, 1) for w in (0, 1) for m in (0, 1)]   # target net, weight, mask


class DistNet(QNet):
    def __init__(self, dims, A, N, softmax) -> None:
        super().__init__(dims)
        self.A, self.N, self.softmax = A, N, softmax

    def forward(self, obs, state=None, info=None):
        x, state = super().forward(obs, state, info)
        x = x.view(-1, self.A, self.N)
        return (torch.softmax(x, dim=-1) if self.softmax else x), state


class DistTable(nn.Module):
    """obs[:, 0] is a row number into a table of raw outputs [rows, A * N]."""

    def __init__(self, table, A, N, softmax) -> None:
        super().__init__()
        self.table = nn.Parameter(torch.as_tensor(table))
        self.A, self.N, self.softmax = A, N, softmax

    def forward(self, obs, state=None, info=None):
        x = self.table[torch.as_tensor(np.asarray(obs)[:, 0]).long()].view(-1, self.A, self.N)
        return (torch.softmax(x, dim=-1) if self.softmax else x), state


def make_algo(kind, model, A, N, double, **kw):
    """The reference learner around `model`; in a float64 run its float32 constants are carried in float64."""
    if kind == "c51":
        pol = C51Policy(model=model, action_space=gym.spaces.Discrete(A), num_atoms=N, v_min=V_MIN, v_max=V_MAX)
        algo = C51(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), gamma=GAMMA, **kw)
        if double:
            pol.support.data = pol.support.data.double()
    else:
        pol = QRDQNPolicy(model=model, action_space=gym.spaces.Discrete(A))
        algo = QRDQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), gamma=GAMMA, num_quantiles=N, **kw)
        if double:
            algo.tau_hat.data = algo.tau_hat.data.double()
    return algo


def emax(a, b):
    return np.float64(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ---- hd / dv / c5 / qr -------------------------------------------------------------------------------------------------
def head_inputs(rs, A, N):
    B = 37
    lat = lambda: rs.randint(-24, 25, (B, A * N)).astype(np.int8)  # noqa: E731
    raw, on, tg = lat(), lat(), lat()
    ramp = np.round(np.linspace(0, 24, N)).astype(np.int8)
    o3 = on[3].reshape(A, N)
    o3[:] = -ramp                          # every action low (the ramp falls) ...
    o3[0] = o3[1] = ramp                   # ... but 0 and 1, which tie at the top: the first one wins
    act = rs.randint(0, A, B).astype(np.int64)
    gpow = (GAMMA ** rs.randint(1, 4, B)).astype(np.float32).astype(np.float64)
    vmask = rs.rand(B) > 0.2
    vmask[5] = False
    weight = (0.5 + rs.rand(B)).astype(np.float32)
    mask = np.zeros((B, A), bool)
    for b in range(B):
        mask[b, rs.choice(A, rs.randint(1, A), replace=False) if A > 1 else 0] = True
    support = support_of(V_MIN, V_MAX, N)

    def gap(row, legal):
        """the smallest top-2 gap of the row's values per action, categorical and quantile, over all and over legal actions"""
        g = np.inf
        for sup in (support, None):
            q = dist_values(row.reshape(1, -1).astype(np.float64) / 8.0, A, N, sup)["q"][0]
            for sel in (q, q[legal]):
                if sel.size > 1:
                    top = np.sort(sel)
                    g = min(g, top[-1] - top[-2])
        return g

    for b in range(B):   # the lattice is coarse at N = 2: redraw a row of `on` whose greedy action is not clear-cut
        while b != 3 and gap(on[b], mask[b]) < 1e-3:
            on[b] = rs.randint(-24, 25, A * N)
    on_atom = float(support[N // 2 + 1]) if N > 2 else 0.3
    vals = np.concatenate([on, tg], 1).astype(np.float64) / 8.0         # every value that can become a quantile target

    def clear(b, m):
        ret = vals[b] * vmask[b] * gpow[b] + m
        r8 = ret * 8.0
        c5 = support * vmask[b] * gpow[b] + m
        return (np.abs(r8 - np.round(r8)).min() > 8 * 4 * DELTA and np.abs(np.abs(c5) - V_MAX).min() > 4 * DELTA)

    mc = np.zeros(B)
    for b in range(B):
        for _ in range(1000):
            m = on_atom if b == 5 else float(np.float32(2.0 * rs.standard_normal()))
            if clear(b, m):
                break
            assert b != 5, "the row on an atom meets a kink: move it"
        else:
            raise AssertionError("no clear reward found")
        mc[b] = m
    return dict(raw=raw, on=on, tg=tg, act=act, mc=mc, gpow=gpow, vmask=vmask, weight=weight, mask=mask)


def head_sections(res):
    rs = np.random.RandomState(15)
    res["cases"] = np.array([f"t{t}w{w}m{m}" for t, w, m in VARIANTS])
    for A, N in GRID:
        inp = head_inputs(rs, A, N)
        p = f"A{A}_N{N}_"
        res.update({"hd_" + p + k: v for k, v in inp.items()})
        B = len(inp["act"])
        raw, on, tg = (inp[k].astype(np.float64) / 8.0 for k in ("raw", "on", "tg"))
        act, mc, gpow, vmask, weight, mask = (inp[k] for k in ("act", "mc", "gpow", "vmask", "weight", "mask"))
        rows = np.arange(B, dtype=np.float32).reshape(B, 1)
        support, tau_hat = support_of(V_MIN, V_MAX, N), tau_hat_of(N)
        # -- dv: the policies' values and greedy actions on `on`
        for kind in ("c51", "qr"):
            out = {}
            for dbl in (True, False):
                algo = make_algo(kind, DistTable(on.astype(np.float64 if dbl else np.float32), A, N, kind == "c51"), A, N, dbl)
                r0 = algo.policy(Batch(obs=rows, info=Batch()))
                r1 = algo.policy(Batch(obs=Batch(obs=rows, mask=mask), info=Batch()))
                q = algo.policy.compute_q_value(r0.logits, None).detach().double().numpy()
                out[dbl] = (q, r0.act, r1.act, r0.logits.detach().double().numpy())
            q64 = out[True][0]
            top = np.sort(q64, 1)
            gaps = top[:, -1] - top[:, -2]
            assert gaps[3] == 0.0 and np.delete(gaps, 3).min() > DELTA and out[True][1][3] == 0
            masked = np.where(mask, q64, -np.inf)
            mtop = np.sort(masked, 1)
            assert all(g > DELTA for b, g in enumerate(mtop[:, -1] - mtop[:, -2]) if b != 3 and np.isfinite(g))
            assert np.array_equal(out[True][1], out[False][1]) and np.array_equal(out[True][2], out[False][2])
            r = dist_values(on, A, N, support if kind == "c51" else None, mask)
            assert np.allclose(r["q"], q64, rtol=1e-12, atol=1e-13) and np.array_equal(r["act"], out[True][2])
            assert np.array_equal(dist_values(on, A, N, support if kind == "c51" else None)["act"], out[True][1])
            if kind == "c51":
                assert np.allclose(r["probs"], out[True][3], rtol=1e-12, atol=1e-300)
            res.update({f"dv_{p}{kind}_q": q64, f"dv_{p}{kind}_q_eref": emax(q64, out[False][0]),
                        f"dv_{p}{kind}_act": out[True][1].astype(np.int64), f"dv_{p}{kind}_act_masked": out[True][2].astype(np.int64)})
        # -- c5 / qr: the heads
        for kind, sec in (("c51", "c5"), ("qr", "qr")):
            keep = {k: [] for k in ("loss", "prio", "prio_eref", "astar", "dout_eref", "ret_eref", "qtaken")}
            for c, (tgt, wgt, msk) in enumerate(VARIANTS):
                out = {}
                for dbl in (True, False):
                    dt = torch.float64 if dbl else torch.float32
                    ndt = np.float64 if dbl else np.float32
                    model = DistTable(np.concatenate([raw, on]).astype(ndt), A, N, kind == "c51")
                    algo = make_algo(kind, model, A, N, dbl, target_update_freq=5 if tgt else 0)
                    if tgt:
                        with torch.no_grad():
                            algo.model_old.module.table[B:] = torch.as_tensor(tg).to(dt)
                    nxt = rows + B
                    obs_next = Batch(obs=nxt, mask=mask) if msk else nxt
                    if kind == "c51":
                        tq = algo._target_q(None, np.arange(B)).detach().numpy().reshape(B, N).copy()
                    else:
                        tq = algo._target_q(_Rows(obs_next), np.arange(B)).detach().numpy().reshape(B, N).copy()
                    assert tq.dtype == ndt
                    tq *= vmask.reshape(-1, 1)                                        # algorithm_base.py:796
                    ret = tq * gpow.reshape(B, 1) + mc.reshape(B, 1)                  # :1213-1215
                    batch = Batch(obs=rows, act=act, obs_next=obs_next, returns=torch.as_tensor(ret).to(dt), info=Batch())
                    if wgt:
                        batch.weight = torch.as_tensor(weight).to(dt)
                    algo._iter = 1   # not a call on which the lagged copy is made: C51 reads the target net after it
                    stats = algo._update_with_batch(batch)
                    out[dbl] = dict(loss=loss_of(stats), prio=batch.weight.detach().double().numpy(), ret=ret.astype(np.float64),
                                    dout=model.table.grad[:B].double().numpy())
                    assert not model.table.grad[B:].any()
                r64, r32 = out[True], out[False]
                fn = c51_head if kind == "c51" else qr_head
                extra = (support, V_MIN, V_MAX) if kind == "c51" else (tau_hat,)
                h = fn(raw, on, tg if tgt else None, mask if msk else None, act, mc, gpow, vmask, weight if wgt else None, *extra,
                       A, N)
                assert abs(h["loss"] - r64["loss"]) <= 1e-11 * abs(r64["loss"]), (kind, A, N, c, h["loss"], r64["loss"])
                assert np.allclose(h["prio"], r64["prio"], rtol=1e-11, atol=1e-13)
                assert np.allclose(h["returns"], r64["ret"], rtol=1e-13, atol=1e-13)
                assert np.allclose(h["d_out"], r64["dout"], rtol=1e-10, atol=1e-15)
                sel = h["d_out"].reshape(B, A, N)[np.arange(B), act]
                assert np.count_nonzero(h["d_out"]) == np.count_nonzero(sel)
                if kind == "qr":
                    u = h["u"]
                    assert np.abs(u).min() > DELTA and np.abs(np.abs(u) - 1.0).min() > DELTA and (np.abs(u) > 1).any()
                else:
                    ret = r64["ret"]
                    assert np.abs(np.abs(ret) - V_MAX).min() > DELTA and (ret > V_MAX).any() and (ret < V_MIN).any()
                    assert N == 2 or (ret[5] == ret[5, 0]).all() and ret[5, 0] in support   # exactly on an atom
                for k, v in (("loss", [r64["loss"], r32["loss"]]), ("prio", r64["prio"]), ("prio_eref", emax(r64["prio"], r32["prio"])),
                             ("astar", h["a_star"].astype(np.int64)), ("dout_eref", emax(r64["dout"], r32["dout"])),
                             ("ret_eref", emax(r64["ret"], r32["ret"])), ("qtaken", h["q_taken"])):
                    keep[k].append(np.asarray(v))
                digest(res, f"{sec}_{p}c{c}_dout", r64["dout"].reshape(-1))
                digest(res, f"{sec}_{p}c{c}_ret", r64["ret"].reshape(-1))
            res.update({f"{sec}_{p}{k}": np.stack(v) for k, v in keep.items()})
        print("heads", A, N, "c51 loss", float(res[f"c5_{p}loss"][0, 0]), "qr loss", float(res[f"qr_{p}loss"][0, 0]))


# ---- up / pr -----------------------------------------------------------------------------------------------------------
UP_N = {"c51": 51, "qr": 32}


def loss_of(stats):
    loss = stats.loss
    return float(loss.mean) if hasattr(loss, "mean") and not isinstance(loss, float) else float(loss)


def up_buffers(gd, cls, **kw):
    d = [int(x) for x in gd["up_dims"]]
    n_env, S, T = d[5], d[6], d[10]
    bufs = {}
    for dbl in (True, False):
        dt = np.float64 if dbl else np.float32
        buf = cls(n_env * S, n_env, **kw)
        for t in range(T):
            buf.add(Batch(obs=gd["up_rows_obs"][t].astype(dt), act=gd["up_rows_act"][t], rew=gd["up_rows_rew"][t].astype(np.float64),
                          terminated=gd["up_rows_term"][t], truncated=gd["up_rows_trunc"][t],
                          obs_next=gd["up_rows_obs_next"][t].astype(dt)), buffer_ids=np.arange(n_env))
        bufs[dbl] = buf
    RB = RestatedBuffer(n_env, S, 1)
    for t in range(T):
        for e in range(n_env):
            RB.add(e, gd["up_rows_rew"][t, e], bool(gd["up_rows_term"][t, e]), bool(gd["up_rows_trunc"][t, e]))
    return bufs, RB


def update_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step, freq, steps = d[4:10]
    A = 5
    class Kink(Exception):
        pass

    def attempt(kind, seed):
        N = UP_N[kind]
        rs = np.random.RandomState(seed)
        torch.manual_seed(seed)
        dims = [6, 32, 32, A * N]
        net = DistNet(dims, A, N, kind == "c51")
        init = flat(net).astype(np.float32)
        res.update({f"up_{kind}_dims": np.array(dims + [A, N], np.int64), f"up_{kind}_init": init})
        algos = {dbl: make_algo(kind, copy.deepcopy(net).double() if dbl else copy.deepcopy(net), A, N, dbl,
                                n_step_return_horizon=n_step, target_update_freq=freq) for dbl in (True, False)}
        bufs, RB = up_buffers(gd, VectorReplayBuffer)
        R = DistqRestatement(init, dims, kind, A, N, target_update_freq=freq, v_min=V_MIN, v_max=V_MAX)
        allidx = bufs[True].sample_indices(0)
        for k in range(steps):
            indices = rs.choice(allidx, B, replace=True).astype(np.int64)
            out = {}
            for dbl, algo in algos.items():
                buf = bufs[dbl]
                batch = algo._preprocess_batch(buf[indices], buf, indices)
                stats = algo._update_with_batch(batch)
                grad = np.concatenate([q.grad.detach().double().reshape(-1).numpy() for q in algo.policy.model.parameters()])
                out[dbl] = (loss_of(stats), flat(algo.policy.model), flat(algo.model_old.module),
                            batch.returns.double().numpy().reshape(-1), grad)
            idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
            o = bufs[False][indices].obs
            on = bufs[False][indices].obs_next if kind == "c51" else bufs[False][idx_n].obs_next   # c51.py:124 / qrdqn.py:95-98
            if R.min_kink_gap(np.concatenate([o, on])) <= DELTA:
                raise Kink
            r = R.update(o, bufs[False][indices].act, on, None, mc, gpow, vmask)
            assert abs(r["loss"] - out[True][0]) <= 1e-10 * abs(out[True][0]), (kind, k, r["loss"], out[True][0])
            assert np.allclose(R.weights(), out[True][1], rtol=1e-9, atol=1e-12) and np.allclose(R.targets(), out[True][2], rtol=1e-9, atol=1e-12)
            assert np.allclose(r["grads"], out[True][4], rtol=1e-9, atol=1e-14)
            assert np.allclose(r["returns"].reshape(-1), out[True][3], rtol=1e-12, atol=1e-13)
            if kind == "qr":
                if not (np.abs(r["u"]).min() > DELTA and np.abs(np.abs(r["u"]) - 1.0).min() > DELTA):
                    raise Kink
            else:
                assert np.abs(np.abs(out[True][3]) - V_MAX).min() > DELTA
                if n_step > 1 and k == 0:   # the quirk shows: the n-step successors would give another loss
                    assert not np.array_equal(bufs[False][indices].obs_next, bufs[False][idx_n].obs_next)
            pk = f"up_{kind}_s{k}_"
            digest(res, pk + "weights", out[True][1])
            digest(res, pk + "targets", out[True][2])
            digest(res, pk + "returns", out[True][3])
            res.update({pk + "indices": indices, pk + "loss": np.array([out[True][0], out[False][0]]),
                        pk + "grad_eref": emax(out[True][4], out[False][4]), pk + "weights_eref": emax(out[True][1], out[False][1]),
                        pk + "returns_eref": emax(out[True][3], out[False][3])})
        print("update losses", kind, [float(res[f"up_{kind}_s{k}_loss"][0]) for k in range(steps)])

    for kind in ("c51", "qr"):   # the first seed whose three updates keep DELTA away from every kink
        for seed in range(31, 131):
            try:
                attempt(kind, seed)
                res[f"up_{kind}_seed"] = np.int64(seed)
                break
            except Kink:
                continue
        else:
            raise AssertionError("no seed without a kink")


def prio_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step, freq = d[4:9]
    A, alpha, beta = 5, 0.6, 0.4
    res.update(pr_alpha=np.float64(alpha), pr_beta=np.float64(beta))
    for kind in ("c51", "qr"):
        N = UP_N[kind]
        dims = [int(x) for x in res[f"up_{kind}_dims"][:4]]
        net = DistNet(dims, A, N, kind == "c51")
        with torch.no_grad():
            o = 0
            for q in net.parameters():
                q.copy_(torch.as_tensor(res[f"up_{kind}_init"][o:o + q.numel()]).reshape(q.shape))
                o += q.numel()
        algos = {dbl: make_algo(kind, copy.deepcopy(net).double() if dbl else copy.deepcopy(net), A, N, dbl,
                                n_step_return_horizon=n_step, target_update_freq=freq) for dbl in (True, False)}
        bufs, _ = up_buffers(gd, PrioritizedVectorReplayBuffer, alpha=alpha, beta=beta)
        bound = bufs[True].weight._bound
        np.random.seed(43)
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
                out[dbl] = (loss_of(stats), w_in, buf.weight._value[bound:bound + n_env * S].copy(),
                            np.array([float(buf._max_prio), float(buf._min_prio)]))
            pk = f"pr_{kind}_s{k}_"
            res.update({pk + "indices": indices, pk + "loss": np.array([out[True][0], out[False][0]]), pk + "weight": out[True][1],
                        pk + "weight_eref": emax(out[True][1], out[False][1]), pk + "leaves": out[True][2],
                        pk + "leaves_eref": emax(out[True][2], out[False][2]), pk + "prio": out[True][3],
                        pk + "prio_eref": emax(out[True][3], out[False][3])})
        print("prioritized losses", kind, [float(res[f"pr_{kind}_s{k}_loss"][0]) for k in range(2)])


# ---- ma / sd / sig -----------------------------------------------------------------------------------------------------
def marl_section(res, gd):
    torch.manual_seed(23)
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    NA = 8
    dims = [D, 16, A * NA]
    env = FakeEnv(N_AG)
    kinds = ["c51", "qr"]
    nets = [DistNet(dims, A, NA, k == "c51") for k in kinds]
    res.update(ma_dims=np.array(dims + [A, NA], np.int64), ma_init=np.stack([flat(n).astype(np.float32) for n in nets]),
               ma_kinds=np.array(kinds))
    out = {}
    for dbl in (True, False):
        dt = np.float64 if dbl else np.float32
        buf = VectorReplayBuffer(n_env * S, n_env)
        for t in range(T):
            ids = np.array([env.agents[a] for a in gd["ma_turn"][t]], dtype=object)
            nxt = np.array([env.agents[(a + 1) % N_AG] for a in gd["ma_turn"][t]], dtype=object)
            buf.add(Batch(obs=Batch(agent_id=ids, obs=gd["ma_obs"][t].astype(dt), mask=gd["ma_mask"][t]), act=gd["ma_act"][t],
                          rew=gd["ma_rew"][t].astype(np.float64), terminated=gd["ma_term"][t], truncated=gd["ma_trunc"][t],
                          obs_next=Batch(agent_id=nxt, obs=gd["ma_obs_next"][t].astype(dt), mask=gd["ma_mask"][t])),
                    buffer_ids=np.arange(n_env))
        algos = [make_algo(k, copy.deepcopy(n).double() if dbl else copy.deepcopy(n), A, NA, dbl, n_step_return_horizon=n_step,
                           target_update_freq=3) for k, n in zip(kinds, nets)]
        ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=env)
        batch, indices = buf.sample(0)
        stats = ma._update_with_batch(ma._preprocess_batch(batch, buf, indices))
        out[dbl] = [loss_of(stats._agent_id_to_stats[a]) for a in env.agents]
    res["ma_loss"] = np.array([out[True], out[False]])
    print("marl losses", out[True])


def statedict_and_signatures(res):
    torch.manual_seed(0)
    for kind, N in (("c51", 51), ("qr", 32)):
        net = Net(state_shape=(6,), action_shape=5, hidden_sizes=[32, 32], softmax=kind == "c51", num_atoms=N)
        algo = make_algo(kind, net, 5, N, False, target_update_freq=2)
        sd = {k: v for k, v in algo.state_dict().items() if isinstance(v, torch.Tensor) and v.dim() > 0}
        res[f"sd_{kind}_keys"] = np.array(list(sd.keys()))
        res[f"sd_{kind}_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    for cls in (C51Policy, C51, QRDQNPolicy, QRDQN):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    gd = dict(np.load(os.path.join(HERE, "dqn.npz")))
    res = {"delta": np.float64(DELTA), "gamma": np.float64(GAMMA), "v_min": np.float64(V_MIN), "v_max": np.float64(V_MAX)}
    head_sections(res)
    update_section(res, gd)
    prio_section(res, gd)
    marl_section(res, gd)
    statedict_and_signatures(res)
    path = os.path.join(HERE, "distq.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
