"""Generate tests/golden/iqn.npz by RUNNING THE REFERENCE's ImplicitQuantileNetwork / CosineEmbeddingNetwork
(utils/net/discrete.py), IQNPolicy and IQN (iqn.py, imported through oracle/ref_shim.py) in float64 and float32, with
e_ref = max |ref32 - ref64| per array.  `torch.rand` is replaced, while the reference runs, by a queue of recorded fractions:
float32 values, carried in float64 in the float64 run, stored here.  The preprocess module `PreNet` is defined here (the
reference's Net casts observations to float32); like Net it ends in its activation.  For the same reason the float64 copy of
a network calls `last`'s nn.Sequential directly (`as_double`).

Sections (every array is data: inputs, indices, fractions, initial weights, expected outputs; large float64 arrays as digests):
  em_*   the embedding and its product with the features, forward and backward, (B, S, C, H) in EM_CASES; inputs are drawn
         from `iqn_restatement`-independent seeded numpy streams (tests/test_host_iqn.py: `em_inputs`), the fractions stored.
  hd_*   shared head inputs per (A, N, N') in GRID, B = 37: out / on / tg i8 = 8 x the values (a lattice of eighths, exact in
         float32), taus, act, mc, gpow, vmask, weight, mask.  Row 3 of `on` ties actions 0 and 1 at the top; row 5 has
         vmask = 0.
  dv_*   values and greedy actions of the policy on `on`, with and without the mask.
  hq_*   QRDQN._target_q + IQN._update_with_batch around a table "network", {target net, none} x {weight, none} x
         {mask, none}: losses, priorities, a*, digests of returns and of d loss / d out.
  up_*   three consecutive updates on dqn.npz's buffer script (preprocess 6-32, C = 8, last 32-32-5, N = N' = 8, B = 37,
         n_step 3, target_update_freq 2, lr 1e-3): fractions, losses, digests of returns, weights and lagged weights.
  pr_*   two updates in front of the reference's PrioritizedVectorReplayBuffer.
  ma_*   MultiAgentOffPolicyAlgorithm with two IQN agents on dqn.npz's hand-filled AEC buffer; every forward over R rows takes
         the first R rows of one stored array of fractions.
  sd_*   reference state_dict keys and shapes;  sig_*  constructor signatures.
The generator asserts that nothing it keeps lies within DELTA of a point of non-smoothness (embedding and MLP
pre-activations at 0 -- RELU_DELTA inside the full updates, see there --, |u| at 1, u at 0, top-2 gaps of q but for the
intended tie) and that the restatement
(tests/iqn_restatement.py) follows the reference's float64 run to 1e-10; it takes the first seed for which that holds.
"""
from __future__ import annotations

import contextlib
import copy
import inspect
import os

import numpy as np

from make_dqn_fixtures import DELTA, GAMMA, FakeEnv, _Rows, digest, flat  # noqa: E402  (installs the shim)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402
from tianshou.algorithm.modelfree.iqn import IQN, IQNPolicy  # noqa: E402
from tianshou.algorithm.multiagent.marl import MultiAgentOffPolicyAlgorithm  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import Net  # noqa: E402
from tianshou.utils.net.discrete import CosineEmbeddingNetwork, ImplicitQuantileNetwork  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from dqn_restatement import RestatedBuffer, nstep_walk  # noqa: E402
from iqn_restatement import IqnRestatement, embed, iqn_head, iqn_values  # noqa: E402
from make_distq_fixtures import emax, loss_of, up_buffers  # noqa: E402
from test_host_iqn import EM_CASES, GRID, em_inputs  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = [(t, w, m) for t in (0, 1) for w in (0, 1) for m in (0, 1)]   # target net, weight, mask
REL = 1e-10
# An update evaluates some 60 000 ReLU pre-activations of size ~0.3 (37 rows x 8 fractions x 32 units, two layers, three
# forwards): about one of them falls within 1e-5 of zero whatever the seed.  What has to hold is that float32 cannot flip a
# unit: a pre-activation is a sum of at most 32 products of that size, good to a few 1e-8 in float32, so 1e-6 leaves a factor
# of ten.  The head's kinks (u at 0, |u| at 1, top-2 gaps of q) keep DELTA.
RELU_DELTA = 1e-6


@contextlib.contextmanager
def fed_rand(queue: list):
    """While active, `torch.rand(R, S, dtype=...)` hands out the next array of `queue` (which must have that shape)."""
    real = torch.rand

    def rand(*shape, dtype=None, device=None, **kw):
        t = np.asarray(queue.pop(0), np.float32)
        assert tuple(shape) == t.shape, (shape, t.shape)
        return torch.as_tensor(t).to(dtype or torch.float32)

    torch.rand = rand
    try:
        yield
    finally:
        torch.rand = real


class PreNet(nn.Module):
    """dims[0] -> ... -> dims[-1], every layer followed by ReLU (as the reference's Net)."""

    def __init__(self, dims) -> None:
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])
        self.out = dims[-1]

    def get_output_dim(self):
        return self.out

    def forward(self, obs, state=None, info=None):
        x = torch.as_tensor(np.asarray(obs), dtype=self.layers[0].weight.dtype)
        for l in self.layers:
            x = F.relu(l(x))
        return x, state


class TauTable(nn.Module):
    """obs[:, 0] is a row number into a table of outputs [rows, S, A]; the fractions come from `taus` [rows, S]."""

    def __init__(self, table, taus) -> None:
        super().__init__()
        self.table = nn.Parameter(torch.as_tensor(table))
        self.taus = torch.as_tensor(taus).to(self.table.dtype)

    def forward(self, obs, sample_size, state=None, info=None):
        idx = torch.as_tensor(np.asarray(obs)[:, 0]).long()
        x = self.table[idx]
        assert x.shape[1] == sample_size, (x.shape, sample_size)
        return (x.transpose(1, 2), self.taus[idx]), state


def as_double(net):
    """A float64 copy of an ImplicitQuantileNetwork.  The reference's MLP.forward casts its input to float32 (common.py:175);
    the copy calls `last`'s nn.Sequential itself, which is all that MLP.forward does after that cast."""
    net = copy.deepcopy(net).double()
    net.last = net.last.model
    return net


def make_algo(model, A, n_on, n_tg, **kw):
    pol = IQNPolicy(model=model, action_space=gym.spaces.Discrete(A), sample_size=n_on, online_sample_size=n_on,
                    target_sample_size=n_tg)
    return IQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), gamma=GAMMA, **kw)


# ---- em ----------------------------------------------------------------------------------------------------------------
def embed_section(res):
    for case in EM_CASES:
        B, S, C, H, act_f = case
        for seed in range(100):
            rs = np.random.RandomState(1000 + seed)
            taus = rs.rand(B, S).astype(np.float32)
            d = em_inputs(case)
            r = embed(d["f"], taus, d["We"], d["be"], bool(act_f), d["d_e"])
            if np.abs(r["pre"]).min() > DELTA and (not act_f or np.abs(d["f"]).min() > DELTA):
                break
        else:
            raise AssertionError("no seed without a kink")
        out = {}
        for dbl in (True, False):
            dt = torch.float64 if dbl else torch.float32
            emb = CosineEmbeddingNetwork(C, H)
            with torch.no_grad():
                emb.net[0].weight.copy_(torch.as_tensor(d["We"]))
                emb.net[0].bias.copy_(torch.as_tensor(d["be"]))
            emb = emb.to(dt)
            f = torch.as_tensor(d["f"]).to(dt).requires_grad_(True)
            g = F.relu(f) if act_f else f
            e = (g.unsqueeze(1) * emb(torch.as_tensor(taus).to(dt))).view(B * S, -1)     # discrete.py:212-215
            e.backward(torch.as_tensor(d["d_e"]).to(dt))
            out[dbl] = [x.detach().double().numpy() for x in (e, f.grad, emb.net[0].weight.grad, emb.net[0].bias.grad)]
        p = "em_B%d_S%d_C%d_H%d_" % case[:4]
        res[p + "taus"] = taus
        for k, a64, a32 in zip(("e", "d_f", "dWe", "dbe"), out[True], out[False]):
            assert np.allclose(r[k], a64, rtol=REL, atol=REL * np.abs(a64).max()), (case, k)
            digest(res, p + k, a64.reshape(-1))
            res[p + k + "_eref"] = emax(a64, a32)
        print("embed", case, "min |pre|", float(np.abs(r["pre"]).min()))


# ---- hd / dv / hq ------------------------------------------------------------------------------------------------------
def head_inputs(rs, A, N, Np):
    B = 37
    lat = lambda n: rs.randint(-24, 25, (B, n, A)).astype(np.int8)  # noqa: E731
    out, on, tg = lat(N), lat(N), lat(Np)
    ramp = np.round(np.linspace(0, 24, N)).astype(np.int8)
    on[3] = -ramp[:, None]                   # every action low ...
    on[3, :, 0] = on[3, :, 1] = ramp         # ... but 0 and 1, which tie at the top: the first one wins
    taus = rs.rand(B, N).astype(np.float32)
    act = rs.randint(0, A, B).astype(np.int64)
    gpow = (GAMMA ** rs.randint(1, 4, B)).astype(np.float32).astype(np.float64)
    vmask = rs.rand(B) > 0.2
    vmask[5] = False
    weight = (0.5 + rs.rand(B)).astype(np.float32)
    mask = np.zeros((B, A), bool)
    for b in range(B):
        mask[b, rs.choice(A, rs.randint(1, A), replace=False) if A > 1 else 0] = True

    def gap(row, legal):
        q = row.astype(np.float64).mean(0) / 8.0
        g = np.inf
        for sel in (q, q[legal]):
            if sel.size > 1:
                top = np.sort(sel)
                g = min(g, top[-1] - top[-2])
        return g

    for b in range(B):   # redraw a row of `on` whose greedy action is not clear-cut
        while b != 3 and gap(on[b], mask[b]) < 1e-3:
            on[b] = rs.randint(-24, 25, (N, A))
    vals = np.concatenate([on.reshape(B, -1), tg.reshape(B, -1)], 1).astype(np.float64) / 8.0

    def clear(b, m):   # every possible target keeps 4 DELTA from the lattice of the current values: u != 0, |u| != 1
        r8 = (vals[b] * vmask[b] * gpow[b] + m) * 8.0
        return np.abs(r8 - np.round(r8)).min() > 8 * 4 * DELTA

    mc = np.zeros(B)
    for b in range(B):
        for _ in range(1000):
            m = float(np.float32(2.0 * rs.standard_normal()))
            if clear(b, m):
                break
        else:
            raise AssertionError("no clear reward found")
        mc[b] = m
    return dict(out=out, on=on, tg=tg, taus=taus, act=act, mc=mc, gpow=gpow, vmask=vmask, weight=weight, mask=mask)


def head_sections(res):
    rs = np.random.RandomState(17)
    res["cases"] = np.array([f"t{t}w{w}m{m}" for t, w, m in VARIANTS])
    for A, N, Np in GRID:
        inp = head_inputs(rs, A, N, Np)
        p = f"A{A}_N{N}_M{Np}_"
        res.update({"hd_" + p + k: v for k, v in inp.items()})
        B = 37
        out_, on, tg = (inp[k].astype(np.float64) / 8.0 for k in ("out", "on", "tg"))
        taus, act, mc, gpow, vmask, weight, mask = (inp[k] for k in ("taus", "act", "mc", "gpow", "vmask", "weight", "mask"))
        rows = np.arange(B, dtype=np.float32).reshape(B, 1)
        tt = np.concatenate([taus, taus])
        # -- dv
        o = {}
        for dbl in (True, False):
            ndt = np.float64 if dbl else np.float32
            algo = make_algo(TauTable(np.concatenate([out_, on]).astype(ndt), tt), A, N, Np)
            r0 = algo.policy(Batch(obs=rows + B, info=Batch()))
            r1 = algo.policy(Batch(obs=Batch(obs=rows + B, mask=mask), info=Batch()))
            assert r0.logits.shape == (B, A, N) and r0.taus.shape == (B, N)
            o[dbl] = (algo.policy.compute_q_value(r0.logits, None).detach().double().numpy(), r0.act, r1.act)
        q64 = o[True][0]
        top = np.sort(q64, 1)
        gaps = top[:, -1] - top[:, -2]
        assert gaps[3] == 0.0 and np.delete(gaps, 3).min() > DELTA and o[True][1][3] == 0
        assert np.array_equal(o[True][1], o[False][1]) and np.array_equal(o[True][2], o[False][2])
        rv = iqn_values(on, mask)
        assert np.allclose(rv["q"], q64, rtol=1e-12, atol=1e-13) and np.array_equal(rv["act"], o[True][2])
        assert np.array_equal(iqn_values(on)["act"], o[True][1])
        res.update({f"dv_{p}q": q64, f"dv_{p}q_eref": emax(q64, o[False][0]), f"dv_{p}act": o[True][1].astype(np.int64),
                    f"dv_{p}act_masked": o[True][2].astype(np.int64)})
        # -- hq
        keep = {k: [] for k in ("loss", "prio", "prio_eref", "astar", "dout_eref", "ret_eref", "qtaken")}
        for c, (tgt, wgt, msk) in enumerate(VARIANTS):
            o = {}
            for dbl in (True, False):
                dt, ndt = (torch.float64, np.float64) if dbl else (torch.float32, np.float32)
                model = TauTable(np.concatenate([out_, on]).astype(ndt), tt)
                algo = make_algo(model, A, N, Np, target_update_freq=5 if tgt else 0)
                if tgt:   # the lagged "network": Np fractions per row, its own values on the successor rows
                    old = algo.model_old.module
                    old.table = nn.Parameter(torch.as_tensor(np.concatenate([np.zeros_like(tg), tg]).astype(ndt)))
                    old.taus = torch.zeros(2 * B, Np, dtype=dt)
                nxt = rows + B
                obs_next = Batch(obs=nxt, mask=mask) if msk else nxt
                tq = algo._target_q(_Rows(obs_next), np.arange(B)).detach().numpy().copy()
                assert tq.dtype == ndt and tq.shape == (B, Np if tgt else N)
                tq *= vmask.reshape(-1, 1)                                        # algorithm_base.py:796
                ret = tq * gpow.reshape(B, 1) + mc.reshape(B, 1)                  # :1213-1215
                batch = Batch(obs=rows, act=act, obs_next=obs_next, returns=torch.as_tensor(ret).to(dt), info=Batch())
                if wgt:
                    batch.weight = torch.as_tensor(weight).to(dt)
                algo._iter = 1
                stats = algo._update_with_batch(batch)
                o[dbl] = dict(loss=loss_of(stats), prio=batch.weight.detach().double().numpy(), ret=ret.astype(np.float64),
                              dout=model.table.grad[:B].double().numpy())
                assert not model.table.grad[B:].any()
            r64, r32 = o[True], o[False]
            h = iqn_head(out_, on, tg if tgt else None, mask if msk else None, taus, act, mc, gpow, vmask, weight if wgt else None)
            assert abs(h["loss"] - r64["loss"]) <= 1e-11 * abs(r64["loss"]), (A, N, Np, c, h["loss"], r64["loss"])
            assert np.allclose(h["prio"], r64["prio"], rtol=1e-11, atol=1e-13)
            assert np.allclose(h["returns"], r64["ret"], rtol=1e-13, atol=1e-13)
            assert np.allclose(h["d_out"], r64["dout"], rtol=1e-10, atol=1e-15)
            sel = h["d_out"][np.arange(B), :, act]
            assert np.count_nonzero(h["d_out"]) == np.count_nonzero(sel)
            u = h["u"]
            assert np.abs(u).min() > DELTA and np.abs(np.abs(u) - 1.0).min() > DELTA and (np.abs(u) > 1).any() and (np.abs(u) < 1).any()
            for k, v in (("loss", [r64["loss"], r32["loss"]]), ("prio", r64["prio"]), ("prio_eref", emax(r64["prio"], r32["prio"])),
                         ("astar", h["a_star"].astype(np.int64)), ("dout_eref", emax(r64["dout"], r32["dout"])),
                         ("ret_eref", emax(r64["ret"], r32["ret"])), ("qtaken", h["q_taken"])):
                keep[k].append(np.asarray(v))
            digest(res, f"hq_{p}c{c}_dout", r64["dout"].reshape(-1))
            digest(res, f"hq_{p}c{c}_ret", r64["ret"].reshape(-1))
        res.update({f"hq_{p}{k}": np.stack(v) for k, v in keep.items()})   # one row per entry of VARIANTS, in its order
        print("heads", A, N, Np, "loss", float(res[f"hq_{p}loss"][0, 0]))


# ---- up / pr -------------------------------------------------------------------------------------------------------------
PRE, HID, A_UP, C_UP, S_UP = [6, 32], [32], 5, 8, 8


def iq_net():
    return ImplicitQuantileNetwork(preprocess_net=PreNet(PRE), action_shape=A_UP, hidden_sizes=HID, num_cosines=C_UP)


def restated(init, freq):
    return IqnRestatement(init, PRE, [PRE[-1], *HID, A_UP], C_UP, feature_act=True, target_update_freq=freq)


def update_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step, freq, steps = d[4:10]

    class Kink(Exception):
        pass

    def attempt(seed):
        rs = np.random.RandomState(seed)
        torch.manual_seed(seed)
        net = iq_net()
        init = flat(net).astype(np.float32)
        res.update(up_dims=np.array(PRE + HID + [A_UP, C_UP, S_UP], np.int64), up_init=init)
        algos = {dbl: make_algo(as_double(net) if dbl else copy.deepcopy(net), A_UP, S_UP, S_UP,
                                n_step_return_horizon=n_step, target_update_freq=freq) for dbl in (True, False)}
        bufs, RB = up_buffers(gd, VectorReplayBuffer)
        R = restated(init, freq)
        allidx = bufs[True].sample_indices(0)
        for k in range(steps):
            indices = rs.choice(allidx, B, replace=True).astype(np.int64)
            taus = rs.rand(3, B, S_UP).astype(np.float32)
            out = {}
            for dbl, algo in algos.items():
                buf = bufs[dbl]
                queue = list(taus)
                with fed_rand(queue):
                    batch = algo._preprocess_batch(buf[indices], buf, indices)
                    stats = algo._update_with_batch(batch)
                assert not queue   # three draws: online and lagged on the successor rows, online on the sampled rows
                grad = np.concatenate([q.grad.detach().double().reshape(-1).numpy() for q in algo.policy.model.parameters()])
                out[dbl] = (loss_of(stats), flat(algo.policy.model), flat(algo.model_old.module),
                            batch.returns.double().numpy().reshape(-1), grad)
            idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
            o, on = bufs[False][indices].obs, bufs[False][idx_n].obs_next
            r = R.update(o, bufs[False][indices].act, on, None, mc, gpow, vmask, taus)
            if r["head_gap"] <= DELTA or r["relu_gap"] <= RELU_DELTA:
                raise Kink
            assert abs(r["loss"] - out[True][0]) <= REL * abs(out[True][0]), (k, r["loss"], out[True][0])
            assert np.allclose(R.weights(), out[True][1], rtol=1e-9, atol=1e-12) and np.allclose(R.targets(), out[True][2], rtol=1e-9, atol=1e-12)
            assert np.allclose(r["grads"], out[True][4], rtol=1e-9, atol=1e-14)
            assert np.allclose(r["returns"].reshape(-1), out[True][3], rtol=1e-12, atol=1e-13)
            pk = f"up_s{k}_"
            digest(res, pk + "weights", out[True][1])
            digest(res, pk + "targets", out[True][2])
            digest(res, pk + "returns", out[True][3])
            res.update({pk + "indices": indices, pk + "taus": taus, pk + "loss": np.array([out[True][0], out[False][0]]),
                        pk + "grad_eref": emax(out[True][4], out[False][4]), pk + "weights_eref": emax(out[True][1], out[False][1]),
                        pk + "returns_eref": emax(out[True][3], out[False][3])})
        print("update losses", [float(res[f"up_s{k}_loss"][0]) for k in range(steps)])

    for seed in range(31, 131):   # the first seed whose three updates keep DELTA away from every kink
        try:
            attempt(seed)
            res["up_seed"] = np.int64(seed)
            break
        except Kink:
            continue
    else:
        raise AssertionError("no seed without a kink")


def load_flat(net, init):
    with torch.no_grad():
        o = 0
        for q in net.parameters():
            q.copy_(torch.as_tensor(init[o:o + q.numel()]).reshape(q.shape))
            o += q.numel()
    return net


def prio_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step, freq = d[4:9]
    alpha, beta = 0.6, 0.4
    res.update(pr_alpha=np.float64(alpha), pr_beta=np.float64(beta))
    net = load_flat(iq_net(), res["up_init"])
    algos = {dbl: make_algo(as_double(net) if dbl else copy.deepcopy(net), A_UP, S_UP, S_UP,
                            n_step_return_horizon=n_step, target_update_freq=freq) for dbl in (True, False)}
    bufs, _ = up_buffers(gd, PrioritizedVectorReplayBuffer, alpha=alpha, beta=beta)
    bound = bufs[True].weight._bound
    np.random.seed(43)
    rs = np.random.RandomState(44)
    for k in range(2):
        indices = bufs[True].sample_indices(B).astype(np.int64)
        taus = rs.rand(3, B, S_UP).astype(np.float32)
        out = {}
        for dbl, algo in algos.items():
            buf = bufs[dbl]
            batch = buf[indices]
            w_in = np.asarray(batch.weight, np.float64).copy()
            with fed_rand(list(taus)):
                batch = algo._preprocess_batch(batch, buf, indices)
                stats = algo._update_with_batch(batch)
            algo._postprocess_batch(batch, buf, indices)
            out[dbl] = (loss_of(stats), w_in, buf.weight._value[bound:bound + n_env * S].copy(),
                        np.array([float(buf._max_prio), float(buf._min_prio)]))
        pk = f"pr_s{k}_"
        res.update({pk + "indices": indices, pk + "taus": taus, pk + "loss": np.array([out[True][0], out[False][0]]),
                    pk + "weight": out[True][1], pk + "weight_eref": emax(out[True][1], out[False][1]), pk + "leaves": out[True][2],
                    pk + "leaves_eref": emax(out[True][2], out[False][2]), pk + "prio": out[True][3],
                    pk + "prio_eref": emax(out[True][3], out[False][3])})
    print("prioritized losses", [float(res[f"pr_s{k}_loss"][0]) for k in range(2)])


# ---- ma / sd / sig -------------------------------------------------------------------------------------------------------
def marl_section(res, gd):
    torch.manual_seed(23)
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    pre, hid, C, NS = [D, 16], [], 4, 4
    env = FakeEnv(N_AG)
    nets = [ImplicitQuantileNetwork(preprocess_net=PreNet(pre), action_shape=A, hidden_sizes=hid, num_cosines=C) for _ in range(N_AG)]
    base = np.random.RandomState(24).rand(n_env * S, NS).astype(np.float32)
    res.update(ma_dims=np.array(pre + [A, C, NS], np.int64), ma_init=np.stack([flat(n).astype(np.float32) for n in nets]),
               ma_taus=base)

    real = torch.rand
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
        algos = [make_algo(as_double(n) if dbl else copy.deepcopy(n), A, NS, NS, n_step_return_horizon=n_step,
                           target_update_freq=3) for n in nets]
        ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=env)
        batch, indices = buf.sample(0)
        torch.rand = lambda R, S_, dtype=None, device=None: torch.as_tensor(base[:R, :S_]).to(dtype)  # noqa: E731
        try:
            stats = ma._update_with_batch(ma._preprocess_batch(batch, buf, indices))
        finally:
            torch.rand = real
        out[dbl] = [loss_of(stats._agent_id_to_stats[a]) for a in env.agents]
    res["ma_loss"] = np.array([out[True], out[False]])
    print("marl losses", out[True])


def statedict_and_signatures(res):
    torch.manual_seed(0)
    net = ImplicitQuantileNetwork(preprocess_net=Net(state_shape=(PRE[0],), hidden_sizes=PRE[1:]), action_shape=A_UP,
                                  hidden_sizes=HID, num_cosines=C_UP)
    algo = make_algo(net, A_UP, S_UP, S_UP, target_update_freq=2)
    sd = {k: v for k, v in algo.state_dict().items() if isinstance(v, torch.Tensor) and v.dim() > 0}
    res["sd_keys"] = np.array(list(sd.keys()))
    res["sd_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    names = [k for k, _ in net.named_parameters()]
    assert names == [k[len("policy.model."):] for k in sd if k.startswith("policy.model.")]   # `parameters()` order
    for cls in (IQNPolicy, IQN):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    gd = dict(np.load(os.path.join(HERE, "dqn.npz")))
    res = {"delta": np.float64(DELTA), "relu_delta": np.float64(RELU_DELTA), "gamma": np.float64(GAMMA)}
    embed_section(res)
    head_sections(res)
    update_section(res, gd)
    prio_section(res, gd)
    marl_section(res, gd)
    statedict_and_signatures(res)
    path = os.path.join(HERE, "iqn.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
