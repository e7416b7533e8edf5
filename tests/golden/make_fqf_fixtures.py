"""Generate tests/golden/fqf.npz by RUNNING THE REFERENCE's FractionProposalNetwork / FullQuantileFunction
(utils/net/discrete.py), FQFPolicy and FQF (fqf.py, imported through oracle/ref_shim.py) in float64 and float32, with
e_ref = max |ref32 - ref64| per array.  `PreNet` and `as_double` are make_iqn_fixtures.py's.  The fractions need no feeding:
they are a deterministic output of the fraction model.

Sections (every array is data: inputs, indices, initial weights, expected outputs; large float64 arrays as digests):
  pp_*   the proposal, forward and backward from a given d_logits, (R, H, N, relu_f) in PP_CASES; inputs from seeded numpy
         streams (tests/test_host_fqf.py: `pp_inputs`).
  hd_*   shared head inputs per (A, N) in GRID, B = 37: out / on / tg i8 = 8 x the values (a lattice of eighths), out_tau i8 =
         16 x the values (odd sixteenths: never on the lattice of out), the fraction logits of the sampled and of the successor
         rows, act, mc, gpow, vmask, weight, mask.  Row 3 of `on` ties actions 0 and 1 at the top; row 5 has vmask = 0.
  dv_*   values and greedy actions of the policy on `on`, with and without the mask.
  hq_*   FQF._target_q + FQF._update_with_batch around a table "network" whose outputs at tau_hats, outputs at the interior
         fractions and fraction logits are parameters (so the reference's autograd gives d loss / d out and d loss / d logits),
         {target net, none} x {weight, none} x {mask, none} x ent_coef {0, 0.01}.
  up_*   three consecutive updates on dqn.npz's buffer script (preprocess 6-32, C = 8, last 32-32-5, N = 8, B = 37, n_step 3,
         target_update_freq 2, both Adam lr 1e-3, ent_coef 0.01): the four statistics, digests of returns, both weight
         vectors and the lagged weights, the gradients' e_ref.
  pr_*   two updates in front of the reference's PrioritizedVectorReplayBuffer.
  ma_*   MultiAgentOffPolicyAlgorithm with two FQF agents on dqn.npz's hand-filled AEC buffer.
  sd_*   reference state_dict keys and shapes;  sig_*  constructor signatures and the fields of FQFTrainingStats.
The generator asserts that nothing it keeps lies within DELTA of a point of non-smoothness (ReLU pre-activations at 0 --
RELU_DELTA inside the full updates, as make_iqn_fixtures.py --, |u| at 1, u at 0, top-2 gaps of q but for the intended tie, the
two sides of every s1 / s2 comparison) and that the restatement (tests/fqf_restatement.py) follows the reference's float64
run to 1e-10; it takes the first seed for which that holds.
"""
from __future__ import annotations

import copy
import dataclasses
import inspect
import os

import numpy as np

from make_dqn_fixtures import DELTA, GAMMA, FakeEnv, _Rows, digest, flat  # noqa: E402  (installs the shim)

import torch  # noqa: E402
from torch import nn  # noqa: E402
from tianshou.algorithm.modelfree.fqf import FQF, FQFPolicy, FQFTrainingStats  # noqa: E402
from tianshou.algorithm.multiagent.marl import MultiAgentOffPolicyAlgorithm  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import Net  # noqa: E402
from tianshou.utils.net.discrete import FractionProposalNetwork, FullQuantileFunction  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from dqn_restatement import nstep_walk  # noqa: E402
from fqf_restatement import FqfRestatement, fqf_head, fqf_values, fractions_of, propose  # noqa: E402
from make_distq_fixtures import emax, loss_of, up_buffers  # noqa: E402
from make_iqn_fixtures import RELU_DELTA, PreNet, as_double, load_flat  # noqa: E402
from test_host_fqf import ENT_COEFS, GRID, PP_CASES, STAT_KEYS, pp_inputs  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = [(t, w, m, e) for e in range(len(ENT_COEFS)) for t in (0, 1) for w in (0, 1) for m in (0, 1)]   # target, weight, mask
REL = 1e-10


def stats_of(stats):
    return np.array([loss_of(stats)] + [float(getattr(stats, k)) for k in STAT_KEYS[1:]])


class RowTable(nn.Module):
    """A row number -> that row of a table of parameters."""

    def __init__(self, table) -> None:
        super().__init__()
        self.table = nn.Parameter(torch.as_tensor(table))

    def forward(self, idx):
        return self.table[idx.long()]


class FqfTable(nn.Module):
    """A stand-in for the quantile network with FullQuantileFunction.forward's interface: obs[:, 0] is a row number into
    `hat` [rows, N, A], the outputs at tau_hats, and `tau` [rows, N - 1, A], those at the interior fractions (given out in
    training mode only, without a graph).  The proposal model (a FractionProposalNetwork whose `net` is a RowTable of fraction
    logits) is handed the row numbers when no fractions come with the call."""

    def __init__(self, hat, tau) -> None:
        super().__init__()
        self.hat, self.tau = nn.Parameter(torch.as_tensor(hat)), nn.Parameter(torch.as_tensor(tau))

    def forward(self, obs, propose_model, fractions=None, state=None, info=None):
        rows = torch.as_tensor(np.asarray(obs)[:, 0]).long()
        given = fractions if fractions is not None else Batch(dict(zip(("taus", "tau_hats", "entropies"), propose_model(rows))))
        interior = self.tau.detach()[rows].transpose(1, 2) if self.training else None
        return (self.hat[rows].transpose(1, 2), given, interior), state


def make_algo(model, frac, A, ent_coef=0.0, **kw):
    pol = FQFPolicy(model=model, fraction_model=frac, action_space=gym.spaces.Discrete(A))
    return FQF(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), fraction_optim=AdamOptimizerFactory(lr=1e-3), gamma=GAMMA,
               ent_coef=ent_coef, **kw)


# ---- pp ----------------------------------------------------------------------------------------------------------------
def propose_section(res):
    for case in PP_CASES:
        R, H, N, act_f = case
        d = pp_inputs(case)
        assert not act_f or np.abs(d["f"]).min() > DELTA
        r = propose(d["f"], d["Wf"], d["bf"], bool(act_f), d["d_logits"])
        out = {}
        for dbl in (True, False):
            dt = torch.float64 if dbl else torch.float32
            net = FractionProposalNetwork(N, H)
            with torch.no_grad():
                net.net.weight.copy_(torch.as_tensor(d["Wf"]))
                net.net.bias.copy_(torch.as_tensor(d["bf"]))
            net = net.to(dt)
            f = torch.as_tensor(d["f"]).to(dt)
            taus, tau_hats, entropies = net(torch.relu(f) if act_f else f)
            # the logits reach autograd through taus and entropies only: d_logits enters as the gradient of the linear layer
            net.net(torch.relu(f) if act_f else f).backward(torch.as_tensor(d["d_logits"]).to(dt))
            out[dbl] = [x.detach().double().numpy() for x in (taus, tau_hats, entropies, net.net.weight.grad, net.net.bias.grad)]
        p = "pp_R%d_H%d_N%d_" % case[:3]
        for k, a64, a32 in zip(("taus", "tau_hats", "entropies", "dWf", "dbf"), out[True], out[False]):
            assert np.allclose(r[k], a64, rtol=REL, atol=REL * np.abs(a64).max()), (case, k)
            digest(res, p + k, a64.reshape(-1))
            res[p + k + "_eref"] = emax(a64, a32)
        print("propose", case, "entropy", float(out[True][2].mean()))


# ---- hd / dv / hq ------------------------------------------------------------------------------------------------------
def head_inputs(rs, A, N):
    B = 37
    lat = lambda n: rs.randint(-24, 25, (B, n, A)).astype(np.int8)  # noqa: E731
    out, on, tg = lat(N), lat(N), lat(N)
    out_tau = (2 * rs.randint(-24, 24, (B, N - 1, A)) + 1).astype(np.int8)      # odd sixteenths
    if A > 1:
        ramp = np.round(np.linspace(0, 24, N)).astype(np.int8)
        on[3] = -ramp[:, None]                   # every action low ...
        on[3, :, 0] = on[3, :, 1] = ramp         # ... but 0 and 1, which tie at the top: the first one wins
    xf, xf_next = (0.5 * rs.standard_normal((B, N))).astype(np.float32), (0.5 * rs.standard_normal((B, N))).astype(np.float32)
    act = rs.randint(0, A, B).astype(np.int64)
    for b in range(B):   # neighbouring interior quantiles of the taken action differ: every s1 / s2 comparison is clear-cut
        for i in range(1, N - 1):
            while out_tau[b, i, act[b]] == out_tau[b, i - 1, act[b]]:
                out_tau[b, i, act[b]] = 2 * rs.randint(-24, 24) + 1
    gpow = (GAMMA ** rs.randint(1, 4, B)).astype(np.float32).astype(np.float64)
    vmask = rs.rand(B) > 0.2
    vmask[5] = False
    weight = (0.5 + rs.rand(B)).astype(np.float32)
    mask = np.zeros((B, A), bool)
    for b in range(B):
        mask[b, rs.choice(A, rs.randint(1, A), replace=False) if A > 1 else 0] = True
    taus_next = fractions_of(xf_next)["taus"]

    def gap(b):
        q = fqf_values(on[b:b + 1].astype(np.float64) / 8.0, taus_next[b:b + 1])["q"][0]
        g = np.inf
        for sel in (q, q[mask[b]]):
            if sel.size > 1:
                top = np.sort(sel)
                g = min(g, top[-1] - top[-2])
        return g

    for b in range(B):   # redraw a row of `on` whose greedy action is not clear-cut
        while not (b == 3 and A > 1) and gap(b) < 1e-3:
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
    return dict(out=out, out_tau=out_tau, on=on, tg=tg, xf=xf, xf_next=xf_next, act=act, mc=mc, gpow=gpow, vmask=vmask,
                weight=weight, mask=mask)


def head_sections(res):
    rs = np.random.RandomState(19)
    res["cases"] = np.array([f"t{t}w{w}m{m}e{e}" for t, w, m, e in VARIANTS])
    res["ent_coefs"] = np.array(ENT_COEFS)
    B = 37
    for A, N in GRID:
        inp = head_inputs(rs, A, N)
        p = f"A{A}_N{N}_"
        res.update({"hd_" + p + k: v for k, v in inp.items()})
        out_, on, tg = (inp[k].astype(np.float64) / 8.0 for k in ("out", "on", "tg"))
        out_tau = inp["out_tau"].astype(np.float64) / 16.0
        xf, xf_next, act, mc, gpow, vmask, weight, mask = (inp[k] for k in ("xf", "xf_next", "act", "mc", "gpow", "vmask", "weight", "mask"))
        rows = np.arange(B, dtype=np.float32).reshape(B, 1)
        taus_next = fractions_of(xf_next)["taus"]

        def tables(ndt, hat_next=on):
            model = FqfTable(np.concatenate([out_, hat_next]).astype(ndt), np.concatenate([out_tau, out_tau]).astype(ndt))
            frac = FractionProposalNetwork(N, N)
            frac.net = RowTable(np.concatenate([xf, xf_next]).astype(ndt))
            return model, frac

        # -- dv
        o = {}
        for dbl in (True, False):
            algo = make_algo(*tables(np.float64 if dbl else np.float32), A)
            r0 = algo.policy(Batch(obs=rows + B, info=Batch()))
            r1 = algo.policy(Batch(obs=Batch(obs=rows + B, mask=mask), info=Batch()))
            assert r0.logits.shape == (B, A, N) and r0.fractions.taus.shape == (B, N + 1) and r0.quantiles_tau.shape == (B, A, N - 1)
            t = r0.fractions.taus
            q = ((t[:, 1:] - t[:, :-1]).unsqueeze(1) * r0.logits).sum(2)
            o[dbl] = (q.detach().double().numpy(), r0.act, r1.act)
        q64 = o[True][0]
        if A > 1:
            top = np.sort(q64, 1)
            gaps = top[:, -1] - top[:, -2]
            assert gaps[3] == 0.0 and np.delete(gaps, 3).min() > DELTA and o[True][1][3] == 0
        assert np.array_equal(o[True][1], o[False][1]) and np.array_equal(o[True][2], o[False][2])
        rv = fqf_values(on, taus_next, mask)
        assert np.allclose(rv["q"], q64, rtol=1e-12, atol=1e-13) and np.array_equal(rv["act"], o[True][2])
        assert np.array_equal(fqf_values(on, taus_next)["act"], o[True][1])
        res.update({f"dv_{p}q": q64, f"dv_{p}q_eref": emax(q64, o[False][0]), f"dv_{p}act": o[True][1].astype(np.int64),
                    f"dv_{p}act_masked": o[True][2].astype(np.int64)})
        # -- hq
        keep = {k: [] for k in ("stats", "prio", "prio_eref", "astar", "dout_eref", "dlog_eref", "ret_eref", "qtaken")}
        for c, (tgt, wgt, msk, e) in enumerate(VARIANTS):
            o = {}
            for dbl in (True, False):
                dt, ndt = (torch.float64, np.float64) if dbl else (torch.float32, np.float32)
                model, frac = tables(ndt)
                algo = make_algo(model, frac, A, ENT_COEFS[e], target_update_freq=5 if tgt else 0)
                if tgt:   # the lagged "network": its own values on the successor rows, at the fractions it is handed
                    algo.model_old.module.hat = nn.Parameter(torch.as_tensor(np.concatenate([np.zeros_like(tg), tg]).astype(ndt)))
                nxt = rows + B
                obs_next = Batch(obs=nxt, mask=mask) if msk else nxt
                tq = algo._target_q(_Rows(obs_next), np.arange(B)).detach().numpy().copy()
                assert tq.dtype == ndt and tq.shape == (B, N)
                tq *= vmask.reshape(-1, 1)                                        # algorithm_base.py:796
                ret = tq * gpow.reshape(B, 1) + mc.reshape(B, 1)                  # :1213-1215
                batch = Batch(obs=rows, act=act, obs_next=obs_next, returns=torch.as_tensor(ret).to(dt), info=Batch())
                if wgt:
                    batch.weight = torch.as_tensor(weight).to(dt)
                algo._iter = 1
                stats = algo._update_with_batch(batch)
                o[dbl] = dict(stats=stats_of(stats), prio=batch.weight.detach().double().numpy(), ret=ret.astype(np.float64),
                              dout=model.hat.grad[:B].double().numpy(), dlog=frac.net.table.grad[:B].double().numpy())
                assert not model.hat.grad[B:].any() and not frac.net.table.grad[B:].any() and model.tau.grad is None
            r64, r32 = o[True], o[False]
            h = fqf_head(out_, out_tau, xf, on, taus_next, tg if tgt else None, mask if msk else None, act, mc, gpow, vmask,
                         weight if wgt else None, ENT_COEFS[e])
            mine = np.array([h["loss"], h["quantile_loss"], h["fraction_loss"], h["entropy_loss"]])
            assert np.allclose(mine, r64["stats"], rtol=1e-11, atol=1e-13), (A, N, c, mine, r64["stats"])
            assert np.allclose(h["prio"], r64["prio"], rtol=1e-11, atol=1e-13)
            assert np.allclose(h["returns"], r64["ret"], rtol=1e-13, atol=1e-13)
            assert np.allclose(h["d_out"], r64["dout"], rtol=1e-10, atol=1e-15)
            assert np.allclose(h["d_logits"], r64["dlog"], rtol=1e-10, atol=1e-15), np.abs(h["d_logits"] - r64["dlog"]).max()
            assert np.count_nonzero(h["d_out"]) == np.count_nonzero(h["d_out"][np.arange(B), :, act])
            u = h["u"]
            assert np.abs(u).min() > DELTA and np.abs(np.abs(u) - 1.0).min() > DELTA and (np.abs(u) > 1).any() and (np.abs(u) < 1).any()
            assert h["cmp_gap"] > DELTA
            for k, v in (("stats", np.stack([r64["stats"], r32["stats"]])), ("prio", r64["prio"]),
                         ("prio_eref", emax(r64["prio"], r32["prio"])), ("astar", h["a_star"].astype(np.int64)),
                         ("dout_eref", emax(r64["dout"], r32["dout"])), ("dlog_eref", emax(r64["dlog"], r32["dlog"])),
                         ("ret_eref", emax(r64["ret"], r32["ret"])), ("qtaken", h["q_taken"])):
                keep[k].append(np.asarray(v))
            digest(res, f"hq_{p}c{c}_dout", r64["dout"].reshape(-1))
            digest(res, f"hq_{p}c{c}_dlog", r64["dlog"].reshape(-1))
            digest(res, f"hq_{p}c{c}_ret", r64["ret"].reshape(-1))
        res.update({f"hq_{p}{k}": np.stack(v) for k, v in keep.items()})   # one row per entry of VARIANTS, in its order
        print("heads", A, N, "stats", res[f"hq_{p}stats"][0, 0])


# ---- up / pr -------------------------------------------------------------------------------------------------------------
PRE, HID, A_UP, C_UP, N_UP, ENT_UP = [6, 32], [32], 5, 8, 8, 0.01


def fq_nets():
    return (FullQuantileFunction(preprocess_net=PreNet(PRE), action_shape=A_UP, hidden_sizes=HID, num_cosines=C_UP),
            FractionProposalNetwork(N_UP, PRE[-1]))


def pair(net, frac, dbl):
    return (as_double(net), copy.deepcopy(frac).double()) if dbl else (copy.deepcopy(net), copy.deepcopy(frac))


def restated(init, frac_init, freq):
    return FqfRestatement(init, frac_init, PRE, [PRE[-1], *HID, A_UP], C_UP, N_UP, feature_act=True, target_update_freq=freq,
                          ent_coef=ENT_UP)


def grads_of(m):
    return np.concatenate([q.grad.detach().double().reshape(-1).numpy() for q in m.parameters()])


def update_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step, freq, steps = d[4:10]

    class Kink(Exception):
        pass

    def attempt(seed):
        rs = np.random.RandomState(seed)
        torch.manual_seed(seed)
        net, frac = fq_nets()
        init, frac_init = flat(net).astype(np.float32), flat(frac).astype(np.float32)
        res.update(up_dims=np.array(PRE + HID + [A_UP, C_UP, N_UP], np.int64), up_init=init, up_frac_init=frac_init,
                   up_ent_coef=np.float64(ENT_UP))
        algos = {dbl: make_algo(*pair(load_flat(net, init), load_flat(frac, frac_init), dbl), A_UP, ENT_UP,
                                n_step_return_horizon=n_step, target_update_freq=freq) for dbl in (True, False)}
        bufs, RB = up_buffers(gd, VectorReplayBuffer)
        R = restated(init, frac_init, freq)
        allidx = bufs[True].sample_indices(0)
        for k in range(steps):
            indices = rs.choice(allidx, B, replace=True).astype(np.int64)
            out = {}
            for dbl, algo in algos.items():
                buf = bufs[dbl]
                batch = algo._preprocess_batch(buf[indices], buf, indices)
                stats = algo._update_with_batch(batch)
                out[dbl] = (stats_of(stats), flat(algo.policy.model), flat(algo.model_old.module),
                            batch.returns.double().numpy().reshape(-1), grads_of(algo.policy.model),
                            flat(algo.policy.fraction_model), grads_of(algo.policy.fraction_model))
            idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
            o, on = bufs[False][indices].obs, bufs[False][idx_n].obs_next
            r = R.update(o, bufs[False][indices].act, on, None, mc, gpow, vmask)
            if r["head_gap"] <= DELTA or r["relu_gap"] <= RELU_DELTA:
                raise Kink
            s64 = out[True][0]
            mine = np.array([r["loss"], r["quantile_loss"], r["fraction_loss"], r["entropy_loss"]])
            assert np.allclose(mine, s64, rtol=REL, atol=1e-14), (k, mine, s64)
            assert np.allclose(R.weights(), out[True][1], rtol=1e-9, atol=1e-12) and np.allclose(R.targets(), out[True][2], rtol=1e-9, atol=1e-12)
            assert np.allclose(R.frac_weights(), out[True][5], rtol=1e-9, atol=1e-12)
            assert np.allclose(r["grads"], out[True][4], rtol=1e-9, atol=1e-14)
            assert np.allclose(r["frac_grads"], out[True][6], rtol=1e-8, atol=1e-16), np.abs(r["frac_grads"] - out[True][6]).max()
            assert np.allclose(r["returns"].reshape(-1), out[True][3], rtol=1e-12, atol=1e-13)
            pk = f"up_s{k}_"
            digest(res, pk + "weights", out[True][1])
            digest(res, pk + "targets", out[True][2])
            digest(res, pk + "returns", out[True][3])
            digest(res, pk + "frac_weights", out[True][5])
            res.update({pk + "indices": indices, pk + "stats": np.stack([out[True][0], out[False][0]]),
                        pk + "grad_eref": emax(out[True][4], out[False][4]), pk + "weights_eref": emax(out[True][1], out[False][1]),
                        pk + "returns_eref": emax(out[True][3], out[False][3]),
                        pk + "frac_grad_eref": emax(out[True][6], out[False][6]),
                        pk + "frac_weights_eref": emax(out[True][5], out[False][5])})
        print("update stats", [res[f"up_s{k}_stats"][0] for k in range(steps)])

    for seed in range(31, 131):   # the first seed whose three updates keep DELTA away from every kink
        try:
            attempt(seed)
            res["up_seed"] = np.int64(seed)
            break
        except Kink:
            continue
    else:
        raise AssertionError("no seed without a kink")


def prio_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step, freq = d[4:9]
    alpha, beta = 0.6, 0.4
    res.update(pr_alpha=np.float64(alpha), pr_beta=np.float64(beta))
    net, frac = fq_nets()
    load_flat(net, res["up_init"]), load_flat(frac, res["up_frac_init"])
    algos = {dbl: make_algo(*pair(net, frac, dbl), A_UP, ENT_UP, n_step_return_horizon=n_step, target_update_freq=freq)
             for dbl in (True, False)}
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
            out[dbl] = (stats_of(stats), w_in, buf.weight._value[bound:bound + n_env * S].copy(),
                        np.array([float(buf._max_prio), float(buf._min_prio)]))
        pk = f"pr_s{k}_"
        res.update({pk + "indices": indices, pk + "stats": np.stack([out[True][0], out[False][0]]),
                    pk + "weight": out[True][1], pk + "weight_eref": emax(out[True][1], out[False][1]), pk + "leaves": out[True][2],
                    pk + "leaves_eref": emax(out[True][2], out[False][2]), pk + "prio": out[True][3],
                    pk + "prio_eref": emax(out[True][3], out[False][3])})
    print("prioritized stats", [res[f"pr_s{k}_stats"][0] for k in range(2)])


# ---- ma / sd / sig -------------------------------------------------------------------------------------------------------
def marl_section(res, gd):
    torch.manual_seed(23)
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    pre, hid, C, NF = [D, 16], [], 4, 4
    env = FakeEnv(N_AG)
    nets = [(FullQuantileFunction(preprocess_net=PreNet(pre), action_shape=A, hidden_sizes=hid, num_cosines=C),
             FractionProposalNetwork(NF, pre[-1])) for _ in range(N_AG)]
    res.update(ma_dims=np.array(pre + [A, C, NF], np.int64), ma_init=np.stack([flat(n).astype(np.float32) for n, _ in nets]),
               ma_frac_init=np.stack([flat(f).astype(np.float32) for _, f in nets]), ma_ent_coef=np.float64(ENT_UP))
    for (n, f), wi, fi in zip(nets, res["ma_init"], res["ma_frac_init"]):
        load_flat(n, wi), load_flat(f, fi)
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
        algos = [make_algo(*pair(n, f, dbl), A, ENT_UP, n_step_return_horizon=n_step, target_update_freq=3) for n, f in nets]
        ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=env)
        batch, indices = buf.sample(0)
        stats = ma._update_with_batch(ma._preprocess_batch(batch, buf, indices))
        out[dbl] = [stats_of(stats._agent_id_to_stats[a]) for a in env.agents]
    res["ma_stats"] = np.array([out[True], out[False]])
    print("marl stats", out[True])


def statedict_and_signatures(res):
    torch.manual_seed(0)
    net = FullQuantileFunction(preprocess_net=Net(state_shape=(PRE[0],), hidden_sizes=PRE[1:]), action_shape=A_UP,
                               hidden_sizes=HID, num_cosines=C_UP)
    algo = make_algo(net, FractionProposalNetwork(N_UP, PRE[-1]), A_UP, target_update_freq=2)
    sd = {k: v for k, v in algo.state_dict().items() if isinstance(v, torch.Tensor) and v.dim() > 0}
    res["sd_keys"] = np.array(list(sd.keys()))
    res["sd_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    for cls in (FQFPolicy, FQF):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])
    res["sig_FQFTrainingStats"] = np.array([f.name for f in dataclasses.fields(FQFTrainingStats)])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    gd = dict(np.load(os.path.join(HERE, "dqn.npz")))
    res = {"delta": np.float64(DELTA), "relu_delta": np.float64(RELU_DELTA), "gamma": np.float64(GAMMA)}
    propose_section(res)
    head_sections(res)
    update_section(res, gd)
    prio_section(res, gd)
    marl_section(res, gd)
    statedict_and_signatures(res)
    path = os.path.join(HERE, "fqf.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
