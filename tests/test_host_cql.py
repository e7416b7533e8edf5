"""CPU tests of the offline continuous learners CQL / Cal-QL and TD3+BC: the float64 restatement (tests/cql_restatement.py)
against the reference's own float64 run in tests/golden/cql.npz at 1e-10, a central difference of the closed-form CQL head,
constructor signatures against the reference's, the host-side refusals of the new wrappers and of `tsm_cql_check`, and the
ownership of the uniform draw's Philox words.  Nothing is launched."""
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "cql.npz")

import cql_restatement as R  # noqa: E402
from dqn_restatement import RestatedBuffer, nstep_walk  # noqa: E402
from dsac_restatement import alpha_state  # noqa: E402
from sampling_restatement import cac_normal  # noqa: E402

from tianshou_marl_amd import _abi, _build, ops  # noqa: E402

N_CQL, N_TD3BC = 6, 2


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def cql_cases(g):
    out = []
    for i, c in enumerate(g["cql_cases"]):
        lag, cal, temp, no_c2, alpha, lo, hi, amax = str(c).split("|")
        out.append(dict(i=i, lagrange=bool(int(lag)), calibrated=bool(int(cal)), temperature=float(temp), no_c2=bool(int(no_c2)),
                        alpha=alpha, min_action=float(lo), max_action=float(hi), alpha_max=float(amax)))
    return out


def td3bc_cases(g):
    return [dict(i=i, n_step=int(str(c).split("|")[0]), prio=bool(int(str(c).split("|")[1]))) for i, c in enumerate(g["td3bc_cases"])]


def buffer_rows(g, seed, steps):
    """The generator's hand-filled buffer, drawn again from its seed: per time step the rows of every env."""
    D, Ad = int(g["dims"][0]), int(g["dims"][1])
    n_env, S = int(g["dims"][5]), int(g["dims"][6])
    rs = np.random.RandomState(seed + 1000)
    rows, RB = [], RestatedBuffer(n_env, S, 1)
    for _ in range(steps):
        term, trunc = rs.rand(n_env) < 0.12, rs.rand(n_env) < 0.08
        rew = rs.standard_normal(n_env).astype(np.float32)
        obs = rs.standard_normal((n_env, D)).astype(np.float32)
        act = rs.uniform(-1, 1, (n_env, Ad)).astype(np.float32)
        nxt = rs.standard_normal((n_env, D)).astype(np.float32)
        rows.append(dict(obs=obs, act=act, rew=rew, terminated=term, truncated=trunc, obs_next=nxt))
        for e in range(n_env):
            RB.add(e, rew[e], bool(term[e]), bool(trunc[e]))
    return rows, RB


def flat_rows(g, rows):
    """obs, act, obs_next, rew, done by flat index env * S + slot."""
    n_env, S = int(g["dims"][5]), int(g["dims"][6])
    keys = ("obs", "act", "obs_next", "rew", "terminated", "truncated")
    out = {k: np.zeros((n_env * S,) + rows[0][k].shape[1:], rows[0][k].dtype) for k in keys}
    for t, r in enumerate(rows):
        for k in keys:
            out[k][np.arange(n_env) * S + t] = r[k]
    out["done"] = out["terminated"] | out["truncated"]
    return out


def cql_restatement_of(g, c):
    D, Ad, h1, h2 = (int(x) for x in g["dims"][:4])
    pk = f"q{c['i']}_"
    init = {n: g[pk + "init_" + n] for n in ("actor", "critic", "critic2") if pk + "init_" + n in g}
    fixed, la, te = g["sac"]
    lr_a, w, thr, mgn = (float(x) for x in g["cql"])
    return R.CqlRestatement(init, [D, h1, h2, 2 * Ad], [D + Ad, h1, h2, 1], float(g["tau"]), float(g["gamma"]), lr=float(g["lr"]),
                            max_action=float(g["max_action"]), alpha=alpha_state(float(la)) if c["alpha"] == "auto" else float(fixed),
                            target_entropy=float(te), alpha_lr=float(g["lr"]), cql_alpha_lr=lr_a, cql_weight=w,
                            temperature=c["temperature"], with_lagrange=c["lagrange"], lagrange_threshold=thr,
                            num_repeat_actions=int(g["dims"][8]), alpha_min=0.0, alpha_max=c["alpha_max"], max_grad_norm=mgn,
                            calibrated=c["calibrated"])


def td3bc_restatement_of(g, c):
    D, Ad, h1, h2 = (int(x) for x in g["dims"][:4])
    pk = f"t{c['i']}_"
    init = {n: g[pk + "init_" + n] for n in ("actor", "critic", "critic2")}
    pn, nc, freq, bc = g["td3"]
    return R.Td3bcRestatement(init, [D, h1, h2, Ad], [D + Ad, h1, h2, 1], float(g["tau"]), lr=float(g["lr"]),
                              max_action=float(g["max_action"]), policy_noise=float(pn), noise_clip=float(nc),
                              update_actor_freq=int(freq), bc_alpha=float(bc))


def cql_stats(r):
    nn = lambda v: np.nan if v is None else v  # noqa: E731
    return np.array([r["actor_loss"], r["critic1_loss"], r["critic2_loss"], r["alpha"], nn(r["alpha_loss"]), nn(r["cql_alpha"]),
                     nn(r["cql_alpha_loss"])])


CQL_NETS = ["actor", "critic", "critic_old", "critic2", "critic2_old"]
TD3_NETS = ["actor", "critic", "critic_old", "critic2", "critic2_old", "actor_old"]


@pytest.mark.parametrize("ci", range(N_CQL))
def test_cql_restatement_follows_the_reference_float64_run(g, ci):
    c = cql_cases(g)[ci]
    assert len(cql_cases(g)) == N_CQL
    pk = f"q{ci}_"
    rows, _ = buffer_rows(g, int(g[pk + "seed"]), int(g["dims"][9]))
    fr = flat_rows(g, rows)
    Rst = cql_restatement_of(g, c)
    for k in range(2):
        sk = f"{pk}s{k}_"
        idx = g[sk + "indices"]
        calib = g[pk + "calib"][idx] if c["calibrated"] else None
        r = Rst.update(fr["obs"][idx], fr["act"][idx], fr["rew"][idx], fr["done"][idx], fr["obs_next"][idx], calib,
                       g[sk + "z_actor"], g[sk + "z_target"], g[sk + "z_cur"], g[sk + "z_next"], g[sk + "u"])
        assert np.allclose(cql_stats(r), g[sk + "stats"], rtol=1e-10, atol=1e-13, equal_nan=True)
        assert np.isclose(r["cql_log_alpha"], g[sk + "cql_log_alpha"][0], rtol=1e-10, atol=1e-14)
        assert np.allclose(r["target"], g[sk + "target"], rtol=1e-12, atol=0)
        for n, gv in r["grads"].items():
            assert np.allclose(gv, g[f"{sk}grad_{n}"], rtol=1e-10, atol=1e-15), (k, n)
    for n in CQL_NETS:
        assert np.allclose(Rst.weights(n), g[f"{pk}s1_w_{n}"], rtol=1e-10, atol=1e-13), n
    assert Rst.kink > float(g["delta"]) and Rst.calib_gap > float(g["delta"])
    if c["alpha_max"] < 1.0:   # the clamp is active from the start: no gradient, the multiplier stays where it began
        assert r["d_log_alpha"] == 0.0 and r["cql_log_alpha"] == 0.0 and r["cql_alpha"] == c["alpha_max"]


def test_calibration_returns_restatement_follows_the_reference(g):
    for c in cql_cases(g):
        if not c["calibrated"]:
            continue
        pk = f"q{c['i']}_"
        rows, _ = buffer_rows(g, int(g[pk + "seed"]), int(g["dims"][9]))
        fr = flat_rows(g, rows)
        n_env, S, T = int(g["dims"][5]), int(g["dims"][6]), int(g["dims"][9])
        orders = [e * S + np.arange(T) for e in range(n_env)]
        mine = R.calibration_returns(fr["rew"], fr["done"], orders, float(g["gamma"]))
        assert np.allclose(mine, g[pk + "calib"], rtol=1e-12, atol=0)
        done = fr["done"].reshape(n_env, S)
        assert done[:, :-1].any(1).all() and not done[:, -1].any()   # a finished episode and an unfinished tail per sub-buffer


@pytest.mark.parametrize("ci", range(N_TD3BC))
def test_td3bc_restatement_follows_the_reference_float64_run(g, ci):
    c = td3bc_cases(g)[ci]
    assert len(td3bc_cases(g)) == N_TD3BC
    pk = f"t{ci}_"
    rows, RB = buffer_rows(g, int(g[pk + "seed"]), int(g["dims"][7]))
    fr = flat_rows(g, rows)
    Rst = td3bc_restatement_of(g, c)
    for k in range(2):
        sk = f"{pk}s{k}_"
        idx = g[sk + "indices"]
        idx_n, mc, gpow, vmask = nstep_walk(RB, idx, c["n_step"], float(g["gamma"]), 0)
        r = Rst.update(fr["obs"][idx], fr["act"][idx], fr["obs_next"][idx_n], mc, gpow, vmask, weight=g.get(sk + "weight_in"),
                       z_target=g[sk + "z_target"])
        mine = np.array([r["actor_loss"], r["critic1_loss"], r["critic2_loss"]])
        assert np.allclose(mine, g[sk + "stats"], rtol=1e-10, atol=0)
        assert np.allclose(r["returns"], g[sk + "returns"], rtol=1e-10, atol=1e-13)
        assert np.allclose(r["prio"], g[sk + "prio"], rtol=1e-10, atol=1e-13)
        assert ("actor" in r["grads"]) == bool(g[sk + "actor_stepped"]) == (k == 0)
        for n, gv in r["grads"].items():
            assert np.allclose(gv, g[f"{sk}grad_{n}"], rtol=1e-10, atol=1e-15), (k, n)
    for n in TD3_NETS:
        assert np.allclose(Rst.weights(n), g[f"{pk}s1_w_{n}"], rtol=1e-10, atol=1e-13), n
    assert Rst.kink > float(g["delta"])


@pytest.mark.parametrize("calibrated,lagrange", [(False, False), (True, True)])
def test_closed_form_cql_head_gradient_matches_a_central_difference(calibrated, lagrange):
    rs = np.random.RandomState(4)
    B, Rn, Ad, T, w, thr = 3, 2, 2, 0.7, 1.3, 0.4
    n = B + 3 * B * Rn
    q1, q2, tgt = rs.standard_normal(n), rs.standard_normal(n), rs.standard_normal(B)
    lpc, lpn = rs.standard_normal(B * Rn), rs.standard_normal(B * Rn)
    calib = rs.standard_normal(B) if calibrated else None
    la = 0.3 if lagrange else None

    def loss(qa, qb):
        h = R.head(qa, qb, tgt, lpc, lpn, Rn, Ad, calib, T, w, 0.0, 1e6, la)
        f = R.finalize(h, thr, 0.0, 1e6, la)
        return f["critic1_loss"], f["critic2_loss"]

    h = R.head(q1, q2, tgt, lpc, lpn, Rn, Ad, calib, T, w, 0.0, 1e6, la)
    assert not calibrated or ((h["dq1"][B:] == 0).any() and (h["dq1"][B:] != 0).any())   # both sides of the calibration max
    eps = 1e-6
    for j in range(n):
        for k, q in enumerate((q1, q2)):
            keep = q[j]
            q[j] = keep + eps
            up = loss(q1, q2)[k]
            q[j] = keep - eps
            dn = loss(q1, q2)[k]
            q[j] = keep
            assert abs((up - dn) / (2 * eps) - h[f"dq{k + 1}"][j]) < 1e-7, (j, k)
    # the multiplier's gradient: d cql_alpha_loss / d log_alpha by a central difference, and zero where the clamp is active
    if lagrange:
        f = lambda x: R.finalize(R.head(q1, q2, tgt, lpc, lpn, Rn, Ad, calib, T, w, 0.0, 1e6, x), thr, 0.0, 1e6, x)  # noqa: E731
        assert abs((f(la + eps)["cql_alpha_loss"] - f(la - eps)["cql_alpha_loss"]) / (2 * eps) - f(la)["d_log_alpha"]) < 1e-7
        assert R.finalize(R.head(q1, q2, tgt, lpc, lpn, Rn, Ad, calib, T, w, 0.0, 1.2, la), thr, 0.0, 1.2, la)["d_log_alpha"] == 0.0


def test_td3bc_actor_head_gradient_matches_a_central_difference():
    rs = np.random.RandomState(5)
    B, Ad, M, alpha = 4, 3, 1.5, 2.5
    raw, a_data, c, b = rs.standard_normal((B, Ad)), rs.uniform(-1, 1, (B, Ad)), rs.standard_normal((B, Ad)), rs.standard_normal(B)
    q_of = lambda r: (c * (M * np.tanh(r))).sum(1) + b   # noqa: E731  (a linear critic)
    lmbda = alpha / np.abs(q_of(raw)).mean()              # detached

    def loss(r):
        return float(-lmbda * q_of(r).mean() + ((M * np.tanh(r) - a_data) ** 2).mean())

    a, omt2 = R.det_action(raw, M)
    h = R.td3bc_actor_head(c, omt2, q_of(raw), a, a_data, alpha, M)
    assert np.isclose(h["loss"], loss(raw), rtol=1e-13) and np.isclose(h["lmbda"], lmbda, rtol=1e-13)
    eps = 1e-6
    for i in range(B):
        for k in range(Ad):
            up, dn = raw.copy(), raw.copy()
            up[i, k] += eps
            dn[i, k] -= eps
            assert abs((loss(up) - loss(dn)) / (2 * eps) - h["d_raw"][i, k]) < 1e-7


def test_signatures_and_defaults_are_the_reference_ones(g):
    from tianshou_marl_amd.algorithm import CQL, TD3BC

    for cls in (CQL, TD3BC):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        mine = [f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}" for q in ps]
        ref = [str(x) for x in g[f"sig_{cls.__name__}"]]
        assert mine[:len(ref)] == ref, (cls.__name__, mine, ref)
        assert all(q.default is not inspect.Parameter.empty for q in ps[len(ref):])
        assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for q in ps)


def test_uniform_site_owns_words_disjoint_from_the_normal_site():
    """At the counters the learner passes -- the policy's `_sample_ctr` for the normals, its own `_uniform_ctr` for the uniforms,
    each advanced by elements, under the same seed -- two successive draws of each site and the two sites own disjoint words."""
    B, Rn, Ad, seed = 12, 3, 3, 0x1234ABCD5678
    useds, ctr_n, ctr_u = [], 2**32 - 5, 0
    for _ in range(2):
        for n in (B * Ad, B * Ad, 2 * B * Rn * Ad):   # the actor step, the target, the stacked conservative rows
            useds.append(cac_normal(n, seed, ctr_n)[1])
            ctr_n += n
        v, u = R.uniform(B * Rn * Ad, 1.0, 2.0, seed, ctr_u)
        assert len(u) == B * Rn * Ad and v.dtype == np.float32 and v.min() >= 1.0 and v.max() < 2.0
        useds.append(u)
        ctr_u += B * Rn * Ad
    seen = set()
    for u in useds:
        assert not (seen & u)
        seen |= u
    assert (R.uniform(7, 1.0, 1.0, seed, 3)[0] == 1.0).all()   # quirk Q70: uniform_(1, 1)


def test_wrappers_refuse_cpu_tensors():
    z, q = torch.zeros(4, 3), torch.zeros(4)
    calls = [lambda: ops.cql_uniform(8, 0.0, 1.0, 0, device="cpu"), lambda: ops.cql_rows(torch.zeros(4, 5), torch.zeros(4, 5), z, z, 1),
             lambda: ops.cql_head(torch.zeros(16), torch.zeros(16), q, q, q, 1, 3),
             lambda: ops.cql_finalize(torch.zeros(6, dtype=torch.float64), 4, 1, torch.zeros(6)),
             lambda: ops.td3bc_actor_head(z, z, q, z, z, 2.5)]
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


def test_cql_check_bounds_through_the_abi():
    _build.build()
    _abi.load()
    assert _abi.CQL_ROWS_PER_BLOCK == 256
    _abi.call("tsm_cql_check", 1, 1)
    _abi.call("tsm_cql_check", _abi.CAC_MAX_ACT_DIM, 10)
    with pytest.raises(ValueError, match=r"act_dim = 65 outside \[1, 64\]"):
        _abi.call("tsm_cql_check", _abi.CAC_MAX_ACT_DIM + 1, 1)
    with pytest.raises(ValueError, match=r"act_dim = 0 outside"):
        ops.cql_check(0)
    with pytest.raises(ValueError, match="at least 1 but got: 0"):
        ops.cql_check(3, 0)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_cql_head", None, None, None, None, None, None, 4, 2, 0.0, 1.0, 1.0, 0.0, 1.0, None, None, None, None, None)
    with pytest.raises(ValueError, match="interval .* is empty"):
        _abi.call("tsm_cql_uniform", 1, 4, 2.0, 1.0, 0, 0, None, None)
    with pytest.raises(ValueError, match="temperature = 0 must be positive"):
        _abi.call("tsm_cql_head", 1, 1, 1, 1, 1, None, 4, 2, 0.0, 0.0, 1.0, 0.0, 1.0, None, 1, 1, 1, None)
