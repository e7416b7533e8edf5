"""CPU tests of the shape sweeps that tests/test_gpu_ctde_shapes.py runs on the device (inputs and yardsticks:
tests/ctde_cases.py).  For every case: the reference's own float32 error `e_ref` is finite and the float32 restatement alone
stays inside the bar the device test applies to the kernel (test_gpu_distq._bar for mix/TD and the CTDE head, equality for
tsm_ctde_finalize and tsm_global_state); the head's precondition holds; both ELU branches, the exact zeros, the terminated
kinds, the planted maxima and the exact sums are present where promised; the mix/TD yardstick, fed QmixRestatement's own
hypernetwork outputs, reproduces QmixRestatement.learn; and the C-ABI's argument checks accept every case's sizes (the calls
pass null pointers: they return the size error, if any, before the null-pointer error and before any launch)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ctde_cases as cc  # noqa: E402
from qmix_restatement import QmixRestatement  # noqa: E402
from test_host_offpolicy_shapes import _inside_bar  # noqa: E402


# ---- QMIX mix / TD ----------------------------------------------------------------------------------------------------------
def test_mix_cases_are_the_sweep_asked_for():
    shapes = {(c["E"], c["N"], c["A"], c["B"]) for c in cc.MIX_CASES if not c["offset"]}
    assert {(32, 3, 5, b) for b in (1, 7, 8, 9, 31, 32, 33, 4099)} | {(64, 3, 5, b) for b in (1, 3, 4, 5, 15, 16, 17, 4099)} <= shapes
    for E in (32, 64):
        assert {(E, 1, 1, 17), (E, 8, 64, 33), (E, 8, 3, 33), (E, 1, 64, 4099)} <= shapes
        assert {(c["N"], c["A"], c["B"]) for c in cc.MIX_CASES if c["offset"] and c["E"] == E} == {(3, 5, 33), (8, 3, 33)}
        R = cc.rows_per_block(E)
        assert R == {32: 32, 64: 16}[E] and -(-4099 // R) > 64
        # the block's [nr][A] segment moves as float4 plus a scalar tail: a last workgroup with both, and one with a tail only
        last = [(c["B"] - (c["B"] - 1) // R * R) * c["A"] for c in cc.MIX_CASES if c["E"] == E]
        assert any(n > 4 and n % 4 for n in last) and any(n < 4 for n in last) and any(n % 4 == 0 for n in last)
    assert {c["term"] for c in cc.MIX_CASES} == {"mixed", "all", "none"}
    assert len(cc.MIX_CASES) == 16 + 8 + 4 and len({cc.case_id(c) for c in cc.MIX_CASES}) == len(cc.MIX_CASES)


@pytest.mark.parametrize("c", cc.MIX_CASES, ids=cc.case_id)
def test_mix_case(c):
    d, ref = cc.mix_inputs(c), cc.mix_td_reference(c)
    E, N, A, B = c["E"], c["N"], c["A"], c["B"]
    assert d["q"].shape == d["q_next"].shape == (N, B, A) and d["w1raw"].shape == d["tw1raw"].shape == (B, N * E)
    assert d["act"].min() >= 0 and d["act"].max() < A
    term = d["term"].astype(bool)
    assert {"all": term.all(), "none": not term.any(), "mixed": term.any() and not term.all()}[c["term"]]
    for k in ("w1raw", "w2raw", "tw1raw", "tw2raw"):
        assert (d[k] > 0).any() and (d[k] < 0).any(), k
        zeros = int((d[k] == 0.0).sum())
        assert zeros == (max(1, int(round(cc.ZERO_SHARE * d[k].size))) if B >= 15 else 0), (k, zeros)
    worst = 0.0
    for mono in cc.MIX_MONOTONIC:
        r = ref[mono]
        assert (r["pre"] > 0).any() and (r["pre"] <= 0).any(), mono        # both ELU branches
        for k in cc.MIX_KEYS:
            worst = max(worst, _inside_bar(f"mix {mono} {k}", r["e_ref"][k], r[k]))
        rows = np.arange(B)
        off = r["dq"].copy()
        for i in range(N):
            off[i, rows, d["act"][i]] = 0.0
        assert not off.any()
        for k in ("dw1", "dw2"):
            z = r["zero"][k]
            if mono:
                assert not r[k][z].any()                                    # the gradient of torch.abs at 0
            elif z.any():
                assert np.abs(r[k][z]).max() > 0                            # the unsigned product
                _inside_bar(f"mix {mono} {k}@0", r["e_ref"][k + "@0"], r[k][z])
    print(f"mix {cc.case_id(c)}: worst e_ref / bar {worst:.3g}")


def test_mix_yardstick_reproduces_the_restatement():
    """The small QMIX fixture's round-0 rows at its initial weights: QmixRestatement's own Q rows and hypernetwork outputs, fed
    into ctde_cases.mix_td, give the loss and mean q_tot of QmixRestatement.learn (which tests/test_host_qmix.py pins to the
    reference) to 1e-12."""
    g = np.load(os.path.join(HERE, "golden", "qmix.npz"))
    N, D, A, H, S, E, Hh, B, _, mono = (int(x) for x in g["small_dims"])
    R = QmixRestatement(g["small_init"], (N, D, A, H, S, E, Hh), monotonic=bool(mono), gamma=float(g["gamma"]))
    rows = {f: g[f"small_r0_{f}"] for f in ("obs", "obs_next", "act", "rew", "term")}
    gs, gsn = (rows[f].transpose(1, 0, 2).reshape(B, S) for f in ("obs", "obs_next"))
    with torch.no_grad():
        d = dict(q=np.stack([R._actor(R.params, i, R._t(rows["obs"][i])).numpy() for i in range(N)]),
                 q_next=np.stack([R._actor(R.target, i, R._t(rows["obs_next"][i])).numpy() for i in range(N)]),
                 act=rows["act"], rew=rows["rew"], term=rows["term"])
        for side, ps, s in (("", R.params, gs), ("t", R.target, gsn)):
            for name, x in zip(("w1raw", "b1", "w2raw", "b2"), R._hyper(ps, R._t(s))):
                d[side + name] = x.reshape(B, -1).numpy()
    got = cc.mix_td(d, bool(mono), float(g["gamma"]), torch.float64)
    want = R.learn(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"], gs, gsn)
    assert want["loss"] == pytest.approx(float(g["small_r0_loss"][0]), rel=1e-12, abs=0)
    assert got["loss"] == pytest.approx(want["loss"], rel=1e-12, abs=0)
    assert got["mean_q"] == pytest.approx(want["q_values"], rel=1e-12, abs=1e-15)
    assert got["dq"].shape == (N, B, A) and got["dw1"].shape == (B, N * E)


# ---- epsilon-greedy ---------------------------------------------------------------------------------------------------------
def test_egreedy_case_has_duplicated_maxima():
    d = cc.egreedy_inputs()
    N, B, A = d["q"].shape
    assert (N, A, B) == (8, 64, 17) and d["act"].shape == (B, N) and d["planted"].sum() >= N
    for i in range(N):
        for b in range(B):
            n_max = int((d["q"][i, b] == d["q"][i, b].max()).sum())
            assert n_max == (3 if d["planted"][i, b] else 1)
            assert d["act"][b, i] == int(np.flatnonzero(d["q"][i, b] == d["q"][i, b].max())[0])


# ---- CTDE head --------------------------------------------------------------------------------------------------------------
def test_head_cases_are_the_sweep_asked_for():
    shapes = {(c["n_out"], c["A"], c["B"]) for c in cc.HEAD_CASES}
    assert shapes == {(1, 5, b) for b in (1, 63, 64, 65, 255, 256, 257, 4099, 65793)} | {(1, 1, 257), (3, 5, 257), (8, 64, 257)}
    assert -(-65793 // 256) == 258
    for c in cc.HEAD_CASES:   # every seed is the first of the sequence for which the precondition holds
        for k in range(200):
            if cc.preconditions_hold(dict(c, seed=cc._seed(k))):
                break
        assert c["seed"] == cc._seed(k), (cc.case_id(c), k)


@pytest.mark.parametrize("c", cc.HEAD_CASES, ids=cc.case_id)
def test_head_case(c):
    d, r = cc.head_inputs(c), cc.ctde_head_reference(c)
    assert abs(r["mean_adv"]) >= cc.MIN_ABS_MEAN_ADV, r["mean_adv"]
    assert r["dq"].shape == (c["B"], c["n_out"]) and r["dlogits"].shape == (c["B"], c["A"])
    assert d["act"].min() >= 0 and d["act"].max() < c["A"]     # the head indexes logits with act unchecked
    worst = max(_inside_bar(f"head {k}", r["e_ref"][k], r[k]) for k in cc.HEAD_KEYS)
    if c["A"] == 1:
        assert not r["dlogits"].any()
    print(f"head {cc.case_id(c)}: mean adv {r['mean_adv']:.3g}, worst e_ref / bar {worst:.3g}")


def test_head_product_of_means_is_the_broadcast():
    """Beyond OUTER_MAX entries the (B, B) product is restated as the product of the means: equal to 1e-12 at B = 4099."""
    c = next(c for c in cc.HEAD_CASES if c["B"] == 4099)
    d = cc.head_inputs(c)
    assert 4099 ** 2 <= cc.OUTER_MAX < 65793 ** 2
    a, b = cc.ctde_head(d, torch.float64, outer=True), cc.ctde_head(d, torch.float64, outer=False)
    assert a["actor_loss"] == pytest.approx(b["actor_loss"], rel=1e-12, abs=0)
    assert np.abs(a["dlogits"] - b["dlogits"]).max() <= 1e-12 * np.abs(a["dlogits"]).max()


# ---- tsm_ctde_finalize --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.FINALIZE_CASES, ids=cc.case_id)
def test_finalize_case_is_exact(c):
    from fractions import Fraction

    d, r = cc.finalize_inputs(c), cc.finalize_reference(c)
    B = c["B"]
    assert B & (B - 1) == 0 and d["pc"].shape == (c["nb_c"], 4) and d["pa"].shape == (c["nb_a"], 4)
    assert (d["pc"][:, 2:] == cc.FINALIZE_POISON).all() and (d["pa"][:, 1:] == cc.FINALIZE_POISON).all()
    assert (d["pc"][:, 0] < 0).any() or c["nb_c"] == 1
    read = (d["pc"][:, 0], d["pc"][:, 1], d["pa"][:, 0])
    for x in read:
        assert np.array_equal(x * 8, np.round(x * 8)) and np.abs(x).max() <= 8.0
    s_adv, s_sq, s_logp = (sum(Fraction(float(v)) for v in x) for x in read)     # in rational arithmetic
    want = [-(s_logp / B) * (s_adv / B), s_sq / B]
    assert all(Fraction(float(np.float64(w))) == w for w in want)               # representable: float64 rounds nothing
    assert np.array_equal(r["scalars"], np.array([float(w) for w in want]).astype(np.float32))
    assert r["mean_adv"] == np.float32(float(s_adv / B)) and np.isfinite(r["scalars"]).all()


def test_finalize_cases_are_the_sweep_asked_for():
    assert [(c["nb_c"], c["nb_a"]) for c in cc.FINALIZE_CASES] == [(1, 1), (63, 65), (64, 64), (65, 1), (257, 130)]


# ---- tsm_global_state ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.GLOBAL_CASES, ids=cc.case_id)
def test_global_case(c):
    obs, r = cc.global_inputs(c), cc.global_reference(c)
    N, D, B = c["N"], c["D"], c["B"]
    assert r["concatenate"].shape == (B, N * D) and r["mean"].shape == (B, D) and r["mean"].dtype == np.float32
    for a in range(N):
        assert np.array_equal(r["concatenate"][:, a * D:(a + 1) * D], obs[a])
    assert np.isfinite(r["mean"]).all()
    assert np.abs(r["mean"] - obs.astype(np.float64).mean(0)).max() <= 1e-5 * max(np.abs(obs).max(), 1.0)


def test_global_cases_are_the_sweep_asked_for():
    shapes = {(c["N"], c["D"], c["B"]) for c in cc.GLOBAL_CASES}
    assert {(1, 1, 1), (3, 18, 37), (64, 1, 4), (64, 7, 33), (5, 51, 1), (5, 51, 2)} <= shapes
    assert {255, 256, 257} <= {n * d * b for n, d, b in shapes if (n, d) == (1, 1)}


# ---- the C-ABI accepts every case's sizes -----------------------------------------------------------------------------------
def test_entry_points_accept_every_case_without_a_device():
    from tianshou_marl_amd import _abi, ops

    def passes_the_size_checks(fn):
        with pytest.raises(ValueError, match="null pointer"):   # the last check of every entry point, after the sizes
            fn()

    ag = _abi.tsm_qmix_agents()
    for c in cc.MIX_CASES:
        E, N, A, B = c["E"], c["N"], c["A"], c["B"]
        ops.qmix_check(N, E, A)
        passes_the_size_checks(lambda: _abi.call("tsm_qmix_mix_td", _abi.C.byref(ag), N, A, B, E, *[None] * 9, cc.GAMMA, 1,
                                                 *[None] * 7))
        assert _abi.call("tsm_qmix_partial_elems", B, E) == 2 * -(-B // cc.rows_per_block(E))
    c = cc.EGREEDY_CASE
    ops.qmix_check(c["N"], 32, c["A"])
    passes_the_size_checks(lambda: _abi.call("tsm_qmix_egreedy", None, c["N"], c["B"], c["A"], None, 0, 0, None, None, c["N"], None))
    for c in cc.HEAD_CASES:
        passes_the_size_checks(lambda: _abi.call("tsm_ctde_td_head", None, None, c["n_out"], None, None, cc.GAMMA, None, None, c["A"],
                                                 c["B"], None, None, None, None, None))
        assert _abi.call("tsm_ctde_head_partial_elems", c["B"]) == 3 * -(-c["B"] // 256)
    for c in cc.FINALIZE_CASES:
        passes_the_size_checks(lambda: _abi.call("tsm_ctde_finalize", None, c["nb_c"], None, c["nb_a"], c["B"], None, None, None))
    for c in cc.GLOBAL_CASES:
        for mode in (0, 1):
            passes_the_size_checks(lambda: _abi.call("tsm_global_state", None, c["N"], c["B"], c["D"], mode, None, None))
    with pytest.raises(ValueError, match="bad sizes"):
        _abi.call("tsm_global_state", None, 65, 4, 1, 0, None, None)
    assert _abi.call("tsm_global_state", None, 64, 0, 1, 0, None, None) is None   # B = 0: nothing to do, nothing touched
