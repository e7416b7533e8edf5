"""CPU tests of the env-kernel edge cases that tests/test_gpu_env_shapes.py runs on the device (cases and yardsticks:
tests/env_cases.py).  Everything the cases promise is asserted here from the float64 oracles alone, so that no GPU assertion is
vacuous: the cases are the sweep asked for and hold float32 numbers; every branch of the step kernels is reached (pairs of every
type on each side of the force cutoff and of the contact threshold, the z > 0 side of the soft-plus, collision counts of 0, 1, 2
and 3, each piece of the boundary penalty and its cap, the speed clamp taken and not taken per team); no crafted contact decision
is close (the oracle's post-step distance is off its threshold by more than 1e-5, on the intended side -- float32 evaluation of
sqrt(dx^2 + dy^2) at these magnitudes errs by under 1e-7, so a kernel that decides the other way is wrong, not unlucky); and in
the random worlds at most 1 % of the decisions are within 1e-5 of a threshold (the seeds in env_cases are the ones for which this
holds).  The float32 restatements the device is held to bit for bit (observation layout, no-force step) are checked against the
oracle here as well."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import env_cases as ec  # noqa: E402


def test_cases_are_the_sweep_asked_for():
    assert [t[2:] for t in ec.PAIR_TYPES] == [("agent-agent", 0, 1, 0.30), ("adv-adv", 0, 1, 0.15), ("adv-good", 0, 2, 0.125),
                                              ("good-good", 2, 3, 0.10), ("adv-obst", 0, 4, 0.275), ("good-obst", 2, 4, 0.25)]
    assert [ec._sep(s, 1.0) for s in ec.PAIR_SEPS] == [0.2, 1 - 5e-3, 1 - 0.5e-3, 1 + 0.5e-3, 1 + 5e-3, 1 + 50e-3, 1 + 104e-3,
                                                      1 + 106e-3, 2.0]
    assert len(ec.DIRS) >= 3 and sum(0.0 in d for d in ec.DIRS) >= 2
    assert ec.CONTACT_D == (1e-4, 0.0099, 0.0101, 0.05)
    assert ec.BOUND_X == (0.85, 0.8999, 0.9001, 0.95, 0.9999, 1.0001, 1.5, 2.15, 2.16, 3.0)
    assert ec.RATIOS == (0.0, 0.3, 0.5, 1.0) and [c["cfg"]["local_ratio"] for c in ec.RATIO_CASES] == list(ec.RATIOS)
    got = {(c["kind"], c["sizes"], c["n_env"]) for c in ec.CROWDED_CASES}
    want = {("spread", (n,), e) for n in (1, 2, 3, 5, 8) for e in (1, 15, 16, 17, 35)} | {
        ("tag", s, e) for s in ((1, 1, 0), (1, 1, 4), (7, 1, 0), (1, 7, 4), (4, 4, 4), (3, 1, 2), (2, 3, 1)) for e in (1, 15, 16, 17, 35)}
    assert got == want and len(ec.CROWDED_CASES) == len(want)
    assert {c["auto_reset"] for c in ec.RESET_CASES} == {True, False} and all(c["n_env"] == 35 for c in ec.RESET_CASES)
    assert {c["kind"] for c in ec.RESET_CASES} == {"spread", "tag"}
    names = [c["name"] for c in ec.ALL_CASES]
    assert len(set(names)) == len(names)
    assert len(ec.ROLLOUT_SPREAD) == 3 and len(ec.ROLLOUT_TAG) == 3
    for c in ec.ALL_CASES:
        assert c["apos"].dtype == c["avel"].dtype == c["lpos"].dtype == np.float32 and c["act"].dtype == np.int32
        assert c["act"].min() >= 0 and c["act"].max() <= 4 and c["steps"].dtype == np.int32 and c["episode"].dtype == np.int64
        assert ec.n_agents(c) <= 8 and (c["kind"] == "spread" or c["sizes"][2] <= 4)
        assert max(c["n_env"] for c in ec.ALL_CASES) <= 108


def test_crafted_scenarios_are_isolated():
    """Outside the placed pairs every collidable pair of a crafted case is beyond the force cutoff (idle entities: a lattice of
    spacing >= 1), idle agents are at rest under noop, and no two entities coincide anywhere."""
    for c in ec.CRAFTED_CASES:
        names, gap = ec.pre_pairs(c)
        NA = ec.n_agents(c)
        pairs = [(a, b) for a in range(NA) for b in range(a + 1, NA + (0 if c["kind"] == "spread" else c["sizes"][2]))]
        m = c["meta"]
        placed = {m["pair"]} if c["family"] == "pairs" else \
            {tuple(sorted((m["centre"], k))) for k in m["movers"]} if c["family"] == "contacts" else set()
        for k, ab in enumerate(pairs):
            if ab not in placed:
                assert (gap[:, k] > 0.2).all(), (c["name"], ab)
        idle = ec.idle_agents(c)
        assert len(idle) >= (0 if c["family"] == "clamp" else 1) and (c["avel"][:, idle] == 0).all() and (c["act"][:, idle] == 0).all()
        if len(idle) > 1:
            p = c["apos"][0, idle].astype(np.float64)
            d = np.linalg.norm(p[:, None] - p[None], axis=-1) + 9 * np.eye(len(idle))
            assert d.min() >= 1.0
    for c in ec.ALL_CASES:
        _, gap = ec.pre_pairs(c)
        r = ec.reference(c)
        assert np.isfinite(r["apos"]).all() and np.isfinite(r["rew"]).all()
        if gap.size:                                                      # nothing coincident: dist > 1e-3 everywhere
            assert (gap > -0.1 + 1e-3).all() or c["family"] in ("crowded", "ratio", "reset", "pairs"), c["name"]


def test_every_force_branch_is_reached():
    """Per pair type: pairs beyond the cutoff (force skipped), inside it with z < 0, and overlapping (z > 0), counted on the
    pre-step states; the at-rest pairs at dmin + 0.05 feel a force float32 can hold and those beyond the cutoff none."""
    seen = {}
    for c in ec.PAIR_CASES:
        a, b = c["meta"]["pair"]
        names, gap = ec.pre_pairs(c)
        NA = ec.n_agents(c)
        pairs = [(i, j) for i in range(NA) for j in range(i + 1, NA + (0 if c["kind"] == "spread" else c["sizes"][2]))]
        k = pairs.index((a, b))
        g = gap[:, k]
        label = ("spread " if c["kind"] == "spread" else "") + names[k]
        seen[label] = (int((g > ec.CUTOFF).sum()), int(((g > 0) & (g < ec.CUTOFF)).sum()), int((g < 0).sum()))
        assert np.array_equal(g > ec.CUTOFF, c["meta"]["beyond"])
        sep = np.array([ec._sep(ec.PAIR_SEPS[s], c["meta"]["dmin"]) for s in c["meta"]["sep"]])
        assert np.abs(g + c["meta"]["dmin"] - sep).max() < 1e-7           # float32 rounding of the placed coordinates
        assert {(s, r) for s, r in zip(c["meta"]["sep"], c["meta"]["rest"])} == {(s, r) for s in range(9) for r in (False, True)}
        # at rest, noop: the whole velocity is the contact force's; the lower index sits on either side
        r, rest = ec.reference(c), c["meta"]["rest"]
        dv = np.abs(r["avel"][:, a]).max(-1)
        at50 = rest & (c["meta"]["sep"] == ec.PAIR_SEPS.index("+50"))
        assert at50.sum() == 6 and (dv[at50] > ec.REST_MIN).all() and (dv[at50] < 1e-20).all()
        assert (dv[rest & (c["meta"]["sep"] == ec.PAIR_SEPS.index("+104"))] < 1e-45).all()   # float32 cannot hold it: 0 on the device
        assert (dv[rest & c["meta"]["beyond"]] < 1e-45).all()
        side = np.sign(((c["apos"][:, a] - (c["apos"][:, b] if b < NA else c["lpos"][:, b - NA])) * np.array(ec.DIRS[2])).sum(-1))
        assert set(side.tolist()) == {-1.0, 1.0}
    print("pairs (beyond cutoff, in range z < 0, overlapping z > 0):", seen)
    assert set(seen) == {"spread agent-agent", "adv-adv", "adv-good", "good-good", "adv-obst", "good-obst"}
    assert all(min(v) > 0 for v in seen.values()), seen
    # the crowded worlds overlap in every pair type too
    crowd = {}
    for c in ec.CROWDED_CASES:
        names, gap = ec.pre_pairs(c)
        for n in set(names.tolist()):
            g = gap[:, names == n]
            t = crowd.setdefault((c["kind"], n), [0, 0, 0])
            t[0] += int((g > ec.CUTOFF).sum()); t[1] += int(((g > 0) & (g < ec.CUTOFF)).sum()); t[2] += int((g < 0).sum())
    assert len(crowd) == 6 and all(min(v) > 0 for v in crowd.values()), crowd


def test_contact_counts_and_crafted_decisions_are_clear():
    """Collision counts 0, 1, 2 and 3; every (d, side) combination; the oracle's post-step distance of a placed pair is where the
    bisection aimed (1e-7) and, as every other decision of a crafted case, more than 1e-5 off the threshold on the intended side."""
    for c in ec.CRAFTED_CASES:
        r = ec.reference(c)
        assert not r["close"].any() and np.abs(r["dist"] - r["thr"]).min() > ec.CLEAR, c["name"]
    for c in ec.CONTACT_CASES:
        r, m = ec.reference(c), c["meta"]
        if c["kind"] == "spread":
            got = np.stack([r["dist"][:, m["centre"], k] for k in m["movers"]], 1)
            counts = r["count"][:, m["centre"]]
            assert (r["count"][:, list(m["movers"])] == m["inside"]).all()
        elif m["centre"] >= c["sizes"][0]:                                # one good agent among three adversaries
            got = np.stack([r["dist"][:, k, m["centre"] - c["sizes"][0]] for k in m["movers"]], 1)
            counts = r["touch"][:, m["centre"] - c["sizes"][0]]
        else:                                                             # one adversary among three good agents
            got = np.stack([r["dist"][:, m["centre"], k - c["sizes"][0]] for k in m["movers"]], 1)
            counts = r["total"]
            assert (r["touch"][:, [k - c["sizes"][0] for k in m["movers"]]] == m["inside"]).all()
        assert np.abs(got - m["want"]).max() < 1e-7
        assert np.array_equal(got < r["thr"], m["inside"]) and np.array_equal(counts, m["inside"].sum(1))
        assert set(counts.tolist()) == {0, 1, 2, 3}
        if c["kind"] == "tag":
            assert np.array_equal(r["total"], m["inside"].sum(1)) and set(r["total"].tolist()) == {0, 1, 2, 3}
        rel = np.round(got / r["thr"] - 1, 6)
        assert set(np.abs(rel).ravel().tolist()) == set(ec.CONTACT_D)
        assert {(abs(x), x < 0) for x in rel.ravel().tolist()} == {(d, s) for d in ec.CONTACT_D for s in (False, True)}
        band = np.abs(got ** 2 - r["thr"] ** 2) <= (1.01 ** 2 - 1) * r["thr"] ** 2
        assert band.any() and not band.all()                              # the sqrt band of mpe_local_penalty: both in and out


def test_boundary_pieces_and_the_cap():
    (c,) = ec.BOUNDARY_CASES
    r = ec.reference(c)
    assert np.array_equal(r["apos"], c["apos"].astype(np.float64)) and (r["avel"] == 0).all()    # post == pre exactly
    piece = r["piece"]
    counts = {p: int((piece == p).sum()) for p in range(4)}
    print("boundary pieces (none, linear, exp, cap):", counts)
    assert all(v > 0 for v in counts.values())
    assert (piece.min(-1) > 0).any()                                      # both axes at once
    x = np.abs(c["apos"][:, 1:].astype(np.float64))
    assert ((x >= 1 + np.log(10) / 2) == (piece == 3)).all() and set(np.round(x[x > 0], 4).tolist()) >= set(ec.BOUND_X)
    assert (np.sign(c["apos"][:, 1:]) == -1).any() and (np.sign(c["apos"][:, 1:]) == 1).any()
    assert (r["touch"] == 0).all()


def test_clamp_is_taken_and_not_taken_per_team():
    seen = {}
    for c in ec.CLAMP_CASES:
        sp, vmax, r = ec.unclamped_speed(c), ec.vmax_of(c), ec.reference(c)
        out = np.linalg.norm(r["avel"], axis=-1)
        for t in sorted(set(ec.teams(c))):
            i = [k for k, x in enumerate(ec.teams(c)) if x == t]
            taken = sp[:, i] > vmax[i]
            seen[(c["name"], t)] = (int(taken.sum()), int((~taken).sum()))
            lim = np.broadcast_to(vmax[i], taken.shape)
            assert np.allclose(out[:, i][taken], lim[taken], rtol=1e-12) and np.allclose(out[:, i][~taken], sp[:, i][~taken], rtol=1e-12)
            rel = sp[:, i] / (1.0 if c["name"] == "clamp-spread-default" else lim)
            for k, (_, scale) in enumerate(ec.CLAMP_TARGETS):
                if scale is not None:
                    assert np.abs(rel[c["meta"]["target"] == k] - scale).max() < 1e-6
        v5 = c["meta"]["target"] == 3
        assert np.allclose(np.linalg.norm(c["avel"][v5].astype(np.float64), axis=-1), 5.0, rtol=1e-6)
    print("clamp (taken, not taken):", seen)
    assert seen[("clamp-spread-default", "agent")][0] == 0               # no limit: v = 5 passes
    c = ec.CLAMP_CASES[2]
    assert np.linalg.norm(ec.reference(c)["avel"], axis=-1).max() > 3.7
    assert all(min(v) > 0 for k, v in seen.items() if k[0] != "clamp-spread-default"), seen
    assert {k[1] for k in seen} == {"adv", "good", "agent"}


def test_random_worlds_are_mostly_clear():
    """Share of (env, pair) decisions within 1e-5 of their threshold, on the oracle: at most 1 % in every random case."""
    worst, hits = 0.0, 0
    for c in ec.RANDOM_CASES:
        mask, share = ec.excluded(c)
        assert share <= ec.CAP, (c["name"], share)
        worst, hits = max(worst, share), hits + int((~mask).sum())
    print(f"random worlds: worst close share {worst:.4f}; {hits} rewards held exactly")
    contacts = sum(int(np.sum(ec.reference(c)["dist"] < ec.reference(c)["thr"])) for c in ec.CROWDED_CASES)
    assert contacts > 500                                                # dense: the reward paths see many contacts


def test_reset_cases_finish_exactly_the_chosen_envs():
    for c in ec.RESET_CASES:
        r = ec.reference(c)
        assert np.array_equal(np.flatnonzero(r["trunc"]), np.array(ec.FINISHING))
        assert np.array_equal(r["trunc"], c["steps"] + 1 >= c["max_cycles"]) and len(set(c["episode"].tolist())) == 4
        # both sides of the 16-env workgroup edge finish and carry on
        assert {e // 16 for e in ec.FINISHING} == {0, 1, 2} and {15, 16} <= set(ec.FINISHING) and 14 not in ec.FINISHING


def test_float32_restatements_agree_with_the_oracle():
    """obs_layout on the oracle's own post-step state is the oracle's observation (float32 rounding apart), and the no-force step is
    the oracle's step wherever no force acts."""
    for c in ec.ROLLOUT_SPREAD + ec.ROLLOUT_TAG + ec.BOUNDARY_CASES:
        r = ec.reference(c)
        lay = ec.obs_layout(c, r["apos"], r["avel"], c["lpos"])
        assert lay.shape == r["obs"].shape and np.abs(lay - r["obs"]).max() < 1e-6
    for c in ec.PAIR_CASES:
        r, beyond = ec.reference(c), c["meta"]["beyond"]
        for pos, vel in ec.no_force_variants(c):
            assert np.abs(pos[beyond] - r["apos"][beyond]).max() < 1e-6 and np.abs(vel[beyond] - r["avel"][beyond]).max() < 1e-6


@pytest.mark.parametrize("kind", ["spread", "tag"])
def test_oracle_defaults_are_unchanged(kind):
    """The spread oracle's optional speed limit is off by default (MPE's simple_spread has none)."""
    w = ec._world(kind, (3,) if kind == "spread" else (3, 1, 2))
    assert kind == "tag" or w.max_speed is None
