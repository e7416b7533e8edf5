"""TEST INFRASTRUCTURE ONLY -- cases, inputs and float64 yardsticks for the simple_spread / simple_tag step kernels at their
edges (csrc/mpe.hip, csrc/mpe_tag.hip, mpe_dev.h, mpe_tag_dev.h).  numpy only, no GPU: tests/test_host_env_shapes.py asserts on
the CPU what the cases promise, tests/test_gpu_env_shapes.py runs them on the device.

A case is a dict: env kind ("spread" / "tag"), sizes ((N,) / (n_adv, n_good, n_obst)), n_env, cfg overrides (fields of the
env's config struct), apos / avel / lpos (the pre-step state, float32), steps and episode counters, act, max_cycles and
auto_reset, and per-env `meta` that says what was placed where.  Every state is drawn or constructed in float64 and ROUNDED TO
FLOAT32 FIRST, so the device and the oracle (oracle/mpe_oracle.py, oracle/mpe_tag_oracle.py, float64) start from identical
numbers; the yardstick of a case is the oracle's one step from that state (`reference`).

Crafted scenarios occupy a few agents of an env near the origin; every other entity sits idle (zero velocity, noop) on a lattice
of spacing 1.25, at least 5 away from the scenario: outside every force range, so its force is exactly 0.

Families:
  pairs     one pair per env for each pair type (spread: agent-agent, dmin 0.30; tag: adv-adv 0.15, adv-good 0.125, good-good
            0.10, adv-obstacle 0.275, good-obstacle 0.25) at the pre-step separations 0.2 dmin, dmin - {5, 0.5}e-3,
            dmin + {0.5, 5, 50, 104, 106}e-3 and 2 dmin, in three directions (two axis-aligned: one component exactly 0), the
            lower-index entity on either side, once at rest with noop (the tiny force at dmin + 0.05 is then all there is: a relative
            check sees a cutoff that comes too early) and once moving under actions.  Beyond dmin + 0.105 the post-step state
            must be bit-equal to "no force at all" (`no_force_variants`).
  contacts  the contact decisions on the NEW positions (spread: collision count at 0.30; tag: catches at 0.125).  The pre-step
            separation of every pair comes from a bisection on the float64 oracle, so that the oracle's post-step distance is
            thr (1 +- d), d in {1e-4, 0.0099, 0.0101, 0.05}: inside the +-1 % band in which mpe_local_penalty takes the sqrt,
            either side of both band edges, and well clear.  Three pairs around one centre agent per env, every in / out pattern:
            counts of 0, 1, 2 and 3; in tag once a good agent among three adversaries and once an adversary among three good agents.
  boundary  tag: isolated good agents at rest, |x| in BOUND_X, both signs, each axis and both at once; post == pre exactly.
  clamp     isolated agents whose velocity and action put |v'| at 0.999, 1.001 and 3 times the limit, and v = 5; adversaries
            (1.0) and good agents (1.3); spread with max_speed 1.0 on the config struct and with the default -1 (v = 5 passes).
  ratio     spread, local_ratio in {0, 0.3, 0.5, 1} on a crowded world.
  crowded   random worlds (agent positions scaled by 0.3, velocities up to the limit, random actions) at the size limits, each
            at n_env in {1, 15, 16, 17, 35} (a workgroup stages 16 envs).
  reset     n_env 35, `steps` preset so that envs FINISHING reach max_cycles in this step and the others do not; auto_reset on / off.

Not covered: coincident entities (0 / 0 on both sides of the comparison), and parity with pettingzoo itself, which stays
unpinned as the kernels' headers say."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

import mpe_oracle  # noqa: E402
import mpe_tag_oracle  # noqa: E402

F32 = np.float32
MARGIN, CUTOFF = 1e-3, 105e-3           # contact_margin; the kernels skip a pair beyond dmin + 105 margins
BAR = 2e-5                              # single-step bar of test_gpu_pipeline.py / test_gpu_tag.py: |got - ref| <= BAR (1 + |ref|)
CLEAR, CAP = 1e-5, 0.01                 # a decision within CLEAR of its threshold is "close"; at most CAP of them may be
# A pair at rest under noop: dv = 100 margin exp(z) dist^-1 delta dt with z = -(dist - dmin) / margin.  In float32 dist carries
# ~1.5 ulp (4e-8 at 0.3) and dmin one more, so z is off by <= 1e-4 absolute and exp(z) by <= 1e-4 relative (expf / log1pf
# themselves: a few ulp); REST_REL leaves a factor 10 on that.  A force that is skipped altogether is off by 100 %.
REST_REL, REST_MIN = 1e-3, 1e-30
MAX_CYCLES, SEED = 25, 11
DT, DAMP = 0.1, 0.25
SPREAD_THR, SPREAD_ACCEL = 0.30, 5.0
TAG_THR = 0.125
TAG_SIZE = {"adv": 0.075, "good": 0.05, "obst": 0.2}
TAG_ACCEL, TAG_VMAX = {"adv": 3.0, "good": 4.0}, {"adv": 1.0, "good": 1.3}
PAIR_SEPS = ("0.2dmin", "-5", "-0.5", "+0.5", "+5", "+50", "+104", "+106", "2dmin")
DIRS = ((1.0, 0.0), (0.0, 1.0), (float(np.cos(2.2)), float(np.sin(2.2))))
CONTACT_D = (1e-4, 0.0099, 0.0101, 0.05)
BOUND_X = (0.85, 0.8999, 0.9001, 0.95, 0.9999, 1.0001, 1.5, 2.15, 2.16, 3.0)
CLAMP_TARGETS = (("under", 0.999), ("over", 1.001), ("far", 3.0), ("v5", None))
RATIOS = (0.0, 0.3, 0.5, 1.0)
N_ENVS = (1, 15, 16, 17, 35)
SPREAD_SIZES = ((1,), (2,), (3,), (5,), (8,))
TAG_SIZES = ((1, 1, 0), (1, 1, 4), (7, 1, 0), (1, 7, 4), (4, 4, 4), (3, 1, 2), (2, 3, 1))
FINISHING = (0, 5, 15, 16, 31, 34)
CENTRE = np.array([0.1, -0.2])


def case_id(c) -> str:
    return c["name"]


def n_agents(c) -> int:
    return c["sizes"][0] if c["kind"] == "spread" else c["sizes"][0] + c["sizes"][1]


def n_landmarks(c) -> int:
    return c["sizes"][0] if c["kind"] == "spread" else c["sizes"][2]


def teams(c) -> list:
    """Team of every agent ("adv" / "good"; spread agents are "agent")."""
    return ["agent"] * c["sizes"][0] if c["kind"] == "spread" else ["adv"] * c["sizes"][0] + ["good"] * c["sizes"][1]


def idle_agents(c) -> list:
    """Agents of a crafted case that no scenario uses: at rest on the lattice under noop."""
    m, NA = c["meta"], n_agents(c)
    used = {k for k in m["pair"] if k < NA} if c["family"] == "pairs" else {m["centre"], *m["movers"]} if c["family"] == "contacts" \
        else set(range(1, NA)) if c["family"] == "boundary" else set(range(NA))
    return [i for i in range(NA) if i not in used]


def accel_of(c) -> np.ndarray:
    return np.array([SPREAD_ACCEL if t == "agent" else TAG_ACCEL[t] for t in teams(c)])


def vmax_of(c) -> np.ndarray:
    """Speed limit per agent; inf where there is none."""
    if c["kind"] == "spread":
        ms = c["cfg"].get("max_speed", -1.0)
        return np.full(c["sizes"][0], ms if ms > 0 else np.inf)
    return np.array([TAG_VMAX[t] for t in teams(c)])


def _idle_agent(k):
    return (-4.0 + 1.25 * k, 6.0)


def _idle_obst(l):
    return (-4.0 + 1.25 * l, 8.0)


def _case(family, name, kind, sizes, apos, avel, lpos, act, steps=None, episode=None, cfg=None, auto_reset=False, **meta):
    apos, avel = np.asarray(apos, np.float64).astype(F32), np.asarray(avel, np.float64).astype(F32)
    n_env = len(apos)
    c = dict(family=family, name=name, kind=kind, sizes=tuple(sizes), n_env=n_env, cfg=dict(cfg or {}), apos=apos, avel=avel,
             act=np.asarray(act, np.int32), max_cycles=MAX_CYCLES, auto_reset=bool(auto_reset), meta=meta)
    c["lpos"] = np.asarray(lpos, np.float64).astype(F32).reshape(n_env, n_landmarks(c), 2)
    c["steps"] = np.zeros(n_env, np.int32) if steps is None else np.asarray(steps, np.int32)
    c["episode"] = np.ones(n_env, np.int64) if episode is None else np.asarray(episode, np.int64)
    NA = n_agents(c)
    assert apos.shape == avel.shape == (n_env, NA, 2) and c["act"].shape == (n_env, NA)
    return c


def _blank(kind, sizes, n_env, seed):
    """Every entity idle on its lattice slot; spread landmarks (no collisions) at seeded random places."""
    NA = sizes[0] if kind == "spread" else sizes[0] + sizes[1]
    apos = np.tile(np.array([_idle_agent(k) for k in range(NA)]), (n_env, 1, 1))
    if kind == "spread":
        lpos = np.random.default_rng(seed).uniform(-1, 1, (n_env, NA, 2))
    else:
        lpos = np.tile(np.array([_idle_obst(l) for l in range(sizes[2])]).reshape(sizes[2], 2), (n_env, 1, 1))
    return apos, np.zeros((n_env, NA, 2)), lpos, np.zeros((n_env, NA), np.int32)


# ---- pair forces ------------------------------------------------------------------------------------------------------------------
# (kind, sizes, name of the pair type, entity a, entity b (agents first, then obstacles), dmin)
PAIR_TYPES = (("spread", (3,), "agent-agent", 0, 1, 0.30),
              ("tag", (2, 2, 1), "adv-adv", 0, 1, 0.15), ("tag", (2, 2, 1), "adv-good", 0, 2, 0.125),
              ("tag", (2, 2, 1), "good-good", 2, 3, 0.10), ("tag", (2, 2, 1), "adv-obst", 0, 4, 0.275),
              ("tag", (2, 2, 1), "good-obst", 2, 4, 0.25))


def _sep(label, dmin):
    return 0.2 * dmin if label == "0.2dmin" else 2 * dmin if label == "2dmin" else dmin + float(label) * 1e-3


def _pair_case(kind, sizes, tname, a, b, dmin):
    combos = [(s, d, side, rest) for s in range(len(PAIR_SEPS)) for d in range(len(DIRS)) for side in (1, -1) for rest in (True, False)]
    apos, avel, lpos, act = _blank(kind, sizes, len(combos), seed=1)
    NA = apos.shape[1]
    for e, (s, d, side, rest) in enumerate(combos):
        half = 0.5 * _sep(PAIR_SEPS[s], dmin) * side * np.array(DIRS[d])
        apos[e, a] = CENTRE + half
        if b < NA:
            apos[e, b] = CENTRE - half
        else:
            lpos[e, b - NA] = CENTRE - half
        if not rest:
            avel[e, a], act[e, a] = (0.11, -0.07), 1 + e % 4
            if b < NA:
                avel[e, b], act[e, b] = (-0.05, 0.13), (e + 2) % 5
    m = np.array(combos)
    return _case("pairs", f"pairs-{kind}-{tname}", kind, sizes, apos, avel, lpos, act, pair=(a, b), dmin=dmin, sep=m[:, 0],
                 rest=m[:, 3].astype(bool), beyond=np.array([_sep(PAIR_SEPS[s], dmin) > dmin + CUTOFF for s in m[:, 0]]))


# ---- contact decisions ------------------------------------------------------------------------------------------------------------
def _world(kind, sizes, cfg=None):
    if kind == "spread":
        cfg = cfg or {}
        return mpe_oracle.SimpleSpreadWorld(sizes[0], MAX_CYCLES, cfg.get("local_ratio", 0.5), max_speed=cfg.get("max_speed"))
    return mpe_tag_oracle.SimpleTagWorld(*sizes, max_cycles=MAX_CYCLES)


def _bisect_sep(kind, speed, mover_team, target, lo, hi):
    """Pre-step separation at which the float64 oracle's post-step distance of (a centre agent at rest, a second agent that flies at
    it with `speed`) is `target`: bisection on the oracle, the state rounded to float32 as the case will hold it."""
    sizes = (2,) if kind == "spread" else (1, 1, 0)
    w = _world(kind, sizes)
    mover = 1 if kind == "spread" or mover_team == "good" else 0
    d = np.array(DIRS[2])

    def post(s):
        apos, avel = np.zeros((2, 2)), np.zeros((2, 2))
        apos[1 - mover], apos[mover], avel[mover] = CENTRE, CENTRE + s * d, -speed * d
        w.set_state(apos.astype(F32), avel.astype(F32), np.zeros((sizes[0], 2)) if kind == "spread" else np.zeros((0, 2)))
        w.step([0, 0])
        return float(np.linalg.norm(w.apos[0] - w.apos[1]))

    assert post(lo) < target < post(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if post(mid) < target else (lo, mid)
    return 0.5 * (lo + hi)


def _contact_case(kind, sizes, name, centre, movers, mover_team, speed, thr):
    """Env (di, pattern): pair k (centre, movers[k]) lands at thr (1 - d) where bit k of `pattern` is set, at thr (1 + d) elsewhere,
    d = CONTACT_D[(di + k) % 4]: every (d, side) occurs, and so does every number of contacts from 0 to 3."""
    combos = [(di, pat) for di in range(len(CONTACT_D)) for pat in range(8)]
    apos, avel, lpos, act = _blank(kind, sizes, len(combos), seed=2)
    dirs = [np.array([np.cos(t), np.sin(t)]) for t in (0.3, 0.3 + 2 * np.pi / 3, 0.3 + 4 * np.pi / 3)]
    sep = {}
    want = np.zeros((len(combos), 3))
    for e, (di, pat) in enumerate(combos):
        apos[e, centre] = CENTRE
        for k, m in enumerate(movers):
            d = CONTACT_D[(di + k) % 4]
            want[e, k] = thr * (1 - d if pat >> k & 1 else 1 + d)
            if want[e, k] not in sep:
                sep[want[e, k]] = _bisect_sep(kind, speed, mover_team, want[e, k], thr + 0.01, thr + 0.5)
            apos[e, m], avel[e, m] = CENTRE + sep[want[e, k]] * dirs[k], -speed * dirs[k]
    return _case("contacts", name, kind, sizes, apos, avel, lpos, act, centre=centre, movers=tuple(movers), want=want,
                 inside=np.array([[pat >> k & 1 for k in range(3)] for _, pat in combos], bool))


# ---- boundary penalty -------------------------------------------------------------------------------------------------------------
def _boundary_case():
    sizes = (1, 3, 0)
    spots = [[(x, 0), (-x, 0), (0, x)] for x in BOUND_X] + [[(0, -x), (x, x), (-x, -x)] for x in BOUND_X] + \
            [[(x, -x), (-x, 0.5 * x), (0.5 * x, x)] for x in BOUND_X]
    apos, avel, lpos, act = _blank("tag", sizes, len(spots), seed=3)
    apos[:, 1:] = np.array(spots, np.float64)
    return _case("boundary", "boundary-tag", "tag", sizes, apos, avel, lpos, act)


# ---- speed clamp ------------------------------------------------------------------------------------------------------------------
def _clamp_case(kind, sizes, name, cfg=None):
    combos = [(t, d, a) for t in range(len(CLAMP_TARGETS)) for d in range(len(DIRS)) for a in (0, 2, 3)]
    apos, avel, lpos, act = _blank(kind, sizes, len(combos), seed=4)
    apos[:] = np.array([(0.5, 0.5), (-0.5, 0.5), (0.5, -0.5), (-0.5, -0.5)])
    c0 = dict(kind=kind, sizes=sizes, cfg={"max_speed": 1.0})              # the limit the velocities are sized for
    vmax, accel = vmax_of(c0), accel_of(c0)
    for e, (t, d, a) in enumerate(combos):
        u = np.array([(a == 2) - (a == 1), (a == 4) - (a == 3)], np.float64)
        for i in range(4):
            scale = CLAMP_TARGETS[t][1]
            avel[e, i] = 5.0 * np.array(DIRS[d]) if scale is None else (scale * vmax[i] * np.array(DIRS[d]) - u * accel[i] * DT) / (1 - DAMP)
        act[e] = a
    return _case("clamp", name, kind, sizes, apos, avel, lpos, act, cfg=cfg, target=np.array([t for t, _, _ in combos]))


# ---- crowded random worlds --------------------------------------------------------------------------------------------------------
def _crowded(family, name, kind, sizes, n_env, seed, cfg=None, steps=None, episode=None, auto_reset=True):
    rng = np.random.default_rng(seed)
    NA = sizes[0] if kind == "spread" else sizes[0] + sizes[1]
    c0 = dict(kind=kind, sizes=sizes, cfg={"max_speed": 1.0})
    apos = rng.uniform(-1, 1, (n_env, NA, 2)) * 0.3
    ang, speed = rng.uniform(0, 2 * np.pi, (n_env, NA)), rng.uniform(0, 1, (n_env, NA)) * vmax_of(c0)
    avel = np.stack([np.cos(ang), np.sin(ang)], -1) * speed[..., None]
    lpos = rng.uniform(-1, 1, (n_env, NA, 2)) if kind == "spread" else rng.uniform(-0.9, 0.9, (n_env, sizes[2], 2))
    return _case(family, name, kind, sizes, apos, avel, lpos, rng.integers(0, 5, (n_env, NA)), steps=steps, episode=episode, cfg=cfg,
                 auto_reset=auto_reset)


def _size_name(kind, sizes):
    return f"{kind}{sizes[0]}" if kind == "spread" else "tag{}v{}o{}".format(*sizes)


def _build():
    pairs = [_pair_case(*t) for t in PAIR_TYPES]
    contacts = [_contact_case("spread", (5,), "contacts-spread", 0, (1, 2, 3), "agent", 2.0, SPREAD_THR),
                _contact_case("tag", (4, 4, 2), "contacts-tag-good-among-adv", 4, (0, 1, 2), "adv", 1.2, TAG_THR),
                _contact_case("tag", (4, 4, 2), "contacts-tag-adv-among-good", 0, (4, 5, 6), "good", 1.2, TAG_THR)]
    boundary = [_boundary_case()]
    clamp = [_clamp_case("tag", (2, 2, 0), "clamp-tag"), _clamp_case("spread", (4,), "clamp-spread-max1", {"max_speed": 1.0}),
             _clamp_case("spread", (4,), "clamp-spread-default")]
    ratio = [_crowded("ratio", f"ratio-spread5-{lr}", "spread", (5,), 17, 50 + k, cfg={"local_ratio": lr}) for k, lr in enumerate(RATIOS)]
    crowded, k = [], 0
    for kind, all_sizes in (("spread", SPREAD_SIZES), ("tag", TAG_SIZES)):
        for sizes in all_sizes:
            for n_env in N_ENVS:
                crowded.append(_crowded("crowded", f"crowded-{_size_name(kind, sizes)}-E{n_env}", kind, sizes, n_env, 100 + k))
                k += 1
    reset = []
    for kind, sizes in (("spread", (3,)), ("spread", (8,)), ("tag", (1, 1, 0)), ("tag", (3, 1, 2)), ("tag", (4, 4, 4))):
        for auto in (True, False):
            e = np.arange(35)
            steps = np.where(np.isin(e, FINISHING), MAX_CYCLES - 1, (e * 7) % (MAX_CYCLES - 1))
            reset.append(_crowded("reset", f"reset-{_size_name(kind, sizes)}-{'auto' if auto else 'manual'}", kind, sizes, 35, 300 + k,
                                  steps=steps, episode=1 + e % 4, auto_reset=auto))
            k += 1
    return pairs, contacts, boundary, clamp, ratio, crowded, reset


PAIR_CASES, CONTACT_CASES, BOUNDARY_CASES, CLAMP_CASES, RATIO_CASES, CROWDED_CASES, RESET_CASES = _build()
CRAFTED_CASES = PAIR_CASES + CONTACT_CASES + BOUNDARY_CASES + CLAMP_CASES
RANDOM_CASES = RATIO_CASES + CROWDED_CASES + RESET_CASES
ALL_CASES = CRAFTED_CASES + RANDOM_CASES
# the crowded states the fused rollouts start from (tests/test_gpu_env_shapes.py): dense multi-contact worlds, ragged workgroups
ROLLOUT_SPREAD = [c for c in CROWDED_CASES if c["name"] in ("crowded-spread8-E35", "crowded-spread3-E17", "crowded-spread5-E35")]
ROLLOUT_TAG = [c for c in CROWDED_CASES if c["name"] in ("crowded-tag4v4o4-E35", "crowded-tag3v1o2-E17", "crowded-tag1v1o0-E15")]


# ---- yardsticks -------------------------------------------------------------------------------------------------------------------
def bound_pen(x):
    """The three pieces of simple_tag's boundary penalty and which one applies (0: none, 1: linear, 2: exp, 3: the cap at 10)."""
    x = abs(float(x))
    if x < 0.9:
        return 0.0, 0
    if x < 1.0:
        return (x - 0.9) * 10, 1
    v = float(np.exp(2 * x - 2))
    return (10.0, 3) if v > 10 else (v, 2)


_REF: dict = {}


def reference(c) -> dict:
    """The oracle's one step from the case's state (float64), env by env, and what its rewards are made of:
    apos / avel [E, NA, 2], rew [E, NA], obs [E, NA, D], trunc [E];
    dist -- the post-step distances the contact decisions are taken on (spread [E, N, N], inf on the diagonal; tag [E, n_adv, n_good]),
    thr, close = |dist - thr| <= CLEAR;
    spread: count [E, N] collisions per agent, glob [E] = -sum of the landmark minima;
    tag: touch [E, n_good] adversaries touching each good agent, total [E], bound [E, n_good] and piece [E, n_good, 2]."""
    if c["name"] in _REF:
        return _REF[c["name"]]
    E, NA = c["n_env"], n_agents(c)
    w = _world(c["kind"], c["sizes"], c["cfg"])
    r = dict(apos=np.zeros((E, NA, 2)), avel=np.zeros((E, NA, 2)), rew=np.zeros((E, NA)), trunc=np.zeros(E, bool), obs=[])
    for e in range(E):
        w.set_state(c["apos"][e], c["avel"][e], c["lpos"][e], steps=int(c["steps"][e]))
        obs, rew, term, trunc = w.step(c["act"][e])
        assert not term.any() and trunc.all() == trunc.any()
        r["apos"][e], r["avel"][e], r["rew"][e], r["trunc"][e] = w.apos, w.avel, rew, trunc[0]
        r["obs"].append(obs)
    r["obs"] = np.stack(r["obs"])
    p = r["apos"]
    if c["kind"] == "spread":
        d = np.linalg.norm(p[:, :, None] - p[:, None], axis=-1)
        d[:, np.arange(NA), np.arange(NA)] = np.inf
        lp = c["lpos"].astype(np.float64)
        r.update(dist=d, thr=SPREAD_THR, count=(d < SPREAD_THR).sum(-1),
                 glob=-np.linalg.norm(p[:, :, None] - lp[:, None], axis=-1).min(1).sum(-1))
        lr = c["cfg"].get("local_ratio", 0.5)
        assert np.allclose(r["rew"], r["glob"][:, None] * (1 - lr) - r["count"] * lr, rtol=0, atol=1e-12)
    else:
        na = c["sizes"][0]
        d = np.linalg.norm(p[:, :na, None] - p[:, None, na:], axis=-1)
        bp = np.array([[[bound_pen(x) for x in q] for q in env] for env in p[:, na:]]).reshape(E, NA - na, 2, 2)
        r.update(dist=d, thr=TAG_THR, touch=(d < TAG_THR).sum(1), total=(d < TAG_THR).sum((1, 2)), bound=bp[..., 0].sum(-1),
                 piece=bp[..., 1].astype(int))
        assert np.allclose(r["rew"][:, na:], -10.0 * r["touch"] - r["bound"], rtol=0, atol=1e-12)
        assert np.array_equal(r["rew"][:, :na], np.repeat(10.0 * r["total"][:, None], na, 1))
    r["close"] = np.abs(r["dist"] - r["thr"]) <= CLEAR
    _REF[c["name"]] = r
    return r


def excluded(c, r=None):
    """Rewards that hang on a close decision: (mask [E, NA] of the rewards left out of the exact check, share of close decisions
    among all decisions of the case).  A pair (i, j) of spread touches the rewards of i and j; an (adversary, good agent) pair of tag
    the good agent's reward and every adversary's."""
    r = r or reference(c)
    close = r["close"]
    if c["kind"] == "spread":
        N = c["sizes"][0]
        return close.any(-1), (close.sum() / (c["n_env"] * N * (N - 1)) if N > 1 else 0.0)
    na = c["sizes"][0]
    mask = np.concatenate([np.repeat(close.any((1, 2))[:, None], na, 1), close.any(1)], 1)
    return mask, close.sum() / close.size


def pre_pairs(c):
    """Every collidable pair of the pre-step state: (type name [P], gap = distance - dmin [E, P]) in float64."""
    NA, NL = n_agents(c), 0 if c["kind"] == "spread" else c["sizes"][2]
    size = {"agent": 0.15, **TAG_SIZE}
    kinds = teams(c) + ["obst"] * NL
    pos = np.concatenate([c["apos"], c["lpos"][:, :NL]], 1).astype(np.float64)
    names, gaps = [], []
    for a in range(NA):
        for b in range(a + 1, NA + NL):
            names.append(f"{kinds[a]}-{kinds[b]}")
            gaps.append(np.linalg.norm(pos[:, a] - pos[:, b], axis=-1) - (size[kinds[a]] + size[kinds[b]]))
    return np.array(names), (np.stack(gaps, 1) if gaps else np.zeros((c["n_env"], 0)))


def unclamped_speed(c):
    """|v'| before the clamp where no contact force acts (clamp family: isolated agents): |0.75 v + u accel dt|, float64 [E, NA]."""
    a = c["act"]
    u = np.stack([(a == 2) * 1.0 - (a == 1), (a == 4) * 1.0 - (a == 3)], -1)
    return np.linalg.norm(c["avel"].astype(np.float64) * (1 - DAMP) + u * accel_of(c)[None, :, None] * DT, axis=-1)


# ---- float32 restatements the device is held to bit for bit ------------------------------------------------------------------------
def obs_layout(c, apos, avel, lpos) -> np.ndarray:
    """The documented observation rows from a float32 state, every entry one float32 subtraction (or a copy, or 0):
    spread (6N): [vel 2, pos 2, landmarks rel 2N, others rel 2(N-1), comm 0 x 2(N-1)];
    tag: [vel 2, pos 2, obstacles rel, others rel 2(NA-1), velocities of the good agents other than oneself, zero padding]."""
    apos, avel, lpos = (np.asarray(x, F32) for x in (apos, avel, lpos))
    E, NA, NL = apos.shape[0], n_agents(c), n_landmarks(c)
    na = 0 if c["kind"] == "spread" else c["sizes"][0]
    D = 6 * NA if c["kind"] == "spread" else 4 + 2 * NL + 2 * (NA - 1) + 2 * c["sizes"][1]
    out = np.zeros((E, NA, D), F32)
    for i in range(NA):
        parts = [avel[:, i], apos[:, i]]
        parts += [lpos[:, l] - apos[:, i] for l in range(NL)]
        parts += [apos[:, j] - apos[:, i] for j in range(NA) if j != i]
        if c["kind"] == "tag":
            parts += [avel[:, j] for j in range(na, NA) if j != i]
        row = np.concatenate(parts, -1)
        assert row.dtype == F32
        out[:, i, :row.shape[-1]] = row
    return out


def no_force_variants(c):
    """Post-step (pos, vel) of every agent of the case under NO contact force and no clamp, evaluated in float32:
    v' = v 0.75 + u accel dt, p' = p + v' dt.  A compiler may contract either product of a sum into a fused multiply-add, so there
    are three float32 evaluations of v' and two of p' per v': all six, as (pos, vel) float32 arrays.  Products of two float32
    are exact in float64, so a float64 sum rounded once to float32 is the fused result."""
    p, v = c["apos"].astype(np.float64), c["avel"].astype(np.float64)
    a = c["act"]
    u = np.stack([(a == 2) * 1.0 - (a == 1), (a == 4) * 1.0 - (a == 3)], -1)
    f = (u * accel_of(c)[None, :, None]).astype(F32).astype(np.float64)
    keep, dt = float(F32(1) - F32(DAMP)), float(F32(DT))
    r = lambda x: x.astype(F32).astype(np.float64)  # noqa: E731
    vs = [r(r(v * keep) + r(f * dt)), r(v * keep + r(f * dt)), r(r(v * keep) + f * dt)]
    return [((p + q(w * dt)).astype(F32), w.astype(F32)) for w in vs for q in (r, lambda x: x)]
