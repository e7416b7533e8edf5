"""GPU tests (`-m gpu`) of the persistent rollouts' buffer bookkeeping across ring wrap-around: `VrbLane` (csrc/vrb_dev.h) in
csrc/rollout.hip, csrc/rollout_rows.hip and csrc/rollout_tag.hip, the stores of a launch that writes a slot more than once, the
`ignore_obs_next` variants on a wrapped ring, and the compact episode record at and beyond its capacity.

Every case runs the same job three times from the same seeds:
  big           unfused collector, a buffer that never wraps and is never reset: the run's time-ordered truth (what a rollout
                computes does not depend on the buffer's size)
  ring-unfused  sub-buffers of S slots, `fused_rollout=False, use_graph=False`
  ring-fused    sub-buffers of S slots, the persistent launch
and asserts, all with `torch.equal` / `np.array_equal` on bit patterns (nothing here takes a tolerance):
  (a) ring-fused == ring-unfused: every store both write, `buf.index.state` with its error flag word after EVERY collect, the env
      state, `returns / lens / n_collected_episodes` of every collect, the per-step outputs ws["ptr" / "ep_idx" / "ep_len" / "ep_rew"]
      (every form of every kernel writes all four in compact mode too: `VrbLane::add` the first three, `EpReturns::fold` ep_rew);
  (b) both ring runs == tests/rollout_ring_cases.py's answers computed from big: the stores `expected_ring`, the index state after
      every collect, the per-step outputs and the per-collect lens / returns `expected_index` -- an error that vrb_add_row and VrbLane
      shared would not hide.  V(obs_next), which only the persistent launches store, is held to a critic pass over big's
      obs_next rows put through `expected_ring`; the actor-only rollout stores neither V(obs) nor V(obs_next);
  (c) the case exercised what it claims: total steps > S, a launch with n_steps > S and episode ends on slot S - 1 and on slot 0
      where the case's definition predicts them (`_predict`, from the schedule alone), error flag word 0.

Schedules (`_schedule`): two_short = two collects each shorter than S, the second crossing the ring end from a non-zero insertion
index; exact = one collect of exactly S steps (the index state behind it is checked: insertion folded to 0), then 2 more steps so
that the run is longer than the ring; double = one collect of 2 S + 1 steps, every slot written at least twice in one launch;
reset = a collect, `reset_buffer(keep_statistics=True)`, a wrapping collect of S + 2 steps (the trainer's sequence).

Episode phase: `env.steps` is the within-episode counter the truncation reads (csrc/mpe.hip, csrc/mpe_tag.hip and the rollouts:
`stp = steps + 1; tr = stp >= max_cycles`; csrc/mpe_dev.h only carries `max_cycles`); staggered cases write it with
`arange(n_env) % max_cycles` before the first collect, in all three runs, so that every lane has its own episode start.

Which size stands for which form (the library has no query for the launch geometry; rules read from the launchers in
csrc/rollout.hip and csrc/rollout_rows.hip).  64-wide spread rollout, `rollout_form=2` (wave-autonomous): a wave owns 16 // N envs
and a workgroup has 1 wave up to 256 waves in all, 2 up to 512, 4 above -- (300, 3), (600, 3) and (1024, 3), the sizes
tests/test_gpu_rollout.py documents for 1 / 2 / 4 waves, are 60 / 120 / 205 waves and all take ONE wave per workgroup under that
rule; (1300, 3) = 260 waves takes two and (2600, 3) = 520 waves four (no older test reaches four), so all five are here.  `rollout_form=1` (tile): eight waves
up to 256 workgroups of 16 // N envs -- (5, 3) one tile, (7, 3) a ragged second tile, (1, 3) a single env, (6, 4) the generic
instantiation, (1024, 3) 205 workgroups -- and four waves above: (2100, 2) = 263 workgroups.  Actor-only 128-wide rollout: wave form
by default, the tile form under `rollout_form=1` for observation widths up to 32 -- (9, 2), (21, 4); (37, 6) and (9, 2) have partial
last waves, (33, 8) takes the `<3, 8>` specialisation.  Tag rollout: one kernel, one policy per team or one shared policy."""
import contextlib
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollout_ring_cases as rc  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm import GenericPPO
    from tianshou_marl_amd.algorithm.multiagent import FlexibleMultiAgentPolicyManager
    from tianshou_marl_amd.algorithm.ppo import PPO, policy_within_training_step
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.env.mpe_tag import DeviceSimpleTagVectorEnv
    from tianshou_marl_amd.utils.net import DiscreteActorCritic, MLPActorCritic

DEV = "cuda"
SEED = 3
SS = (1, 2, 3, 5, 7)
SCHEDULES = ("two_short", "exact", "double", "reset")
CYCLES = ("smaller", "equal", "larger", "coprime")
FORMS = ("wave1", "wave1_600", "wave1_1024", "wave2", "wave4", "tile8", "tile8_ragged", "tile8_single", "tile8_generic_n",
         "tile8_205", "tile4", "actor_wave", "actor_tile", "tag_teams", "tag_shared")


def _schedule(name, S):
    return {"two_short": {3: [2, 2], 5: [3, 4], 7: [4, 5]}.get(S), "exact": [S, 2], "double": [2 * S + 1],
            "reset": [max(S - 1, 1), "reset", S + 2]}[name]


def case(id, form, shape, S, sched, mc, stagger=False, generic=0, mode=1, **flags):
    kind = "actor" if form.startswith("actor") else "tag" if form.startswith("tag") else "spread"
    rollout_form = 0 if kind == "tag" else 1 if "tile" in form else 2
    return dict(id=id, form=form, kind=kind, shape=shape, n_env=shape[0], S=S, sched=sched, ops=_schedule(sched, S), mc=mc,
                stagger=stagger, rollout_form=rollout_form, generic=generic, mode=mode, flags=flags)


# id, form, shape -- (n_env, N) | actor (n_env, N) | tag (n_env, n_adv, n_good, n_obst) --, S, schedule, max_cycles, staggered, ...
CASES = [
    # ---- 64-wide spread rollout (csrc/rollout.hip) ----
    case("t8-S1-double", "tile8", (5, 3), 1, "double", 2),
    case("t8r-S2-exact-stag", "tile8_ragged", (7, 3), 2, "exact", 2, True),
    case("t8s-S3-short", "tile8_single", (1, 3), 3, "two_short", 2),
    case("t8r-S5-reset-stag", "tile8_ragged", (7, 3), 5, "reset", 3, True),
    case("t8r-S7-double", "tile8_ragged", (7, 3), 7, "double", 4),
    case("t8r-S3-double-generic", "tile8_ragged", (7, 3), 3, "double", 3, generic=1),
    case("t8r-S3-double-specialised", "tile8_ragged", (7, 3), 3, "double", 3, generic=0),
    case("t8r-S5-short-argmax-stag", "tile8_ragged", (7, 3), 5, "two_short", 7, True, mode=2),
    case("t8r-S5-short-sample-stag", "tile8_ragged", (7, 3), 5, "two_short", 7, True, mode=1),
    case("t8n4-S2-double", "tile8_generic_n", (6, 4), 2, "double", 3),
    case("t8-205wg-S7-double", "tile8_205", (1024, 3), 7, "double", 3),
    case("t4-S3-double-stag", "tile4", (2100, 2), 3, "double", 2, True),
    case("t4-S5-reset", "tile4", (2100, 2), 5, "reset", 7),
    case("t4-S1-reset-stag", "tile4", (2100, 2), 1, "reset", 2, True),
    case("w1-S3-double-stag", "wave1", (300, 3), 3, "double", 2, True),
    case("w1-S5-short", "wave1_600", (600, 3), 5, "two_short", 3),
    case("w1-S2-reset-stag", "wave1_1024", (1024, 3), 2, "reset", 3, True),
    case("w2-S7-exact-stag", "wave2", (1300, 3), 7, "exact", 5, True),
    case("w2-S2-double", "wave2", (1300, 3), 2, "double", 2),
    case("w4-S1-reset", "wave4", (2600, 3), 1, "reset", 2),
    case("w4-S3-double-stag", "wave4", (2600, 3), 3, "double", 4, True),
    case("w1-S2-exact-generic-argmax", "wave1", (7, 3), 2, "exact", 3, True, generic=1, mode=2),
    # ... the same launch carrying the PPO update's permutation request (rollout_kernel<.., PERM>), and the record staged in HBM
    case("t8r-S5-reset-stag-prep", "tile8_ragged", (7, 3), 5, "reset", 3, True, prep=True),
    case("t8r-S3-double-prep", "tile8_ragged", (7, 3), 3, "double", 2, prep=True),
    case("t8r-S3-double-staged-record", "tile8_ragged", (7, 3), 3, "double", 2, True, stage=True),
    # ... on ignore_obs_next buffers
    case("t8r-S3-double-stag-ign", "tile8_ragged", (7, 3), 3, "double", 2, True, ign=True),
    case("w1-S5-reset-ign", "wave1", (300, 3), 5, "reset", 3, ign=True),
    case("t4-S2-double-ign", "tile4", (2100, 2), 2, "double", 3, True, ign=True),
    # ---- actor-only 128-wide rollout (csrc/rollout_rows.hip) ----
    case("aw-37x6-S3-double-stag", "actor_wave", (37, 6), 3, "double", 2, True, glob=False),
    case("aw-9x2-S1-double-glob", "actor_wave", (9, 2), 1, "double", 3, glob=True),
    case("aw-33x8-S7-exact-stag-glob", "actor_wave", (33, 8), 7, "exact", 4, True, glob=True),
    case("at-9x2-S5-short-stag", "actor_tile", (9, 2), 5, "two_short", 2, True, glob=False),
    case("at-21x4-S2-reset-glob", "actor_tile", (21, 4), 2, "reset", 3, glob=True),
    case("aw-9x2-S2-double-ign", "actor_wave", (9, 2), 2, "double", 3, glob=False, ign=True),
    case("at-9x2-S3-short-stag-ign", "actor_tile", (9, 2), 3, "two_short", 2, True, glob=True, ign=True),
    # ---- tag rollout (csrc/rollout_tag.hip) ----
    case("tag-9-S3-double-stag", "tag_teams", (9, 1, 1, 0), 3, "double", 2, True),
    case("tag-14-S1-double", "tag_teams", (14, 3, 2, 4), 1, "double", 2),
    case("tag-40-S5-reset-stag", "tag_teams", (40, 4, 2, 3), 5, "reset", 3, True),
    case("tag-64-S2-double-shared", "tag_shared", (64, 3, 1, 2), 2, "double", 3),
    case("tag-64-S7-short-shared-stag", "tag_shared", (64, 3, 1, 2), 7, "two_short", 5, True),
]


def _steps(c):
    return [o for o in c["ops"] if o != "reset"]


def _resets(c):
    """The steps before whose add the buffer is reset."""
    t, out = 0, []
    for o in c["ops"]:
        if o == "reset":
            out.append(t)
        else:
            t += o
    return out


def _predict(c):
    """From the case's definition alone: does a launch exceed S; the slots on which episodes end (lock-step: after every max_cycles
    steps; staggered: env e starts max_cycles - e % max_cycles steps from its first end)."""
    T, S, mc = sum(_steps(c)), c["S"], c["mc"]
    slots = rc.slot_of_step(T, S, _resets(c))
    phases = range(min(c["n_env"], mc)) if c["stagger"] else [0]
    ends = {int(slots[t]) for p in phases for t in range(T) if (t + 1 + p) % mc == 0}
    return dict(launch_gt_S=max(_steps(c)) > S, ends=ends, both_edges={0, S - 1} <= ends)


def _cycle_relation(c):
    S, mc = c["S"], c["mc"]
    out = {"smaller" if mc < S else "equal" if mc == S else "larger"}
    if np.gcd(S, mc) == 1 and S > 1 and mc > 1:
        out.add("coprime")
    return out


def test_every_axis_value_is_covered():
    assert {c["S"] for c in CASES} == set(SS) and {c["sched"] for c in CASES} == set(SCHEDULES)
    assert {c["form"] for c in CASES} == set(FORMS)
    assert set().union(*(_cycle_relation(c) for c in CASES)) == set(CYCLES)
    assert {c["stagger"] for c in CASES} == {False, True}
    assert len({c["id"] for c in CASES}) == len(CASES)
    for kind in ("spread", "actor", "tag"):   # every kernel: a launch longer than the ring, every S edge, both phases, a reset
        mine = [c for c in CASES if c["kind"] == kind]
        assert any(_predict(c)["launch_gt_S"] for c in mine) and {1, 2} <= {c["S"] for c in mine}, kind
        assert {c["stagger"] for c in mine} == {False, True} and any(c["sched"] == "reset" for c in mine), kind
        assert any(_predict(c)["both_edges"] and c["S"] > 1 for c in mine), kind
    spread = [c for c in CASES if c["kind"] == "spread"]
    assert {c["generic"] for c in spread} == {0, 1} and {c["mode"] for c in spread} == {1, 2}
    # every form of the spread and the actor-only rollout writes a slot twice in one launch somewhere
    assert {c["form"].split("_")[0] for c in CASES if _predict(c)["launch_gt_S"]} >= {"wave1", "wave2", "wave4", "tile8", "tile4", "actor", "tag"}
    assert {c["form"] for c in CASES if _predict(c)["launch_gt_S"]} >= {"actor_wave", "actor_tile", "tag_teams", "tag_shared"}
    assert {(c["form"], c["flags"].get("glob")) for c in CASES if c["kind"] == "actor"} >= {
        ("actor_wave", False), ("actor_wave", True), ("actor_tile", False), ("actor_tile", True)}
    ign = {c["form"].split("_")[0] for c in CASES if c["flags"].get("ign")}
    assert ign >= {"tile8", "tile4", "wave1", "actor"}
    assert any(c["flags"].get("prep") for c in CASES) and any(c["flags"].get("stage") for c in CASES)
    # the cycle relations over the run visit every slot with an episode end somewhere
    assert any(_predict(c)["ends"] == set(range(c["S"])) and c["S"] >= 3 for c in CASES)


# ---- the three runs ----
def _make(c, slots, fused, ign=False):
    """-> env, the policy object the collector drives, buffer, collector, per agent column the 64-wide net whose critic stored
    V(obs_next) (None: the kernel stores none)."""
    n_env, mc, fl = c["n_env"], c["mc"], c["flags"]
    if c["kind"] == "tag":
        _, n_adv, n_good, n_obst = c["shape"]
        env = DeviceSimpleTagVectorEnv(n_env, n_good, n_adv, n_obst, max_cycles=mc, device=DEV, seed=11)
        mk = lambda s: PPO(net=DiscreteActorCritic(env.obs_dim, 5, 64, device=DEV, seed=s), seed=s)  # noqa: E731
        if c["form"] == "tag_shared":
            pol = FlexibleMultiAgentPolicyManager(mk(21), env, mode="shared")
        else:
            pol = FlexibleMultiAgentPolicyManager({"adversaries": mk(21), "good": mk(22)}, env, mode="grouped",
                                                  agent_groups=env.agent_groups)
        critics = [pol.policy_map[a].net for a in env.agents]
    else:
        N = c["shape"][1]
        env = DeviceSimpleSpreadVectorEnv(n_env, N, max_cycles=mc, device=DEV, seed=SEED)
        if c["kind"] == "actor":
            glob = fl["glob"]
            net = MLPActorCritic(env.obs_dim, 5, (128, 128), critic_obs_dim=N * env.obs_dim if glob else None, device=DEV, seed=SEED)
            pol = GenericPPO(net=net, critic_input="global" if glob else "local", n_agent=N, seed=SEED, shuffle="numpy",
                             dispatch="pooled")
            critics = None
        else:
            net = DiscreteActorCritic(env.obs_dim, env.n_act, 64, device=DEV, seed=SEED)
            pol = PPO(net=net, seed=SEED, deterministic_eval=c["mode"] == 2)
            critics = [net] * N
    buf = DeviceVectorReplayBuffer(n_env * slots, n_env, env.n_agent, env.obs_dim, device=DEV, ignore_obs_next=ign)
    assert buf.sub_size == slots
    col = Collector(pol, env, buf, fused_rollout=fused, use_graph=False)
    col.reset()
    assert col._can_fuse() == fused
    if c["kind"] == "actor":
        assert col._can_fuse_actor() == fused
    if c["stagger"]:
        env.steps.copy_(torch.arange(n_env, device=DEV) % mc)
    return env, pol, buf, col, critics


def _bits(t):
    t = t.detach().clone()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _stats(st):
    return dict(returns=np.asarray(st.returns, np.float64).copy(), lens=np.asarray(st.lens).astype(np.int64),
                n=int(st.n_collected_episodes))


_STORES = dict(obs="obs_store", obs_next="obs_next_store", act="act_store", rew="rew_store", term="term_store", trunc="trunc_store",
               done="done_store", logp="logp_store", vs="vs_store", vnext="vnext_store")


def _snapshot(c, env, buf, collects):
    stores = {k: _bits(getattr(buf, a)) for k, a in _STORES.items() if getattr(buf, a) is not None}
    envs = {k: _bits(getattr(env, k)) for k in ("agent_pos", "agent_vel", "landmark_pos", "steps", "episode_ctr", "obs_cur", "rng_tick")}
    return dict(stores=stores, env=envs, collects=collects)


def _run(c, slots, fused, ign=False, ring=True, prep=False, stage=False, hook=None):
    """The case's schedule on one collector.  ring=False: the big run (never reset).  hook(col, n_iter, k): called before collect k."""
    env, pol, buf, col, critics = _make(c, slots, fused, ign)
    col.stage_episode_record = stage
    seen, perm = [], None
    if prep:   # a hand-made request, as tests/test_gpu_rollout_prep.py hands one over: 3 permutations of 75 entries
        perm = dict(out=torch.full((3, 75), -1, dtype=torch.int64, device=DEV), ctr=torch.tensor([12345], dtype=torch.int64, device=DEV))
        req = dict(out=perm["out"], n=75, n_perm=3, seed=SEED ^ 0x5DEECE66D, counter_dev=perm["ctr"], scale=3, group_size=1, offset_mul=1)
        pol.rollout_prep_request = lambda b: dict(req, gen=len(seen), key=None)
        pol.rollout_prep_done = lambda r, taken: seen.append(taken)
    collects = []
    ctx = policy_within_training_step(pol) if c["mode"] == 1 else contextlib.nullcontext()
    with ctx, ops.kernel_override(rollout_form=c["rollout_form"], generic_kernels=c["generic"]):
        for op in c["ops"]:
            if op == "reset":
                if ring:
                    col.reset_buffer(keep_statistics=True)
                continue
            if hook is not None:
                hook(col, op, len(collects))
            st = col.collect(n_step=c["n_env"] * op)
            ws = col._device_ws(op)
            collects.append(dict(_stats(st), state=buf.index.state.clone(), ptr=ws["ptr"].clone(), ep_idx=ws["ep_idx"].clone(),
                                 ep_len=ws["ep_len"].clone(), ep_rew=_bits(ws["ep_rew"])))
        torch.cuda.synchronize()
        if prep:
            assert seen == [True] * len(collects)   # every launch took the request: the PERM instantiation ran
            want = ops.random_permutations(75, 3, SEED ^ 0x5DEECE66D, counter_dev=perm["ctr"], scale=3, group_size=1, offset_mul=1)
            assert torch.equal(perm["out"], want)
    return _snapshot(c, env, buf, collects), env, buf, critics


def _truth(c, big, buf, critics, T):
    """Time-ordered rows [T][n_env]... of every stored field (bit patterns), done flags and float32 rewards."""
    rows = {k: v[:T].cpu().numpy() for k, v in big["stores"].items() if k != "vnext"}
    if critics is not None:   # V(obs_next): the column's own critic over the row's obs_next, as the kernels store it (a2c.py:124)
        vn = torch.zeros(T, c["n_env"], len(critics), device=DEV)
        with ops.kernel_override(generic_kernels=c["generic"]):
            for a, net in enumerate(critics):
                x = buf.obs_next_store[:T, :, a].reshape(-1, buf.obs_dim).contiguous()
                vn[:, :, a] = ops.policy_forward(net.flat.data, x, 5, 64, mode="none")["value"].reshape(T, c["n_env"])
        rows["vnext"] = _bits(vn).cpu().numpy()
    done = big["stores"]["done"][:T].cpu().numpy().astype(bool)
    rew = buf.rew_store[:T].cpu().numpy()
    return rows, done, rew


def _written(c, fused, ign):
    """The stores a path writes.  Unfused: everything but V(obs_next); the actor-only rollout: neither V(obs) nor V(obs_next)."""
    keys = set(_STORES) - ({"obs_next"} if ign else set())
    if not fused:
        return keys - {"vnext"}
    return keys - ({"vs", "vnext"} if c["kind"] == "actor" else set())


def _check_against_truth(c, tag, run, fused, ign, rows, done, rew, check_env=None):
    S, resets, steps = c["S"], _resets(c), _steps(c)
    for k in sorted(_written(c, fused, ign)):
        want = rc.expected_ring(rows[k], S, resets, init=0)
        assert np.array_equal(run["stores"][k].cpu().numpy(), want), (tag, k)
    t0 = 0
    exp = rc.expected_index(done, rew, S, resets)
    for k, (n, col) in enumerate(zip(steps, run["collects"])):
        t1 = t0 + n
        pre = rc.expected_index(done[:t1], rew[:t1], S, [r for r in resets if r < t1])
        assert np.array_equal(col["state"].cpu().numpy(), rc.pack_state(pre["state"])), (tag, "state", k)
        for f in ("ptr", "ep_idx", "ep_len"):
            assert np.array_equal(col[f].cpu().numpy(), exp[f][t0:t1]), (tag, f, k)
        assert np.array_equal(col["ep_rew"].cpu().numpy(), exp["ep_rew"][t0:t1].view(np.int64)), (tag, "ep_rew", k)
        lens, rets = rc.episodes_between(exp, t0, t1)
        assert col["n"] == len(lens) and np.array_equal(col["lens"], lens), (tag, "lens", k)
        if len(lens):
            assert np.array_equal(col["returns"].view(np.int64), rets.view(np.int64)), (tag, "returns", k)
        t0 = t1
    return exp


def _check_same(tag, a, b, keys=None):
    for k in sorted(keys if keys is not None else a["stores"].keys() & b["stores"].keys()):
        assert torch.equal(a["stores"][k], b["stores"][k]), (tag, k)
    for k in a["env"]:
        assert torch.equal(a["env"][k], b["env"][k]), (tag, k)
    assert len(a["collects"]) == len(b["collects"])
    for i, (x, y) in enumerate(zip(a["collects"], b["collects"])):
        for f in ("state", "ptr", "ep_idx", "ep_len", "ep_rew"):
            assert torch.equal(x[f], y[f]), (tag, f, i)
        assert x["n"] == y["n"] and np.array_equal(x["lens"], y["lens"]), (tag, "lens", i)
        assert x["returns"].shape == y["returns"].shape and np.array_equal(x["returns"].view(np.int64), y["returns"].view(np.int64)), (tag, "returns", i)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_wrapped_ring_holds_the_unfused_bits_and_the_expected_rows(c):
    S, steps, fl = c["S"], _steps(c), c["flags"]
    T, ign = sum(steps), bool(fl.get("ign"))
    big, _, big_buf, critics = _run(c, T, False, ring=False)
    rows, done, rew = _truth(c, big, big_buf, critics, T)
    unf, _, _, _ = _run(c, S, False, ign=ign)
    fus, _, fbuf, _ = _run(c, S, True, ign=ign, prep=bool(fl.get("prep")), stage=bool(fl.get("stage")))
    # (a) the persistent launch against the unfused adds
    _check_same("fused vs unfused", fus, unf, keys=_written(c, True, ign) & _written(c, False, ign))
    for k in big["env"]:   # ... and the env state does not depend on the buffer
        assert torch.equal(big["env"][k], fus["env"][k]), k
    # (b) both against the numpy expectations from the big run
    _check_against_truth(c, "unfused", unf, False, ign, rows, done, rew)
    exp = _check_against_truth(c, "fused", fus, True, ign, rows, done, rew)
    if ign:
        # stores other than obs_next: bit-identical to the full-buffer persistent run; obs_next is READ as obs[next(index)]
        full, _, _, _ = _run(c, S, True)
        _check_same("ignore_obs_next vs full buffer", fus, full, keys=_written(c, True, True))
        assert fbuf.obs_next_store is None
        idx = np.arange(c["n_env"] * S)
        got = fbuf[idx]
        st = exp["state"]
        nxt = rc.expected_next(rc.expected_ring(done, S, _resets(c)), st["last_index"], st["lengths"], S)
        assert np.array_equal(fbuf.next(idx), nxt)
        obs_flat = rc.expected_ring(rows["obs"], S, _resets(c)).transpose(1, 0, 2, 3).reshape(len(idx), *rows["obs"].shape[2:])
        assert np.array_equal(got.obs.view(np.int32), obs_flat) and np.array_equal(got.obs_next.view(np.int32), obs_flat[nxt])
    # (c) the case exercised what it claims
    pred = _predict(c)
    assert T > S
    assert (max(steps) > S) == pred["launch_gt_S"]
    end_slots = {int(s) for s in np.unique((exp["ptr"] % S)[done])}
    assert end_slots == pred["ends"]
    if pred["both_edges"]:
        assert {0, S - 1} <= end_slots
    for run in (unf, fus):
        assert all(int(col["state"][-1]) == 0 for col in run["collects"])


# ---- the compact episode record at its limits ----
def _record_case(kind):
    # max_cycles 2, 7 steps from phase 0: every env finishes 3 episodes (steps 1, 3, 5) in one launch; S = 3: the ring wraps twice;
    # a second collect of 7 steps follows on a fresh collector
    if kind == "spread":
        return case("rec-spread", "tile8_ragged", (7, 3), 3, "double", 2)
    return case("rec-tag", "tag_teams", (9, 1, 1, 0), 3, "double", 2)


def _record_run(c, slots, fused, max_ep=None, ring=True):
    """collect 7 (the record preset to max_ep entries per env) -> a fresh collector with the default record -> collect 7."""
    env, pol, buf, col, critics = _make(c, slots, fused)
    out = dict(collects=[], rec=None, error=None)

    def snap(st, col_, n):
        ws = col_._device_ws(n)
        out["collects"].append(dict(({} if st is None else _stats(st)), state=buf.index.state.clone(), ptr=ws["ptr"].clone(),
                                    ep_idx=ws["ep_idx"].clone(), ep_len=ws["ep_len"].clone(), ep_rew=_bits(ws["ep_rew"])))

    with policy_within_training_step(pol), ops.kernel_override(rollout_form=c["rollout_form"]):
        if max_ep is not None:
            col._device_ws(7)["max_ep"] = max_ep   # (the collector computes it only when absent)
        try:
            st = col.collect(n_step=c["n_env"] * 7)
        except RuntimeError as e:   # reading the statistics (collect() resolves them) found the record overflowed
            st, out["error"] = None, str(e)
        torch.cuda.synchronize()
        if fused:
            out["rec"] = col._device_ws(7)["last_slot"]["rec_h"].numpy().copy()
        snap(st, col, 7)
        col2 = Collector(pol, env, buf, fused_rollout=fused, use_graph=False)
        col2.reset(reset_buffer=False)
        st2 = col2.collect(n_step=c["n_env"] * 7)
        if fused:
            assert col2._device_ws(7)["max_ep"] == 7 // 2 + 2
        snap(st2, col2, 7)
        torch.cuda.synchronize()
    out.update(_snapshot(c, env, buf, out["collects"]))
    return out, buf, critics


@pytest.mark.parametrize("kind", ["spread", "tag"])
@pytest.mark.parametrize("max_ep", [3, 2, 1])
def test_compact_episode_record_at_and_beyond_its_capacity(kind, max_ep):
    """3 episodes per env in one launch against a record of 3 (exactly full: no error, every entry right), 2 and 1 entries per env
    (reading the statistics raises the RuntimeError that names the record size; the count words still read 3, the first max_ep
    entries are still the right ones, and the rollout itself -- every store, the index state, the env, the per-step outputs, the
    next collect on a fresh collector -- is what the unfused run leaves)."""
    c = _record_case(kind)
    E, S, T = c["n_env"], c["S"], 14
    big, big_buf, critics = _record_run(c, T, False)
    rows, done, rew = _truth(c, big, big_buf, critics, T)
    unf, _, _ = _record_run(c, S, False)
    fus, _, _ = _record_run(c, S, True, max_ep=max_ep)
    assert unf["error"] is None and np.array_equal(done[:7].sum(0), np.full(E, 3))
    if max_ep >= 3:
        assert fus["error"] is None
    else:
        assert fus["error"] is not None and f"the episode record holds {max_ep}" in fus["error"] and "finished 3 episodes" in fus["error"]
    exp = rc.expected_index(done, rew, S)
    # the record itself: [E] count | [E][max_ep] step << 32 | length | [E][max_ep][N] f64 return
    N = rew.shape[2]
    rec = fus["rec"]
    assert len(rec) == E * (1 + max_ep * (1 + N))
    assert np.array_equal(rec[:E], np.full(E, 3))
    key = rec[E:E + E * max_ep].reshape(E, max_ep)
    ret = rec[E + E * max_ep:].reshape(E, max_ep, N)
    for e in range(E):
        mine = (exp["env"] == e) & (exp["step"] < 7)
        assert mine.sum() == 3
        assert np.array_equal(key[e] >> 32, exp["step"][mine][:max_ep]), e
        assert np.array_equal(key[e] & 0xFFFFFFFF, exp["lens"][mine][:max_ep]), e
        assert np.array_equal(ret[e], exp["returns"][mine][:max_ep].view(np.int64)), e
    # an overflowing record does not disturb the rollout: stores, index state, env, per-step outputs, the next collect
    keys = _written(c, True, False) & _written(c, False, False)
    for k in sorted(keys):
        assert torch.equal(fus["stores"][k], unf["stores"][k]), k
    for k in fus["env"]:
        assert torch.equal(fus["env"][k], unf["env"][k]) and torch.equal(fus["env"][k], big["env"][k]), k
    for tag, run, written in (("unfused", unf, _written(c, False, False)), ("fused", fus, _written(c, True, False))):
        for k in sorted(written):
            assert np.array_equal(run["stores"][k].cpu().numpy(), rc.expected_ring(rows[k], S)), (tag, k)
        for i, col in enumerate(run["collects"]):
            t0, t1 = 7 * i, 7 * i + 7
            assert np.array_equal(col["state"].cpu().numpy(), rc.pack_state(rc.expected_index(done[:t1], rew[:t1], S)["state"])), (tag, i)
            for f in ("ptr", "ep_idx", "ep_len"):
                assert np.array_equal(col[f].cpu().numpy(), exp[f][t0:t1]), (tag, f, i)
            assert np.array_equal(col["ep_rew"].cpu().numpy(), exp["ep_rew"][t0:t1].view(np.int64)), (tag, i)
            if "lens" in col:   # (the overflowed collect has no statistics)
                lens, rets = rc.episodes_between(exp, t0, t1)
                assert col["n"] == len(lens) and np.array_equal(col["lens"], lens), (tag, i)
                assert np.array_equal(col["returns"].view(np.int64), rets.view(np.int64)), (tag, i)
    assert ("lens" in fus["collects"][0]) == (max_ep >= 3) and "lens" in fus["collects"][1]
