"""GPU tests (`-m gpu`) of the simple_spread / simple_tag step kernels (csrc/mpe.hip, csrc/mpe_tag.hip, mpe_dev.h, mpe_tag_dev.h)
at their edges: pairs placed on the force cutoff and the contact threshold, contact decisions either side of the +-1 % sqrt band,
every piece of the boundary penalty, the speed clamp of either team and of spread's config struct, local_ratio, crowded worlds at
the size limits and at n_env around the 16 envs a workgroup stages, and an auto-reset that only some envs of a workgroup take.
Cases, inputs and float64 yardsticks: tests/env_cases.py (tests/test_host_env_shapes.py checks their promises on the CPU).

Every case writes its state into env.agent_pos / agent_vel / landmark_pos / steps / episode_ctr, sets its overrides on the env's
config struct, takes ONE step_device and reads everything back; a twin env does the same and must give the same bits.  Bars:
  * new position and velocity (from env.agent_pos / agent_vel, or from obs_next[..., 0:4] where a reset has overwritten them):
    the single-step bar of test_gpu_pipeline.py / test_gpu_tag.py, |got - ref64| <= 2e-5 (1 + |ref64|), against the oracle;
  * observations: exact, as int32 views, against numpy float32 subtraction of the device's own post-step state in the documented
    layout (zero padding and the silent communication channel included) -- obs_next always, obs_cur where no reset happened;
  * rewards: contact counts exact -- in crafted cases without exclusion, in random worlds leaving out only the decisions the oracle
    finds within 1e-5 of a threshold (their share held to the 1 % cap); the continuous parts at 2e-5 of the reward's scale;
    tag adversaries all carry the same bits;
  * beyond the force cutoff, for idle lattice agents and where the clamp is not taken: bit-equal to a float32 evaluation of the
    no-force step (env_cases.no_force_variants); a pair at rest inside the cutoff: its velocity within 1e-3 relative of the
    oracle's wherever float32 can hold it (env_cases.REST_REL);
  * truncated / terminated / done_env / steps / episode_ctr: exact; a finishing env's new state and obs_cur equal, bit for bit, a
    twin env on which reset_device(ids) was called at that episode number.
Every case prints a `PARITY env ...` line with its worst ratio to the bar (profiles/env_parity.txt holds one run's)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import env_cases as ec  # noqa: E402
from test_gpu_offpolicy_shapes import _same_bits  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.ppo import policy_within_training_step
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.env.mpe_tag import DeviceSimpleTagVectorEnv


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _exact(name, what, got, ref):
    got, ref = _bits(got), _bits(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.argwhere(got != ref)
    if len(bad):
        print(f"PARITY env {name} {what}: DIFFERS at {bad[:6].tolist()} ({len(bad)} of {got.size} entries)")
    assert not len(bad), (name, what, bad[:6].tolist())


def _make_env(c):
    if c["kind"] == "spread":
        env = DeviceSimpleSpreadVectorEnv(c["n_env"], c["sizes"][0], max_cycles=c["max_cycles"], device=DEV, seed=ec.SEED,
                                          auto_reset=c["auto_reset"])
        cfg = env._cfg
    else:
        na, ng, no = c["sizes"]
        env = DeviceSimpleTagVectorEnv(c["n_env"], ng, na, no, max_cycles=c["max_cycles"], device=DEV, seed=ec.SEED,
                                       auto_reset=c["auto_reset"])
        cfg = env._tag_cfg
    for k, v in c["cfg"].items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return env


def _load(env, c, counters=True):
    NL = ec.n_landmarks(c)
    env.agent_pos.copy_(_t(c["apos"]))
    env.agent_vel.copy_(_t(c["avel"]))
    if NL:
        env.landmark_pos[:, :NL].copy_(_t(c["lpos"]))
    if counters:
        env.steps.copy_(_t(c["steps"]))
        env.episode_ctr.copy_(_t(c["episode"]))


def _step(c):
    """One step of the case on two envs: the same bits; everything read back as numpy."""
    outs = []
    for _ in range(2):
        env = _make_env(c)
        _load(env, c)
        obs_next, rew, term, trunc, done = env.step_device(_t(c["act"]))
        outs.append(dict(obs_next=obs_next, obs_cur=env.obs_cur, rew=rew, term=term, trunc=trunc, done=done, apos=env.agent_pos,
                         avel=env.agent_vel, lpos=env.landmark_pos, steps=env.steps, ep=env.episode_ctr, tick=env.rng_tick))
    _same_bits(f"env {c['name']}", outs[0], outs[1])
    return {k: v.cpu().numpy() for k, v in outs[0].items()}


def _check(c, o, exclude=False):
    """The bars every case is held to.  Returns the device's post-step (pos, vel) and the mask of finishing envs that were reset."""
    name, r = c["name"], ec.reference(c)
    E, NA, NL = c["n_env"], ec.n_agents(c), ec.n_landmarks(c)
    # flags and counters
    tr = c["steps"] + 1 >= c["max_cycles"]
    fin = tr & c["auto_reset"]
    assert np.array_equal(tr, r["trunc"])
    _exact(name, "truncated", o["trunc"], np.repeat(tr[:, None], NA, 1).astype(np.uint8))
    _exact(name, "terminated", o["term"], np.zeros((E, NA), np.uint8))
    _exact(name, "done_env", o["done"], tr.astype(np.uint8))
    _exact(name, "steps", o["steps"], np.where(fin, 0, c["steps"] + 1).astype(np.int32))
    _exact(name, "episode_ctr", o["ep"], c["episode"] + fin)
    assert int(o["tick"][0]) == 0
    # new state: against the oracle at the single-step bar
    pos = np.where(fin[:, None, None], o["obs_next"][..., 2:4], o["apos"])
    vel = np.where(fin[:, None, None], o["obs_next"][..., 0:2], o["avel"])
    ratio = {k: float(np.max(np.abs(g.astype(np.float64) - r[k]) / (ec.BAR * (1 + np.abs(r[k])))))
             for k, g in (("apos", pos), ("avel", vel))}
    # observations: exact
    lay = ec.obs_layout(c, pos, vel, c["lpos"])
    _exact(name, "obs_next", o["obs_next"], lay)
    _exact(name, "obs_cur (no reset)", o["obs_cur"][~fin], lay[~fin])
    if NL:
        _exact(name, "landmarks (no reset)", o["lpos"][~fin][:, :NL], c["lpos"][~fin])
    if fin.any():  # the finishing envs: a twin env reset for those ids at that episode number
        ids = np.flatnonzero(fin)
        twin = _make_env(c)
        twin.steps.fill_(7)
        twin.episode_ctr.copy_(_t(c["episode"]))
        obs = twin.reset_device(_t(ids)).cpu().numpy()
        _exact(name, "reset obs_cur", o["obs_cur"][ids], obs[ids])
        _exact(name, "reset agent_pos", o["apos"][ids], twin.agent_pos.cpu().numpy()[ids])
        _exact(name, "reset agent_vel", o["avel"][ids], np.zeros((len(ids), NA, 2), np.float32))
        _exact(name, "reset landmarks", o["lpos"][ids], twin.landmark_pos.cpu().numpy()[ids])
        _exact(name, "reset episode_ctr", o["ep"][ids], twin.episode_ctr.cpu().numpy()[ids])
        assert (twin.steps.cpu().numpy()[ids] == 0).all() and not np.array_equal(_bits(o["obs_cur"][ids]), _bits(o["obs_next"][ids]))
    # rewards
    mask, share = ec.excluded(c, r)
    assert share <= ec.CAP and (exclude or not mask.any()), (name, share)
    keep = ~mask
    rew = o["rew"].astype(np.float64)
    err = np.abs(rew - r["rew"]) / (ec.BAR * (1 + np.abs(r["rew"])))
    ratio["rew"] = float(err[keep].max()) if keep.any() else 0.0
    if c["kind"] == "spread":
        lr = c["cfg"].get("local_ratio", 0.5)
        if lr > 0:
            count = -np.rint((rew - r["glob"][:, None] * (1 - lr)) / lr)
            _exact(name, "collision counts", count[keep], r["count"][keep].astype(np.float64))
    else:
        na = c["sizes"][0]
        touch = np.rint((-rew[:, na:] - r["bound"]) / 10)
        _exact(name, "touches per good agent", touch[keep[:, na:]], r["touch"][keep[:, na:]].astype(np.float64))
        _exact(name, "adversaries share one reward", o["rew"][:, :na], np.repeat(o["rew"][:, :1], na, 1))
        _exact(name, "catches", o["rew"][:, 0][keep[:, 0]], (10.0 * r["total"][keep[:, 0]]).astype(np.float32))
    print(f"PARITY env {name}: E {E}, ratio to the 2e-5 bar: pos {ratio['apos']:.3g}, vel {ratio['avel']:.3g}, rew {ratio['rew']:.3g}; "
          f"close decisions excluded {share:.4f} (cap {ec.CAP}); obs / flags / counts exact")
    assert max(ratio.values()) <= 1.0, (name, ratio)
    return pos, vel, fin


def _check_no_force(c, pos, vel, mask, what):
    """Bit-equal to one float32 evaluation of the no-force step on every agent of `mask` [E, NA]."""
    if not mask.any():
        return
    hits = [bool(np.array_equal(_bits(pos[mask]), _bits(p[mask])) and np.array_equal(_bits(vel[mask]), _bits(v[mask])))
            for p, v in ec.no_force_variants(c)]
    print(f"PARITY env {c['name']} no-force ({what}): {int(mask.sum())} agents, float32 evaluations matched: {hits}")
    assert any(hits), (c["name"], what)


def _idle_mask(c):
    mask = np.zeros((c["n_env"], ec.n_agents(c)), bool)
    mask[:, ec.idle_agents(c)] = True
    return mask


# ---- crafted families --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.PAIR_CASES, ids=ec.case_id)
def test_pair_forces(c):
    o = _step(c)
    pos, vel, _ = _check(c, o)
    m, r, NA = c["meta"], ec.reference(c), ec.n_agents(c)
    mask = _idle_mask(c) | m["beyond"][:, None]
    _check_no_force(c, pos, vel, mask, "beyond the cutoff and idle")
    # at rest under noop the velocity is the contact force's alone: relative, wherever float32 holds it
    worst = 0.0
    for i in [k for k in m["pair"] if k < NA]:
        ref, got = r["avel"][m["rest"], i], vel[m["rest"], i].astype(np.float64)
        big = np.abs(ref) >= ec.REST_MIN
        worst = max(worst, float(np.max(np.abs(got[big] - ref[big]) / np.abs(ref[big]))))
        assert (np.abs(got[~big]) <= ec.REST_MIN).all()
    print(f"PARITY env {c['name']} at rest: max relative velocity error {worst:.3g} (bar {ec.REST_REL})")
    assert worst <= ec.REST_REL


@pytest.mark.parametrize("c", ec.CONTACT_CASES, ids=ec.case_id)
def test_contact_decisions(c):
    pos, vel, _ = _check(c, _step(c))
    _check_no_force(c, pos, vel, _idle_mask(c), "idle")


@pytest.mark.parametrize("c", ec.BOUNDARY_CASES, ids=ec.case_id)
def test_boundary_penalty(c):
    pos, vel, _ = _check(c, _step(c))
    _exact(c["name"], "post == pre", pos, c["apos"])
    _exact(c["name"], "at rest", vel, np.zeros_like(vel))


@pytest.mark.parametrize("c", ec.CLAMP_CASES, ids=ec.case_id)
def test_speed_clamp(c):
    pos, vel, _ = _check(c, _step(c))
    taken = ec.unclamped_speed(c) > ec.vmax_of(c)
    if c["name"] == "clamp-spread-default":
        assert not taken.any() and np.linalg.norm(vel.astype(np.float64), axis=-1).max() > 3.7     # v = 5 passes unclamped
    else:
        speed = np.linalg.norm(vel.astype(np.float64), axis=-1)
        lim = np.broadcast_to(ec.vmax_of(c), speed.shape)
        assert taken.any() and np.abs(speed[taken] / lim[taken] - 1).max() <= ec.BAR
    _check_no_force(c, pos, vel, ~taken, "clamp not taken")


# ---- random worlds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.RATIO_CASES, ids=ec.case_id)
def test_local_ratio(c):
    _check(c, _step(c), exclude=True)


@pytest.mark.parametrize("c", ec.CROWDED_CASES, ids=ec.case_id)
def test_crowded_worlds(c):
    _check(c, _step(c), exclude=True)


@pytest.mark.parametrize("c", ec.RESET_CASES, ids=ec.case_id)
def test_partial_auto_reset(c):
    o = _step(c)
    _, _, fin = _check(c, o, exclude=True)
    assert np.array_equal(np.flatnonzero(o["done"]), np.array(ec.FINISHING))
    assert np.array_equal(np.flatnonzero(fin), np.array(ec.FINISHING) if c["auto_reset"] else np.zeros(0, int))
    if not c["auto_reset"]:   # nothing is re-drawn and steps counts on
        assert (o["steps"][list(ec.FINISHING)] == c["max_cycles"]).all() and np.array_equal(o["ep"], c["episode"])
        _exact(c["name"], "obs_cur == obs_next", o["obs_cur"], o["obs_next"])


# ---- the fused rollouts from the same states -----------------------------------------------------------------------------------------
def _start_from(env, c):
    """Behind the collector's reset: the case's crowded state in the env, the matching observation in obs_cur."""
    _load(env, c, counters=False)
    env.obs_cur.copy_(_t(ec.obs_layout(c, c["apos"], c["avel"], c["lpos"])))


def _collected(env, buf, st, stores):
    d = {k: getattr(buf, k + "_store").clone() for k in stores}
    d.update(state=buf.index.state.clone(), apos=env.agent_pos.clone(), avel=env.agent_vel.clone(), lpos=env.landmark_pos.clone(),
             steps=env.steps.clone(), ep=env.episode_ctr.clone(), obs_cur=env.obs_cur.clone(), tick=env.rng_tick.clone(),
             ret=st.returns, lens=st.lens, n=st.n_collected_episodes)
    return d


def _same_collects(name, a, b):
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), (name, k)
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (name, k)
        else:
            assert a[k] == b[k], (name, k)
    print(f"PARITY env {name}: fused == unfused over 3 steps, {len(a)} outputs, bit for bit")


STORES = ("obs", "obs_next", "act", "rew", "trunc", "term", "logp", "done")


@pytest.mark.parametrize("form", ["wave", "tile"])
@pytest.mark.parametrize("net", ["ppo64", "actor128"])
@pytest.mark.parametrize("c", ec.ROLLOUT_SPREAD, ids=ec.case_id)
def test_fused_spread_rollouts_from_crowded_states(c, net, form):
    """csrc/rollout.hip (ppo64) and csrc/rollout_rows.hip (actor128), both forms, evaluate the pair forces on other threads
    (mpe_pair_tasks / mpe_pair_fold): from a dense multi-contact state they must give the unfused step's bits.  Episodes of two
    steps: the third step starts from re-drawn worlds."""
    from test_gpu_rollout import _job, _job128

    outs = []
    for fused in (False, True):
        if net == "ppo64":
            env, _, algo, buf, col = _job(c["n_env"], c["sizes"][0], 2, fused, slots=4)
        else:
            env, _, algo, buf, col = _job128(c["n_env"], c["sizes"][0], 2, fused, False, slots=4)
        assert col._can_fuse() == fused
        _start_from(env, c)
        with policy_within_training_step(algo), ops.kernel_override(rollout_form=1 if form == "tile" else 2):
            st = col.collect(n_step=c["n_env"] * 3)
        outs.append(_collected(env, buf, st, STORES + (("vs",) if net == "ppo64" else ())))
    assert outs[0]["n"] == c["n_env"] and (outs[0]["rew"][:2] != 0).any()
    _same_collects(f"{c['name']} rollout {net} {form}", *outs)


@pytest.mark.parametrize("c", ec.ROLLOUT_TAG, ids=ec.case_id)
def test_fused_tag_rollout_from_crowded_states(c):
    """csrc/rollout_tag.hip, phase D: the pair forces of a step spread over threads, on dense multi-contact states."""
    from test_gpu_tag import _tag_job

    outs = []
    for fused in (False, True):
        env, mgr, buf, col = _tag_job(c["n_env"], *c["sizes"], 2, fused, 4)
        assert col._can_fuse() == fused
        _start_from(env, c)
        with policy_within_training_step(mgr):
            st = col.collect(n_step=c["n_env"] * 3)
        outs.append(_collected(env, buf, st, STORES + ("vs",)))
    assert outs[0]["n"] == c["n_env"]
    _same_collects(f"{c['name']} rollout tag", *outs)
