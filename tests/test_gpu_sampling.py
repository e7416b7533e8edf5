"""GPU tests (`-m gpu`): every device sampling site against tests/sampling_restatement.py, the float64 / integer restatement of
what its kernel is documented to draw (tests/test_host_sampling.py pins the Philox underneath to the Random123 known answers).

Common edges: seeds 0, 0x1234ABCD5678 and one with bit 63 set; host offsets 0, 2^32 - 3 (the rows of one call cross the carry into
the high counter word) and 2^40 + 5 split between the host offset and a device counter; rows 1, 255, 256, 257, 1000.

Bars
  bit for bit   permutations, IQN fractions, QMIX and DQN actions, PER indices, simple_spread's positions
  2^-23         simple_tag's positions: lo + (hi - lo) u is one rounding of the product and one of the sum at magnitude <= 1,
                or one of an fma
  test_gpu_distq.py's `_bar`   the normals (tsm_cac_normal, tsm_maddpg_act): max |hip - ref64| <= 1e-5 max |ref64| + e_ref, e_ref the
                float32-against-float64 difference of the restatement itself
  categorical   actions exact and logp within rtol 1e-5 / atol 1e-6 on every row whose u is further than 8 A 2^-24 s from every
                partial sum of the float64 CDF; the rows left out are at most 1 %
Every comparison prints `PARITY ...`."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import sampling_restatement as sr  # noqa: E402
from philox_restatement import M64, philox4, u01  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_gpu_dqn import _d  # noqa: E402
from test_host_sampling import COMMON, ROWS, categorical_cases, categorical_share  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.ppo import PPO, policy_within_training_step
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.env.mpe_tag import DeviceSimpleTagVectorEnv
    from tianshou_marl_amd.utils.net import DiscreteActorCritic


def _ctr_dev(v):
    """A device counter holding v (u64 on the ABI), or None."""
    if v is None:
        return None
    v = int(v) & M64
    return torch.tensor([v - 2**64 if v >= 2**63 else v], dtype=torch.int64, device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _exact(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    bad = int((got != ref).sum())
    print(f"PARITY {name}: {bad} of {ref.size} differ (bit for bit)")
    assert got.shape == ref.shape and bad == 0, (name, bad)


# ---- categorical ---------------------------------------------------------------------------------------------------------------
def _categorical_check(name, lg, act, logp, seed, off, dev):
    """-> the share of rows left out."""
    d, _ = sr.categorical_sample(lg, seed, off, offset_dev=dev)
    ok = ~d["ambiguous"]
    share = categorical_share(d)
    bad = int((np.asarray(act)[ok] != d["act"][ok]).sum())
    print(f"PARITY {name}: {bad} of {int(ok.sum())} actions differ; excluded share = {share:.3g}")
    assert share <= 0.01 and bad == 0, (name, share, bad)
    if logp is not None:
        np.testing.assert_allclose(np.asarray(logp, np.float64)[ok], d["logp"][ok], rtol=1e-5, atol=1e-6)
    return share


def test_categorical_sample_matches_the_restatement():
    worst = 0.0
    for name, lg in categorical_cases().items():
        for seed, off, dev in COMMON:
            act, logp = ops.categorical_sample(_d(lg), seed, offset=off, offset_dev=_ctr_dev(dev))
            worst = max(worst, _categorical_check(f"categorical {name} seed {seed:#x}", lg, _np(act), _np(logp), seed, off, dev))
    print(f"PARITY categorical: worst excluded share = {worst:.3g}")
    lg = categorical_cases()["A5_B257"]
    act, _ = ops.categorical_sample(_d(lg), 3, offset=7, deterministic=True)
    _exact("categorical mode", _np(act), sr.categorical_sample(lg, 3, 7, deterministic=True)[0]["act"])


@pytest.mark.parametrize("B", [1, 257, 1000])
def test_fused_sampled_forward_matches_the_restatement_on_its_own_logits(B):
    """csrc/mlp_fused.hip, mode "sample": the launch yields its logits; the draw is the categorical site's."""
    net = DiscreteActorCritic(18, 5, 64, device=DEV, seed=5)
    obs = _d(np.random.RandomState(B).standard_normal((B, 18)).astype(np.float32))
    for seed, off, dev in COMMON:
        o = ops.policy_forward(net.flat.data, obs, 5, 64, mode="sample", seed=seed, offset=off, offset_dev=_ctr_dev(dev))
        _categorical_check(f"fused forward B{B} seed {seed:#x}", _np(o["logits"]), _np(o["act"]), _np(o["logp"]), seed, off, dev)


@pytest.mark.parametrize("form", ["wave", "tile"])
def test_persistent_rollout_steps_match_the_restatement(form):
    """csrc/rollout.hip: row e N + i of step t draws at counter (policy counter) + (device tick) + t E N + row.  The rollout
    yields no logits: they are the unfused forward's on the stored observations (bit for bit the rollout's own,
    tests/test_gpu_rollout.py)."""
    E, N, T, seed = 21, 3, 2, 0x8000000000000003
    env = DeviceSimpleSpreadVectorEnv(E, N, max_cycles=25, device=DEV, seed=11)
    net = DiscreteActorCritic(env.obs_dim, env.n_act, 64, device=DEV, seed=5)
    algo = PPO(net=net, seed=seed)
    buf = DeviceVectorReplayBuffer(E * (T + 1), E, N, env.obs_dim, device=DEV)
    col = Collector(algo, env, buf, fused_rollout=True, use_graph=False)
    col.reset()
    assert col._can_fuse()
    ctr0, tick0 = int(algo._sample_ctr), int(env.rng_tick.item())
    with policy_within_training_step(algo), ops.kernel_override(rollout_form=1 if form == "tile" else 2):
        col.collect(n_step=E * T)
    assert int(env.rng_tick.item()) == tick0 + T * E * N
    for t in range(T):
        o = ops.policy_forward(net.flat.data, buf.obs_store[t].reshape(E * N, env.obs_dim), 5, 64, mode="none")
        _categorical_check(f"rollout ({form}) step {t}", _np(o["logits"]), _np(buf.act_store[t]).reshape(-1),
                           _np(buf.logp_store[t]).reshape(-1), seed, ctr0 + tick0 + t * E * N, None)


# ---- permutations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 256, 257, 1000])
def test_random_permutations_match_the_restatement(n):
    kw = dict(scale=3, group_size=2, offset_mul=7)
    for seed, off, dev in COMMON:
        ref, _ = sr.random_permutations(n, 3, seed, off, dev, **kw)
        got = ops.random_permutations(n, 3, seed, counter=off, counter_dev=_ctr_dev(dev), device=DEV, **kw)
        _exact(f"permutations n{n} seed {seed:#x}", _np(got), ref)
        # the form that advances the device counter itself: the same draws at *counter_dev, then the counter moves on
        total = (off + (dev or 0)) & M64
        ctr, done = _ctr_dev(total), torch.zeros(1, dtype=torch.int32, device=DEV)
        got = ops.random_permutations(n, 3, seed, counter_dev=ctr, device=DEV, advance=3, done_ctr=done, **kw)
        _exact(f"permutations (advance) n{n} seed {seed:#x}", _np(got), ref)
        assert int(ctr.item()) & M64 == (total + 3) & M64 and int(done.item()) == 0
        got = ops.random_permutations(n, 3, seed, counter_dev=ctr, device=DEV, advance=3, done_ctr=done, **kw)
        _exact(f"permutations (advance, second call) n{n}", _np(got), sr.random_permutations(n, 3, seed, total + 3, None, **kw)[0])


# ---- prioritized replay --------------------------------------------------------------------------------------------------------
def test_per_sample_matches_the_restatement():
    prio = np.load(os.path.join(HERE, "golden", "per.npz"))["sm_prio"]
    assert len(prio) == 37
    for size, leaves in ((37, prio), (1, np.array([0.3]))):
        t = ops.DeviceSegmentTree(size, device=DEV)
        t[np.arange(size)] = leaves
        tree = _np(t.tree)
        for seed, off, dev in COMMON:
            for n in ROWS:
                got = ops.per_sample(t, n, seed, offset=off, offset_dev=_ctr_dev(dev))
                ref, _ = sr.per_sample(tree, size, n, seed, off, dev)
                _exact(f"per_sample {size} leaves n{n} seed {seed:#x}", _np(got), ref["index"])
                assert (leaves[ref["index"]] != 0).all()                      # no draw lands on a zero-weight leaf


# ---- epsilon-greedy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 3, 4, 5, 9])
def test_dqn_egreedy_matches_the_restatement(A):
    rs = np.random.RandomState(A)
    for seed, off, dev in COMMON:
        for R in ROWS:
            q = rs.standard_normal((R, A)).astype(np.float32)
            mask = (rs.random_sample((R, A)) < 0.6).astype(np.uint8)
            mask[0] = 0                                                   # a row with no legal action
            if R > 2:
                mask[2] = 0
            for m in (None, mask):
                for eps in (0.5, 1.0):
                    got = ops.dqn_egreedy(_d(q), _d(np.array([eps], np.float32)), seed, offset=off, offset_dev=_ctr_dev(dev),
                                          mask=None if m is None else _d(m))
                    ref, _ = sr.dqn_egreedy(q, eps, seed, off, dev, mask=m)
                    _exact(f"dqn_egreedy A{A} R{R} eps {eps} mask {m is not None} seed {seed:#x}", _np(got), ref["act"])


def test_dqn_egreedy_random_rows_take_their_uniforms_from_sub_1_on():
    """Independence: the coin is word 0 of sub 0; a row it sends to a random action draws uniform[a] from sub 1 + a / 4 -- not from
    the coin's block, which would tie uniform[0] to the coin (always < eps)."""
    A, R, seed, off = 4, 1000, 0x1234ABCD5678, 2**32 - 3
    q = np.zeros((R, A), np.float32)
    got = _np(ops.dqn_egreedy(_d(q), _d(np.array([0.5], np.float32)), seed, offset=off))
    ref, _ = sr.dqn_egreedy(q, 0.5, seed, off)
    rnd = ref["random"]
    assert 0.4 < rnd.mean() < 0.6
    _exact("dqn_egreedy random rows", got[rnd], ref["act"][rnd])
    assert not got[~rnd].any()                                          # greedy rows of an all-zero q: the first maximum
    sub0 = u01(philox4(seed, sr.counters(off, None, np.arange(R)), 0), np.float32)
    wrong = np.array([sr.dqn_random_action(sub0[r], None) for r in range(R)])
    differ = float((wrong[rnd] != ref["act"][rnd]).mean())
    print(f"PARITY dqn_egreedy independence: uniforms of sub 0 would change {differ:.3g} of the random rows")
    assert differ > 0.5


@pytest.mark.parametrize("N", [1, 3])
def test_qmix_egreedy_matches_the_restatement(N):
    A = 5
    rs = np.random.RandomState(N)
    for seed, off, dev in COMMON:
        for B in (1, 15, 16, 17, 255, 256, 257, 1000):                    # ROWS, and 16 rows per workgroup
            q = [rs.standard_normal((B, A)).astype(np.float32) for _ in range(N)]
            for eps in (0.5, 1.0):
                got = ops.qmix_egreedy([_d(x) for x in q], _d(np.array([eps], np.float32)), seed, offset=off,
                                       offset_dev=_ctr_dev(dev))
                ref, _ = sr.qmix_egreedy(q, eps, seed, off, dev)
                _exact(f"qmix_egreedy N{N} B{B} eps {eps} seed {seed:#x}", _np(got), ref["act"])


def test_qmix_coin_and_first_rows_action_share_a_block_not_a_word():
    """Independence: with eps = 1 every coin says random (word 1 of counter c + i), and row 0's action of agent i is word 0 of the
    same block; with eps = 0.5 both the coins and the actions are the restatement's."""
    N, B, A, seed, off = 3, 33, 64, 0x8000000000C0FFEE, 2**32 - 3
    q = [np.zeros((B, A), np.float32)] * N
    w = philox4(seed, sr.counters(off, None, np.arange(N)), 0)
    got = _np(ops.qmix_egreedy([_d(x) for x in q], _d(np.ones(1, np.float32)), seed, offset=off))
    _exact("qmix row 0 = word 0 of the coin's block", got[0], (w[:, 0].astype(np.uint64) * np.uint64(A)) >> np.uint64(32))
    _exact("qmix eps 1", got, sr.qmix_egreedy(q, 1.0, seed, off)[0]["act"])
    for eps in (0.3, 0.5, 0.7):
        ref, _ = sr.qmix_egreedy(q, eps, seed, off)
        assert np.array_equal(ref["random"], u01(w[:, 1], np.float32) < np.float32(eps))
        got = _np(ops.qmix_egreedy([_d(x) for x in q], _d(np.array([eps], np.float32)), seed, offset=off))
        _exact(f"qmix coins at eps {eps}", got, ref["act"])


# ---- IQN -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 4, 5, 32, 33])
def test_iqn_taus_match_the_restatement(S):
    if S == 1:   # the entry point serves sample sizes 2 to 64, as the reference's `assert sample_size > 1`: nothing to draw
        with pytest.raises(ValueError, match="sample_size = 1"):
            ops.iqn_taus(7, 1, 0, DEV)
        return
    for seed, off, dev in COMMON:
        for R in ROWS:
            got = ops.iqn_taus(R, S, seed, DEV, offset=off, offset_dev=_ctr_dev(dev))
            _exact(f"iqn_taus S{S} R{R} seed {seed:#x}", _np(got).view(np.int32), sr.iqn_taus(R, S, seed, off, dev)[0].view(np.int32))


def test_device_philox_gives_the_random123_known_answer():
    """seed = the fraction key gives Philox key 0; counter 0, S = 4: the first Random123 vector, 6627e8d5 e169c58d bc57ac4c 9b00dbd8."""
    got = _np(ops.iqn_taus(1, 4, sr.TAU_KEY, DEV, offset=0))
    want = np.array([0x6627E8, 0xE169C5, 0xBC57AC, 0x9B00DB], np.float64) / 2.0 ** 24
    _exact("device known answer", got.astype(np.float64)[0], want)


# ---- normals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025])
def test_cac_normal_matches_the_restatement(n):
    for seed, off, dev in COMMON:
        got = ops.cac_normal(n, seed, offset=off, offset_dev=_ctr_dev(dev), device=DEV)
        z64, _ = sr.cac_normal(n, seed, off, dev)
        e_ref = float(np.abs(z64 - sr.cac_normal(n, seed, off, dev, np.float32)[0]).max())
        _bar(f"cac_normal n{n} seed {seed:#x}", _np(got), z64, e_ref)


@pytest.mark.parametrize("Ad", [1, 3])
def test_maddpg_act_matches_the_restatement(Ad):
    rs = np.random.RandomState(Ad)
    for seed, off, dev in COMMON:
        # E N rows: ROWS with one agent (256 rows x Ad = 1 fills the last workgroup exactly), 255 and 3000 rows with three
        for N, E in [(1, R) for R in ROWS] + [(3, 85), (3, 1000)]:
            # mu = 0, sigma = 1, no bounds: out = z
            mu = [np.zeros((E, Ad), np.float32)] * N
            one = _d(np.ones(1, np.float32))
            got = ops.maddpg_act([_d(m) for m in mu], one, seed, offset=off, offset_dev=_ctr_dev(dev))
            z64, _ = sr.maddpg_act(mu, 1.0, seed, off, dev)
            e_ref = float(np.abs(z64 - sr.maddpg_act(mu, 1.0, seed, off, dev, dtype=np.float32)[0]).max())
            _bar(f"maddpg_act z Ad{Ad} N{N} E{E} seed {seed:#x}", _np(got), z64, e_ref)
            # mu, sigma and bounds
            mu = [rs.standard_normal((E, Ad)).astype(np.float32) for _ in range(N)]
            lo, hi = -np.linspace(0.5, 1.0, Ad).astype(np.float32), np.linspace(0.75, 1.5, Ad).astype(np.float32)
            sg = np.float32(0.3)
            got = ops.maddpg_act([_d(m) for m in mu], _d(np.array([sg])), seed, offset=off, offset_dev=_ctr_dev(dev), low=_d(lo),
                                 high=_d(hi))
            a64, _ = sr.maddpg_act(mu, sg, seed, off, dev, lo, hi)
            e_ref = float(np.abs(a64 - sr.maddpg_act(mu, sg, seed, off, dev, lo, hi, dtype=np.float32)[0]).max())
            _bar(f"maddpg_act bounded Ad{Ad} N{N} E{E} seed {seed:#x}", _np(got), a64, e_ref)
            g = _np(got)
            assert (g >= lo).all() and (g <= hi).all()
            if E > 50:
                assert (g == lo).any() and (g == hi).any()                # the clamp fires on both sides
            # sigma == 0 and no bounds: the actors' bits
            got = ops.maddpg_act([_d(m) for m in mu], _d(np.zeros(1, np.float32)), seed, offset=off)
            _exact("maddpg_act sigma 0", _np(got).view(np.int32), np.stack(mu, 1).reshape(E * N, Ad).view(np.int32))


# ---- the environments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 8])
def test_simple_spread_resets_match_the_restatement(N):
    E = 21
    for seed in (0, 0x1234ABCD5678, 0x8000000000C0FFEE):
        env = DeviceSimpleSpreadVectorEnv(E, N, max_cycles=1, device=DEV, seed=seed)
        obs = _np(env.reset_device()).copy()
        ref, _ = sr.mpe_reset(seed, E, N, 0)
        _exact(f"spread reset N{N} seed {seed:#x}: agents", _np(env.agent_pos).view(np.int32), ref["agent_pos"].view(np.int32))
        _exact("spread reset: landmarks", _np(env.landmark_pos).view(np.int32), ref["landmark_pos"].view(np.int32))
        _exact("spread reset: observed position", obs[..., 2:4].view(np.int32), ref["agent_pos"].view(np.int32))
        rel = ref["landmark_pos"][:, None, :, :] - ref["agent_pos"][:, :, None, :]              # [E, agent, landmark, 2] in f32
        _exact("spread reset: observed landmarks", obs[..., 4:4 + 2 * N].view(np.int32), rel.reshape(E, N, 2 * N).view(np.int32))
        ids = torch.tensor([0, 5, 20])
        env.reset_device(ids)                                                                  # these envs: episode 1
        ep = np.zeros(E, np.int64)
        ep[_np(ids)] = 1
        ref, _ = sr.mpe_reset(seed, E, N, ep)
        _exact("spread partial reset", _np(env.agent_pos).view(np.int32), ref["agent_pos"].view(np.int32))
        assert np.array_equal(_np(env.episode_ctr), ep + 1)
        # one step of a one-step episode: every env ends and is reset in the step kernel, env e at its own episode number
        env.step_device(torch.zeros(E, N, dtype=torch.int32, device=DEV))
        assert _np(env.done_env).all() and np.array_equal(_np(env.episode_ctr), ep + 2)
        ref, _ = sr.mpe_reset(seed, E, N, ep + 1)
        _exact("spread auto-reset: agents", _np(env.agent_pos).view(np.int32), ref["agent_pos"].view(np.int32))
        _exact("spread auto-reset: landmarks", _np(env.landmark_pos).view(np.int32), ref["landmark_pos"].view(np.int32))
        _exact("spread auto-reset: observed position", _np(env.obs_cur)[..., 2:4].view(np.int32), ref["agent_pos"].view(np.int32))
        assert not _np(env.agent_vel).any()


def _tag_bar(name, got, ref):
    ratio = float(np.abs(np.asarray(got, np.float64) - ref).max()) / 2.0 ** -23
    print(f"PARITY {name}: max |hip - ref64| / 2^-23 = {ratio:.3g}")
    assert got.shape == ref.shape and ratio <= 1.0, (name, ratio)
    return ratio


@pytest.mark.parametrize("n_adv,n_good,n_obst", [(3, 1, 2), (1, 1, 3), (1, 1, 4)])
def test_simple_tag_resets_match_the_restatement(n_adv, n_good, n_obst):
    """(1, 1, 3) and (1, 1, 4): more obstacles than agent lanes, so a lane of the auto-reset draws several."""
    E, NA = 21, n_adv + n_good
    for seed in (0, 0x1234ABCD5678, 0x8000000000C0FFEE):
        env = DeviceSimpleTagVectorEnv(E, n_good, n_adv, n_obst, max_cycles=1, device=DEV, seed=seed)
        obs = _np(env.reset_device()).copy()
        ref, _ = sr.mpe_tag_reset(seed, E, n_adv, n_good, n_obst, 0)
        tag = f"tag {n_adv}v{n_good}+{n_obst} seed {seed:#x}"
        _tag_bar(f"{tag} reset: agents", _np(env.agent_pos), ref["agent_pos"])
        _tag_bar(f"{tag} reset: obstacles", _np(env.landmark_pos)[:, :n_obst], ref["obstacle_pos"])
        _exact(f"{tag} reset: observed position", obs[..., 2:4].view(np.int32), _np(env.agent_pos).view(np.int32))
        ids = torch.tensor([0, 5, 20])
        env.reset_device(ids)
        ep = np.zeros(E, np.int64)
        ep[_np(ids)] = 1
        env.step_device(torch.zeros(E, NA, dtype=torch.int32, device=DEV))
        assert _np(env.done_env).all() and np.array_equal(_np(env.episode_ctr), ep + 2)
        ref, _, drawn = sr.mpe_tag_reset_lanes(seed, E, n_adv, n_good, n_obst, ep + 1)
        assert max(len(v) for v in drawn.values()) == 1 + -(-n_obst // NA)
        _tag_bar(f"{tag} auto-reset: agents", _np(env.agent_pos), ref["agent_pos"])
        _tag_bar(f"{tag} auto-reset: obstacles", _np(env.landmark_pos)[:, :n_obst], ref["obstacle_pos"])
        _exact(f"{tag} auto-reset: observed position", _np(env.obs_cur)[..., 2:4].view(np.int32), _np(env.agent_pos).view(np.int32))
        assert not _np(env.agent_vel).any()
