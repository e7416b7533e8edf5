"""CPU tests of the yardsticks of tests/test_gpu_sampling.py: tests/philox_restatement.py against the Random123 known-answer
vectors of Philox4x32-10, and tests/sampling_restatement.py's own properties -- the Feistel permutation is a bijection, every
uniform lies in its documented interval, the share of categorical rows the GPU test has to leave out is small, and two successive
calls of every site, at the counters its Python caller gives them, own disjoint sets of (key, counter, sub, word)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sampling_restatement as sr  # noqa: E402
from philox_restatement import M32, MUL0, MUL1, WEYL0, WEYL1, philox4, philox4x32_10, u01  # noqa: E402

BIT63 = 0x8000000000C0FFEE
# (seed, host offset, device counter): 2^32 - 3 makes the rows of one call cross the carry into the high counter word; the last
# is 2^40 + 5 split between the host offset and the device counter
COMMON = [(0, 0, None), (0x1234ABCD5678, 2**32 - 3, None), (BIT63, 5, 2**40)]
ROWS = [1, 255, 256, 257, 1000]


# ---- Philox --------------------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((M32,) * 4, (M32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def _scalar_philox(c, k):
    """The ten rounds on Python ints, one block."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = MUL0 * c[0], MUL1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + WEYL0) & M32, (k[1] + WEYL1) & M32]
    return tuple(c)


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_gives_the_random123_known_answers(ctr, key, want):
    got = philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
    assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want
    assert _scalar_philox(ctr, key) == want


def test_philox4x32_10_is_vectorised_over_counters_and_keys():
    rs = np.random.RandomState(1)
    c = rs.randint(0, 2**32, size=(7, 3, 4), dtype=np.uint64)
    k = rs.randint(0, 2**32, size=(3, 2), dtype=np.uint64)
    got = philox4x32_10(c, k)
    assert got.shape == (7, 3, 4)
    for i in range(7):
        for j in range(3):
            assert tuple(int(x) for x in got[i, j]) == _scalar_philox([int(x) for x in c[i, j]], [int(x) for x in k[j]])
    # all three known answers in one call
    got = philox4x32_10(np.array([t[0] for t in KAT], np.uint64), np.array([t[1] for t in KAT], np.uint64))
    assert [tuple(int(x) for x in r) for r in got] == [t[2] for t in KAT]


def test_philox4_is_the_general_function_on_the_projects_words_across_the_carry():
    """counter + i carried in 64 bits: at 2^32 - 3 the rows of one call cross into the high counter word."""
    for seed in (0, 0x1234ABCD5678, BIT63):
        key = np.array([seed & M32, seed >> 32], np.uint64)
        for base in (2**32 - 3, 2**40 + 5, 2**64 - 2):
            ctr = sr.counters(base, None, np.arange(6))
            assert [int(c) for c in ctr] == [(base + i) % 2**64 for i in range(6)]
            for sub in (0, 1, 7):
                got = philox4(seed, ctr, sub)
                words = np.array([[((base + i) % 2**64) & M32, ((base + i) % 2**64) >> 32, sub, 0] for i in range(6)], np.uint64)
                assert np.array_equal(got, philox4x32_10(words, key))
        lo, hi = philox4(seed, [2**32 - 1], 0), philox4(seed, [2**32], 0)
        wrapped = philox4x32_10(np.array([0, 0, 0, 0], np.uint64), key)        # what a dropped carry would draw at 2^32
        assert not np.array_equal(hi[0], wrapped) and not np.array_equal(hi, lo)
    # a host offset plus a device counter is their 64-bit sum; Python-int counters and uint64 counters agree
    assert np.array_equal(sr.counters(5, 2**40, np.arange(4)), sr.counters(2**40 + 5, None, np.arange(4)))
    assert np.array_equal(philox4(3, [2**40 + 5, 2**63 + 1], [0, 2]), philox4(3, np.array([2**40 + 5, 2**63 + 1], np.uint64), [0, 2]))
    # the upper half of the seed is key word 1
    assert not np.array_equal(philox4(1, [0], 0), philox4(1 | 1 << 63, [0], 0))
    assert tuple(int(x) for x in philox4(0, 0, [0])[0]) == KAT[0][2]


def test_u01_is_the_top_24_bits():
    w = np.array([0, 255, 256, M32, 0x6627E8D5], np.uint32)
    assert np.array_equal(u01(w), np.array([0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0x6627E8 / 2.0 ** 24]))
    assert np.array_equal(u01(w, np.float32).astype(np.float64), u01(w))       # exact in float32


# ---- the permutation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 1000])
def test_feistel_restatement_is_a_bijection(n):
    for seed, off, dev in COMMON:
        out, used = sr.random_permutations(n, 3, seed, off, dev, scale=3, group_size=2, offset_mul=7)
        assert out.shape == (3, n) and len(used) == 3 * 4
        for p in range(3):
            x = out[p] - (p // 2) * 7
            assert (x % 3 == 0).all() and np.array_equal(np.sort(x // 3), np.arange(n))
    assert [sr.half_bits(k) for k in (1, 2, 3, 4, 5, 16, 17, 256, 257, 1000)] == [1, 1, 1, 1, 2, 2, 3, 4, 5, 5]


def test_feistel_restatement_differs_between_keys_and_mixes():
    a, _ = sr.random_permutations(1000, 3, 5, 0)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    assert (a[0] != np.arange(1000)).mean() > 0.99
    b, _ = sr.random_permutations(1000, 1, 5, 1)
    assert np.array_equal(b[0], a[1])                                          # permutation p draws at counter ctr + p


# ---- intervals -----------------------------------------------------------------------------------------------------------------
def test_every_restated_uniform_lies_in_its_documented_interval():
    seed, off, dev = COMMON[1]
    n = 20000
    taus, _ = sr.iqn_taus(n // 5, 5, seed, off, dev)
    assert taus.dtype == np.float32 and taus.min() >= 0.0 and taus.max() < 1.0
    tree = np.array([0.0, 0.3], np.float64)
    d, _ = sr.per_sample(tree, 1, n, seed, off, dev)
    assert d["u"].min() >= 0.0 and d["u"].max() <= 1.0 - 2.0 ** -52 and not d["index"].any()
    lg = np.random.RandomState(0).standard_normal((n, 5))
    d, _ = sr.categorical_sample(lg, seed, off, offset_dev=dev)
    s = np.exp(lg - lg.max(1, keepdims=True)).sum(1)
    assert (d["u"] >= 0).all() and (d["u"] < s).all() and d["act"].min() >= 0 and d["act"].max() < 5
    q = [np.zeros((n // 4, 7), np.float32)] * 3
    d, _ = sr.qmix_egreedy(q, 1.0, seed, off, dev)
    assert d["random"].all() and d["act"].min() >= 0 and d["act"].max() < 7 and set(np.unique(d["act"])) == set(range(7))
    d, _ = sr.dqn_egreedy(np.zeros((500, 9), np.float32), 1.0, seed, off, dev)
    assert d["uniform"].dtype == np.float32 and d["uniform"].min() >= 0.0 and d["uniform"].max() < 1.0
    z, _ = sr.cac_normal(n, seed, off, dev)
    assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2.0))   # u1 >= 2^-24: the logarithm never sees 0
    z, _ = sr.maddpg_act([np.zeros((n // 2, 2))], 1.0, seed, off, dev)
    assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2.0))
    d, _ = sr.mpe_reset(seed, 300, 8, 3)
    for k in ("agent_pos", "landmark_pos"):
        assert d[k].dtype == np.float32 and d[k].min() >= -1.0 and d[k].max() < 1.0
    d, _ = sr.mpe_tag_reset(seed, 300, 3, 1, 2, 3)
    assert d["agent_pos"].min() >= -1.0 and d["agent_pos"].max() < 1.0
    assert d["obstacle_pos"].min() >= -np.float32(0.9) and d["obstacle_pos"].max() < np.float32(0.9)
    # the ends of the word range
    assert u01(np.uint32(M32)) < 1.0 and 1.0 - u01(np.uint32(M32), np.float32) > 0 and u01(np.uint32(0)) == 0.0


# ---- categorical: the rows the GPU comparison leaves out ------------------------------------------------------------------------
def categorical_cases():
    """{name: logits f32 [B, A]}: random logits at A in {1, 2, 5, 64} and every row count, and at A = 5 rows with a dominant logit
    (+40) and rows with -inf entries."""
    rs = np.random.RandomState(20241019)
    cases = {f"A{A}_B1000": (2.0 * rs.standard_normal((1000, A))).astype(np.float32) for A in (1, 2, 5, 64)}
    for B in ROWS[:-1]:
        cases[f"A5_B{B}"] = (2.0 * rs.standard_normal((B, 5))).astype(np.float32)
    lg = rs.standard_normal((257, 5)).astype(np.float32)
    lg[0::3, 2] += 40.0
    lg[1::3, 0] = -np.inf
    lg[1::6, 4] = -np.inf
    lg[4::6, 1:4] = -np.inf
    cases["edges_A5"] = lg
    return cases


def categorical_share(d) -> float:
    return float(d["ambiguous"].mean())


def test_categorical_restatement_leaves_out_few_rows_and_handles_the_edges():
    worst = 0.0
    for name, lg in categorical_cases().items():
        B, A = lg.shape
        for seed, off, dev in COMMON:
            d, used = sr.categorical_sample(lg, seed, off, offset_dev=dev)
            share = categorical_share(d)
            worst = max(worst, share)
            print(f"PARITY categorical {name} seed {seed:#x}: restatement's excluded share = {share:.3g} of {B} rows")
            assert share <= 0.01, (name, share)
            assert len(used) == B
            assert np.isfinite(d["logp"][~d["ambiguous"]]).all() and (d["logp"] <= 1e-12).all()
            if A == 1:
                assert not d["act"].any() and np.array_equal(d["logp"], np.zeros(B))
            if name == "edges_A5":
                assert (d["act"][0::3] == 2).all()                                   # the dominant logit takes the row
                ok = ~d["ambiguous"]
                assert np.isfinite(lg[np.arange(B), d["act"]][ok]).all()             # never an action of probability 0
            g, _ = sr.categorical_sample(lg, seed, off, deterministic=True, offset_dev=dev)
            assert np.array_equal(g["act"], lg.argmax(1))
    # over many rows the share is about (A - 1) 16 A 2^-24 for uniform u
    lg = (2.0 * np.random.RandomState(3).standard_normal((200000, 64))).astype(np.float32)
    share = categorical_share(sr.categorical_sample(lg, 7, 0)[0])
    print(f"PARITY categorical A64 x 200000: restatement's excluded share = {share:.3g} (expected about {63 * 16 * 64 * 2.0 ** -24:.3g})")
    assert 0.5 * 63 * 16 * 64 * 2.0 ** -24 <= share <= 2.0 * 63 * 16 * 64 * 2.0 ** -24


# ---- the lane-wise auto-reset of simple_tag ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_adv,n_good,n_obst", [(3, 1, 2), (1, 1, 3), (1, 1, 4), (2, 2, 0), (4, 4, 4)])
def test_lane_wise_tag_reset_draws_every_entity_once_and_equals_the_env_reset(n_adv, n_good, n_obst):
    ep = np.arange(21) % 3
    a, used_a = sr.mpe_tag_reset(BIT63, 21, n_adv, n_good, n_obst, ep)
    b, used_b, drawn = sr.mpe_tag_reset_lanes(BIT63, 21, n_adv, n_good, n_obst, ep)
    assert sorted(e for v in drawn.values() for e in v) == list(range(n_adv + n_good + n_obst))
    assert used_a == used_b and len(used_a) == 21 * (n_adv + n_good + n_obst) * 2
    assert np.array_equal(a["agent_pos"], b["agent_pos"]) and np.array_equal(a["obstacle_pos"], b["obstacle_pos"])


# ---- counter advance -----------------------------------------------------------------------------------------------------------
def _disjoint(*useds):
    """Successive calls own disjoint words, and none owns a word twice (the sizes are checked by the callers below)."""
    seen = set()
    for u in useds:
        assert not (seen & u), sorted(seen & u)[:4]
        seen |= u


def _policy_counter():
    """tianshou_marl_amd/utils/learner.py sample_counter on a bare object: the advance every `act_device` uses."""
    from tianshou_marl_amd.utils.learner import sample_counter

    pol = SimpleNamespace(_sample_ctr=2**32 - 7)
    return pol, lambda draws, row_offset=0, offset_dev=None: sample_counter(pol, draws, row_offset, offset_dev)


def test_counter_advance_policy_draws():
    """categorical (ppo_generic.py / ctde.py / dsac.py: one draw per row), DQN (dqn.py: R), QMIX (qmix.py: B N), MADDPG and the
    continuous policies' exploration (maddpg.py: E N Ad; cac.py `_emit`: act.numel()) through `sample_counter`.  The counter code
    is the callers' own; the number of draws each caller passes to it is restated here from the files named, so a caller that
    came to pass fewer would not fail this test."""
    seed = 0x1234ABCD5678
    pol, ctr = _policy_counter()
    lg = np.zeros((37, 5), np.float32)
    us = [sr.categorical_sample(lg, seed, ctr(37))[1] for _ in range(3)]
    assert all(len(u) == 37 for u in us)
    _disjoint(*us)
    # DiscreteSACPolicy.forward: offset = _sample_ctr, then _sample_ctr += rows (dsac.py) -- the same stream as act_device
    us.append(sr.categorical_sample(lg, seed, pol._sample_ctr)[1])
    pol._sample_ctr += 37
    us.append(sr.categorical_sample(lg, seed, ctr(37))[1])
    _disjoint(*us)
    for A in (1, 3, 4, 5, 9):
        q = np.zeros((37, A), np.float32)
        us = [sr.dqn_egreedy(q, 0.5, seed, ctr(37))[1] for _ in range(3)]
        assert all(len(u) == 37 * (1 + A) for u in us)
        _disjoint(*us)
    for N in (1, 3):
        q = [np.zeros((21, 5), np.float32)] * N
        us = [sr.qmix_egreedy(q, 0.5, seed, ctr(21 * N))[1] for _ in range(3)]
        # agent i's coin (word 1) and the action of row 0, agent i (word 0) share a block, not a word
        assert all(len(u) == 21 * N + N and len(sr.blocks_of(u)) == 21 * N for u in us)
        _disjoint(*us)
    for N, Ad in ((1, 1), (3, 1), (1, 3), (3, 3)):
        mu = [np.zeros((21, Ad))] * N
        us = [sr.maddpg_act(mu, 1.0, seed, ctr(21 * N * Ad))[1] for _ in range(3)]
        assert all(len(u) == 21 * N * Ad * 2 for u in us)
        _disjoint(*us)


def test_counter_advance_under_the_collectors_device_tick():
    """data/collector.py: every step passes offset_dev = env.rng_tick and the env step adds E N to it; the policy's own counter
    stands still.  MultiAgentPolicy gives agent column a0 the row offset a0 E (multiagent/marl.py).  The tick's advance and the row
    offsets are restated here from those files, not run (they need the device)."""
    seed, E, N = BIT63, 7, 3
    pol, ctr = _policy_counter()
    ticks = [2**40 + k * E * N for k in range(3)]
    _disjoint(*[sr.categorical_sample(np.zeros((E * N, 5), np.float32), seed, ctr(E * N, 0, t), offset_dev=t)[1] for t in ticks])
    _disjoint(*[sr.dqn_egreedy(np.zeros((E * N, 9), np.float32), 0.5, seed, ctr(E * N, 0, t), t)[1] for t in ticks])
    _disjoint(*[sr.qmix_egreedy([np.zeros((E, 5), np.float32)] * N, 0.5, seed, ctr(E * N, 0, t), t)[1] for t in ticks])
    # one policy object serving the columns one by one: rows [a0 E, (a0 + 1) E) of every tick
    _disjoint(*[sr.categorical_sample(np.zeros((E, 5), np.float32), seed, ctr(E, a0 * E, t), offset_dev=t)[1]
                for t in ticks for a0 in range(N)])
    assert pol._sample_ctr == 2**32 - 7


def _recorder(monkeypatch, name, result=None):
    """`ops.<name>` replaced by a function that records its arguments: the callers below run their own counter code on bare
    objects, with no device."""
    from tianshou_marl_amd import ops

    calls = []

    def fake(*args, **kw):
        calls.append((args, kw))
        return result

    monkeypatch.setattr(ops, name, fake)
    return calls


def test_counter_advance_iqn_fractions(monkeypatch):
    """algorithm/iqn.py: the update stream draws R rows at `_tau_ctr` and adds R -- `IQNPolicy.net_forward` itself runs here, on
    a bare object whose net records the (seed, offset) it is handed.  Acting draws at the epsilon draw's counter (advance R,
    `sample_counter`) under the acting seed.  Both under seed ^ TAU_KEY: no epsilon draw shares the key."""
    from tianshou_marl_amd.algorithm.iqn import IQNPolicy

    seed = 0x1234ABCD5678
    for S in (1, 3, 4, 5, 32, 33):
        handed = []
        net = SimpleNamespace(dims=[4], forward=lambda rows, S_, taus=None, save=False, seed=0, offset=0, **kw: (
            handed.append((seed, offset, rows.shape[0], S_)), (None, None))[1])
        pol = SimpleNamespace(tau_feed=[], model=net, seed=seed, _tau_ctr=2**32 - 3, device=None, _sample_count=lambda old: S)
        for R in (37, 37, 5):
            IQNPolicy.net_forward(pol, np.zeros((R, 4), np.float32))
        assert [h[2:] for h in handed] == [(37, S), (37, S), (5, S)] and pol._tau_ctr == 2**32 - 3 + 79
        assert len({h[0] for h in handed}) == 1 and handed[0][0] != seed            # the update stream's own seed
        us = [sr.iqn_taus(R, S_, sd, off)[1] for sd, off, R, S_ in handed]
        assert [len(u) for u in us] == [37 * S, 37 * S, 5 * S]
        _disjoint(*us)
    eg = sr.dqn_egreedy(np.zeros((37, 9), np.float32), 0.5, seed, 11)[1]
    _disjoint(eg, sr.iqn_taus(37, 8, seed, 11)[1])                      # the same counters, another key


def test_counter_advance_normals_of_the_continuous_learners(monkeypatch):
    """algorithm/cac.py: the learners' `_normal` draws n = B Ad normals at the one counter `_sample_ctr`, then adds n --
    `ContinuousActionRows._normal` itself runs here on a bare object.  `SACPolicy._sample` advances alike (it needs the
    actor's forward, so its `+= n` is restated below, not run: a change there would not fail this test); `_emit` draws its n at
    counters `_sample_ctr` .. + n - 1 under the plain seed, through `sample_counter`."""
    from tianshou_marl_amd.algorithm.cac import ContinuousActionRows

    seed = BIT63
    calls = _recorder(monkeypatch, "cac_normal", SimpleNamespace(view=lambda *a: None))
    algo = SimpleNamespace(policy=SimpleNamespace(act_dim=3, seed=seed, _sample_ctr=2**32 - 3), noise_source=None, device=None)
    for B in (1, 2, 341, 5):
        ContinuousActionRows._normal(algo, B)
    assert [a[0] for a, _ in calls] == [3, 6, 1023, 15] and algo.policy._sample_ctr == 2**32 - 3 + 1047
    us = [sr.cac_normal(a[0], a[1], kw["offset"])[1] for a, kw in calls]
    _disjoint(*us)
    c, us = algo.policy._sample_ctr, us[:]
    for n in (1, 3, 4, 5, 1023, 1025):
        us.append(sr.cac_normal(n, seed, c)[1])
        assert len(us[-1]) == 2 * ((n + 1) // 2) and len(sr.blocks_of(us[-1])) == (n + 3) // 4
        c += n
    us.append(sr.maddpg_act([np.zeros((5, 3))], 1.0, seed, c)[1])
    c += 15
    us.append(sr.cac_normal(15, seed, c)[1])
    _disjoint(*us)


def test_counter_advance_prioritized_replay(monkeypatch):
    """data/buffer.py: `per_sample(.., offset=_sample_ctr)`, then `_sample_ctr += batch_size` --
    `PrioritizedVectorReplayBuffer.sample_indices_device` itself runs here on a bare object."""
    from tianshou_marl_amd.data.buffer import PrioritizedVectorReplayBuffer

    tree = np.array([0.0, 1.0, 0.25, 0.75, 0.25, 0.0, 0.5, 0.25], np.float64)
    calls = _recorder(monkeypatch, "per_sample")
    buf = SimpleNamespace(_has_rows=True, weight=None, seed=9, _sample_ctr=2**32 - 3)
    for n in (64, 64, 7):
        PrioritizedVectorReplayBuffer.sample_indices_device(buf, n)
    assert buf._sample_ctr == 2**32 - 3 + 135 and [a[1] for a, _ in calls] == [64, 64, 7]
    us = [sr.per_sample(tree, 4, a[1], a[2], kw["offset"])[1] for a, kw in calls]
    assert [len(u) for u in us] == [128, 128, 14]
    _disjoint(*us)


def test_counter_advance_ppo_permutations(monkeypatch):
    """algorithm/ppo.py, ppo_generic.py under the key seed ^ 0x5DEECE66D.  `update()`: permutation p of the G * repeat of one update
    draws at counter opt_step + p -- `PPO._device_perm` itself runs here for the eager form, on a bare object -- and the update
    takes G * repeat * n_minibatches >= G * repeat optimizer steps.  `learn()`: one permutation per repeat at the device counter
    `_perm_ctr`, which the launch (or tsm_u64_add) advances by 1.  That the base is the optimizer step count, and both advances, are
    restated here from ppo.py, not run (they need the device): a change there would not fail this test."""
    from tianshou_marl_amd.algorithm.ppo import PPO

    seed = 0x1234ABCD5678
    key = seed ^ 0x5DEECE66D
    calls = _recorder(monkeypatch, "random_permutations", [None])
    algo = SimpleNamespace(seed=seed, device=None)
    for G, repeat, n_mb in ((1, 1, 1), (3, 2, 1), (2, 4, 3)):
        step, us = 2**32 - 3, []
        for _ in range(3):
            us.append(sr.random_permutations(5, G * repeat, key, counter_dev=step, scale=G, group_size=repeat, offset_mul=1)[1])
            # the eager update draws the same blocks one by one: agent a, repeat r at perm_base + a * repeat + r
            del calls[:]
            for a in range(G):
                for r in range(repeat):
                    PPO._device_perm(algo, 5, step, a, repeat, r)
            eager = set()
            for args, kw in calls:
                assert args[:3] == (5, 1, key)
                eager |= sr.random_permutations(5, 1, key, kw["counter"])[1]
            assert eager == us[-1]
            step += G * repeat * n_mb
        _disjoint(*us)
    _disjoint(*[sr.random_permutations(5, 1, key, counter_dev=k)[1] for k in range(2**32 - 2, 2**32 + 2)])
    # known and unchanged: the two paths count apart under one key, so a program that mixes them on one object can
    # draw a permutation twice -- update() from step 0 (2 permutations, 8 steps), then the first learn() at _perm_ctr = 0
    up = sr.random_permutations(5, 2, key, counter_dev=0)[1]
    assert sr.random_permutations(5, 1, key, counter_dev=0)[1] <= up
    _disjoint(up, sr.random_permutations(5, 1, key, counter_dev=8)[1])       # what a shared counter would give


def test_counter_advance_env_resets():
    """One block per (episode, env, entity): distinct (episode, env) never share a block, and neither do two envs' entities."""
    ep = np.array([0, 0, 1, 5, 2, 0, 1], np.uint64)
    for N in (1, 3, 8):
        us = [sr.mpe_reset(BIT63, 7, N, ep + k)[1] for k in range(3)]
        assert all(len(u) == 7 * N * 4 for u in us)
        _disjoint(*us)
        assert not (sr.mpe_reset(BIT63, 7, N, 0)[1] & sr.mpe_reset(BIT63, 7, N, 1)[1])
    for n_adv, n_good, n_obst in ((3, 1, 2), (4, 4, 4)):
        us = [sr.mpe_tag_reset(BIT63, 7, n_adv, n_good, n_obst, ep + k)[1] for k in range(3)]
        assert all(len(u) == 7 * (n_adv + n_good + n_obst) * 2 for u in us)
        _disjoint(*us)
        assert not (sr.mpe_tag_reset(BIT63, 7, n_adv, n_good, n_obst, 0)[1] & sr.mpe_tag_reset(BIT63, 7, n_adv, n_good, n_obst, 1)[1])
