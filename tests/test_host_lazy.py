"""CPU tests of host-side helpers that carry no arithmetic: the lazily resolved statistics mappings `PPO.learn` and
`CTDEPolicy.learn` return and the ring of result slots behind every collect() / update() (tianshou_marl_amd/data/stats.py,
algorithm/ppo.py, algorithm/multiagent/ctde.py)."""
import json

import pytest

torch = pytest.importorskip("torch")

from tianshou_marl_amd.algorithm.multiagent.ctde import LazyScalars  # noqa: E402
from tianshou_marl_amd.algorithm.ppo import LazyLosses  # noqa: E402
from tianshou_marl_amd.data.stats import LazyDict, LazyStats, ResultRing  # noqa: E402


class _Event:
    def __init__(self):
        self.waits = 0

    def synchronize(self):
        self.waits += 1


def _slot():
    h = torch.tensor([[1.0, 2.0, 3.0, 4.0], [3.0, 4.0, 5.0, 6.0]])
    return dict(h=h, event=_Event(), pending=None)


def test_lazy_losses_resolve_once_on_first_read_and_behave_like_a_dict():
    slot = _slot()
    d = LazyLosses(slot)
    slot["pending"] = d
    assert slot["event"].waits == 0            # nothing read yet: the host has not waited
    assert d["loss"] == 2.0 and slot["event"].waits == 1
    assert d == {"loss": 2.0, "actor_loss": 3.0, "vf_loss": 4.0, "ent_loss": 5.0}
    assert set(d) == {"loss", "actor_loss", "vf_loss", "ent_loss"} and len(d) == 4 and "vf_loss" in d
    assert d.get("nope", 7) == 7 and dict(d)["ent_loss"] == 5.0 and {**d}["actor_loss"] == 3.0
    assert json.loads(json.dumps(d)) == dict(d)  # (resolved by now: the C encoder walks the dict storage itself)
    assert slot["event"].waits == 1 and slot["pending"] is None  # resolved exactly once, slot released


@pytest.mark.parametrize("reader", [lambda d: list(d.items()), lambda d: list(d.values()), lambda d: repr(d), lambda d: d.copy(),
                                    lambda d: json.dumps(d, indent=1), lambda d: dict(d), lambda d: d == {}, lambda d: len(d)])
def test_every_way_of_reading_lazy_losses_waits_for_the_statistics(reader):
    slot = _slot()
    d = LazyLosses(slot)
    reader(d)
    assert slot["event"].waits == 1 and dict.__len__(d) == 4


def test_two_lazy_results_compare_by_value():
    a, b = LazyLosses(_slot()), LazyLosses(_slot())
    assert a == b and not (a != b)
    with pytest.raises(TypeError):
        hash(a)


# ---- the same cases on the CTDE learner's mapping ----------------------------------------------------------------------
NAMES = ("actor_loss", "critic_loss")


def _slot2():
    return dict(h=torch.tensor([1.5, -2.0]), event=_Event(), pending=None)


def test_lazy_scalars_resolve_once_on_first_read_and_behave_like_a_dict():
    slot = _slot2()
    d = LazyScalars(slot, NAMES)
    slot["pending"] = d
    assert slot["event"].waits == 0
    assert d["actor_loss"] == 1.5 and slot["event"].waits == 1
    assert d == {"actor_loss": 1.5, "critic_loss": -2.0}
    assert set(d) == set(NAMES) and len(d) == 2 and "critic_loss" in d
    assert d.get("nope", 7) == 7 and dict(d)["critic_loss"] == -2.0 and {**d}["actor_loss"] == 1.5
    assert json.loads(json.dumps(d)) == dict(d)
    assert slot["event"].waits == 1 and slot["pending"] is None


@pytest.mark.parametrize("reader", [lambda d: list(d.items()), lambda d: list(d.values()), lambda d: repr(d), lambda d: d.copy(),
                                    lambda d: json.dumps(d, indent=1), lambda d: dict(d), lambda d: d == {}, lambda d: len(d)])
def test_every_way_of_reading_lazy_scalars_waits_for_the_statistics(reader):
    slot = _slot2()
    d = LazyScalars(slot, NAMES)
    reader(d)
    assert slot["event"].waits == 1 and dict.__len__(d) == 2


def test_two_lazy_scalars_compare_by_value():
    a, b = LazyScalars(_slot2(), NAMES), LazyScalars(_slot2(), NAMES)
    assert a == b and not (a != b) and a.copy() == {"actor_loss": 1.5, "critic_loss": -2.0}
    with pytest.raises(TypeError):
        hash(a)


def test_both_mappings_are_the_one_lazy_dict_and_resolve_is_public():
    assert issubclass(LazyLosses, LazyDict) and issubclass(LazyScalars, LazyDict)
    slot = _slot()
    d = LazyLosses(slot)
    assert d.resolve() is d and slot["event"].waits == 1 and dict.__len__(d) == 4
    d._force()
    assert slot["event"].waits == 1


# ---- the ring of result slots ------------------------------------------------------------------------------------------
def _ring():
    made = []

    def make_slot():
        made.append(dict(event=_Event(), pending=None, value=len(made)))
        return made[-1]

    return ResultRing(make_slot), made


def _result(slot, log):
    """A lazy result as update() hands it out: reading it waits for the slot's event and releases the slot."""
    def build():
        slot["event"].synchronize()
        slot["pending"] = None
        log.append(slot["value"])
        return slot["value"]

    out = LazyStats(build)
    slot["pending"] = out
    return out


def test_ring_makes_four_slots_without_waiting_then_goes_round():
    ring, made = _ring()
    first = [ring.take() for _ in range(4)]
    assert len(made) == 4 and all(a is b for a, b in zip(first, made)) and len({id(s) for s in first}) == 4
    assert all(s["event"].waits == 0 for s in made)
    for k in range(9):  # calls 5, 6, ...: slots 0, 1, 2, 3, 0, ... and one wait each for the slot's previous use
        assert ring.take() is made[k % 4]
    assert len(made) == 4 and [s["event"].waits for s in made] == [3, 2, 2, 2]


@pytest.mark.parametrize("wait", [True, False])
def test_ring_resolves_an_unread_result_before_its_slot_is_reused(wait):
    ring, made = _ring()
    log = []
    held = [_result(ring.take("resolve", wait=wait), log) for _ in range(4)]
    assert log == [] and made[0]["event"].waits == 0
    slot = ring.take("resolve", wait=wait)
    assert slot is made[0] and log == [0] and slot["pending"] is None  # read on the caller's behalf, slot released
    assert slot["event"].waits == 1 + wait  # the result's own wait, then the ring's
    assert held[0].resolve() == 0 and log == [0] and slot["event"].waits == 1 + wait  # the holder still gets the old numbers
    assert made[1]["pending"] is held[1] and made[1]["event"].waits == 0  # the other slots are untouched


def test_ring_expires_an_unread_result_with_the_callers_message_at_no_extra_wait():
    ring, made = _ring()
    log = []
    held = [_result(ring.take("expire", "not read within 4 calls"), log) for _ in range(4)]
    slot = ring.take("expire", "not read within 4 calls")
    assert slot is made[0] and log == [] and slot["event"].waits == 1  # only the ring's wait for the slot's event
    slot["pending"] = None  # (the caller stores the new result here)
    with pytest.raises(RuntimeError, match="not read within 4 calls"):
        held[0].resolve()
    assert slot["event"].waits == 1
    assert held[1].resolve() == 1  # not recycled yet: still readable


@pytest.mark.parametrize("unread", ["resolve", "expire"])
def test_ring_leaves_a_result_that_was_read_alone(unread):
    ring, made = _ring()
    log = []
    held = [_result(ring.take(unread, "gone"), log) for _ in range(4)]
    assert held[0].resolve() == 0 and made[0]["pending"] is None and made[0]["event"].waits == 1
    assert ring.take(unread, "gone") is made[0] and made[0]["event"].waits == 2 and log == [0]
    assert held[0].resolve() == 0  # (still the numbers it read)
    ring.take(unread, "gone", wait=False)  # slot 1, unread
    assert made[1]["event"].waits == (1 if unread == "resolve" else 0)


def test_ring_recycles_lazy_dicts_and_collect_stats_alike():
    """Every result class has `resolve()`; the two that a ring may drop unread take the message as `expire(why)`."""
    from tianshou_marl_amd.data.collector import LazyCollectStats

    ring = ResultRing(_slot2, depth=1)
    slot = ring.take()
    d = LazyScalars(slot, NAMES)
    slot["pending"] = d
    assert ring.take("resolve", wait=False) is slot and dict.__len__(d) == 2 and slot["pending"] is None
    cs = LazyCollectStats(None, slot, 5)
    slot["pending"] = cs
    ring.take("expire", "too late")
    assert slot["pending"] is None and cs.n_collected_steps == 5
    with pytest.raises(RuntimeError, match="too late"):
        cs.returns
