"""Host tests of what the flat-parameter networks share (`FlatNet`, utils/net.py): the storage claim, twins, the ONE statement of
a net's parameters with the checkpoint and the optimizer split derived from it -- per class of tests/flat_net_cases.py, against
tests/golden/flat_nets.npz, which tests/golden/make_flat_net_fixtures.py recorded before the plumbing was stated once."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flat_net_cases import CASES, SEED, adam_shapes, load_fixture  # noqa: E402
from tianshou_marl_amd.utils.net import FlatAdam, lagged_copy  # noqa: E402

ARRAYS, META = load_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_nets.npz"))
TWINS = [name for name, (_, has_twin) in CASES.items() if has_twin]


def _net(name, seed=SEED):
    return CASES[name][0](seed)


def _blank(name, net):
    """A fresh net of `net`'s shape over zeroed storage: a twin where the class has twins, else one built again."""
    other = net.clone_over(torch.zeros_like(net.flat.data)) if CASES[name][1] else _net(name, SEED + 1)
    other.flat.data.zero_()
    return other


def _inside(v, flat):
    """`v`'s data pointer lies inside `flat`'s range."""
    return flat.data_ptr() <= v.data_ptr() < flat.data_ptr() + 4 * flat.numel()


def test_the_fixture_covers_every_case():
    assert list(META) == list(CASES) and {k.split("/")[0] for k in ARRAYS} == set(CASES)
    assert {k for k in ARRAYS if k.endswith("/lagged")} == {f"{name}/lagged" for name in TWINS}


@pytest.mark.parametrize("name", list(CASES))
def test_init_checkpoint_and_optimizer_layout_are_the_recorded_ones(name):
    net, meta = _net(name), META[name]
    assert np.array_equal(net.flat.data.numpy(), ARRAYS[f"{name}/flat"])   # the init, bit for bit
    sd = net.to_reference_state_dict()
    assert list(sd) == meta["keys"] and [list(v.shape) for v in sd.values()] == meta["shapes"]
    assert all(v.is_contiguous() and v.data_ptr() != net.flat.data_ptr() for v in sd.values())   # host copies, not views
    assert adam_shapes(net) == meta["adam"] == [list(s) for s in net.param_shapes()]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("which", ["checkpoint", "optimizer"])
def test_views_alias_the_vector_and_tile_it_exactly(name, which):
    """Of the net's own vector and of any vector of its layout, in the checkpoint's statement and in the optimizer's."""
    net = _net(name)
    for flat in (None, torch.zeros_like(net.flat.data)):
        views = [v for _, v in net.reference_named_views(flat)] if which == "checkpoint" else net.param_views(flat)
        vec = net.flat.data if flat is None else flat
        assert sum(v.numel() for v in views) == vec.numel()
        assert all(_inside(v, vec) for v in views)
        vec.zero_()
        for i, v in enumerate(views):
            assert not v.any()   # nothing an earlier view wrote: no overlap
            v.fill_(i + 1)
        got = np.bincount(vec.numpy().astype(np.int64), minlength=len(views) + 1)
        assert got.tolist() == [0] + [v.numel() for v in views]


@pytest.mark.parametrize("name", list(CASES))
def test_checkpoint_round_trip_under_a_prefix_is_exact(name):
    net = _net(name)
    sd = net.to_reference_state_dict(prefix="p.")
    assert list(sd) == ["p." + k for k in META[name]["keys"]]
    into = {"kept": 1}
    assert net.to_reference_state_dict("q.", into) is into and len(into) == 1 + len(sd)
    other = _blank(name, net)
    other.load_reference_state_dict(sd, prefix="p.")
    assert torch.equal(other.flat.data, net.flat.data)
    other = _blank(name, net)
    other.load_reference_state_dict({k: v.numpy() for k, v in sd.items()}, "p.")   # numpy entries serve as well
    assert torch.equal(other.flat.data, net.flat.data)
    with pytest.raises(KeyError):
        other.load_reference_state_dict(sd, prefix="r.")


@pytest.mark.parametrize("name", list(CASES))
def test_adam_moment_round_trip_is_exact(name):
    net = _net(name)
    gen = torch.Generator().manual_seed(11)
    opt = FlatAdam(net)
    opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=gen))
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=gen))
    opt.step_count = 3
    sd = opt.state_dict()
    assert [list(e["exp_avg"].shape) for e in sd["state"].values()] == META[name]["adam"]
    assert all(e["exp_avg"].is_contiguous() and float(e["step"]) == 3.0 for e in sd["state"].values())
    other = FlatAdam(_blank(name, net))
    other.load_state_dict(sd)
    assert other.step_count == 3 and torch.equal(other.exp_avg, opt.exp_avg) and torch.equal(other.exp_avg_sq, opt.exp_avg_sq)


def test_a_bare_vector_is_one_parameter():
    vec = torch.zeros(7)
    opt = FlatAdam(vec)
    opt.step_count = 1
    assert opt.param.data_ptr() == vec.data_ptr() and [tuple(e["exp_avg"].shape) for e in opt.state_dict()["state"].values()] == [(7,)]


def test_the_twin_of_a_ctde_net_is_the_bare_mlp_of_its_shape():
    """The CTDE constructors take no storage; their targets are read through `FlatMLP.forward`."""
    from tianshou_marl_amd.algorithm.multiagent.ctde import CentralizedCritic, DecentralizedActor
    from tianshou_marl_amd.utils.net import FlatMLP, join_nets, lagged_twins

    nets = [DecentralizedActor(6, 4, 8, device="cpu", seed=1), CentralizedCritic(12, 2, 8, device="cpu", seed=2)]
    flat, offs = join_nets(nets, "cpu")
    target_flat, twins = lagged_twins(nets, flat, offs)
    assert [type(t) for t in twins] == [FlatMLP, FlatMLP] and [t.dims for t in twins] == [n.dims for n in nets]
    assert torch.equal(target_flat, flat) and target_flat.data_ptr() != flat.data_ptr()
    assert all(torch.equal(t.flat.data, n.flat.data) for t, n in zip(twins, nets))


@pytest.mark.parametrize("name", TWINS)
def test_clone_over_refuses_storage_that_is_not_the_vector(name):
    net = _net(name)
    n = net.flat.numel()
    msg = f"{type(net).__name__}: storage must be a contiguous f32 vector of {n} elements"
    for bad in (torch.zeros(n + 1), torch.zeros(n, dtype=torch.float64), torch.zeros(2 * n)[::2]):
        with pytest.raises(ValueError, match=msg):
            net.clone_over(bad)
    twin = net.clone_over(torch.zeros(n))
    assert type(twin) is type(net) and twin.flat.numel() == n


@pytest.mark.parametrize("name", TWINS)
def test_lagged_copy_is_the_recorded_one_and_draws_nothing(name, monkeypatch):
    net = _net(name)
    torch.manual_seed(123)
    before = torch.get_rng_state()
    with monkeypatch.context() as m:   # (`torch.manual_seed` seeds the device generators as well, which no host test sees)
        m.setattr(torch, "manual_seed", lambda seed: pytest.fail("a twin seeded the global generators"))
        twin = lagged_copy(net)
    assert torch.equal(torch.get_rng_state(), before)
    assert type(twin) is type(net) and twin.flat.data_ptr() != net.flat.data_ptr()
    assert np.array_equal(twin.flat.data.numpy(), ARRAYS[f"{name}/lagged"]) and torch.equal(twin.flat.data, net.flat.data)
    assert twin.to_reference_state_dict().keys() == net.to_reference_state_dict().keys()
