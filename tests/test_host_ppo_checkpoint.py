"""Host tests of the on-policy learners' checkpoints and snapshots (`PPO.state_dict` / `load_state_dict` / `__deepcopy__`, and
A2C, Reinforce and GenericPPO under them): per case of tests/ppo_checkpoint_cases.py, against
tests/golden/ppo_checkpoint_layout.npz, which tests/golden/make_ppo_checkpoint_fixtures.py recorded while PPO still kept its
Adam state by hand and every class wrote its own snapshot."""
import copy
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ppo_checkpoint_cases import CASES, SEED, SNAPSHOT_CASES, layout, load_fixture, plant  # noqa: E402

ARRAYS, META = load_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_checkpoint_layout.npz"))


def _params(sd):
    return [(k, v) for k, v in sd.items() if k != "_optimizers"]


def _assert_same_checkpoint(got, want):
    """Two `state_dict()`s: keys in order, parameters and moments bit for bit, groups and engine entries whole."""
    (ga, gm), (wa, wm) = layout(got), layout(want)
    assert gm == wm and list(ga) == list(wa) and all(np.array_equal(ga[k], wa[k]) for k in wa)
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(_params(got), _params(want)))


def _assert_image_in_sync(net):
    if net.image is not None:
        assert torch.equal(net.image[net.image_map.long()], net.flat.data)


def test_the_fixture_covers_every_case():
    assert list(META) == list(CASES) and {k.split("/")[0] for k in ARRAYS} == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_is_the_recorded_layout(name):
    algo = plant(CASES[name](SEED))
    sd = algo.state_dict()
    arrays, meta = layout(sd)
    assert meta == META[name]   # key order, shapes, state indices and steps, param_groups[0] whole, tsm_engine
    assert {f"{name}/{k}" for k in arrays} == {k for k in ARRAYS if k.startswith(name + "/")}
    assert all(np.array_equal(v, ARRAYS[f"{name}/{k}"]) and v.dtype == ARRAYS[f"{name}/{k}"].dtype for k, v in arrays.items())
    # the parameter entries are copies of the net's own views, under their names and in their order
    views = algo.net.reference_named_views()
    assert [k for k, _ in views] == [k for k, _ in _params(sd)]
    assert all(torch.equal(v, sd[k]) and sd[k].data_ptr() != v.data_ptr() for k, v in views)
    # and the moments tile the optimizer's vectors in that order
    state = sd["_optimizers"][0]["state"]
    assert torch.equal(torch.cat([state[i]["exp_avg"].reshape(-1) for i in range(len(views))]), algo.exp_avg)
    assert torch.equal(torch.cat([state[i]["exp_avg_sq"].reshape(-1) for i in range(len(views))]), algo.exp_avg_sq)


@pytest.mark.parametrize("name", list(CASES))
def test_no_optimizer_state_before_the_first_step(name):
    sd = CASES[name](SEED).state_dict()
    assert sd["_optimizers"][0]["state"] == {} and sd["_optimizers"][0]["tsm_engine"]["opt_step"] == 0
    fresh = plant(CASES[name](SEED + 1))
    fresh.load_state_dict(sd)
    assert fresh.opt_step == 0 and not fresh.exp_avg.any() and not fresh.exp_avg_sq.any()


@pytest.mark.parametrize("name", list(CASES))
def test_a_fresh_instance_loads_it_and_gives_it_back(name):
    sd = plant(CASES[name](SEED)).state_dict()
    fresh = CASES[name](SEED + 1)
    assert not torch.equal(fresh.net.flat.data, torch.cat([v.reshape(-1) for _, v in _params(sd)]))
    version = fresh.param_version
    fresh.load_state_dict(sd)
    _assert_same_checkpoint(fresh.state_dict(), sd)
    _assert_image_in_sync(fresh.net)
    assert fresh.param_version == version + 1 and fresh.opt_step == 3
    assert fresh.lr == sd["_optimizers"][0]["param_groups"][0]["lr"] == float(fresh._lr_dev)
    with pytest.raises(KeyError):
        fresh.load_state_dict({k: v for k, v in sd.items() if not k.startswith("critic.last")})


def test_changed_adam_constants_drop_the_captured_workspaces():
    algo = plant(CASES["PPO"](SEED))
    sd = algo.state_dict()
    algo._ws["kept"] = 1
    algo.load_state_dict(sd)
    assert algo._ws == {"kept": 1}
    sd["_optimizers"][0]["param_groups"][0]["betas"] = (0.8, 0.99)
    algo.load_state_dict(sd)
    assert algo._ws == {} and tuple(algo.betas) == (0.8, 0.99)
    assert algo.state_dict()["_optimizers"][0]["param_groups"][0]["betas"] == (0.8, 0.99)


@pytest.mark.parametrize("name", list(SNAPSHOT_CASES))
def test_a_snapshot_holds_the_same_state_over_its_own_vector_and_draws_nothing(name, monkeypatch):
    algo = plant(SNAPSHOT_CASES[name](SEED))
    algo.eval()
    torch.manual_seed(123)
    before = torch.get_rng_state()
    with monkeypatch.context() as m:   # (`torch.manual_seed` seeds the device generators as well, which no host test sees)
        m.setattr(torch, "manual_seed", lambda seed: pytest.fail("a snapshot seeded the global generators"))
        snap = copy.deepcopy(algo)
    assert torch.equal(torch.get_rng_state(), before)
    assert type(snap) is type(algo) and type(snap.net) is type(algo.net) and snap.training is False
    _assert_same_checkpoint(snap.state_dict(), algo.state_dict())
    assert snap.net.flat.data_ptr() != algo.net.flat.data_ptr() and snap.exp_avg.data_ptr() != algo.exp_avg.data_ptr()
    _assert_image_in_sync(snap.net)
    # the constructor's arguments, a subclass's own included, are the original's
    for attr in ("lr", "gamma", "gae_lambda", "vf_coef", "ent_coef", "max_grad_norm", "eps_clip", "dispatch", "shuffle", "seed",
                 "use_graph", "return_scaling", "deterministic_eval"):
        assert getattr(snap, attr) == getattr(algo, attr), attr
    for attr in ("return_standardization", "critic_input", "n_agent", "graph", "fused_actor"):
        assert getattr(snap, attr, None) == getattr(algo, attr, None), attr
    # and the two no longer move together
    snap.net.flat.data.add_(1.0)
    snap.exp_avg.add_(1.0)
    snap.opt_step += 1
    assert not torch.equal(snap.net.flat.data, algo.net.flat.data) and not torch.equal(snap.exp_avg, algo.exp_avg)
    assert (snap.opt_step, algo.opt_step) == (4, 3)


def test_the_fused_net_keeps_its_image_in_sync_and_its_layers_by_name():
    from tianshou_marl_amd.utils.net import DiscreteActorCritic, lagged_copy

    net = DiscreteActorCritic(6, 4, 64, device="cpu", seed=SEED)
    _assert_image_in_sync(net)
    joint = torch.zeros(5 + net.flat.numel())
    before = net.flat.data.clone()
    net.rebind(joint[5:])   # (a slice of a joint vector: the values move, the image holds them already)
    assert net.flat.data_ptr() == joint[5:].data_ptr() and torch.equal(net.flat.data, before)
    _assert_image_in_sync(net)
    other = DiscreteActorCritic(6, 4, 64, device="cpu", seed=SEED + 1)
    other.load_reference_state_dict(net.to_reference_state_dict())
    assert torch.equal(other.flat.data, net.flat.data)
    _assert_image_in_sync(other)
    _assert_image_in_sync(lagged_copy(net))
    # `view("actor.w0")` ... `view("critic.b2")` alias the vector in its order; `load_layers` fills them and the image
    names = [f"{trunk}.{kind}{i}" for trunk in ("actor", "critic") for i in range(3) for kind in "wb"]
    views = [net.view(name) for name in names]
    assert [tuple(v.shape) for v in views] == [(64, 6), (64,), (64, 64), (64,), (4, 64), (4,), (64, 6), (64,), (64, 64), (64,), (1, 64), (1,)]
    assert all(v.data_ptr() == r.data_ptr() for v, (_, r) in zip(views, net.reference_named_views()))
    layers = [[(other.view(f"{t}.w{i}").numpy() + 1, other.view(f"{t}.b{i}") + 1) for i in range(3)] for t in ("actor", "critic")]
    net.load_layers(*layers)
    assert torch.equal(net.flat.data, other.flat.data + 1)
    _assert_image_in_sync(net)
    with pytest.raises(ValueError):
        net.view("policy.w0")


@pytest.mark.parametrize("fused", [True, False])
def test_a_snapshot_keeps_the_key_names_of_the_modules_its_net_was_built_from(fused):
    from tianshou_marl_amd.algorithm.ppo import PPO
    from tianshou_marl_amd.algorithm.ppo_generic import GenericPPO
    from tianshou_marl_amd.utils.net import DiscreteActorCritic, MLPActorCritic

    keys = {"actor": [(f"trunk.{i}.weight", f"trunk.{i}.bias") for i in range(3)], "critic": None}
    if fused:
        algo = PPO(net=DiscreteActorCritic(6, 4, 64, device="cpu", seed=SEED, ref_keys=keys), device="cpu")
    else:
        algo = GenericPPO(net=MLPActorCritic(6, 4, (12, 8), device="cpu", seed=SEED, ref_keys=keys), device="cpu")
    names = list(algo.state_dict())
    assert names[0] == "policy.actor.trunk.0.weight" and names[6] == "critic.preprocess.model.model.0.weight"
    assert list(copy.deepcopy(algo).state_dict()) == names
