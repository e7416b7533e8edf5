"""CPU tests of the plumbing the off-policy learners share (utils/net.py, algorithm/optim.py): lagged copies that leave the
global torch RNG alone, nets joined into one flat vector, the Adam hand-over, and the reference's key names with the export /
load pair.  Nets are [3, 4, 2] and the mixer has 2 agents, a 3-wide state and 4-wide hypernetworks: the smallest with a hidden
layer, two agents and a bare-Linear hypernetwork.  Its mixing width is 32, the smallest `QMIXMixer` builds (the kernels serve
32 and 64)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tianshou_marl_amd.algorithm import DQN, DiscreteSAC, DiscreteSACPolicy  # noqa: E402
from tianshou_marl_amd.algorithm.dqn import DiscreteQLearningPolicy  # noqa: E402
from tianshou_marl_amd.algorithm.multiagent.maddpg import MADDPGPolicy  # noqa: E402
from tianshou_marl_amd.algorithm.multiagent.qmix import QMIXMixer, QMIXPolicy  # noqa: E402
from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory, LRSchedulerFactoryLinear, flat_adam_of  # noqa: E402
from tianshou_marl_amd.utils.net import (FlatAdam, FlatMLP, ImplicitQuantileNet, join_nets, lagged_copy, lagged_twins,  # noqa: E402
                                         ref_layer_keys)

DIMS = [3, 4, 2]


class _Discrete:
    def __init__(self, n):
        self.n = n


class _Box:
    def __init__(self, n):
        self.shape, self.low, self.high = (n,), np.full(n, -1.0, np.float32), np.full(n, 1.0, np.float32)


def _mlp(seed=0, dims=DIMS):
    return FlatMLP(list(dims), device="cpu", seed=seed)


def _mixer(seed=5):
    return QMIXMixer(n_agents=2, state_dim=3, mixing_embed_dim=32, hypernet_embed_dim=4, device="cpu", seed=seed)


def _rng_untouched(make):
    """make() with the global generator's state compared byte for byte around it."""
    torch.manual_seed(123)
    before = torch.get_rng_state()
    made = make()
    assert torch.equal(torch.get_rng_state(), before)
    return made


# ---- lagged copies --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_mlp, _mixer, lambda: ImplicitQuantileNet([3, 32], 2, num_cosines=8, device="cpu", seed=0)],
                         ids=["FlatMLP", "QMIXMixer", "ImplicitQuantileNet"])
def test_lagged_copy_equals_its_source_and_draws_nothing(make):
    net = make()
    twin = _rng_untouched(lambda: lagged_copy(net))
    assert type(twin) is type(net)
    assert torch.equal(twin.flat.data, net.flat.data) and twin.flat.data_ptr() != net.flat.data_ptr()
    storage = torch.full_like(net.flat.data, 7.0)
    over = lagged_copy(net, storage)
    assert over.flat.data_ptr() == storage.data_ptr() and torch.equal(storage, net.flat.data)
    twin.flat.data.add_(1.0)   # storage of its own
    assert not torch.equal(twin.flat.data, net.flat.data)


def test_learner_constructors_draw_nothing_from_the_global_generator():
    qmix = _rng_untouched(lambda: QMIXPolicy([_mlp(0), _mlp(1)], _mixer(), action_space=_Discrete(2)))
    assert torch.equal(qmix.target_flat, qmix.flat) and qmix.target_flat.data_ptr() != qmix.flat.data_ptr()
    critics = [_mlp(10 + i, [2 * (3 + 2), 4, 1]) for i in range(2)]
    maddpg = _rng_untouched(lambda: MADDPGPolicy([_mlp(0), _mlp(1)], critics, None, _Box(2), 2))
    assert torch.equal(maddpg.target_flat, maddpg.flat) and maddpg.target_flat.data_ptr() != maddpg.flat.data_ptr()
    pol = DiscreteSACPolicy(actor=_mlp(0), action_space=_Discrete(2))
    sac = _rng_untouched(lambda: DiscreteSAC(policy=pol, policy_optim=AdamOptimizerFactory(), critic=_mlp(1),
                                             critic_optim=AdamOptimizerFactory()))
    for twin, src in ((sac.critic2, sac.critic), (sac.critic_old, sac.critic), (sac.critic2_old, sac.critic2)):
        assert torch.equal(twin.flat.data, src.flat.data) and twin.flat.data_ptr() != src.flat.data_ptr()
    qpol = DiscreteQLearningPolicy(model=_mlp(0), action_space=_Discrete(2))
    dqn = _rng_untouched(lambda: DQN(policy=qpol, optim=AdamOptimizerFactory(), target_update_freq=1))
    assert torch.equal(dqn.model_old.flat.data, qpol.model.flat.data) and dqn.target_flat.data_ptr() == dqn.model_old.flat.data_ptr()
    assert dqn.target_flat.data_ptr() != qpol.model.flat.data_ptr()


# ---- joint vectors -----------------------------------------------------------------------------------------------------------
def _check_views(flat, nets, offsets, before):
    for net, o, want in zip(nets, offsets, before):
        assert net.flat.data_ptr() == flat.data_ptr() + 4 * o
        assert torch.equal(net.flat.data, want)
    assert torch.equal(flat, torch.cat(before))


def test_join_nets_layout_values_and_aliasing():
    nets = [_mlp(0), _mlp(1, [3, 2]), _mixer()]
    before = [n.flat.data.clone() for n in nets]
    flat, offs = join_nets(nets, "cpu")
    assert offs == [0, 26, 34, 34 + nets[2].flat.numel()] and flat.numel() == offs[-1] and flat.dtype == torch.float32
    _check_views(flat, nets, offs, before)
    nets[0].weight(0)[1, 2] = 9.0
    assert flat[1 * 3 + 2] == 9.0
    hypers = nets[2].nets   # the mixer's rebind goes down to every hypernetwork
    o = offs[2]
    for h in hypers:
        assert h.flat.data_ptr() == flat.data_ptr() + 4 * o
        o += h.flat.numel()
    assert o == offs[3]
    hypers[2].weight(0)[0, 0] = -5.0   # hyper_b1, the bare Linear
    assert flat[offs[2] + hypers[0].flat.numel() + hypers[1].flat.numel()] == -5.0
    target_flat, twins = _rng_untouched(lambda: lagged_twins(nets, flat, offs))
    assert torch.equal(target_flat, flat) and target_flat.data_ptr() != flat.data_ptr()
    _check_views(target_flat, twins, offs, [n.flat.data for n in nets])
    assert [type(t) for t in twins] == [FlatMLP, FlatMLP, QMIXMixer] and twins[1].dims == [3, 2]


def test_mixer_rebind_moves_every_hypernetwork():
    mixer = _mixer()
    before = mixer.flat.data.clone()
    parts = [h.flat.data.clone() for h in mixer.nets]
    storage = torch.zeros(before.numel() + 3)[3:]
    mixer.rebind(storage)
    assert mixer.flat.data_ptr() == storage.data_ptr() and torch.equal(storage, before)
    o = 0
    for h, want in zip(mixer.nets, parts):
        assert h.flat.data_ptr() == storage.data_ptr() + 4 * o and torch.equal(h.flat.data, want)
        o += want.numel()
    mixer.hyper_b2.bias(1)[0] = 3.0
    assert storage[-1] == 3.0


# ---- the Adam hand-over -------------------------------------------------------------------------------------------------------
HYPER = dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)


def _torch_adam(**kw):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], **kw)


def _is(opt, vec, coef64, lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01):
    assert isinstance(opt, FlatAdam) and opt.param.data_ptr() == vec.data_ptr() and opt.param.numel() == vec.numel()
    assert (opt.lr, tuple(opt.betas), opt.eps, opt.weight_decay, opt.coef64) == (lr, betas, eps, weight_decay, coef64)


@pytest.mark.parametrize("coef64", [False, True])
def test_adam_hand_over_accepts_every_kind(coef64):
    net = _mlp()
    vec = net.flat.data
    opt, sched = flat_adam_of(None, vec, "X: optim", coef64, ("none", "adam"))
    _is(opt, vec, coef64, 1e-3, (0.9, 0.999), 1e-8, 0.0)
    assert sched is None
    opt, sched = flat_adam_of(AdamOptimizerFactory(**HYPER), net, "X: optim", coef64, ("factory", "flat"))
    _is(opt, vec, coef64)
    assert sched is None
    factory = AdamOptimizerFactory(**HYPER).with_lr_scheduler_factory(LRSchedulerFactoryLinear(2, 10, 5))
    opt, sched = flat_adam_of(factory, net, "X: optim", coef64, ("factory",))
    assert sched is not None and sched.target is opt and opt.lr == 3e-4
    sched.step()
    assert opt.lr == pytest.approx(3e-4 * 0.75)
    own = FlatAdam(net, lr=0.5)
    assert flat_adam_of(own, net, "X: optim", coef64, ("factory", "flat")) == (own, None)
    opt, _ = flat_adam_of(_torch_adam(**HYPER), vec, "X: optim", coef64, ("none", "adam"))
    _is(opt, vec, coef64)
    two = _torch_adam(**HYPER)
    two.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=1.0))   # "adam" reads the first group only
    _is(flat_adam_of(two, vec, "X: optim", coef64, ("none", "adam"))[0], vec, coef64)
    opt, _ = flat_adam_of([_torch_adam(**HYPER), _torch_adam(**HYPER)], vec[:5], "X: optims", coef64, ("none", "adams"))
    _is(opt, vec[:5], coef64)


def test_adam_hand_over_refuses_the_rest():
    net = _mlp()
    for given, kinds in ((_torch_adam(), ("factory", "flat")), (None, ("factory",)), (AdamOptimizerFactory(), ("none", "adam")),
                         (torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), ("none", "adam")),
                         ([_torch_adam(), "x"], ("none", "adams")), ([], ("none", "adams")), (FlatAdam(net), ("factory",))):
        with pytest.raises(TypeError, match="X: optim must be "):
            flat_adam_of(given, net, "X: optim", True, kinds)
    with pytest.raises(TypeError, match="an AdamOptimizerFactory or a FlatAdam, got Adam"):
        flat_adam_of(_torch_adam(), net, "X: optim", True, ("factory", "flat"))
    for bad in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="amsgrad / maximize"):
            flat_adam_of(_torch_adam(**bad), net, "X: optim", False, ("none", "adam"))
        with pytest.raises(ValueError, match="amsgrad / maximize"):
            flat_adam_of([_torch_adam(), _torch_adam(**bad)], net, "X: optim", True, ("none", "adams"))
    with pytest.raises(ValueError, match="differ in their hyper-parameters"):
        flat_adam_of([_torch_adam(lr=1e-3), _torch_adam(lr=2e-3)], net, "X: optim", True, ("none", "adams"))
    with pytest.raises(ValueError, match="own flat parameter vector"):
        flat_adam_of(FlatAdam(_mlp()), net, "X: optim", True, ("factory", "flat"))


def test_each_learner_keeps_its_kinds_and_coefficients():
    """DQN: factory or FlatAdam, coef64; Discrete SAC: factories, coef64; QMIX: None or one torch Adam, plain coefficients;
    MADDPG: None or a list of torch Adams that agree, coef64."""
    qpol = DiscreteQLearningPolicy(model=_mlp(0), action_space=_Discrete(2))
    _is(DQN(policy=qpol, optim=AdamOptimizerFactory(**HYPER)).optim, qpol.model.flat.data, True)
    with pytest.raises(TypeError, match="AdamOptimizerFactory or a FlatAdam"):
        DQN(policy=qpol, optim=None)
    with pytest.raises(ValueError, match="own flat parameter vector"):
        DQN(policy=qpol, optim=FlatAdam(_mlp()))
    pol = DiscreteSACPolicy(actor=_mlp(0), action_space=_Discrete(2))
    sac = DiscreteSAC(policy=pol, policy_optim=AdamOptimizerFactory(**HYPER), critic=_mlp(1), critic_optim=AdamOptimizerFactory())
    _is(sac.policy_optim, pol.actor.flat.data, True)
    _is(sac.critic2_optim, sac.critic2.flat.data, True, 1e-3, (0.9, 0.999), 1e-8, 0)
    assert sac.lr_scheduler is None
    with pytest.raises(TypeError, match="DiscreteSAC: critic_optim must be an AdamOptimizerFactory"):
        DiscreteSAC(policy=pol, policy_optim=AdamOptimizerFactory(), critic=_mlp(1), critic_optim=FlatAdam(_mlp(1)))
    qmix = QMIXPolicy([_mlp(0), _mlp(1)], _mixer(), action_space=_Discrete(2), optimizer=_torch_adam(**HYPER))
    _is(qmix.optimizer, qmix.flat, False)
    plain = QMIXPolicy([_mlp(0), _mlp(1)], _mixer(), action_space=_Discrete(2))
    _is(plain.optimizer, plain.flat, False, 1e-3, (0.9, 0.999), 1e-8, 0.0)
    with pytest.raises(TypeError, match="QMIXPolicy: optimizer must be None or a torch.optim.Adam"):
        QMIXPolicy([_mlp(0), _mlp(1)], _mixer(), action_space=_Discrete(2), optimizer=[_torch_adam()])
    with pytest.raises(ValueError, match="amsgrad"):
        QMIXPolicy([_mlp(0), _mlp(1)], _mixer(), action_space=_Discrete(2), optimizer=_torch_adam(amsgrad=True))
    critics = lambda: [_mlp(10 + i, [2 * (3 + 2), 4, 1]) for i in range(2)]  # noqa: E731
    maddpg = MADDPGPolicy([_mlp(0), _mlp(1)], critics(), None, _Box(2), 2, optimizer_critics=[_torch_adam(**HYPER)] * 2)
    _is(maddpg.optimizer_actors, maddpg.flat[:maddpg.n_actor_params], True, 1e-3, (0.9, 0.999), 1e-8, 0.0)
    _is(maddpg.optimizer_critics, maddpg.flat[maddpg.n_actor_params:], True)
    with pytest.raises(TypeError, match="MADDPGPolicy: optimizer_actors must be None or a list of torch.optim.Adam"):
        MADDPGPolicy([_mlp(0), _mlp(1)], critics(), None, _Box(2), 2, optimizer_actors=AdamOptimizerFactory())


# ---- reference key names ----------------------------------------------------------------------------------------------------
def _wb(stems):
    return [(s + ".weight", s + ".bias") for s in stems]


KEYS = {
    ("body", 1): _wb(["model.model.0"]),
    ("body", 2): _wb(["model.model.0", "model.model.2"]),
    ("body", 3): _wb(["model.model.0", "model.model.2", "model.model.4"]),
    ("head", 1): _wb(["last.model.0"]),
    ("head", 2): _wb(["preprocess.model.model.0", "last.model.0"]),
    ("head", 3): _wb(["preprocess.model.model.0", "preprocess.model.model.2", "last.model.0"]),
    ("fc", 1): _wb(["fc1"]),
    ("fc", 2): _wb(["fc1", "fc2"]),
    ("fc", 3): _wb(["fc1", "fc2", "fc3"]),
    ("seq", 1): _wb(["0"]),
    ("seq", 2): _wb(["0", "2"]),
    ("seq", 3): _wb(["0", "2", "4"]),
}


@pytest.mark.parametrize("scheme,L", sorted(KEYS))
def test_key_table_and_export_load_round_trip(scheme, L):
    keys = ref_layer_keys(L, scheme)
    assert keys == KEYS[scheme, L]
    dims = [3, 4, 5, 2][:L] + [2]
    net, other = _mlp(0, dims), _mlp(1, dims)
    sd = net.export_layers(keys, "p.")
    assert list(sd) == ["p." + k for kk in keys for k in kk]
    assert all(v.data_ptr() != net.flat.data_ptr() for v in sd.values())
    assert [tuple(v.shape) for v in sd.values()] == [s for i in range(L) for s in ((dims[i + 1], dims[i]), (dims[i + 1],))]
    assert net.export_layers(keys, "q.", sd) is sd and len(sd) == 4 * L
    other.import_layers(sd, keys, "q.")
    assert torch.equal(other.flat.data, net.flat.data)
    with pytest.raises(KeyError):
        other.import_layers(sd, keys, "r.")


def test_unknown_scheme_is_refused():
    with pytest.raises(KeyError):
        ref_layer_keys(2, "nope")


def test_fc_names_are_the_nets_own_reference_state_dict():
    net, other = _mlp(0), _mlp(1)
    sd = net.to_reference_state_dict()
    assert list(sd) == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    other.load_reference_state_dict(sd)
    assert torch.equal(other.flat.data, net.flat.data)


def test_mixer_state_dict_names_and_round_trip():
    mixer, other = _mixer(5), _mixer(6)
    sd = mixer.state_dict()
    assert list(sd) == [f"{n}.{k}" for n, ks in (("hyper_w1", ("0.weight", "0.bias", "2.weight", "2.bias")),
                                                 ("hyper_w2", ("0.weight", "0.bias", "2.weight", "2.bias")),
                                                 ("hyper_b1", ("weight", "bias")),
                                                 ("hyper_b2", ("0.weight", "0.bias", "2.weight", "2.bias"))) for k in ks]
    assert "hyper_b1.weight" in sd and "hyper_b1.0.weight" not in sd
    other.load_state_dict(sd)
    assert torch.equal(other.flat.data, mixer.flat.data)
    pol = QMIXPolicy([_mlp(0), _mlp(1)], mixer, action_space=_Discrete(2))
    psd = pol.state_dict()
    assert list(psd) == ["mixer." + k for k in sd] + ["target_mixer." + k for k in sd]
    pol2 = QMIXPolicy([_mlp(2), _mlp(3)], other, action_space=_Discrete(2))
    pol2.target_mixer.flat.data.zero_()
    pol2.load_state_dict(psd)
    assert torch.equal(pol2.mixer.flat.data, pol.mixer.flat.data) and torch.equal(pol2.target_mixer.flat.data, pol.target_mixer.flat.data)
