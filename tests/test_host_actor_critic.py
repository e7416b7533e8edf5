"""CPU tests of the actor-critic learners' shared core (algorithm/actor_critic.py): DDPG, TD3, SAC, REDQ and DiscreteSAC, with
a fixed and an auto-tuned alpha where the learner has one, are built on the host at small sizes (nothing is launched).

The literal key lists below were taken by running this file's `build` at the commit before `DiscreteSAC` moved onto
`ActorDualCriticsOffPolicyAlgorithm` and the entropy coefficient became one mixin: a checkpoint of either side loads at the other
only while they stay as they are, in this order.
"""
import pytest
import torch

D, H, A, AD, E = 6, 16, 5, 3, 3   # obs, hidden, discrete actions, Box components, ensemble members


class _Discrete:
    def __init__(self, n):
        self.n = n


class _Box:
    def __init__(self, n):
        self.low, self.high, self.shape = [-1.0] * n, [1.0] * n, (n,)


def build(kind: str):
    """kind: ddpg | td3 | sac_fix | sac_auto | redq_fix | redq_auto | dsac_fix | dsac_auto."""
    from tianshou_marl_amd.algorithm import (DDPG, REDQ, SAC, TD3, AutoAlpha, ContinuousDeterministicPolicy, DiscreteSAC,
                                             DiscreteSACPolicy, REDQPolicy, SACPolicy)
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.utils.net import (ContinuousActorDeterministic, ContinuousActorProbabilistic, ContinuousCritic,
                                             EnsembleCritic, FlatMLP)

    opt = lambda: AdamOptimizerFactory(lr=1e-3)  # noqa: E731
    name, _, alpha = kind.partition("_")
    alpha = dict(alpha=AutoAlpha(-1.0, -0.5, opt()) if alpha == "auto" else 0.2) if alpha else {}
    if name == "dsac":
        pol = DiscreteSACPolicy(actor=FlatMLP([D, H, A], device="cpu", seed=0), action_space=_Discrete(A))
        return DiscreteSAC(policy=pol, policy_optim=opt(), critic=FlatMLP([D, H, A], device="cpu", seed=1), critic_optim=opt(),
                           **alpha)
    crit = lambda s: ContinuousCritic(D, AD, (H,), device="cpu", seed=s)  # noqa: E731
    if name in ("ddpg", "td3"):
        pol = ContinuousDeterministicPolicy(actor=ContinuousActorDeterministic(D, AD, (H,), device="cpu", seed=0),
                                            action_space=_Box(AD))
        more = dict(critic2=crit(2)) if name == "td3" else {}
        return (TD3 if name == "td3" else DDPG)(policy=pol, policy_optim=opt(), critic=crit(1), critic_optim=opt(), **more)
    actor = ContinuousActorProbabilistic(D, AD, (H,), conditioned_sigma=True, device="cpu", seed=0)
    if name == "sac":
        return SAC(policy=SACPolicy(actor=actor, action_space=_Box(AD)), policy_optim=opt(), critic=crit(1), critic_optim=opt(),
                   critic2=crit(2), **alpha)
    return REDQ(policy=REDQPolicy(actor=actor, action_space=_Box(AD)), policy_optim=opt(),
                critic=EnsembleCritic(D, AD, E, (H,), device="cpu", seed=1), critic_optim=opt(), ensemble_size=E, subset_size=2,
                **alpha)


STATE_KEYS = {
    "ddpg": ["policy.actor", "critic", "critic_old.module", "actor_old.module", "policy_optim", "critic_optim", "sample_ctr"],
    "td3": ["policy.actor", "critic", "critic_old.module", "critic2", "critic2_old.module", "actor_old.module", "policy_optim",
            "critic_optim", "critic2_optim", "sample_ctr", "_cnt", "_last"],
    "sac_fix": ["policy.actor", "critic", "critic_old.module", "critic2", "critic2_old.module", "policy_optim", "critic_optim",
                "critic2_optim", "sample_ctr"],
    "redq_fix": ["policy.actor", "critic", "critic_old.module", "policy_optim", "critic_optim", "sample_ctr",
                 "critic_gradient_step", "_last_actor_loss"],
    "dsac_fix": ["policy.actor", "critic", "critic_old.module", "critic2", "critic2_old.module", "policy_optim", "critic_optim",
                 "critic2_optim"],
}
REFERENCE_KEYS = {
    "ddpg": [
        "policy.actor.preprocess.model.model.0.weight", "policy.actor.preprocess.model.model.0.bias",
        "policy.actor.last.model.0.weight", "policy.actor.last.model.0.bias",
        "critic.preprocess.model.model.0.weight", "critic.preprocess.model.model.0.bias",
        "critic.last.model.0.weight", "critic.last.model.0.bias",
        "critic_old.module.preprocess.model.model.0.weight", "critic_old.module.preprocess.model.model.0.bias",
        "critic_old.module.last.model.0.weight", "critic_old.module.last.model.0.bias",
        "actor_old.module.preprocess.model.model.0.weight", "actor_old.module.preprocess.model.model.0.bias",
        "actor_old.module.last.model.0.weight", "actor_old.module.last.model.0.bias"],
    "td3": [
        "policy.actor.preprocess.model.model.0.weight", "policy.actor.preprocess.model.model.0.bias",
        "policy.actor.last.model.0.weight", "policy.actor.last.model.0.bias",
        "critic.preprocess.model.model.0.weight", "critic.preprocess.model.model.0.bias",
        "critic.last.model.0.weight", "critic.last.model.0.bias",
        "critic_old.module.preprocess.model.model.0.weight", "critic_old.module.preprocess.model.model.0.bias",
        "critic_old.module.last.model.0.weight", "critic_old.module.last.model.0.bias",
        "critic2.preprocess.model.model.0.weight", "critic2.preprocess.model.model.0.bias",
        "critic2.last.model.0.weight", "critic2.last.model.0.bias",
        "critic2_old.module.preprocess.model.model.0.weight", "critic2_old.module.preprocess.model.model.0.bias",
        "critic2_old.module.last.model.0.weight", "critic2_old.module.last.model.0.bias",
        "actor_old.module.preprocess.model.model.0.weight", "actor_old.module.preprocess.model.model.0.bias",
        "actor_old.module.last.model.0.weight", "actor_old.module.last.model.0.bias"],
    "sac_fix": [
        "policy.actor.preprocess.model.model.0.weight", "policy.actor.preprocess.model.model.0.bias",
        "policy.actor.mu.model.0.weight", "policy.actor.mu.model.0.bias",
        "policy.actor.sigma.model.0.weight", "policy.actor.sigma.model.0.bias",
        "critic.preprocess.model.model.0.weight", "critic.preprocess.model.model.0.bias",
        "critic.last.model.0.weight", "critic.last.model.0.bias",
        "critic_old.module.preprocess.model.model.0.weight", "critic_old.module.preprocess.model.model.0.bias",
        "critic_old.module.last.model.0.weight", "critic_old.module.last.model.0.bias",
        "critic2.preprocess.model.model.0.weight", "critic2.preprocess.model.model.0.bias",
        "critic2.last.model.0.weight", "critic2.last.model.0.bias",
        "critic2_old.module.preprocess.model.model.0.weight", "critic2_old.module.preprocess.model.model.0.bias",
        "critic2_old.module.last.model.0.weight", "critic2_old.module.last.model.0.bias"],
    "redq_fix": [
        "policy.actor.preprocess.model.model.0.weight", "policy.actor.preprocess.model.model.0.bias",
        "policy.actor.mu.model.0.weight", "policy.actor.mu.model.0.bias",
        "policy.actor.sigma.model.0.weight", "policy.actor.sigma.model.0.bias",
        "critic.preprocess.model.model.0.weight", "critic.preprocess.model.model.0.bias_weights",
        "critic.last.model.0.weight", "critic.last.model.0.bias_weights",
        "critic_old.module.preprocess.model.model.0.weight", "critic_old.module.preprocess.model.model.0.bias_weights",
        "critic_old.module.last.model.0.weight", "critic_old.module.last.model.0.bias_weights"],
    "dsac_fix": [
        "policy.actor.preprocess.model.model.0.weight", "policy.actor.preprocess.model.model.0.bias",
        "policy.actor.last.model.0.weight", "policy.actor.last.model.0.bias",
        "critic.preprocess.model.model.0.weight", "critic.preprocess.model.model.0.bias",
        "critic.last.model.0.weight", "critic.last.model.0.bias",
        "critic_old.module.preprocess.model.model.0.weight", "critic_old.module.preprocess.model.model.0.bias",
        "critic_old.module.last.model.0.weight", "critic_old.module.last.model.0.bias",
        "critic2.preprocess.model.model.0.weight", "critic2.preprocess.model.model.0.bias",
        "critic2.last.model.0.weight", "critic2.last.model.0.bias",
        "critic2_old.module.preprocess.model.model.0.weight", "critic2_old.module.preprocess.model.model.0.bias",
        "critic2_old.module.last.model.0.weight", "critic2_old.module.last.model.0.bias"],
}
for _k in ("sac", "redq", "dsac"):   # an auto-tuned alpha was, and stays, the one further and last entry of both layouts
    STATE_KEYS[f"{_k}_auto"] = STATE_KEYS[f"{_k}_fix"] + ["alpha"]
    REFERENCE_KEYS[f"{_k}_auto"] = REFERENCE_KEYS[f"{_k}_fix"] + ["alpha._log_alpha"]
ALPHA_KEYS = ["log_alpha", "exp_avg", "exp_avg_sq", "step", "alpha"]
COUNTERS = {"td3": dict(_cnt=5, _last=-0.75), "redq": dict(critic_gradient_step=7, _last_actor_loss=-0.25)}
KINDS = sorted(STATE_KEYS)


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_keys_are_the_recorded_ones(kind):
    algo = build(kind)
    sd = algo.state_dict()
    assert list(sd.keys()) == STATE_KEYS[kind]
    assert list(algo.to_reference_state_dict().keys()) == REFERENCE_KEYS[kind]
    if kind.endswith("_auto"):
        assert list(sd["alpha"].keys()) == ALPHA_KEYS


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trips_nets_counters_and_alpha(kind):
    algo, other = build(kind), build(kind)
    name = kind.partition("_")[0]
    for i, (_, net) in enumerate(algo._nets()):
        net.flat.data.add_(0.125 * (i + 1))
    for k, v in COUNTERS.get(name, {}).items():
        setattr(algo, k, v)
    algo.policy._sample_ctr = 123
    if kind.endswith("_auto"):
        algo.alpha.set_log_alpha(-0.25)
        algo.alpha._exp_avg.fill_(0.5)
        algo.alpha._step.fill_(3)
    other.load_state_dict(algo.state_dict())
    for (_, a), (_, b) in zip(algo._nets(), other._nets()):
        assert torch.equal(a.flat.data, b.flat.data)
    for k, v in COUNTERS.get(name, {}).items():
        assert getattr(other, k) == v
    assert other.policy._sample_ctr == (0 if name == "dsac" else 123)   # Discrete SAC's checkpoint never carried the counter
    if kind.endswith("_auto"):
        assert float(other.alpha._log_alpha) == -0.25 and float(other.alpha._exp_avg) == 0.5 and int(other.alpha._step) == 3
        assert torch.equal(other.alpha._alpha_dev, algo.alpha._alpha_dev)
    again = other.state_dict()
    assert list(again.keys()) == STATE_KEYS[kind]
    ref = algo.to_reference_state_dict()
    third = build(kind)
    third.load_reference_state_dict(ref)
    for (_, a), (_, b) in zip(algo._nets(), third._nets()):
        assert torch.equal(a.flat.data, b.flat.data)
    if kind.endswith("_auto"):
        assert float(third.alpha._log_alpha) == -0.25


def test_discrete_sac_stands_on_the_twin_critic_base_and_alpha_is_one_object():
    from tianshou_marl_amd import algorithm
    from tianshou_marl_amd.algorithm import actor_critic, cac, dsac

    assert actor_critic.ActorDualCriticsOffPolicyAlgorithm in dsac.DiscreteSAC.__mro__
    assert cac.ActorDualCriticsOffPolicyAlgorithm is actor_critic.ActorDualCriticsOffPolicyAlgorithm
    assert dsac.Alpha is actor_critic.Alpha is algorithm.Alpha
    assert dsac.AutoAlpha is actor_critic.AutoAlpha is algorithm.AutoAlpha
    assert dsac.FixedAlpha is actor_critic.FixedAlpha is algorithm.FixedAlpha
    assert dsac.DiscreteSAC is algorithm.DiscreteSAC


def test_lr_scheduler_is_none_without_a_scheduler_and_steps_each_once():
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory, LRSchedulerFactoryLinear

    for kind in KINDS:
        assert build(kind).lr_scheduler is None, kind
    from tianshou_marl_amd.algorithm import DiscreteSAC, DiscreteSACPolicy
    from tianshou_marl_amd.utils.net import FlatMLP

    sched = lambda: AdamOptimizerFactory(lr=1e-3).with_lr_scheduler_factory(LRSchedulerFactoryLinear(2, 10, 5))  # noqa: E731
    pol = DiscreteSACPolicy(actor=FlatMLP([D, H, A], device="cpu", seed=0), action_space=_Discrete(A))
    algo = DiscreteSAC(policy=pol, policy_optim=sched(), critic=FlatMLP([D, H, A], device="cpu", seed=1),
                       critic_optim=AdamOptimizerFactory(), critic2_optim=sched())
    assert len(algo.lr_scheduler.scheds) == 2
    before = [s.last_epoch for s in algo.lr_scheduler.scheds]
    algo.lr_scheduler.step()
    assert [s.last_epoch for s in algo.lr_scheduler.scheds] == [b + 1 for b in before]
