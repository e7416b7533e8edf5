"""CPU tests of the Gaussian-policy entries: `tsm_gauss_check` and the `ops` wrappers refuse act_dim 0 and 65 and CPU tensors
before anything is launched, and `GaussianActorCritic` lays out one vector under the reference's checkpoint keys."""
import pytest

torch = pytest.importorskip("torch")

from tianshou_marl_amd import _abi, _build, ops  # noqa: E402
from tianshou_marl_amd.utils.net import GaussianActorCritic  # noqa: E402


def test_act_dim_bounds_and_cpu_tensors_are_refused():
    _build.build()
    _abi.load()
    ops.gauss_check(1)
    ops.gauss_check(_abi.CAC_MAX_ACT_DIM)
    cfg = ops.make_ppo_cfg()
    q = torch.zeros(4)
    for Ad, msg in ((0, r"act_dim = 0 outside \[1, 64\]"), (65, r"act_dim = 65 outside \[1, 64\]")):
        raw, sg = torch.zeros(4, Ad), torch.zeros(Ad)
        calls = [lambda: ops.gauss_check(Ad), lambda: _abi.call("tsm_gauss_check", Ad),
                 lambda: ops.gauss_sample(raw, 0, sigma_param=sg), lambda: ops.gauss_sample(torch.zeros(4, 2 * Ad), 0),
                 lambda: ops.gauss_logp_entropy(raw, raw, sigma_param=sg), lambda: ops.gauss_ppo_head(raw, raw, q, q, cfg, sigma_param=sg),
                 lambda: ops.gauss_sigma_fold(torch.zeros(1, Ad, dtype=torch.float64), 1, torch.zeros(2, Ad)),
                 lambda: _abi.call("tsm_gauss_sigma_fold", None, 1, Ad, 1, None, 0, None)]
        for f in calls:
            with pytest.raises(ValueError, match=msg):
                f()
    raw, sg = torch.zeros(4, 3), torch.zeros(3)
    for f in (lambda: ops.gauss_sample(raw, 0, sigma_param=sg), lambda: ops.gauss_logp_entropy(torch.zeros(4, 6), raw),
              lambda: ops.gauss_ppo_head(raw, raw, q, q, cfg, sigma_param=sg),
              lambda: ops.gauss_sigma_fold(torch.zeros(1, 3, dtype=torch.float64), 1, torch.zeros(2, 3))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


@pytest.mark.parametrize("cond", [False, True])
def test_gaussian_actor_critic_is_one_vector_under_the_reference_keys(cond):
    net = GaussianActorCritic(6, 3, (16, 16), conditioned_sigma=cond, critic_obs_dim=12, device="cpu", seed=0)
    n_mlp = 16 * 6 + 16 + 16 * 16 + 16 + (6 if cond else 3) * 17
    assert (net.n_actor, net.n_critic) == (n_mlp + (0 if cond else 3), 16 * 12 + 16 + 16 * 16 + 16 + 17)
    assert net.flat.numel() == net.n_actor + net.n_critic and (net.obs_dim, net.critic_obs_dim, net.act_dim) == (6, 12, 3)
    assert net.actor.flat.data_ptr() == net.flat.data_ptr() and net.critic.flat.data_ptr() == net.flat.data[net.n_actor:].data_ptr()
    keys = [k for k, _ in net.reference_named_views()]
    head = ["policy.actor.sigma_param"] if not cond else []
    tail = ["policy.actor.sigma.model.0.weight", "policy.actor.sigma.model.0.bias"] if cond else []
    assert keys == head + [f"policy.actor.preprocess.model.model.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")] + \
        ["policy.actor.mu.model.0.weight", "policy.actor.mu.model.0.bias"] + tail + \
        [f"critic.preprocess.model.model.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")] + \
        ["critic.last.model.0.weight", "critic.last.model.0.bias"]
    assert sum(v.numel() for v in net.param_views()) == net.flat.numel()
    if not cond:
        assert not net.actor.sigma_param.any() and net.actor.sigma_param.data_ptr() == net.flat.data[n_mlp:].data_ptr()
    sd = net.to_reference_state_dict()
    other = GaussianActorCritic(6, 3, (16, 16), conditioned_sigma=cond, critic_obs_dim=12, device="cpu", seed=1, init="default")
    assert not torch.equal(other.flat.data, net.flat.data)
    other.load_reference_state_dict(sd)
    assert torch.equal(other.flat.data, net.flat.data)
