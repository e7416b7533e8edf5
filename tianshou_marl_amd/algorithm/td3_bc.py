"""TD3+BC (arXiv:2106.06860): TD3 on a recorded dataset with a behaviour-cloning term in the actor loss, on the HIP path.

Mirror of tianshou/algorithm/imitation/td3_bc.py (`TD3BC` :14-127) on cac.py's `TD3`: the critics' steps, the
delayed actor update (quirk Q45), `_last` and the priority write-back are TD3's; only the actor's loss head differs --
`tsm_td3bc_actor_head` (csrc/cql.hip) in place of `tsm_cac_det_actor_head`.  The dataset lives in a device
`VectorReplayBuffer(act_dim=k)`; `update(buffer, sample_size)` is the off-policy learners'.
"""
from __future__ import annotations

from .. import ops
from ..utils.net import ContinuousCritic
from .cac import TD3, ContinuousDeterministicPolicy
from .optim import AdamOptimizerFactory


class TD3BC(TD3):
    """td3_bc.py:14-127."""

    def __init__(self, *, policy: ContinuousDeterministicPolicy, policy_optim: AdamOptimizerFactory, critic: ContinuousCritic,
                 critic_optim: AdamOptimizerFactory, critic2: ContinuousCritic | None = None,
                 critic2_optim: AdamOptimizerFactory | None = None, tau: float = 0.005, gamma: float = 0.99,
                 policy_noise: float = 0.2, update_actor_freq: int = 2, noise_clip: float = 0.5, alpha: float = 2.5,
                 n_step_return_horizon: int = 1) -> None:
        super().__init__(policy=policy, policy_optim=policy_optim, critic=critic, critic_optim=critic_optim, critic2=critic2,
                         critic2_optim=critic2_optim, tau=tau, gamma=gamma, policy_noise=policy_noise,
                         update_actor_freq=update_actor_freq, noise_clip=noise_clip, n_step_return_horizon=n_step_return_horizon)
        self.alpha = alpha

    def _det_actor_head(self, dq_da, omt2, q_pi, act_pi, act) -> dict:
        """actor_loss = -lmbda q.mean() + mse(act, batch.act) with lmbda = alpha / |q|.mean(), detached (td3_bc.py:114-117)."""
        return ops.td3bc_actor_head(dq_da, omt2, q_pi, act_pi, act, self.alpha, self.policy.actor.max_action)
