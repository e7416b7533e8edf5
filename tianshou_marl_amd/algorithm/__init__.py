"""Algorithms on the device-resident rollout (mirror of tianshou.algorithm for the north-star path)."""
from .distq import C51, QRDQN, C51Policy, QRDQNPolicy
from .dqn import DQN, DiscreteQLearningPolicy
from .iqn import IQN, IQNPolicy
from .fqf import FQF, FQFPolicy, FQFTrainingStats
from .rainbow import RainbowDQN, RainbowPolicy
from .actor_critic import Alpha, AutoAlpha, FixedAlpha
from .dsac import DiscreteSAC, DiscreteSACPolicy, DiscreteSACTrainingStats
from .cac import (DDPG, SAC, TD3, ContinuousDeterministicPolicy, DDPGTrainingStats, GaussianNoise, SACPolicy,
                  SACTrainingStats, TD3TrainingStats)
from .redq import REDQ, REDQPolicy, REDQTrainingStats
from .cql import CQL, CQLTrainingStats
from .td3_bc import TD3BC
from .bcq import BCQ, BCQPolicy, BCQTrainingStats
from .bdqn import BDQN, BDQNPolicy
from .pg import A2C, Reinforce
from .ppo import PPO, policy_within_training_step
from .ppo_generic import GenericPPO
from .icm import ICMOffPolicyWrapper, ICMOnPolicyWrapper, ICMTrainingStats
from .gail import GAIL, GailTrainingStats

__all__ = ["PPO", "A2C", "Reinforce", "GenericPPO", "DQN", "DiscreteQLearningPolicy", "C51", "C51Policy", "QRDQN",
           "QRDQNPolicy", "IQN", "IQNPolicy", "FQF", "FQFPolicy", "FQFTrainingStats", "RainbowDQN", "RainbowPolicy",
           "DiscreteSAC", "DiscreteSACPolicy", "DiscreteSACTrainingStats", "Alpha", "FixedAlpha", "AutoAlpha",
           "DDPG", "TD3", "SAC", "ContinuousDeterministicPolicy", "SACPolicy", "DDPGTrainingStats", "TD3TrainingStats",
           "SACTrainingStats", "GaussianNoise", "REDQ", "REDQPolicy", "REDQTrainingStats", "BDQN", "BDQNPolicy",
           "policy_within_training_step", "ICMOnPolicyWrapper", "ICMOffPolicyWrapper", "ICMTrainingStats",
           "GAIL", "GailTrainingStats", "CQL", "CQLTrainingStats", "TD3BC", "BCQ", "BCQPolicy",
           "BCQTrainingStats"]
