"""Multi-agent layer: policy containers, dispatch, CTDE and the training coordinators
(mirror of /root/reference/tianshou/algorithm/multiagent/__init__.py)."""
from ...data.stats import MapTrainingStats
from .ctde import CentralizedCritic, CTDEPolicy, DecentralizedActor, GlobalStateConstructor
from .flexible_policy import FlexibleMultiAgentPolicyManager
from .maddpg import MADDPGPolicy
from .qmix import QMIXMixer, QMIXPolicy
from .marl import MARLDispatcher, MultiAgentOffPolicyAlgorithm, MultiAgentOnPolicyAlgorithm, MultiAgentPolicy
from .training_coordinator import (
    LeaguePlayTrainer,
    MATrainer,
    SelfPlayTrainer,
    SequentialTrainer,
    SimultaneousTrainer,
    agent_batches_from_buffer,
)

__all__ = [
    "MultiAgentPolicy", "MultiAgentOnPolicyAlgorithm", "MultiAgentOffPolicyAlgorithm", "MARLDispatcher", "MapTrainingStats",
    "FlexibleMultiAgentPolicyManager", "MATrainer", "SimultaneousTrainer", "SequentialTrainer",
    "SelfPlayTrainer", "LeaguePlayTrainer", "agent_batches_from_buffer", "CTDEPolicy", "GlobalStateConstructor",
    "DecentralizedActor", "CentralizedCritic", "QMIXMixer", "QMIXPolicy", "MADDPGPolicy",
]
