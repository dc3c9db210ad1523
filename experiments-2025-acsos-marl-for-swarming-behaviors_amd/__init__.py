"""MI355X-native hot path of davidedomini/experiments-2025-acsos-marl-for-swarming-behaviors.

Import as ``swarm_amd`` (the top-level shim ``swarm_amd.py`` maps that name to
this directory).  Public surface mirrors the reference:

    from swarm_amd import make_env, GoToPositionScenario, ObstacleAvoidanceScenario
    from swarm_amd import GCN, GAT3, DQNTrainer, GraphReplayBuffer, Simulator, set_seed, get_scenario
    from swarm_amd import SwarmEngine          # the fused device engine underneath
    from swarm_amd import SwarmGat3Engine      # the three-layer GAT's learner (unfused device tick)
    from swarm_amd import SwarmPopulation, PopulationTrainer   # many seeds in one launch
    from swarm_amd import SwarmGat3Population, Gat3PopulationTrainer   # ... of the three-layer GAT
    from swarm_amd import ActorPopulation, PopulationSimulator # many policies in one rollout launch

The compute path is libswarm_hip.so (csrc/, C ABI in include/swarm_hip.h); there
is no CPU fallback.
"""
from ._lib import load as load_library  # noqa: F401
from .engine import SwarmEngine, SwarmGat3Engine, flatten_state_dict, unflatten_params  # noqa: F401
from .graph import (Batch, Data, create_graph_from_observations, create_knn_graph_from_observations,  # noqa: F401
                    create_radius_graph_from_observations)
from .gcn import GAT3, GCN  # noqa: F401
from .scenarios import (BaseScenario, FlockingScenario, GoToPositionScenario, ObstacleAvoidanceScenario,  # noqa: F401
                        get_scenario)
from .env import Environment, make_env  # noqa: F401
from .population import ActorPopulation, SwarmGat3Population, SwarmPopulation  # noqa: F401
from .dqn import DQNTrainer, Gat3PopulationTrainer, GraphReplayBuffer, PopulationTrainer, set_seed  # noqa: F401
from .simulator import PopulationSimulator, Simulator  # noqa: F401

__all__ = ["SwarmEngine", "SwarmGat3Engine", "SwarmPopulation", "PopulationTrainer", "SwarmGat3Population", "Gat3PopulationTrainer", "ActorPopulation", "PopulationSimulator", "Data", "Batch", "GCN", "GAT3", "make_env", "Environment", "GoToPositionScenario",
           "ObstacleAvoidanceScenario", "FlockingScenario", "BaseScenario", "get_scenario", "DQNTrainer", "GraphReplayBuffer",
           "set_seed", "Simulator", "create_graph_from_observations", "create_knn_graph_from_observations",
           "create_radius_graph_from_observations"]
