"""pednstream_amd -- MI355X-native engine for PedNStream's per-timestep ``network_loading`` hot path.

Public surface (mirrors the reference's for this path):
    NetworkEnvGenerator   scenario directory -> Network            (reference src/utils/env_loader.py)
    Network               network_loading(t), links, nodes, ...    (reference src/LTM/network.py)
    load_config           YAML/JSON scenario -> config dict         (reference src/utils/config.py)
    RolloutStore, gae, compute_gae   on-policy rollouts and GAE on the device (reference rl/agents/PPO_org.py, rl/rl_utils.py)
    ReplayStore           off-policy replay ring with stacked observations on the device (reference rl/rl_utils.py ReplayBuffer, rl/agents/SAC.py)
    StackedActors         the stacked SAC / PPO actors of all agents for all envs in one launch (reference rl/agents/SAC.py, PPO_org.py)
    SacTargets            SAC TD targets of a minibatch and the Polyak update of every target critic, one launch each (reference rl/agents/SAC.py)
    PpoTargets            PPO's value critics and old log-probabilities of a whole rollout in one launch (reference rl/agents/PPO_org.py)
"""
from .config import load_config
from .env_loader import NetworkEnvGenerator
from .network import Network
from .policy import StackedActors
from .ppo import PpoTargets
from .replay import ReplayStore
from .rollout import RolloutStore, compute_gae, gae
from .sac import SacTargets

__all__ = ["NetworkEnvGenerator", "Network", "load_config", "RolloutStore", "gae", "compute_gae", "ReplayStore", "StackedActors", "SacTargets", "PpoTargets"]
__version__ = "0.1.0"
