"""Environment factory (reference gcbf/env/__init__.py:11-26)."""
import torch

from typing import Optional

from .base import MultiAgentEnv
from .point_agent import PointAgentEnv
from .simple_car import SimpleCar
from .simple_drone import SimpleDrone
from .dubins_car import DubinsCar
from .batched import SceneBatch


def make_env(env: str, num_agents: int, device: torch.device, dt: float = 0.03,
             params: Optional[dict] = None,
             max_neighbors: Optional[int] = None,
             device_reset: Optional[bool] = None) -> MultiAgentEnv:
    """``device_reset``: sample episode resets on the device; ``None`` keeps
    the env's default (off unless GCBF_AMD_DEVICE_RESET=1)."""
    if env == "SimpleCar":
        e = SimpleCar(num_agents, device, dt, params, max_neighbors)
    elif env == "SimpleDrone":
        e = SimpleDrone(num_agents, device, dt, params, max_neighbors)
    elif env == "DubinsCar":
        e = DubinsCar(num_agents, device, dt, params, max_neighbors)
    else:
        raise NotImplementedError("Env name not supported!")
    if device_reset is not None:
        e.set_device_reset(device_reset)
    return e


__all__ = ["MultiAgentEnv", "PointAgentEnv", "SimpleCar", "SimpleDrone", "DubinsCar",
           "SceneBatch", "make_env"]
