"""The games whose rules live entirely in the reference tree plus a tiny registry
standing in for `gym.make` (reference pantheonrl/envs/__init__.py:3-21)."""
from .rps import RPSEnv, RPSWeightedAgent  # noqa: F401
from .liar import LiarEnv, LiarDefaultAgent  # noqa: F401
from .blockworld import (BlockEnv, DefaultConstructorAgent, SBWDefaultAgent, SBWEasyPartner,  # noqa: F401
                         SimpleBlockEnv)

REGISTRY = {"RPS-v0": RPSEnv, "LiarsDice-v0": LiarEnv, "BlockEnv-v0": SimpleBlockEnv, "BlockEnv-v1": BlockEnv}


def make(env_id: str, **kwargs):
    if env_id not in REGISTRY:
        raise KeyError(f"unknown environment id {env_id!r}; known: {sorted(REGISTRY)}")
    return REGISTRY[env_id](**kwargs)
