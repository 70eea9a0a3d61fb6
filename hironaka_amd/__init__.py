"""hironaka_amd -- MI355X-native batched Hironaka-game environment."""
__version__ = "0.1.0"

_VEC_ENVS = ("HironakaHostVecEnv", "HironakaAgentVecEnv")
__all__ = list(_VEC_ENVS) + ["ReplayBuffer"]


def __getattr__(name):
    # resolved on first use: importing the package alone loads neither torch nor the HIP library
    if name in _VEC_ENVS:
        from . import vec_env
        return getattr(vec_env, name)
    if name == "ReplayBuffer":
        from .replay_buffer import ReplayBuffer
        return ReplayBuffer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
