"""hironaka_amd -- MI355X-native batched Hironaka-game environment."""
__version__ = "0.1.0"

_VEC_ENVS = ("HironakaHostVecEnv", "HironakaAgentVecEnv")
_DQN = ("fit_network", "td_loss", "td_target", "update_target_net", "polyak_update", "zip_equal")
_OPTIM = ("Adam", "AdamW", "SGD", "clip_grad_norm_", "safe_clip_grads_", "from_torch")
_LOSS = ("policy_value_loss", "compute_loss", "clip_log")
_NETS = ("create_mlp", "expand_net_list", "FusedSequential", "fuse", "BaseFeaturesExtractor", "HostFeatureExtractor",
         "AgentFeatureExtractor")
_HOSTS = ("Spivakovsky", "RandomSpivakovsky")
_TRAINERS = {"Trainer": "trainer", "DQNTrainer": "dqn_trainer"}
__all__ = (list(_VEC_ENVS) + ["ReplayBuffer"] + list(_DQN) + list(_OPTIM) + list(_LOSS) + list(_NETS) + list(_HOSTS)
           + list(_TRAINERS))


def __getattr__(name):
    # resolved on first use: importing the package alone loads neither torch nor the HIP library
    if name in _VEC_ENVS:
        from . import vec_env
        return getattr(vec_env, name)
    if name == "ReplayBuffer":
        from .replay_buffer import ReplayBuffer
        return ReplayBuffer
    if name in _DQN:
        from . import dqn
        return getattr(dqn, name)
    if name in _OPTIM:
        from . import optim
        return getattr(optim, name)
    if name in _LOSS:
        from . import loss
        return getattr(loss, name)
    if name in _NETS:
        from . import nets
        return getattr(nets, name)
    if name in _HOSTS:
        from . import host
        return getattr(host, name)
    if name in _TRAINERS:
        import importlib
        return getattr(importlib.import_module(f".{_TRAINERS[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
