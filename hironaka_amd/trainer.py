"""``Trainer`` -- the base of the DQN trainers, the counterpart of ``hironaka/trainer/trainer.py:24-606``: it reads the
one nested config, builds the two Q-networks, their optimisers, schedulers and replay buffers and the ``FusedGame``, and
offers roll-outs, evaluation, copying and saving.  A subclass implements ``_train`` (``dqn_trainer.DQNTrainer``).

What differs from the reference, all of it because everything lives on a HIP device:
  * networks are ``nets.create_mlp`` stacks (one launch per forward), optimisers ``hironaka_amd.optim.Adam`` / ``SGD``
    (``dqn.fit_network`` then clips and steps in two launches), the replay buffer ``replay_buffer.ReplayBuffer``, the
    points ``HipPoints``;
  * ``collect_rollout`` pushes through ``FusedGame.collect``: no ``[keep]`` whose size comes back to the host;
  * ``get_rho_for_pair`` and ``count_actions(..., er=0.0)`` play through ``FusedGame.evaluate``: two kernels around the
    two network launches per move, the accounting on the device, nothing read back;
  * ``use_cuda: false`` raises ``FusedGame``'s TypeError (there is no CPU path); more than one entry in ``use_cuda_ids``
    (DataParallel) raises NotImplementedError; ``use_tensorboard: true`` needs tensorboard and raises an ImportError
    naming the key without it;
  * ``set_learning_rate`` skips a role without a scheduler instead of stopping at it.
"""
import abc
import contextlib
import logging
from copy import deepcopy
from typing import Any, Callable, Dict, List, Optional, Type, Union

import torch
import yaml
from torch import nn

from . import optim
from .core import HipPoints
from .fused_game import FusedGame, Timer
from .host_action_preprocess import HostActionEncoder
from .nets import AgentFeatureExtractor, HostFeatureExtractor, create_mlp
from .player_modules import (AllCoordHostModule, ChooseFirstAgentModule, DummyModule, RandomAgentModule,
                             RandomHostModule)
from .replay_buffer import ReplayBuffer
from .scheduler import (ConstantScheduler, ExponentialERScheduler, ExponentialLRScheduler, InverseLRScheduler,
                        Scheduler)

ROLES = ("host", "agent")


def _summary_writer(comment: str):
    """tensorboard's SummaryWriter, imported only where `use_tensorboard` asks for it"""
    try:
        from torch.utils.tensorboard import SummaryWriter
    except ImportError as err:
        raise ImportError("'use_tensorboard: true' needs the tensorboard package, which is not installed. Install it or "
                          "set 'use_tensorboard: false'.") from err
    return SummaryWriter(comment=comment)


class Trainer(abc.ABC):
    """All hyperparameters come from `config` (a nested dict, or the path of a YAML file); no key has a default in the
    class.  Role-specific keys that are plain assignments are listed in `role_specific_hyperparameters` and become
    `self.{role}_{key}`; `get_all_role_specific_param(role)` returns them as a dict.

    A role present in the config is trained unless its net is a DummyModule; a role absent from the config must be
    given a net and is not trained.  Implement `_train()`."""

    optim_dict = {"adam": optim.Adam, "sgd": optim.SGD}
    lr_scheduler_dict = {"constant": ConstantScheduler, "exponential": ExponentialLRScheduler,
                         "inverse": InverseLRScheduler}
    er_scheduler_dict = {"constant": ConstantScheduler, "exponential": ExponentialERScheduler}
    replay_buffer_dict = {"base": ReplayBuffer}

    role_specific_hyperparameters = ["batch_size", "initial_rollout_size", "max_rollout_step"]

    def __init__(self, config: Union[Dict[str, Any], str], device_num: int = 0, host_net: Optional[nn.Module] = None,
                 agent_net: Optional[nn.Module] = None, reward_func: Optional[Callable] = None,
                 point_cls: Optional[Type[HipPoints]] = HipPoints,
                 dtype: Optional[Union[Type, torch.dtype]] = torch.float32, use_cuda_ids: Optional[List[int]] = None,
                 fused_training: bool = False):
        self.logger = logging.getLogger(__class__.__name__)
        self.device_num = device_num
        if isinstance(config, str):
            self.config = self.load_yaml(config)
        elif isinstance(config, dict):
            self.config = config
        else:
            raise TypeError(f"config must be either a str or dict. Got{type(config)}.")
        self.total_num_steps = 0

        # -------- the mandatory top-level keys -------- #
        self.use_tensorboard = self.config["use_tensorboard"]
        self.layerwise_logging = self.config["layerwise_logging"]
        self.log_time = self.config["log_time"]
        self.use_cuda = self.config["use_cuda"]
        self.scale_observation = self.config["scale_observation"]
        self.version_string = self.config["version_string"]
        self.use_cuda_ids = use_cuda_ids if use_cuda_ids else [self.device_num]
        if len(self.use_cuda_ids) > 1:
            raise NotImplementedError(f"more than one entry in use_cuda_ids (DataParallel) is not supported. Got "
                                      f"{self.use_cuda_ids}.")
        self.device = torch.device(f"cuda:{device_num}") if self.use_cuda else torch.device("cpu")
        if self.device.type != "cuda":  # what FusedGame says at the end of the constructor, said before anything is built
            raise TypeError(f"FusedGame steps HipPoints on a HIP device (there is no CPU path). Got {self.device}.")

        self.dimension = self.config["dimension"]
        self.host_action_encoder = HostActionEncoder(self.dimension)
        self.max_num_points = self.config["max_num_points"]
        self.max_value = self.config["max_value"]
        self.point_cls = point_cls
        self.dtype = dtype
        self.fused_training = fused_training

        # the features of a state are its rows, reordered
        self.feature_shape = torch.Size((self.max_num_points, self.dimension))
        self.feature_dim = self.max_num_points * self.dimension

        self.host_net = host_net
        self.agent_net = agent_net
        assert any(role in self.config for role in ROLES), \
            "Must have at least one role out of ['host', 'agent'] in the config."
        self.trained_roles = []
        for role, net in zip(ROLES, [host_net, agent_net]):
            if role in self.config and not isinstance(net, DummyModule):
                self.trained_roles.append(role)
            elif role not in self.config:
                assert net is not None, f"{role} is not present in config. A network must be given during init."

        self.time_log = dict()
        self.string_suffix = f"-{self.version_string}-cuda_{device_num}"
        if self.use_tensorboard:
            self.tb_writer = _summary_writer(self.string_suffix)

        heads = {"host": HostFeatureExtractor, "agent": AgentFeatureExtractor}
        input_dims = {"host": self.feature_dim, "agent": self.feature_dim + self.dimension}
        output_dims = {"host": 2 ** self.dimension - self.dimension - 1, "agent": self.dimension}
        pretrained_nets = {"host": host_net, "agent": agent_net}
        self.reward_func = reward_func
        self.use_replay_buffer = False
        self.last_evaluation = None  # the EvalResult of the latest get_rho_for_pair / count_actions(er=0.0)

        for role in ROLES:
            if role not in self.config:
                continue
            self._make_network(role, heads[role], input_dims[role], output_dims[role], pretrained_nets[role])
            self._make_er_scheduler(role)
            setattr(self, f"{role}_optim_config", self.config[role]["optim"])
            if not isinstance(self.get_net(role), DummyModule):
                self._make_optimizer_and_lr(role)
                self._make_replay_buffer(role, output_dims[role])

        assert self.host_net is not None and self.agent_net is not None
        self._make_fused_game()
        if self.use_replay_buffer:
            for role in self.trained_roles:
                self.collect_rollout(role, getattr(self, f"{role}_initial_rollout_size"))

    def replace_nets(self, host_net: nn.Module = None, agent_net: nn.Module = None) -> None:
        """Override host_net and / or agent_net.  Input and output widths are the caller's responsibility."""
        for role, net in zip(ROLES, [host_net, agent_net]):
            if net is not None:
                setattr(self, f"{role}_net", net.to(self.device))
                if isinstance(net, DummyModule):
                    self.trained_roles.remove(role)
                elif role in self.config:
                    self._set_optim(role)
        self._make_fused_game()

    def set_trainable(self, players: List[str]):
        for role in players:
            if role not in ROLES:
                continue
            assert not isinstance(self.get_net(role), DummyModule), f"{role} net cannot be DummyModule."
            if role not in self.trained_roles:
                self.trained_roles.append(role)

    def replace_reward_func(self, reward_func: Callable):
        self.reward_func = reward_func
        self._make_fused_game()

    def train(self, steps: int, evaluation_interval: int = 1000, **kwargs):
        """`steps` steps of `_train`, in training mode; the nets are back in eval mode afterwards."""
        self.set_training(True)
        with Timer("train_total", self.time_log, active=self.log_time, use_cuda=self.use_cuda):
            self._train(steps, evaluation_interval=evaluation_interval, **kwargs)
        self.set_training(False)

    def collect_rollout(self, role: str, num_of_games: int):
        """Play `num_of_games` fresh games for up to `max_rollout_step` moves and push every experience of `role` into
        its replay buffer (`FusedGame.collect`: one push per move, the finished games masked out on the device)."""
        net = self.get_net(role)
        if net is None:
            self.logger.error(f"{role} network is not set.")
            return
        if isinstance(net, DummyModule):  # no replay buffer
            return
        param = self.get_all_role_specific_param(role)
        replay_buffer = self.get_replay_buffer(role)
        er = self.get_er(role)
        points = self._generate_random_points(num_of_games, self.device)
        for _ in range(param["max_rollout_step"]):
            if points.ended:
                break
            self.fused_game.collect(points, role, replay_buffer, scale_observation=self.scale_observation,
                                    exploration_rate=er)

    def get_rollout(self, role: str, num_of_games: int, steps: int, er: Optional[float] = None) -> List:
        """the experiences (obs, act, rew, done, next_obs) of up to `steps` moves of `num_of_games` fresh games"""
        er = self.get_er(role) if er is None else er
        points = self._generate_random_points(num_of_games, self.device)
        exps = []
        for _ in range(steps):
            if not points.ended:
                exps.append(self.fused_game.step(points, role, scale_observation=self.scale_observation,
                                                 exploration_rate=er))
        return exps

    @torch.inference_mode()
    def evaluate_rho(self, num_samples: int = 100, max_steps: int = 100, use_graph: bool = False) -> List[torch.Tensor]:
        """rho for host_net vs (agent_net, RandomAgent, ChooseFirstAgent) and (RandomHost, AllCoordHost) vs agent_net"""
        if self.host_net.training or self.agent_net.training:
            self.logger.error("Host net or agent net is still in training mode. Eval will not be executed")
            return []
        dummy_param = (self.dimension, self.max_num_points, self.device)
        hosts = [self.host_net] * 3 + [RandomHostModule(*dummy_param), AllCoordHostModule(*dummy_param)]
        agents = [self.agent_net, RandomAgentModule(*dummy_param), ChooseFirstAgentModule(*dummy_param)] \
            + [self.agent_net] * 2
        return [self.get_rho_for_pair(host, agent, num_samples, max_steps, use_graph=use_graph)
                for host, agent in zip(hosts, agents)]

    @torch.inference_mode()
    def get_rho_for_pair(self, host_candidate: nn.Module, agent_candidate: nn.Module, num_samples: int,
                         max_steps: int, use_graph: bool = False) -> torch.Tensor:
        """(games not over at the start) / (moves played) over `num_samples` fresh games of greedy play, a 0-d tensor"""
        points = self._generate_random_points(num_samples, self.device)
        fused_game = FusedGame(host_candidate, agent_candidate, device=self.device, log_time=False,
                               reward_func=self.reward_func, dtype=self.dtype)
        self.last_evaluation = fused_game.evaluate(points, max_steps, scale_observation=self.scale_observation,
                                                   use_graph=use_graph)
        return self.last_evaluation.rho

    @torch.inference_mode()
    def count_actions(self, role: str, games: int, max_steps: int = 100, er: Optional[float] = None) -> torch.Tensor:
        """how often `role` chose each of its actions over roll-outs of `games` fresh games.  er=0.0: greedy play through
        `FusedGame.evaluate`; otherwise `get_rollout` at the exploration rate `er` (None: the schedule's) and bincount."""
        if self.get_net(role).training:
            self.logger.error("Host net or agent net is still in training mode. Eval will not be executed")
            return None
        if role == "host":
            max_num = 2 ** self.dimension - self.dimension - 1
        elif role == "agent":
            max_num = self.dimension
        else:
            raise Exception(f"role must be either host or agent. Got {role}.")
        if er is not None and er == 0.0:
            points = self._generate_random_points(games, self.device)
            self.last_evaluation = self.fused_game.evaluate(points, max_steps, scale_observation=self.scale_observation,
                                                            count_for=role)
            return self.last_evaluation.counts.to(torch.int64)
        count = torch.zeros(max_num, dtype=torch.int64, device=self.device)
        for rollout in self.get_rollout(role, games, max_steps, er=er):
            count += torch.bincount(rollout[1].flatten(), minlength=max_num)
        return count

    def copy(self):
        """a new object over copies of the nets and the same config (the replay buffers are NOT copied)"""
        return self.__class__(self.config, device_num=self.device_num, host_net=deepcopy(self.get_net("host")),
                              agent_net=deepcopy(self.get_net("agent")), reward_func=self.reward_func,
                              point_cls=self.point_cls, dtype=self.dtype, fused_training=self.fused_training)

    def _saved(self) -> dict:
        return {"host_net": self.get_net("host"), "agent_net": self.get_net("agent"), "config": self.config,
                "reward_func": self.reward_func, "point_cls": self.point_cls, "dtype": self.dtype}

    def save(self, path: str):
        """the nets and the config as a dict (the replay buffers are NOT saved)"""
        torch.save(self._saved(), path)

    def save_replay_buffer(self, path: str):
        torch.save({"host_replay_buffer": self.get_replay_buffer("host"),
                    "agent_replay_buffer": self.get_replay_buffer("agent")}, path)

    def load_replay_buffer(self, path: str):
        saved = torch.load(path, weights_only=False)
        for key in ["host_replay_buffer", "agent_replay_buffer"]:
            if key not in saved or saved[key] is None:
                continue
            if saved[key].actions.shape != getattr(self, key).actions.shape:
                self.logger.warning(f"The shape of the replay buffers might be different! Got {saved[key].actions.shape} "
                                    f"and {getattr(self, key).actions.shape} on action attributes.")
            setattr(self, key, saved[key])

    @classmethod
    def load(cls, path: str, **kwargs):
        """the Trainer that `save` wrote; keyword arguments override the constructor's"""
        saved = torch.load(path, weights_only=False)
        new_trainer = cls(saved["config"], **cls._load_param(saved, kwargs))
        new_trainer._after_load(saved)
        return new_trainer

    @staticmethod
    def _load_param(saved: dict, kwargs: dict) -> dict:
        param = {"device_num": 0, "host_net": saved["host_net"], "agent_net": saved["agent_net"],
                 "reward_func": saved.get("reward_func"), "point_cls": saved.get("point_cls", HipPoints),
                 "dtype": saved.get("dtype", torch.float32), "use_cuda_ids": None, "fused_training": False}
        for key in param:
            if key in kwargs:
                param[key] = kwargs[key]
        return param

    def _after_load(self, saved: dict):
        """what a subclass restores beyond the constructor's arguments"""

    @abc.abstractmethod
    def _train(self, steps: int, evaluation_interval: int = 1000, **kwargs):
        pass

    # -------- role-specific getters -------- #
    def get_all_role_specific_param(self, role):
        if not hasattr(self, f"{role}_all_param"):
            setattr(self, f"{role}_all_param",
                    {key: getattr(self, f"{role}_{key}") for key in self.role_specific_hyperparameters})
        return getattr(self, f"{role}_all_param")

    def get_net(self, role) -> nn.Module:
        return getattr(self, f"{role}_net")

    def get_optim(self, role):
        return getattr(self, f"{role}_optimizer", None)

    def get_lr_scheduler(self, role) -> Scheduler:
        return getattr(self, f"{role}_lr_scheduler", None)

    def get_er_scheduler(self, role) -> Scheduler:
        return getattr(self, f"{role}_er_scheduler", None)

    def get_er(self, role) -> float:
        return self.get_er_scheduler(role)(self.total_num_steps)

    def get_replay_buffer(self, role) -> ReplayBuffer:
        return getattr(self, f"{role}_replay_buffer", None)

    def get_batch_size(self, role) -> int:
        return getattr(self, f"{role}_batch_size")

    def is_dummy(self, role) -> bool:
        return isinstance(self.get_net(role), DummyModule)

    # -------- setters used outside initialisation -------- #
    def set_learning_rate(self):
        for role in ROLES:
            optimizer, scheduler = self.get_optim(role), self.get_lr_scheduler(role)
            if optimizer is None or scheduler is None:
                continue
            self._update_learning_rate(optimizer, scheduler(self.total_num_steps))

    def set_training(self, training_mode: bool):
        for role in ROLES:
            self.get_net(role).train(training_mode)

    @contextlib.contextmanager
    def inference_mode(self):
        self.set_training(False)
        try:
            yield
        finally:
            self.set_training(True)

    # -------- private utilities -------- #
    @staticmethod
    def _update_learning_rate(optimizer, new_lr):
        for param_group in optimizer.param_groups:
            param_group["lr"] = new_lr

    def _make_network(self, role: str, head_cls: Any, input_dim: int, output_dim: int, pretrained_net: nn.Module):
        for key in self.role_specific_hyperparameters:
            setattr(self, f"{role}_{key}", self.config[role][key])
        if pretrained_net is not None:
            assert self.get_net(role) is not None
            setattr(self, f"{role}_net", pretrained_net.to(self.device))
        else:
            net_arch = self.config[role]["net_arch"]
            assert isinstance(net_arch, list), f"'net_arch' must be a list. Got {type(net_arch)}."
            head = head_cls(input_dim)
            net = self._create_network(head, net_arch, head.feature_dim, output_dim).to(self.device)
            setattr(self, f"{role}_net", net)

    def _make_fused_game(self):
        self.fused_game = FusedGame(self.host_net, self.agent_net, device=self.device, log_time=self.log_time,
                                    reward_func=self.reward_func, dtype=self.dtype)

    def _set_optim(self, role: str):
        """(re-)build `self.{role}_optimizer` over `self.{role}_net.parameters()` from `self.{role}_optim_config`"""
        cfg = getattr(self, f"{role}_optim_config")
        setattr(self, f"{role}_optimizer", self.optim_dict[cfg["name"]](self.get_net(role).parameters(), **cfg["args"]))

    def _make_replay_buffer(self, role: str, output_dim: int):
        cfg = self.config["replay_buffer"]
        self.use_replay_buffer = not cfg.get("deactivate", False)
        if not self.use_replay_buffer:
            return
        device = self.device if cfg["use_cuda"] else torch.device("cpu")  # (the buffer refuses the CPU itself)
        if role == "host":
            input_shape = self.feature_shape
        else:
            input_shape = {"points": self.feature_shape, "coords": (self.dimension,)}
        setattr(self, f"{role}_replay_buffer", self.replay_buffer_dict[cfg["type"]](
            input_shape=input_shape, output_dim=output_dim, device=device, dtype=self.dtype,
            **{k: v for k, v in cfg.items() if k not in ("type", "use_cuda", "deactivate")}))

    def _make_optimizer_and_lr(self, role: str):
        name = self.config[role]["optim"]["name"]
        assert name in self.optim_dict, f"'optim' must be one of {self.optim_dict.keys()}. Got {name}."
        cfg = self.config[role]["optim"]
        lr_scheduler = None
        if "lr_schedule" in cfg:
            lr_scheduler = self.lr_scheduler_dict[cfg["lr_schedule"]["mode"]](cfg["args"]["lr"], **cfg["lr_schedule"])
        setattr(self, f"{role}_lr_scheduler", lr_scheduler)
        self._set_optim(role)

    def _make_er_scheduler(self, role: str):
        cfg = self.config[role]
        if "er_schedule" in cfg:
            er_scheduler = self.er_scheduler_dict[cfg["er_schedule"]["mode"]](cfg["er"], **cfg["er_schedule"])
        else:
            er_scheduler = ConstantScheduler(cfg["er"])
        setattr(self, f"{role}_er_scheduler", er_scheduler)

    def _create_network(self, head: nn.Module, net_arch: list, input_dim: int, output_dim: int) -> nn.Module:
        return create_mlp(head, net_arch, input_dim, output_dim, fused_training=self.fused_training)

    def _generate_random_points(self, samples: int, device: torch.device) -> HipPoints:
        """integers in [0, max_value] drawn on the device -> Newton polytope -> [rescale]"""
        pts = torch.randint(self.max_value + 1, (samples, self.max_num_points, self.dimension), dtype=self.dtype,
                            device=device)
        points = self.point_cls(pts, device=device, dtype=self.dtype)
        points.get_newton_polytope()
        if self.scale_observation:
            points.rescale()
        return points

    @staticmethod
    def load_yaml(file_path: str) -> dict:
        with open(file_path, "r") as stream:
            return yaml.safe_load(stream)
