"""``DQNTrainer`` -- the double-DQN trainer of a (host, agent) pair, the counterpart of
``hironaka/trainer/dqn_trainer/dqn_trainer.py:13-208``: ``DQNTrainer("config.yml").train(steps)``.

A step is, per trained role and in the reference's order: the learning rate from its schedule, the Polyak update of the
target net every ``steps_before_update_target`` steps (``dqn.update_target_net``: one launch per 64 tensors), one fit
of the Q-net on a replay sample (``dqn.fit_network``: the fused TD loss, the clipped optimiser step in two launches), a
roll-out into the replay buffer every ``steps_before_rollout`` steps; then, every ``evaluation_interval`` steps, rho of
the five pairs and the action counts (``FusedGame.evaluate``).

Extra global config key: ``max_grad_norm``.
"""
from copy import deepcopy
from typing import Iterable

import torch
from torch import nn

from . import dqn
from .fused_game import Timer
from .trainer import Trainer

_RHO_NAMES = ("host-agent", "host-random", "host-choosefirst", "random-agent", "allcoord-agent")


class DQNTrainer(Trainer):
    role_specific_hyperparameters = ["batch_size", "gamma", "tau", "initial_rollout_size", "max_rollout_step",
                                     "steps_before_rollout", "steps_before_update_target", "rollout_size"]

    def __init__(self, config, **kwargs):
        super().__init__(config, **kwargs)
        self.max_grad_norm = self.config["max_grad_norm"]
        for role in self.trained_roles:
            self._make_target_net(role)

    def _make_target_net(self, role: str):
        """a copy of the role's net on the device; tau = 1 copies the weights (and the batch norms' statistics)"""
        setattr(self, f"{role}_net_target", deepcopy(self.get_net(role)).to(self.device))
        self._update_target_net(self.get_net(role), self.get_net_target(role), 1)

    def set_trainable(self, players):
        super().set_trainable(players)
        for role in players:
            if role in self.trained_roles and self.get_net_target(role) is None:
                self._make_target_net(role)

    def _timer(self, name: str) -> Timer:
        return Timer(name, self.time_log, active=self.log_time, use_cuda=self.use_cuda)

    def _fit_network(self, q_net: nn.Module, q_net_target: nn.Module, optimizer: torch.optim.Optimizer, replay_buffer,
                     batch_size: int, gamma: float, log_prefix: str = "", current_step: int = 0, **kwargs):
        """one fit step; returns the loss tensor without reading it (tensorboard reads it every 100 steps)"""
        loss = dqn.fit_network(q_net, q_net_target, optimizer, replay_buffer, batch_size, gamma, self.max_grad_norm)
        if self.use_tensorboard and (self.total_num_steps + current_step) % 100 == 0:
            self.tb_writer.add_scalar(f"{log_prefix}/loss", loss.item(), self.total_num_steps + current_step)
        return loss

    def _train(self, steps: int, evaluation_interval: int = 1000, players: Iterable[str] = ("host", "agent"),
               prefix: str = ""):
        players = list(players)
        for role in players:
            if role not in self.trained_roles:
                self.logger.error(f"{role} is not trainable. Either it is not present in config or it was set as a "
                                  f"dummy module.")
                return
        net_param = {role: (self.get_net(role), self.get_net_target(role), self.get_optim(role),
                            self.get_replay_buffer(role)) for role in players}
        param = {role: self.get_all_role_specific_param(role) for role in players}
        model_prefix = f"{prefix}-{self.version_string}-{self.device_num}"
        self.losses = []

        for i in range(steps):
            step = self.total_num_steps + i
            self.set_learning_rate()
            for role in players:
                with self._timer(f"update_{role}_target_net"):
                    if step % param[role]["steps_before_update_target"] == 0:
                        self._update_target_net(net_param[role][0], net_param[role][1], param[role]["tau"])
                with self._timer(f"fit_{role}_net_total"):
                    self.losses.append(self._fit_network(*net_param[role], **param[role],
                                                         log_prefix=f"{role}-{model_prefix}", current_step=i))
                with self._timer(f"collect_{role}_rollouts_total"):
                    if step % param[role]["steps_before_rollout"] == 0:
                        with self.inference_mode():
                            self.collect_rollout(role, param[role]["rollout_size"])
            with self._timer("evaluate_total"):
                if i % evaluation_interval == 0 and i != 0:
                    with self.inference_mode():
                        rhos = self.evaluate_rho()
                        for role in players:
                            self.logger.info(self.count_actions(role, 100, er=0.0))
                        self.logger.info(rhos)
                        if self.use_tensorboard:
                            for name, rho in zip(_RHO_NAMES, rhos):
                                self.tb_writer.add_scalar(f"{model_prefix}/rhos/{name}", rho.item(), step)
        self.total_num_steps += steps

    @staticmethod
    def _update_target_net(q_net: nn.Module, q_net_target: nn.Module, tau: float):
        dqn.update_target_net(q_net, q_net_target, tau)

    def get_net_target(self, role):
        return getattr(self, f"{role}_net_target", None)

    # -------- the target nets travel with the rest -------- #
    def _saved(self) -> dict:
        saved = super()._saved()
        for role in self.trained_roles:
            saved[f"{role}_net_target"] = self.get_net_target(role)
        return saved

    def _after_load(self, saved: dict):
        for role in self.trained_roles:
            target = saved.get(f"{role}_net_target")
            if target is not None:
                setattr(self, f"{role}_net_target", target.to(self.device))
