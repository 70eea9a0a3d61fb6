"""Schedulers of the DQN trainers' learning and exploration rates, the counterpart of ``hironaka/trainer/scheduler.py``:
a value fixed at construction, keyword parameters of which each class demands its ``mandatory_keys``, and
``scheduler(steps)`` for the value at a step.  Plain Python floats: nothing here touches the device."""
import abc
from typing import Union

Number = Union[float, int]


class Scheduler(abc.ABC):
    key_name = None      # where the parameters come from in the config, for the assertion's message
    mandatory_keys = []  # the keyword parameters a subclass cannot do without

    def __init__(self, value: Number, **kwargs):
        self.value = value
        self.kwargs = kwargs
        where = self.key_name if self.key_name is not None else "the config"
        for key in self.mandatory_keys:
            assert key in self.kwargs, f"'{key}' must be in {where}. Got {self.kwargs}."

    def __call__(self, steps: int, **kwargs) -> Number:
        return self.get_value(steps)

    @abc.abstractmethod
    def get_value(self, steps: int) -> Number:
        pass


class ConstantScheduler(Scheduler):
    def get_value(self, steps: int) -> Number:
        return self.value


class _ExponentialScheduler(Scheduler):
    """from kwargs[initial_key] towards `value`: initial * rate^steps + value * (1 - rate^steps)"""
    initial_key = None

    def get_value(self, steps: int) -> Number:
        initial, rate = self.kwargs[self.initial_key], self.kwargs["rate"]
        return initial * (rate ** steps) + self.value * (1 - rate ** steps)


class ExponentialLRScheduler(_ExponentialScheduler):
    key_name = "lr_schedule"
    mandatory_keys = ["initial_lr", "rate"]
    initial_key = "initial_lr"


class InverseLRScheduler(Scheduler):
    """rate / (steps + rate / initial_lr): initial_lr at step 0, then like rate / steps"""
    key_name = "lr_schedule"
    mandatory_keys = ["initial_lr", "rate"]

    def get_value(self, steps: int) -> Number:
        initial_lr, rate = self.kwargs["initial_lr"], self.kwargs["rate"]
        return rate / (steps + rate / initial_lr)


class ExponentialERScheduler(_ExponentialScheduler):
    key_name = "er_schedule"
    mandatory_keys = ["initial_er", "rate"]
    initial_key = "initial_er"
