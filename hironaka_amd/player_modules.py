"""The simple hosts and agents as ``nn.Module``s without parameters, the counterpart of
``hironaka/trainer/player_modules``: they take the observations the Q-networks take and answer with one-hot float32
"Q-values", so that ``FusedGame`` and ``Trainer.evaluate_rho`` play them like any network.  ``DummyModule`` marks them:
a trainer never trains one."""
import abc

import torch
from torch import nn
from torch.nn.functional import one_hot


class DummyModule(abc.ABC):
    pass


class _Player(nn.Module, DummyModule):
    def __init__(self, dimension: int, max_num_points: int, device: torch.device):
        super().__init__()
        self.dimension = dimension
        self.max_num_points = max_num_points
        self.device = device
        self.output_dim = 2 ** dimension - dimension - 1  # of a host


class ChooseFirstAgentModule(_Player):
    """the lowest coordinate of the host's subset"""

    def forward(self, x):
        return one_hot(x["coords"].argmax(1), num_classes=self.dimension).type(torch.float32)


class ChooseLastAgentModule(_Player):
    """the highest coordinate of the host's subset: a small ramp breaks the argmax's tie towards the end"""

    def forward(self, x):
        coords = x["coords"].type(torch.float32)
        ramp = torch.arange(self.dimension, dtype=torch.float32, device=coords.device) * 1e-4
        return one_hot((coords + ramp).argmax(1), num_classes=self.dimension).type(torch.float32)


class RandomAgentModule(_Player):
    """a coordinate of the host's subset, uniformly: the largest of independent uniform draws on the subset"""

    def forward(self, x):
        coords = x["coords"]
        draws = torch.rand((coords.shape[0], self.dimension), device=coords.device) * coords
        return one_hot(draws.argmax(1), num_classes=self.dimension).type(torch.float32)


class RandomHostModule(_Player):
    """a class, uniformly"""

    def forward(self, x):
        r = torch.randint(self.output_dim, (x.shape[0],), device=self.device)
        return one_hot(r.long(), num_classes=self.output_dim).type(torch.float32)


class AllCoordHostModule(_Player):
    """the last class: every coordinate"""

    def forward(self, x):
        r = torch.zeros((x.shape[0], self.output_dim), device=self.device, dtype=torch.float32)
        r[:, -1] = 1.0
        return r
