"""hk_host_select / ops.host_select and the hosts it serves on the GPU: bit for bit against the reference's own
select_coord (tests/golden/hosts.npz, tests/golden/make_host_golden.py), independent of where padding rows sit, at
the batch tails of the launch grid, equal to hk_zeillinger's list semantics for "zeillinger", and through the
package's Host classes and GameHironaka."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd._lib import HironakaHipError
from hironaka_amd.agent import ChooseFirstAgent
from hironaka_amd.core import HipPoints
from hironaka_amd.game import GameHironaka
from hironaka_amd.host import AllCoordHost, WeakSpivakovsky, WeakSpivakovskyMinHitting, Zeillinger, ZeillingerLex

pytestmark = pytest.mark.gpu

HOSTS = ("zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting", "zeillinger")
CLASSES = {"zeillinger_lex": ZeillingerLex, "weak_spivakovsky": WeakSpivakovsky,
           "weak_spivakovsky_min_hitting": WeakSpivakovskyMinHitting, "zeillinger": Zeillinger}


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "hosts.npz"))


def encode(masks):
    """[N, d] 0/1 masks (all -1 = no subset) -> class ids, -1 kept"""
    v = (masks.clip(0).astype(np.int64) << np.arange(masks.shape[1])).sum(1)
    lg = np.floor(np.log2(np.maximum(v, 1))).astype(np.int64)
    return np.where(masks[:, 0] < 0, -1, v - lg - 2)


def padding_in_the_middle(states):
    """the same games with their padding rows moved between the first point and the rest"""
    out = np.empty_like(states)
    for g, st in enumerate(states):
        live, pad = st[st[:, 0] >= 0], st[st[:, 0] < 0]
        out[g] = np.concatenate([live[:1], pad, live[1:]])
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("host", HOSTS)
def test_host_select_matches_the_reference(fixture, host, dtype):
    for d in range(2, 7):
        states, want = fixture[f"sel{d}_states"], encode(fixture[f"sel{d}_{host}"])
        for st in (states, padding_in_the_middle(states)):
            got = ops.host_select(torch.as_tensor(st, dtype=dtype, device="cuda"), host).cpu().numpy()
            assert np.array_equal(got, want), (host, d, np.nonzero(got != want)[0][:8])


def _random_states(rng, b, m, d, hi, holes=0.3):
    p = rng.integers(0, hi + 1, (b, m, d)).astype(np.float32)
    p[rng.random((b, m)) < holes] = -1.0
    return p


@pytest.mark.parametrize("host", HOSTS + ("all_coord",))
def test_batch_tails_stride_and_small_games(host):
    rng = np.random.default_rng(7)
    m, d = 9, 4
    big = _random_states(rng, 4097, m, d, 3)
    big[:5, 1:] = -1.0  # one point
    big[5:9] = -1.0     # no point
    full = torch.as_tensor(big, device="cuda")
    ref = ops.host_select(full, host).cpu().numpy()
    if host != "all_coord":
        assert (ref[:9] == -1).all()
    else:
        assert (ref == (1 << d) - 1 - (d - 1) - 2).all()
    for b in (1, 63, 64, 65, 4097):
        assert np.array_equal(ops.host_select(full[:b].contiguous(), host).cpu().numpy(), ref[:b]), b
    # records wider than m*d: the game is the first m*d elements
    rec = torch.full((4097, m * d + 7), 123.0, device="cuda")
    rec[:, :m * d] = full.reshape(4097, -1)
    assert np.array_equal(ops.host_select(rec, host, spec=(m, d)).cpu().numpy(), ref)


def test_zeillinger_equals_hk_zeillinger_list():
    rng = np.random.default_rng(11)
    for b, m, d in ((65536, 20, 3), (4096, 50, 4)):
        for dtype in (torch.float32, torch.float64):
            p = torch.as_tensor(_random_states(rng, b, m, d, 20), dtype=dtype, device="cuda")
            assert torch.equal(ops.host_select(p, "zeillinger"), ops.zeillinger(p, sem="list")), (b, m, d, dtype)


@pytest.mark.parametrize("host", HOSTS)
def test_host_classes_select_coord(fixture, host):
    st = torch.as_tensor(fixture["sel4_states"], device="cuda")
    got = CLASSES[host]().select_coord(st)
    cls = ops.host_select(st, host)
    want = ops.decode_host_class(cls.clamp(min=0), 4, torch.int32) * (cls >= 0).unsqueeze(1).to(torch.int32)
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), fixture[f"sel4_{host}"].clip(0))


def test_host_classes_refuse_dim_7():
    p = torch.zeros((2, 3, 7), device="cuda")
    for cls in (ZeillingerLex, WeakSpivakovsky, WeakSpivakovskyMinHitting):
        with pytest.raises(ValueError, match="up to 6"):
            cls().select_coord(p)
    assert WeakSpivakovskyMinHitting(dim=16).dim == 16


@pytest.mark.parametrize("host", ["zeillinger_lex", "weak_spivakovsky"])
def test_game_hironaka_replays_the_reference(fixture, host):
    """the reference's GameHironaka (ChooseFirstAgent, scale_observation=False) step by step: every state and every
    host subset, up to the fixture's step cap"""
    g = lambda k: fixture[f"game_{host}_{k}"]  # noqa: E731
    states, masks = g("states"), g("masks")
    pts = HipPoints(torch.as_tensor(g("start")), dtype=torch.float64, semantics="list", value_threshold=1e8)
    game = GameHironaka(pts, CLASSES[host](), ChooseFirstAgent(), scale_observation=False)
    assert np.array_equal(game.state.points.cpu().numpy(), states[0])
    for t in range(len(masks)):
        game.step()
        assert np.array_equal(game.coord_history[-1].cpu().numpy(), masks[t]), t
        assert np.array_equal(game.state.points.cpu().numpy(), states[t + 1]), t


@pytest.mark.parametrize("host", [A.HK_HOST_ZEILLINGER_LEX, A.HK_HOST_WEAK_SPIVAKOVSKY, A.HK_HOST_MIN_HITTING])
def test_rollout_still_refuses_the_new_hosts(host):
    p = ops.generate_points(64, 10, 3, 20, seed=1)
    with pytest.raises(HironakaHipError) as e:
        ops.rollout(p, 4, 7, host_policy=host)
    assert e.value.status == A.HK_ERR_UNSUPPORTED


def test_all_coord_ignores_the_state():
    p = torch.full((3, 4, 5), -1.0, device="cuda")
    assert (ops.host_select(p, "all_coord") == (1 << 5) - 1 - 4 - 2).all()
    assert torch.equal(AllCoordHost()._select_coord(p), torch.ones((3, 5), dtype=torch.int32, device="cuda"))
