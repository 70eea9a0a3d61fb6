"""hk_unified_pvnet_forward, the policy-value forward behind a gate (include/hironaka_hip_unified.h): where the gate is
open the bits are hk_pvnet_forward's on either row tile (the large one forced at a small batch through
HK_PVNET_FORCE_TILE_LARGE); where it is closed the sentinel-filled outputs stay as they were.  Widths [32] x 2 and
[128] x 2, 33 rows: two full 16-row tiles and a tail of one, half of a 64-row tile."""
import numpy as np
import pytest
import torch

import pvnet_rules as R
from hironaka_amd import _abi as A
from test_gpu_mlp import dev, inputs
from test_gpu_pvnet import device_plan

pytestmark = pytest.mark.gpu
ROWS, ACTIONS, SENTINEL = 33, 4, -12345.5
TILES = (A.HK_MLP_TILE_SMALL, A.HK_MLP_TILE_LARGE)


def sentinels():
    return (torch.full((ROWS, ACTIONS), SENTINEL, device="cuda"), torch.full((ROWS,), SENTINEL, device="cuda"))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("width", (32, 128))
def test_open_gate_gives_the_ungated_bits_and_a_closed_gate_leaves_the_outputs(width, tile):
    from hironaka_amd import ops
    rng = np.random.default_rng(width + tile)
    k0 = 63
    net = R.random_net(rng, k0, [width, width], ACTIONS)
    plan = device_plan(net)
    x = dev(inputs(rng, ROWS, k0))
    want_p, want_v = ops.pvnet_forward(x, plan, tile=tile)
    assert R.same_bits(want_p.cpu().numpy(), ops.pvnet_forward(x, plan)[0].cpu().numpy())  # the tiles agree, as ever
    words = torch.tensor([7, 0, 1, -1], dtype=torch.int32, device="cuda")
    for at, word in enumerate(words.tolist()):
        for want in (0, 1):
            p, v = sentinels()
            got = ops.pvnet_forward(x, plan, tile=tile, gate=(words[at: at + 1], want), out=(p, v))
            assert got[0] is p and got[1] is v
            if word == want:
                assert R.same_bits(p.cpu().numpy(), want_p.cpu().numpy()), (width, tile, word, want)
                assert R.same_bits(v.cpu().numpy(), want_v.cpu().numpy()), (width, tile, word, want)
            else:
                assert (p == SENTINEL).all() and (v == SENTINEL).all(), (width, tile, word, want)
    assert words.tolist() == [7, 0, 1, -1]  # the gate is read, never written


def test_gate_is_read_when_the_kernel_runs_not_when_it_is_enqueued():
    """the decision is the device's: a word written by an earlier kernel of the stream opens or closes the launch behind
    it, with no word read back in between"""
    from hironaka_amd import ops
    rng = np.random.default_rng(5)
    net = R.random_net(rng, 18, [32, 32], ACTIONS)
    plan = device_plan(net)
    x = dev(inputs(rng, ROWS, 18))
    want_p, _ = ops.pvnet_forward(x, plan)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        p, v = sentinels()
        word.fill_(1)  # a kernel of the stream
        ops.pvnet_forward(x, plan, gate=(word, 1), out=(p, v))
        word.fill_(0)
        q, w = sentinels()
        ops.pvnet_forward(x, plan, gate=(word, 1), out=(q, w))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert R.same_bits(p.cpu().numpy(), want_p.cpu().numpy())
    assert (q == SENTINEL).all() and (w == SENTINEL).all()


def test_gate_arguments_are_checked():
    from hironaka_amd import ops
    rng = np.random.default_rng(6)
    plan = device_plan(R.random_net(rng, 18, [32], ACTIONS))
    x = dev(inputs(rng, 4, 18))
    with pytest.raises(TypeError):
        ops.pvnet_forward(x, plan, gate=(torch.zeros(1, dtype=torch.int64, device="cuda"), 1))
    with pytest.raises(TypeError):
        ops.pvnet_forward(x, plan, gate=(torch.zeros(2, dtype=torch.int32, device="cuda"), 1))
    with pytest.raises(TypeError):
        ops.pvnet_forward(x, plan, gate=(torch.zeros(1, dtype=torch.int32), 1))
    p = torch.empty((4, ACTIONS), device="cuda")
    with pytest.raises(ValueError):
        ops.pvnet_forward(x, plan, policy=p, out=(p, torch.empty(4, device="cuda")))
