"""The per-(device, stream) workspace caches of ops.py (rollout counters, dqn_td, optim_prepare): first request, reuse,
growth with retirement, one buffer per stream, and what each does when it would have to grow inside a stream capture.
No kernel of the library is launched: the only memory touched is torch's own."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROLLOUT_REFUSAL = ("hk_rollout's counter workspace would have to be (re)allocated inside a stream capture: run the same "
                   "rollout once eagerly on this stream first, or pass workspace=ops.rollout_workspace(...) with "
                   "defer_counts=True")
OPTIM_REFUSAL = ("optim_prepare needs a larger workspace than this stream has, inside a stream capture: run one step "
                 "before capturing, or bring workspace=ops.optim_workspace(...)")
CACHES = (("_ROLLOUT_WORKSPACES", 1 << 16, ROLLOUT_REFUSAL), ("_DQN_WORKSPACES", 1 << 12, None),
          ("_OPTIM_WORKSPACES", 1 << 12, OPTIM_REFUSAL))


@pytest.fixture
def caches(monkeypatch):
    """the three module-level instances, emptied for the test (what other tests left in them comes back afterwards)"""
    from hironaka_amd import ops
    found = []
    for name, floor, refusal in CACHES:
        cache = getattr(ops, name)
        monkeypatch.setattr(cache, "live", {})
        monkeypatch.setattr(cache, "retired", [])
        found.append((cache, floor, refusal))
    return found


def test_first_request_reuse_growth_and_streams(caches):
    dev = torch.device("cuda", torch.cuda.current_device())
    side = torch.cuda.Stream()
    for cache, floor, _ in caches:
        assert cache.floor == floor
        first = cache.get(dev, 24)
        assert first.dtype == torch.uint8 and first.device == dev and first.numel() == floor and not first.any()
        assert cache.get(dev, 24) is first and cache.get(dev, floor) is first and not cache.retired
        grown = cache.get(dev, first.numel() + 1)  # one byte more than there is
        assert grown is not first and grown.numel() == floor + 1 and grown.dtype == torch.uint8 and not grown.any()
        assert len(cache.retired) == 1 and cache.retired[0] is first  # kept alive: a captured graph may hold its address
        assert cache.get(dev, 24) is grown
        with torch.cuda.stream(side):
            other = cache.get(dev, 24)
            assert other is not grown and other.data_ptr() != grown.data_ptr() and other.numel() == floor
            assert not other.any() and cache.get(dev, 24) is other
        assert cache.get(dev, 24) is grown and len(cache.live) == 2 and len(cache.retired) == 1
    torch.cuda.synchronize()


def test_growth_inside_a_stream_capture(caches):
    """rollout and optimiser refuse with their own message; dqn_td hands out a fresh buffer of exactly the bytes asked
    for, from the capture's pool, and keeps nothing.  One capture serves the three: it ends cleanly and replays."""
    dev = torch.device("cuda", torch.cuda.current_device())
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    held = []
    with torch.cuda.stream(warm):  # every cache has this stream's buffer before the capture begins
        for cache, _, _ in caches:
            held.append(cache.get(dev, 24))
    torch.cuda.current_stream().wait_stream(warm)
    graph = torch.cuda.CUDAGraph()
    fresh = None
    with torch.cuda.graph(graph, stream=warm):
        for (cache, floor, refusal), mine in zip(caches, held):
            assert cache.get(dev, floor) is mine  # what fits is served as ever
            if refusal is not None:
                with pytest.raises(RuntimeError) as caught:
                    cache.get(dev, floor + 1)
                assert str(caught.value) == refusal
            else:
                fresh = cache.get(dev, floor + 1)
                assert fresh is not mine and fresh.numel() == floor + 1 and fresh.dtype == torch.uint8
                assert cache.get(dev, floor + 1) is not fresh  # not kept: the next request draws another
            assert len(cache.live) == 1 and next(iter(cache.live.values())) is mine and not cache.retired
    graph.replay()  # the fresh buffer's zero fill was captured with it
    torch.cuda.synchronize()
    assert fresh is not None and not fresh.any()
    for (cache, _, _), mine in zip(caches, held):
        assert len(cache.live) == 1 and not cache.retired and not mine.any()
