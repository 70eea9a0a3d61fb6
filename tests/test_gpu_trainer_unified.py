"""HipTrainer.simulate(..., use_unified_tree=True): with fused_expand=True the searches expand through
recurrent_fn.UnifiedExpander -- gated launches for the dense_resnet networks the trainer builds, both networks for
standin_mlp callables -- and give what fused_expand=False gives, the generic path with its decision on the host; with
use_graph=True a second simulate replays the captured searches; an in-place parameter update changes the next result."""
import pytest
import torch

from hironaka_amd.recurrent_fn import UnifiedExpander
from test_gpu_unified_search import make_trainer, same_bits

pytestmark = pytest.mark.gpu
SPEC = (10, 3)


def same_rollout(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("batch", (33, 256))
@pytest.mark.parametrize("built", (True, False), ids=("dense_resnet", "standin_mlp"))
def test_simulate_with_the_expander_equals_the_generic_path(built, batch):
    fused = make_trainer(SPEC, batch, built, fused_expand=True)
    generic = make_trainer(SPEC, batch, built, fused_expand=False)
    want = generic.simulate(7, "host", use_unified_tree=True)
    got = fused.simulate(7, "host", use_unified_tree=True)
    m, d = SPEC
    assert got[0].shape == (batch * fused.max_length_game, m * d + d) and got[1].shape[1] == 2 ** d - d - 1
    assert same_rollout(got, want)
    # which path ran: the loop carries an expander only with fused_expand, and the built networks are the gateable ones
    e = UnifiedExpander(fused.models["host"], fused.models["agent"], SPEC, fused.discount, True, True)
    assert (e._plan(fused.models["host"]) is not None) == built and (e._plan(fused.models["agent"]) is not None) == built
    # both players' nodes are in the rollout: zero tails and subsets
    tails = got[0][:, m * d:]
    assert bool((tails == 0).all(dim=1).any()) and bool((tails.sum(dim=1) >= 2).any())


def test_trainer_builds_the_expander_under_the_conditions_of_the_other_two(monkeypatch):
    import hironaka_amd.trainer_api as TA
    seen = []
    real = TA.get_evaluation_loop

    def spy(**kw):
        seen.append((kw.get("role_agnostic"), kw.get("use_graph"), type(kw.get("expander")).__name__))
        return real(**kw)

    monkeypatch.setattr(TA, "get_evaluation_loop", spy)
    for kw, want in ((dict(fused_expand=True, use_graph=True), (True, True, "UnifiedExpander")),
                     (dict(fused_expand=True, use_graph=False), (True, False, "UnifiedExpander")),
                     (dict(fused_expand=False, use_graph=True), (True, False, "NoneType")),
                     (dict(fused_expand=True, use_graph=True, dtype=torch.float64), (True, False, "NoneType"))):
        del seen[:]
        make_trainer(SPEC, 33, False, **kw)._sim_fn("host", False, True)
        assert seen == [want], (kw, seen)


@pytest.mark.parametrize("built", (True, False), ids=("dense_resnet", "standin_mlp"))
def test_captured_unified_searches_are_replayed_not_recaptured(monkeypatch, built):
    from hironaka_amd import search as S
    import hironaka_amd.simulation_fn as SF
    made = []
    real = S.CapturedSearch

    class Counting(real):
        def __init__(self, *a, **kw):
            made.append(1)
            super().__init__(*a, **kw)

    monkeypatch.setattr(S, "CapturedSearch", Counting)
    monkeypatch.setattr(SF, "CapturedSearch", Counting)
    t = make_trainer(SPEC, 33, built, use_graph=True)
    first = [x.clone() for x in t.simulate(3, "host", use_unified_tree=True)]
    n_first = len(made)
    again = t.simulate(3, "host", use_unified_tree=True)
    assert n_first == 1 and len(made) == 1, (n_first, len(made))  # one shape, one capture; the second call replays it
    assert same_rollout(first, again)
    eager = make_trainer(SPEC, 33, built, use_graph=False, fused_expand=False).simulate(3, "host", use_unified_tree=True)
    assert same_rollout(first, eager)  # ... and the replay is the generic path's result


@pytest.mark.parametrize("use_graph", (False, True), ids=("eager", "graph"))
def test_in_place_parameter_update_changes_the_next_result(use_graph):
    """the plan (and a capture) points at the parameters' storage: an update in place is seen by the next simulate"""
    t = make_trainer(SPEC, 33, True, use_graph=use_graph)
    first = [x.clone() for x in t.simulate(5, "host", use_unified_tree=True)]
    assert same_rollout(first, t.simulate(5, "host", use_unified_tree=True))
    with torch.no_grad():
        for role in ("host", "agent"):
            for p in t.built_nets[role].parameters():
                p.mul_(-1.5)
    after = t.simulate(5, "host", use_unified_tree=True)
    assert not same_bits(first[1], after[1])  # the improved policies moved with the networks
    fresh = make_trainer(SPEC, 33, True, fused_expand=False)
    with torch.no_grad():
        for role in ("host", "agent"):
            for p, q in zip(fresh.built_nets[role].parameters(), t.built_nets[role].parameters()):
                p.copy_(q)
    assert same_rollout(after, fresh.simulate(5, "host", use_unified_tree=True))
