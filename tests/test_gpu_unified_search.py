"""The search over a role-agnostic tree with recurrent_fn.UnifiedExpander against the same search through the generic
recurrent function (get_unified_recurrent_fn's, which asks the host for the kind of every batch): `action`,
`action_weights` and every field of the tree, embeddings included, must be the same bits -- eagerly and replayed from a
graph, which the generic path cannot be.  The generic run records the kind of every expansion; the test fails by name
unless all-host, all-agent and mixed expansions all occurred, so the reference's once-per-batch decision is exercised on
batches where a per-game decision would differ."""
import pytest
import torch

import hironaka_amd.simulation_fn as SF
from hironaka_amd import search as S
from hironaka_amd.functional import generate_pts
from hironaka_amd.players import get_host_with_flattened_obs
from hironaka_amd.recurrent_fn import UnifiedExpander, get_unified_recurrent_fn
from hironaka_amd.trainer_api import HipTrainer, standin_mlp

pytestmark = pytest.mark.gpu

EVALUATIONS, MAX_DEPTH, CONSIDERED = 12, 8, 2
BASE = {"eval_batch_size": 33, "max_length_game": 4, "max_value": 20, "max_grad_norm": 1.0, "scale_observation": True,
        "reposition": True, "gumbel_scale": 0.3, "use_cuda": True, "version_string": "test", "net_type": "dense_resnet",
        "num_evaluations": EVALUATIONS, "num_evaluations_as_opponent": 4, "eval_on_cpu": False,
        "max_num_considered_actions": CONSIDERED, "discount": 0.99}


def make_trainer(spec, batch, built, **kw):
    """built: dense_resnet networks of the trainer's own (the gated path); otherwise standin_mlp callables (both run)"""
    m, d = spec
    cfg = dict(BASE, eval_batch_size=batch, max_num_points=m, dimension=d)
    if built:
        section = {"net_arch": [64, 64]}  # (not 32: GroupNorm(32) of 32 columns is its bias whatever the input)
        return HipTrainer(42, dict(cfg, host=dict(section), agent=dict(section)), **kw)
    host_net, host_params = standin_mlp(m * d, 2 ** d - d - 1, 3, width=64)
    agent_net, agent_params = standin_mlp(m * d + d, d, 4, width=64)
    return HipTrainer(42, cfg, host_net=host_net, agent_net=agent_net, host_params=host_params,
                      agent_params=agent_params, **kw)


def loop_of(t, expander, use_graph):
    """HipTrainer._eval_loop(unified=True), spelled out"""
    host_on_points = lambda pts, *a, dtype=None, **k: t.policy_fns["host"](pts.reshape(pts.shape[0], -1), *a, **k)  # noqa: E731
    return SF.get_evaluation_loop(
        role="host", role_agnostic=True, use_graph=use_graph, expander=expander,
        policy_fn=get_host_with_flattened_obs(t.spec, host_on_points, truncate_input=True),
        opponent_fn=t.policy_fns["agent"], reward_fn=t.reward_fns["agent"], num_evaluations=EVALUATIONS, spec=t.spec,
        max_depth=MAX_DEPTH, max_num_considered_actions=CONSIDERED, discount=t.discount, rescale_points=False,
        reposition=t.reposition, dtype=torch.float32, gumbel_scale=0.3)


def expander_of(t):
    return UnifiedExpander(t.models["host"], t.models["agent"], t.spec, t.discount, t.scale_observation, t.reposition)


def roots_of(t, seed):
    m, d = t.spec
    pts = generate_pts(seed, (t.eval_batch_size, m, d), t.max_value, torch.float32, False, t.reposition, device=t.device)
    return torch.cat([pts.reshape(t.eval_batch_size, -1), torch.zeros((t.eval_batch_size, d), device=t.device)], dim=1)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def assert_same_output(got, want, what):
    assert same_bits(got.action, want.action), what + ": action"
    assert same_bits(got.action_weights, want.action_weights), what + ": action_weights"
    for name in S.Tree._fields:
        assert same_bits(getattr(got.search_tree, name), getattr(want.search_tree, name)), "%s: tree.%s" % (what, name)


def record_kinds(monkeypatch, spec):
    """the generic recurrent function, recording 'host' / 'agent' / 'mixed' per expansion from the parents it is given"""
    kinds = []
    d = spec[1]
    real = get_unified_recurrent_fn

    def recording(*a, **kw):
        fn = real(*a, **kw)

        def recurrent_fn(params, key, actions, observations):
            host = (observations[:, -d:].abs() <= 1e-8).all(dim=1)
            kinds.append("host" if bool(host.all()) else "mixed" if bool(host.any()) else "agent")
            return fn(params, key, actions, observations)

        recurrent_fn.expander = fn.expander
        return recurrent_fn

    monkeypatch.setattr(SF, "get_unified_recurrent_fn", recording)
    return kinds


@pytest.mark.parametrize("use_graph", (False, True), ids=("eager", "graph"))
@pytest.mark.parametrize("batch", (33, 256))
@pytest.mark.parametrize("spec,built", (((10, 3), True), ((20, 4), False)), ids=("10x3-built", "20x4-standin"))
def test_search_with_the_expander_equals_the_generic_search(monkeypatch, spec, built, batch, use_graph):
    t = make_trainer(spec, batch, built)
    kinds = record_kinds(monkeypatch, spec)
    generic = loop_of(t, None, False)
    monkeypatch.undo()
    fused = loop_of(t, expander_of(t), use_graph)
    args = dict(role_fn_args=(t.host_params,), opponent_fn_args=(t.agent_params,))
    what = "spec %s batch %d %s" % (spec, batch, "graph" if use_graph else "eager")
    for seed in (11, 12):  # the second call of a graph loop replays the capture of the first
        roots = roots_of(t, seed)
        del kinds[:]
        want = generic(seed, roots, **args)
        assert len(kinds) == EVALUATIONS
        # the generic path alone must have met every kind of batch: otherwise the comparison shows nothing about the rule
        assert "host" in kinds, "no all-host expansion occurred: %s" % kinds
        assert "agent" in kinds, "no all-agent expansion occurred: %s" % kinds
        assert "mixed" in kinds, "no mixed expansion occurred: %s" % kinds
        got = fused(seed, roots, **args)
        assert_same_output(got, want, "%s seed %d (kinds %s)" % (what, seed, "".join(k[0] for k in kinds)))


def test_expander_declines_what_the_kernel_does_not_serve():
    t = make_trainer((10, 3), 33, True)
    e = expander_of(t)
    roots = roots_of(t, 1)
    assert e.accepts(roots)
    assert not e.accepts(roots.double()) and not e.accepts(roots[:, :-1]) and not e.accepts(roots.cpu())
    assert not UnifiedExpander(None, None, (10, 6), 0.99, True, True).accepts(torch.zeros((4, 66), device="cuda"))
    assert not UnifiedExpander(None, None, (2047, 4), 0.99, True, True).accepts(torch.zeros((1, 2048 * 4), device="cuda"))
    with pytest.raises(ValueError):
        loop_of(t, None, True)  # no expander: the kind is decided on the host, nothing to capture
    with pytest.raises(TypeError):
        from hironaka_amd.recurrent_fn import HostExpander
        get_unified_recurrent_fn(None, None, t.reward_fns["agent"], t.spec,
                                 expander=HostExpander(None, None, t.spec, 0.99, True, True))


@pytest.mark.parametrize("built", (True, False), ids=("built", "standin"))
def test_one_search_with_the_expander_never_synchronises(built):
    """under torch's sync debug mode "error" a whole _run_search with the expander raises nothing"""
    t = make_trainer((10, 3), 33, built)
    fn = get_unified_recurrent_fn(None, None, t.reward_fns["agent"], t.spec, discount=t.discount, reposition=t.reposition,
                                  expander=expander_of(t))
    roots = roots_of(t, 3)
    a = 2 ** 3 - 3 - 1
    root = S.RootFnOutput(torch.zeros((33, a), device=t.device), torch.zeros(33, device=t.device), roots)
    gumbel = S._draw_gumbel(5, (33, a), 0.3, t.device)
    table = S._considered_visits_table(CONSIDERED, EVALUATIONS, t.device)
    params = ((t.host_params,), (t.agent_params,))
    S._run_search(params, None, root, gumbel, None, table, fn, EVALUATIONS, MAX_DEPTH, CONSIDERED)  # lazy initialisations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = S._run_search(params, None, root, gumbel, None, table, fn, EVALUATIONS, MAX_DEPTH, CONSIDERED)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(out.search_tree.node_visits[:, 0].min()) > 1 and out.action.shape == (33,)
