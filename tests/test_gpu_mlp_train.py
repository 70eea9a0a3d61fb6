"""hk_train_mlp_forward / hk_train_mlp_backward on the device against the rule of tests/mlp_train_rules.py, bit for bit
in every output, and nets.FusedSequential.fused_training through autograd, fit_network and a captured graph."""
import copy
import itertools
import warnings

import numpy as np
import pytest
import torch
from torch import nn

import mlp_rules as R
import mlp_train_rules as T
from mlp_train_rules import F32, same_bits

pytestmark = pytest.mark.gpu
CAP = 1024


def _ops():
    from hironaka_amd import ops
    return ops


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _device_layers(layers):
    ops = _ops()
    return [ops.MlpTrainLayer(*(_cuda(a) for a in l[:6]), l.eps, l.relu, float(l.momentum),
                              torch.zeros((), dtype=torch.int64, device="cuda") if l.bn_mean is not None else None)
            for l in layers]


def _check(x, layers, grad, input_relu=False, x0=None, x1=None):
    """forward and backward of the rule on x (the segments side by side) against the device on x0 [, x1] (default: x)"""
    ops = _ops()
    out, saved, stats = T.forward(x, layers, input_relu)
    want = T.param_grads(layers, T.backward(layers, saved, grad))
    dl = _device_layers(layers)
    x0 = _cuda(x) if x0 is None else x0
    got_out, sv = ops.mlp_train_forward(x0, ops.MlpTrainPlan(dl, input_relu), x1=x1)
    got = ops.mlp_backward(sv, _cuda(grad))
    assert same_bits(_np(got_out), out)
    for i, (l, s, st) in enumerate(zip(layers, saved, stats)):
        act, z, mean, inv = sv.layer(i)
        assert same_bits(_np(act), s["act"]), i
        if l.bn_mean is None:
            assert z is None and mean is None
            continue
        for name, t in (("z", z), ("mean", mean), ("inv", inv)):
            assert same_bits(_np(t), s[name]), (i, name)
        assert same_bits(_np(dl[i].bn_mean), st[0]) and same_bits(_np(dl[i].bn_var), st[1]), i
        assert int(dl[i].num_batches_tracked) == 1
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(_np(g), w), i
    return sv


@pytest.mark.parametrize("batch", [2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, CAP])
def test_every_batch_size(batch):
    rng = np.random.default_rng(batch)
    layers = T.random_layers(rng, (23, 33, 7), last_relu=batch % 2 == 0)
    x = rng.standard_normal((batch, 23)).astype(F32)
    _check(x, layers, T.sparse_grad(rng, batch, 7), input_relu=True)


WIDTHS = (1, 3, 15, 16, 17, 33, 255, 256)


@pytest.mark.parametrize("k", WIDTHS)
def test_every_width(k):
    """k and n independently, on one- and two-layer stacks (two layers: k -> n -> k, so that each width is an input, an
    output and the length of the backward's chain)"""
    rng = np.random.default_rng(100 + k)
    for n in WIDTHS:
        batch = 5 if max(k, n) > 33 else 18
        x = rng.standard_normal((batch, k)).astype(F32)
        _check(x, T.random_layers(rng, (k, n)), rng.standard_normal((batch, n)).astype(F32))
        _check(x, T.random_layers(rng, (k, n, k)), rng.standard_normal((batch, k)).astype(F32))


@pytest.mark.parametrize("bias,bn,affine", [(True, False, True), (False, True, True), (True, True, False),
                                            (False, False, True), (False, True, False)])
def test_without_bias_batch_norm_or_affine(bias, bn, affine):
    rng = np.random.default_rng(7)
    for batch in ((1, 19) if not bn else (19,)):
        x = rng.standard_normal((batch, 20)).astype(F32)
        _check(x, T.random_layers(rng, (20, 17, 40, 3), bias=bias, bn=bn, affine=affine),
               rng.standard_normal((batch, 3)).astype(F32), input_relu=True)


def test_agent_head_strided_and_offset_inputs():
    rng = np.random.default_rng(8)
    batch = 37
    layers = T.random_layers(rng, (63, 32, 3))
    records = rng.standard_normal((batch, 80)).astype(F32)
    x = np.concatenate([records[:, 1:61], records[:, 70:73]], axis=1)
    store = _cuda(records)
    _check(x, layers, T.sparse_grad(rng, batch, 3), input_relu=True, x0=store[:, 1:61], x1=store[:, 70:73])
    # [B, 20, 3] points are flattened; a row stride of 0 repeats one row
    one = rng.standard_normal((1, 60)).astype(F32)
    _check(np.repeat(one, batch, 0), T.random_layers(rng, (60, 16, 3)), T.sparse_grad(rng, batch, 3),
           x0=_cuda(one).view(1, 20, 3).expand(batch, 20, 3))
    # a gradient whose rows lie apart
    ops = _ops()
    layers = T.random_layers(rng, (9, 5))
    x, wide = rng.standard_normal((batch, 9)).astype(F32), rng.standard_normal((batch, 8)).astype(F32)
    out, saved, _ = T.forward(x, layers)
    want = T.param_grads(layers, T.backward(layers, saved, wide[:, 2:7]))
    _, sv = ops.mlp_train_forward(_cuda(x), _device_layers(layers))
    for g, w in zip(ops.mlp_backward(sv, _cuda(wide)[:, 2:7]), want):
        assert same_bits(_np(g), w)


def test_nan_and_inf_in_the_input():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((21, 18)).astype(F32)
    x[3, 4], x[11, 17] = np.nan, np.inf
    for bn in (False, True):
        sv = _check(x, T.random_layers(rng, (18, 20, 4), bn=bn), rng.standard_normal((21, 4)).astype(F32))
        assert np.isnan(_np(sv.out)).any()


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_parameters_statistics_and_gradients_packed_in_flat_buffers(start):
    """64 -> 64 -> 4 with every parameter a view into one flat buffer from element `start`, and what the kernels write
    -- the running statistics and every gradient -- views into a second one, one sentinel between neighbours: 19 rows
    and 257 (both instantiations).  The rule's bits in every output; the first buffer as it was; in the second the new
    statistics, the gradients, and every sentinel between and around them."""
    from test_gpu_mlp import Packed
    ops = _ops()
    rng = np.random.default_rng(70 + start)
    layers = T.random_layers(rng, (64, 64, 4), momentum=0.5)
    for batch in (19, 257):
        x = rng.standard_normal((batch, 64)).astype(F32)
        grad = rng.standard_normal((batch, 4)).astype(F32)
        out, saved, stats = T.forward(x, layers, True)
        want = T.param_grads(layers, T.backward(layers, saved, grad))
        read = Packed([a for l in layers for a in (l.weight, l.bias, l.bn_weight, l.bn_bias)], start)
        running = [a for l in layers for a in (l.bn_mean, l.bn_var)]
        written = Packed(running + [np.full(g.shape, R.F32(-3.5)) for g in want], (start + 1) % 4, gap=1)
        assert read.views[0].data_ptr() % 16 == 4 * start and len({p % 4 for p in written.at}) == 4
        r, w = iter(read.views), iter(written.views)
        dl = []
        for l in layers:
            weight, bias, gamma, beta = (next(r) for _ in range(4))
            dl.append(ops.MlpTrainLayer(weight, bias, next(w), next(w), gamma, beta, l.eps, l.relu, float(l.momentum),
                                        torch.zeros((), dtype=torch.int64, device="cuda")))
        grads = list(w)
        got_out, sv = ops.mlp_train_forward(_cuda(x), ops.MlpTrainPlan(dl, True))
        got = ops.mlp_backward(sv, _cuda(grad), grads=grads)
        assert same_bits(_np(got_out), out)
        assert len(got) == len(want) and all(g is t for g, t in zip(got, grads))
        for i, g in enumerate(want):
            assert same_bits(_np(got[i]), g), (batch, i)
            written.put(len(running) + i, np.ascontiguousarray(g, F32))
        for i, a in enumerate(a for st in stats for a in st):
            written.put(i, a)
        assert read.holds() and written.holds(), batch
        assert [int(l.num_batches_tracked) for l in dl] == [1, 1]
    # the front end's checks of `grads`
    with pytest.raises(ValueError):
        ops.mlp_backward(sv, _cuda(grad), grads=grads[:-1])
    with pytest.raises(ValueError):
        ops.mlp_backward(sv, _cuda(grad), grads=[grads[1]] + grads[1:])
    with pytest.raises(TypeError):
        ops.mlp_backward(sv, _cuda(grad), grads=[grads[0].t().contiguous().t()] + grads[1:])


def test_ops_refuse_what_the_kernels_do_not_take():
    ops = _ops()
    rng = np.random.default_rng(10)
    dl = _device_layers(T.random_layers(rng, (6, 5, 3)))
    with pytest.raises(ValueError):
        ops.mlp_train_forward(torch.zeros(1, 6, device="cuda"), dl)  # a batch norm over one row
    with pytest.raises(ValueError):
        ops.mlp_train_forward(torch.zeros(CAP + 1, 6, device="cuda"), dl)
    with pytest.raises(ValueError):
        ops.mlp_train_forward(torch.zeros(4, 7, device="cuda"), dl)
    with pytest.raises(TypeError):
        ops.mlp_train_forward(torch.zeros(4, 6, device="cuda", dtype=torch.float64), dl)
    out, sv = ops.mlp_train_forward(torch.zeros(4, 6, device="cuda"), dl)
    with pytest.raises(TypeError):
        ops.mlp_backward(sv, torch.zeros(4, 2, device="cuda"))
    plain = _device_layers(T.random_layers(rng, (6, 5, 3), bn=False))
    out, sv = ops.mlp_train_forward(torch.zeros(0, 6, device="cuda"), plain)
    assert out.shape == (0, 3) and all(not g.any() for g in ops.mlp_backward(sv, torch.zeros(0, 3, device="cuda")))


# ---- through nets.FusedSequential ---------------------------------------------------------------------------------------

def _net_input(head, points, coords):
    return _cuda(points) if head == "host" else {"points": _cuda(points), "coords": _cuda(coords)}


def _net_rule(net, head, points, coords, grad):
    from hironaka_amd import nets
    layers, input_relu = T.spec_layers(nets.mlp_spec(net), lambda t: None if t is None else _np(t).copy())
    x = points.reshape(len(points), -1)
    if head == "agent":
        x = np.concatenate([x, coords], axis=1)
    out, saved, stats = T.forward(x, layers, input_relu)
    return out, T.param_grads(layers, T.backward(layers, saved, grad)), stats


@pytest.mark.parametrize("name,head,rows", [("test", "host", 256), ("test", "agent", 256), ("example", "host", 32)])
def test_reference_configs_end_to_end(name, head, rows):
    net = T.seeded_net(name, head, 11, fused_training=True).cuda()
    points, coords = T.seeded_rows(12, rows)
    grad = T.sparse_grad(np.random.default_rng(13), rows, R.HEADS[head][1])
    out, grads, stats = _net_rule(net, head, points, coords, grad)
    assert net.fused_reason is None
    q = net(_net_input(head, points, coords))
    assert net.fused_last_reason is None and q.requires_grad
    q.backward(_cuda(grad))
    assert same_bits(_np(q), out)
    params = list(net.parameters())
    assert len(params) == len(grads)
    for p, g in zip(params, grads):
        assert same_bits(_np(p.grad), g)
    bns = [m for m in net if isinstance(m, nn.BatchNorm1d)]
    for bn, (mean, var) in zip(bns, [s for s in stats if s[0] is not None]):
        assert same_bits(_np(bn.running_mean), mean) and same_bits(_np(bn.running_var), var)
        assert int(bn.num_batches_tracked) == 1
    # eval mode without gradients is hk_mlp_forward's, with the statistics where the training forward left them
    net.eval()
    from hironaka_amd import nets
    with torch.no_grad():
        y = net(_net_input(head, points, coords))
        assert net.fused_last_reason is None
        layers, input_relu, input_bn = R.spec_layers(nets.mlp_spec(net), lambda t: None if t is None else _np(t))
        x = points.reshape(rows, -1) if head == "host" else np.concatenate([points.reshape(rows, -1), coords], axis=1)
        assert same_bits(_np(y), R.forward(x, layers, input_relu, input_bn))


def test_a_training_net_whose_parameters_and_buffers_are_views_of_one_flat_tensor():
    """create_mlp's "test" net (60 -> 16 -> 32 -> 32 -> 16 -> 4: K % 4 == 0 everywhere) with every parameter and running
    statistic re-pointed at a view of one flat tensor: the kernels' path, a new table (every data_ptr changed), the
    rule's bits in the result, in every .grad and in the statistics, and the flat tensor's sentinels and parameters as
    they were"""
    from test_gpu_mlp import SENTINEL, repoint
    net = T.seeded_net("test", "host", 71, fused_training=True).cuda()
    points, coords = T.seeded_rows(72, 37)
    grad = T.sparse_grad(np.random.default_rng(73), 37, R.HEADS["host"][1])
    net(_cuda(points))  # a first call builds the table (and moves the statistics once)
    assert net.fused_last_reason is None
    for tracked, start in enumerate((1, 2, 3, 0), 2):
        plan = net.__dict__["_fused_train_plan"]
        flat, where = repoint(net, start)
        nparams = len(list(net.parameters()))
        before = _np(flat).copy()
        out, grads, stats = _net_rule(net, "host", points, coords, grad)
        net.zero_grad()
        q = net(_cuda(points))
        assert net.fused_last_reason is None and net.__dict__["_fused_train_plan"] is not plan, start
        q.backward(_cuda(grad))
        assert same_bits(_np(q), out)
        for p, g in zip(net.parameters(), grads):
            assert same_bits(_np(p.grad), g), start
        bns = [m for m in net if isinstance(m, nn.BatchNorm1d)]
        expect = before.copy()
        buffers = iter(where[nparams:])
        for bn, (mean, var) in zip(bns, [s for s in stats if s[0] is not None]):
            for a in (mean, var):
                at, size = next(buffers)
                expect[at:at + size] = a
            assert same_bits(_np(bn.running_mean), mean) and same_bits(_np(bn.running_var), var)
            assert int(bn.num_batches_tracked) == tracked
        assert same_bits(_np(flat), expect), start
        assert (expect[:start] == SENTINEL).all() and (expect[-8:] == SENTINEL).all()


def test_two_forwards_before_either_backward():
    net = T.seeded_net("test", "host", 21, fused_training=True).cuda()
    twin = copy.deepcopy(net)
    (pa, _), (pb, _) = T.seeded_rows(22, 24), T.seeded_rows(23, 40)
    ga, gb = (T.sparse_grad(np.random.default_rng(s), len(p), 4) for s, p in ((24, pa), (25, pb)))
    qa, qb = net(_cuda(pa)), net(_cuda(pb))
    qb.backward(_cuda(gb))
    second = [p.grad.clone() for p in net.parameters()]
    net.zero_grad()
    qa.backward(_cuda(ga))
    # each alone, from the same start: the first forward's statistics precede the second's
    ta = twin(_cuda(pa))
    ta.backward(_cuda(ga))
    for p, t in zip(net.parameters(), twin.parameters()):
        assert same_bits(_np(p.grad), _np(t.grad))
    twin.zero_grad()
    tb = twin(_cuda(pb))
    tb.backward(_cuda(gb))
    assert same_bits(_np(qa), _np(ta)) and same_bits(_np(qb), _np(tb))
    for g, t in zip(second, twin.parameters()):
        assert same_bits(_np(g), _np(t.grad))
    assert [int(m.num_batches_tracked) for m in net if isinstance(m, nn.BatchNorm1d)] == [2] * 4


def test_a_parameter_changed_in_place_before_the_backward_is_torchs_error():
    net = T.seeded_net("test", "host", 31, fused_training=True).cuda()
    q = net(_cuda(T.seeded_rows(32, 8)[0]))
    with torch.no_grad():
        net[2].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        q.sum().backward()


def test_the_autograd_graph_dies_with_its_output():
    """no reference cycle through the saved state: a graph that waited for the garbage collector would keep its
    AccumulateGrad nodes, on the stream they were made on, into the next step -- and into a capture on another stream"""
    import gc
    import weakref
    net = T.seeded_net("test", "host", 35, fused_training=True).cuda()
    points = _cuda(T.seeded_rows(36, 8)[0])
    gc.collect()
    gc.disable()
    try:
        q = net(points)
        node = weakref.ref(q.grad_fn)
        q.sum().backward()
        del q
        assert node() is None
    finally:
        gc.enable()


class _Buffer:
    def __init__(self, rng, rows, num_actions):
        points, _ = T.seeded_rows(int(rng.integers(1 << 30)), rows)
        nxt, _ = T.seeded_rows(int(rng.integers(1 << 30)), rows)
        self.batch = (_cuda(points), _cuda(rng.integers(0, num_actions, (rows, 1)).astype(np.int32)),
                      _cuda(rng.integers(-1, 2, (rows, 1)).astype(F32)), _cuda(rng.integers(0, 2, (rows, 1)).astype(bool)),
                      _cuda(nxt))

    def sample(self, batch_size, device=None, clone=True):
        return self.batch


def _flat(tensors):
    return np.concatenate([_np(t).ravel() for t in tensors])


def _state(net):
    return _flat(list(net.parameters()) + [b for b in net.buffers() if b.is_floating_point()])


def test_fit_network_equals_the_steps_composed_by_hand_and_does_not_synchronise():
    from hironaka_amd import dqn, optim
    ops = _ops()
    rows = 64
    buffer = _Buffer(np.random.default_rng(41), rows, 4)

    def fresh(training=True, dtype=torch.float32):
        q_net = T.seeded_net("test", "host", 42, training).to(dtype).cuda()
        target = T.seeded_net("test", "host", 43, training).to(dtype).cuda()
        return q_net, target, optim.Adam(q_net.parameters(), lr=1e-3)

    q_net, target, opt = fresh()
    dqn.fit_network(q_net, target, opt, buffer, rows, 0.99, 0.5)  # workspaces, state and descriptors exist now
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "a prototype feature"
        torch.cuda.set_sync_debug_mode("error")  # a synchronising torch call raises
        try:
            for _ in range(2):
                loss = dqn.fit_network(q_net, target, opt, buffer, rows, 0.99, 0.5)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert q_net.fused_last_reason is None and target.fused_last_reason is None  # both nets in training mode
    # by hand
    h_net, h_target, h_opt = fresh()
    from hironaka_amd import nets
    observations, actions, rewards, dones, next_observations = buffer.batch
    for _ in range(3):
        with torch.no_grad():
            next_q = ops.mlp_train_forward(next_observations, h_target._train_plan(nets.mlp_spec(h_target)))[0]
            q, saved = ops.mlp_train_forward(observations, h_net._train_plan(nets.mlp_spec(h_net)))
            res = ops.dqn_td(q, next_q, actions, rewards, dones, 0.99, want=())
            grads = ops.mlp_backward(saved, res.dq)
        for p, g in zip(h_net.parameters(), grads):
            p.grad = g
        h_opt.clip_and_step(0.5)
    assert float(loss.detach()) == float(res.loss)
    assert same_bits(_state(q_net), _state(h_net)) and same_bits(_state(target), _state(h_target))
    # one step with the switch on, off and in float64: the project's bound, E_on <= 8 max(E_off, 1), on the loss and on
    # every clipped gradient (Adam's first step is lr * sign(g): the parameters themselves measure nothing)
    results = {}
    for key, training, dtype in (("on", True, torch.float32), ("off", False, torch.float32), ("f64", False, torch.float64)):
        q_net, target, opt = fresh(training, dtype)
        batch = tuple(t.to(dtype) if t.dtype == torch.float32 else t for t in buffer.batch)
        stub = _Buffer.__new__(_Buffer)
        stub.batch = batch
        loss = dqn.fit_network(q_net, target, opt, stub, rows, 0.99, 0.5)
        assert (q_net.fused_last_reason is None) == (key == "on")
        results[key] = [np.asarray([float(loss.detach())])] + [_np(p.grad) for p in q_net.parameters()]
    for i, (on, off, ref) in enumerate(zip(results["on"], results["off"], results["f64"])):
        # the bias of a Linear in front of a batch norm has a gradient of zero in exact arithmetic: its error is measured
        # in the units of that Linear's weight gradient (results: the loss, then weight, bias, bn weight, bn bias per block)
        scale = results["f64"][i - 1] if i % 4 == 2 and i + 1 < len(results["on"]) else ref
        e_on, e_off = (float(np.abs(v.astype(np.float64) - ref).max() / (np.abs(scale).max() * R.UNIT)) for v in (on, off))
        print(f"tensor {i}: E_off {e_off:.2f} E_on {e_on:.2f}")
        assert e_on <= 8 * max(e_off, 1), (i, e_on, e_off)


def test_a_whole_fit_step_replays_from_a_graph():
    """sample, both nets, TD, backward, clip_and_step and Polyak captured into one graph and replayed three times equal
    three eager steps bit for bit"""
    from hironaka_amd import dqn, optim
    rows = 32
    buffer = _Buffer(np.random.default_rng(51), rows, 4)
    lrs = [0.05, 0.02, 0.01]

    def fresh():
        q_net = T.seeded_net("test", "host", 52, True).cuda()
        target = T.seeded_net("test", "host", 53, True).cuda()
        lr = torch.tensor([lrs[0]], dtype=torch.float64, device="cuda")
        opt = optim.Adam(q_net.parameters(), lr=lr)
        for p in q_net.parameters():  # static gradients, as a captured step needs them
            p.grad = torch.zeros_like(p)
        return q_net, target, opt, lr

    def step(q_net, target, opt):
        observations, actions, rewards, dones, next_observations = buffer.sample(rows)
        with torch.no_grad():
            next_q = target(next_observations)
        loss = dqn.td_loss(q_net(observations), next_q, actions, rewards, dones, 0.99)
        opt.zero_grad(set_to_none=False)
        loss.backward()
        opt.clip_and_step(0.5)
        dqn.update_target_net(q_net, target, 0.3)
        return loss

    q_net, target, opt, lr = fresh()
    eager = []
    for k in range(3):
        lr.fill_(lrs[k])
        loss = step(q_net, target, opt)
        eager.append((loss.item(), _state(q_net), _state(target)))
    assert eager[0][0] != eager[1][0]
    q_net, target, opt, lr = fresh()
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    tensors = list(q_net.parameters()) + list(q_net.buffers()) + list(target.parameters()) + list(target.buffers())
    state = [t.detach().clone() for t in tensors]
    with torch.cuda.stream(warm):  # one step on the side stream builds state, descriptors and workspaces
        step(q_net, target, opt)
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    with torch.no_grad():  # and is undone: parameters, statistics, Adam's state and the count
        for t, s in zip(tensors, state):
            t.copy_(s)
        for p in q_net.parameters():
            opt.state[p]["exp_avg"].zero_()
            opt.state[p]["exp_avg_sq"].zero_()
        opt._blocks[0].copy_(_ops().optim_state("cuda"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=warm):
        loss = step(q_net, target, opt)
    assert q_net.fused_last_reason is None and target.fused_last_reason is None
    for k in range(3):
        lr.fill_(lrs[k])
        graph.replay()
        torch.cuda.synchronize()
        assert loss.item() == eager[k][0], k
        assert same_bits(_state(q_net), eager[k][1]), k
        assert same_bits(_state(target), eager[k][2]), k
    assert [int(m.num_batches_tracked) for m in q_net if isinstance(m, nn.BatchNorm1d)] == [3] * 4


def test_every_fall_back_is_nn_sequential():
    from hironaka_amd import nets
    points = _cuda(T.seeded_rows(61, 12)[0])

    def both(net, x, reason, grad=True):
        """the net's forward and the plain nn.Sequential's over copies of the same modules, from the same state"""
        plain = nn.Sequential(*copy.deepcopy(net)._modules.values()).train(net.training)
        with torch.set_grad_enabled(grad):
            y, want = net(x), plain(x)
        assert reason in (net.fused_last_reason or ""), net.fused_last_reason
        assert torch.equal(y, want)
        for a, b in zip(net.buffers(), plain.buffers()):
            assert torch.equal(a, b)

    make = lambda name="test", **kw: T.seeded_net(name, "host", 62, True, **kw).cuda()  # noqa: E731
    both(make().eval(), points, "gradients are on")
    both(make(), points.clone().requires_grad_(), "the input requires a gradient")
    net = make()
    for m in net:
        if isinstance(m, nn.BatchNorm1d):
            m.momentum = None
    both(net, points, "momentum=None")
    both(make("doubled_bn"), points, "on the input")
    both(make("residual"), points, "ResidualBlock")
    both(make().double(), points.double(), "float32")
    both(make(), points.repeat(100, 1, 1), "more than 1024 rows")
    one = make()
    with pytest.raises(ValueError):
        one(points[:1])
    assert "a batch of 1" in one.fused_last_reason
    off = T.seeded_net("test", "host", 62, False).cuda()
    both(off, points, "a BatchNorm1d in training mode")
    # served: the same calls with the switch on
    on = make()
    on(points)
    assert on.fused_last_reason is None
    with torch.no_grad():
        on(points)
        assert on.fused_last_reason is None
