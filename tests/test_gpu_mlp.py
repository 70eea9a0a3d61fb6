"""hk_mlp_forward and hironaka_amd.nets on the device against tests/mlp_rules.py (which test_mlp_rules.py pins to
dqn_rules.fma_exact and, within a measured tolerance, to torch) and against tests/golden/mlp_nets.npz.

Everything the kernel writes is compared with the rule bit for bit (NaNs have to sit in the same places).  The shapes
are the smallest that reach every path: widths on both sides of the MFMA's 16 and of 32 / 64 / 256, batches on both
sides of the 16- and 64-row tiles (each forced in turn, and the crossover between them), 1 to 32 layers."""
import copy
import itertools
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import mlp_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A

pytestmark = pytest.mark.gpu
same_bits = R.same_bits
F32 = np.float32
TILES = (A.HK_MLP_TILE_SMALL, A.HK_MLP_TILE_LARGE)
WIDTHS = (1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256)
SENTINEL = -77.25


def _ops():
    from hironaka_amd import ops
    return ops


def _nets():
    from hironaka_amd import nets
    return nets


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def device_layers(layers):
    return [_ops().MlpLayer(*(dev(t) for t in l[:6]), l.eps, l.relu) for l in layers]


def inputs(rng, batch, k):
    """entries in [-1, 1], a few zeros and negative zeros"""
    x = rng.uniform(-1, 1, (batch, k)).astype(F32)
    x[rng.random((batch, k)) < 0.05] = 0
    x[rng.random((batch, k)) < 0.02] = -0.0
    return x


def check(x, layers, tile=None, where=None, **kw):
    got = _ops().mlp_forward(dev(x), device_layers(layers), tile=tile, input_relu=kw.get("input_relu", False),
                             input_bn=None if kw.get("input_bn") is None else device_layers([kw["input_bn"]])[0])
    want = R.forward(x, layers, **kw)
    assert same_bits(got.cpu().numpy(), want), (where, tile)


@pytest.mark.parametrize("tile", TILES)
def test_single_layers_of_every_width(tile):
    """a sparse cross: every k with n in {3, 17, 256} and the reverse, 19 rows (one full MFMA tile and a tail)"""
    rng = np.random.default_rng(10)
    pairs = sorted({(k, n) for k in WIDTHS for n in (3, 17, 256)} | {(k, n) for n in WIDTHS for k in (3, 17, 256)})
    for i, (k, n) in enumerate(pairs):
        layers = R.random_layers(rng, (k, n), bias=i % 3 != 0, bn=i % 2 == 0, affine=i % 4 == 0, last_relu=i % 5 == 0)
        check(inputs(rng, 19, k), layers, tile, (k, n))


@pytest.mark.parametrize("tile", TILES)
def test_every_batch_around_the_tiles(tile):
    rng = np.random.default_rng(11)
    layers = R.random_layers(rng, (37, 70, 5), bn=True)
    x = inputs(rng, 3 * tile + 1, 37)
    for batch in sorted({1, 2, 15, 16, 17, 63, 64, 65, 3 * tile + 1}):
        check(x[:batch], layers, tile, batch)
    assert _ops().mlp_forward(dev(x[:0]), device_layers(layers), tile=tile).shape == (0, 5)


def test_row_tile_crossover():
    """the batch on either side of the crossover, with the tile the library picks itself"""
    rng = np.random.default_rng(12)
    layers = R.random_layers(rng, (5, 9, 3))
    x = inputs(rng, A.HK_MLP_TILE_CROSSOVER + 1, 5)
    from hironaka_amd._lib import lib
    assert lib().hk_mlp_row_tile(len(x) - 1) == A.HK_MLP_TILE_SMALL and lib().hk_mlp_row_tile(len(x)) == A.HK_MLP_TILE_LARGE
    want = R.forward(x, layers)
    for batch in (len(x) - 1, len(x)):
        got = _ops().mlp_forward(dev(x[:batch]), device_layers(layers))
        assert same_bits(got.cpu().numpy(), want[:batch]), batch


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("nlayers", [1, 2, 23, 32])
def test_layer_counts(nlayers, tile):
    rng = np.random.default_rng(nlayers)
    widths = [60] + [int(w) for w in rng.choice([7, 16, 33, 64, 100], nlayers - 1)] + [4]
    # weights of the size that keeps a ReLU stack's activations: the last layers still see non-zero rows
    layers = [l._replace(weight=(l.weight * np.sqrt(6.0)).astype(F32))
              for l in R.random_layers(rng, widths, bn=nlayers % 2 == 0)]
    x = inputs(rng, 33, 60)
    check(x, layers, tile, nlayers, input_relu=True)
    assert np.abs(R.forward(x, layers, input_relu=True)).min() > 0


def test_options():
    rng = np.random.default_rng(13)
    x = inputs(rng, 21, 19)
    for bias, bn, affine, input_relu, last_relu, in_bn in itertools.product((False, True), repeat=6):
        if affine and not bn:
            continue
        layers = R.random_layers(rng, (19, 40, 6), bias=bias, bn=bn, affine=affine, last_relu=last_relu)
        input_bn = R.random_layers(rng, (19, 19), bn=True, affine=affine)[0]._replace(weight=None, bias=None) if in_bn else None
        check(x, layers, None, (bias, bn, affine, input_relu, last_relu, in_bn), input_relu=input_relu, input_bn=input_bn)


class Guarded:
    """a [batch, width] view at an element offset and row stride into a sentinel-filled storage"""

    def __init__(self, batch, width, offset, stride, values=None):
        self.store = torch.full((offset + batch * stride + 8,), SENTINEL, dtype=torch.float32, device="cuda")
        self.view = self.store[offset:offset + batch * stride].view(batch, stride)[:, :width]
        self.expect = np.full(self.store.numel(), SENTINEL, F32)
        self.mask = np.zeros(self.store.numel(), bool)
        for b in range(batch):
            self.mask[offset + b * stride:offset + b * stride + width] = True
        if values is not None:
            self.view.copy_(dev(values))
            self.expect[self.mask] = values.reshape(-1)

    def holds(self, values=None):
        if values is not None:
            self.expect[self.mask] = values.reshape(-1)
        return same_bits(self.store.cpu().numpy(), self.expect)


class Packed:
    """arrays (None: none) back to back, `gap` sentinels between neighbours, in one sentinel-filled flat buffer from element
    `start` on with 8 sentinels behind the last: whatever 4-byte boundary that gives each.  `views` are the tensors,
    `expect` is the buffer as a launch that only reads them must leave it (`put` says what a launch writes)."""

    def __init__(self, arrays, start, gap=0):
        self.at, at = [], start
        for a in arrays:
            self.at.append(None if a is None else at)
            at += 0 if a is None else a.size + gap
        self.expect = np.full(at + 8, SENTINEL, F32)
        for a, p in zip(arrays, self.at):
            if a is not None:
                self.expect[p:p + a.size] = a.ravel()
        self.store = dev(self.expect)
        self.views = [None if a is None else self.store[p:p + a.size].view(*a.shape) for a, p in zip(arrays, self.at)]

    def put(self, i, values):
        self.expect[self.at[i]:self.at[i] + values.size] = values.ravel()

    def holds(self):
        return same_bits(self.store.cpu().numpy(), self.expect)


def repoint(module, start):
    """every parameter and floating-point buffer of `module` re-pointed at a view of ONE flat sentinel-padded tensor,
    back to back from element `start`: (flat, [(view's first element, numel)])"""
    tensors = list(module.parameters()) + [b for b in module.buffers() if b.is_floating_point()]
    flat = torch.full((start + sum(t.numel() for t in tensors) + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    where, at = [], start
    with torch.no_grad():
        for t in tensors:
            view = flat[at:at + t.numel()].view_as(t)
            view.copy_(t)
            t.data = view
            where.append((at, t.numel()))
            at += t.numel()
    return flat, where


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_parameters_packed_in_a_flat_buffer(start):
    """64 -> 64 -> 4 (K % 4 == 0 everywhere: the 16-byte loads of the weights hang on the address alone) with every
    parameter a view into one flat buffer from element `start`; 19 rows, every tile.  The rule's bits, and the buffer
    -- sentinels and parameters -- as it was."""
    rng = np.random.default_rng(17)
    layers = R.random_layers(rng, (64, 64, 4), bn=True)
    input_bn = R.random_layers(rng, (64, 64), bn=True)[0]._replace(weight=None, bias=None)
    x = inputs(rng, 19, 64)
    want = R.forward(x, layers, input_relu=True, input_bn=input_bn)
    packed = Packed([a for l in [input_bn] + layers for a in l[:6]], start)
    assert sorted({(p % 4) for p in packed.at if p is not None}) == [start % 4]  # every size is a multiple of 4 here
    views = iter(packed.views)
    mk = lambda l: _ops().MlpLayer(*(next(views) for _ in range(6)), l.eps, l.relu)  # noqa: E731
    dev_in, dl = mk(input_bn), [mk(l) for l in layers]
    assert dl[0].weight.data_ptr() % 16 == 4 * (start % 4)
    for tile in (None,) + TILES:
        out = Guarded(19, 4, 1, 4)
        _ops().mlp_forward(dev(x), dl, input_relu=True, input_bn=dev_in, out=out.view, tile=tile)
        assert out.holds(want) and packed.holds(), tile
    # tensors of odd sizes one sentinel apart: every boundary at once, K % 4 != 0 next to K % 4 == 0
    layers = R.random_layers(rng, (64, 17, 64, 3), bn=True)
    packed = Packed([a for l in layers for a in l[:6]], start, gap=1)
    assert len({p % 4 for p in packed.at}) == 4
    views = iter(packed.views)
    dl = [mk(l) for l in layers]
    for tile in TILES:
        got = _ops().mlp_forward(dev(x), dl, tile=tile)
        assert same_bits(got.cpu().numpy(), R.forward(x, layers)) and packed.holds(), tile


def test_a_module_whose_parameters_are_views_of_one_flat_tensor(fixture):
    """create_mlp's net re-pointed at one flat tensor (a flattened parameter vector): the kernel's path, the rule's bits,
    a new table (every data_ptr changed), and the flat tensor as it was"""
    key = "test_host"  # 60 -> 16 -> 32 -> 32 -> 16 -> 4: K % 4 == 0 everywhere
    net = fixture_net(fixture, key)
    x = fixture_input(fixture, key)
    want = rule_output(fixture, key, net)
    with torch.inference_mode():
        assert same_bits(net(x).cpu().numpy(), want) and net.fused_last_reason is None
    for start in (1, 2, 3, 0):
        plan = net.__dict__["_fused_plan"]
        flat, where = repoint(net, start)
        before = flat.clone()
        assert next(net.parameters()).data_ptr() == flat.data_ptr() + 4 * start and where[0] == (start, 16 * 60)
        with torch.inference_mode():
            y = net(x)
        assert net.fused_last_reason is None and net.__dict__["_fused_plan"] is not plan, start
        assert same_bits(y.cpu().numpy(), want) and torch.equal(flat, before), start
        assert bool((flat[:start] == SENTINEL).all()) and bool((flat[-8:] == SENTINEL).all())


@pytest.mark.parametrize("tile", TILES)
def test_layouts_and_guards(tile):
    """two segments; offset, strided and record layouts of x0, x1 and out between sentinels that must stay"""
    rng = np.random.default_rng(14)
    batch, k0, k1, n = 37, 60, 3, 4
    layers = R.random_layers(rng, (k0 + k1, 33, n), bn=True)
    a, b = inputs(rng, batch, k0), inputs(rng, batch, k1)
    want = R.forward(np.concatenate([a, b], axis=1), layers, input_relu=True)
    dl = device_layers(layers)
    # (offset, stride) per tensor: dense, offset by one element (no 16-byte alignment), strided, one record of all three
    for case, (ox0, sx0, ox1, sx1, oo, so) in enumerate([(0, k0, 0, k1, 0, n), (1, k0, 3, k1, 1, n), (2, k0 + 5, 1, k1 + 2, 3, n + 7)]):
        x0, x1, out = Guarded(batch, k0, ox0, sx0, a), Guarded(batch, k1, ox1, sx1, b), Guarded(batch, n, oo, so)
        got = _ops().mlp_forward(x0.view, dl, x1=x1.view, input_relu=True, out=out.view, tile=tile)
        assert got is out.view and out.holds(want) and x0.holds() and x1.holds(), case
    stride = k0 + k1 + n + 2  # records [x0 | x1 | out | 2 spare]
    rec = torch.full((batch, stride), SENTINEL, dtype=torch.float32, device="cuda")
    rec[:, :k0], rec[:, k0:k0 + k1] = dev(a), dev(b)
    _ops().mlp_forward(rec[:, :k0], dl, x1=rec[:, k0:k0 + k1], input_relu=True, out=rec[:, k0 + k1:k0 + k1 + n], tile=tile)
    expect = np.full((batch, stride), SENTINEL, F32)
    expect[:, :k0], expect[:, k0:k0 + k1], expect[:, k0 + k1:k0 + k1 + n] = a, b, want
    assert same_bits(rec.cpu().numpy(), expect)
    # a broadcast row (stride 0) and a 3-d input that the front end flattens
    one = _ops().mlp_forward(dev(a[:1]).expand(batch, k0), dl, x1=dev(b), input_relu=True, tile=tile)
    assert same_bits(one.cpu().numpy(), R.forward(np.concatenate([np.repeat(a[:1], batch, 0), b], axis=1), layers, input_relu=True))
    cube = _ops().mlp_forward(dev(a).view(batch, 20, 3), dl, x1=dev(b), input_relu=True, tile=tile)
    assert same_bits(cube.cpu().numpy(), want)


def test_front_end_refuses():
    ops = _ops()
    rng = np.random.default_rng(15)
    layers = R.random_layers(rng, (6, 5, 2))
    dl, x = device_layers(layers), dev(inputs(rng, 4, 6))
    with pytest.raises(TypeError):
        ops.mlp_forward(x.cpu(), dl)
    with pytest.raises(TypeError):
        ops.mlp_forward(x.double(), dl)
    with pytest.raises(TypeError):
        ops.mlp_forward(x, [dl[0]._replace(weight=dl[0].weight.cpu()), dl[1]])
    with pytest.raises(ValueError):
        ops.mlp_forward(x[:, :5], dl)
    with pytest.raises(ValueError):
        ops.mlp_forward(x, dl[::-1])
    with pytest.raises(ValueError):
        ops.mlp_forward(x, dl, out=torch.empty(4, 3, device="cuda"))
    with pytest.raises(ValueError):
        ops.mlp_forward(x, dl, tile=32)
    from hironaka_amd._lib import HironakaHipError
    with pytest.raises(HironakaHipError) as e:  # out overlapping a parameter: the library's own status
        ops.mlp_forward(x[:1], dl, out=dl[1].bias.view(1, 2))
    assert e.value.status == A.HK_ERR_UNSUPPORTED


@pytest.mark.parametrize("tile", TILES)
def test_a_nan_stays_in_its_row(tile):
    rng = np.random.default_rng(16)
    layers = R.random_layers(rng, (20, 48, 48, 3), bn=True)
    x = inputs(rng, 70, 20)
    clean = _ops().mlp_forward(dev(x), device_layers(layers), tile=tile).cpu().numpy()
    x[5, 7], x[66, 0] = np.nan, np.inf
    got = _ops().mlp_forward(dev(x), device_layers(layers), tile=tile).cpu().numpy()
    assert same_bits(got, R.forward(x, layers))
    assert np.isnan(got[5]).all() and not np.isfinite(got[66]).any()
    rest = np.delete(np.arange(70), [5, 66])
    assert same_bits(got[rest], clean[rest])


# ---- through hironaka_amd.nets ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "mlp_nets.npz"))


def fixture_net(fixture, key):
    nets = _nets()
    name, head = key.rsplit("_", 1)
    input_dim, output_dim = R.HEADS[head]
    extractor = nets.HostFeatureExtractor if head == "host" else nets.AgentFeatureExtractor
    net = nets.create_mlp(extractor(input_dim), json.loads(str(fixture[f"{key}_arch"])), input_dim, output_dim)
    state = R.seeded_state(json.loads(str(fixture[f"{key}_shapes"])), int(fixture[f"{key}_seed"]))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return net.eval().cuda()


def fixture_input(fixture, key, dtype=torch.float32):
    points = dev(fixture[f"{key}_points"]).to(dtype)
    return points if key.endswith("_host") else {"points": points, "coords": dev(fixture[f"{key}_coords"]).to(dtype)}


def plain(net):
    return nn.Sequential(*net.children()).train(net.training)


_RULE = {}


def rule_output(fixture, key, net):
    """the rule's output on the fixture's batch, computed once per net"""
    if key not in _RULE:
        layers, input_relu, input_bn = R.spec_layers(_nets().mlp_spec(net), lambda t: None if t is None
                                                     else t.detach().cpu().numpy())
        x = fixture[f"{key}_points"].reshape(R.ROWS, -1)
        if key.endswith("_agent"):
            x = np.concatenate([x, fixture[f"{key}_coords"]], axis=1)
        _RULE[key] = R.forward(x, layers, input_relu, input_bn)
        _RULE[key].setflags(write=False)
    return _RULE[key]


@pytest.mark.parametrize("key", [f"{n}_{h}" for n in R.NET_ARCHS if n not in R.RESIDUAL for h in R.HEADS])
def test_fixture_nets_end_to_end(fixture, key):
    net = fixture_net(fixture, key)
    x = fixture_input(fixture, key)
    with torch.inference_mode():
        assert net.fused_reason is None
        y = net(x)
        by_torch = plain(net)(x)
        y64 = copy.deepcopy(plain(net)).double()(fixture_input(fixture, key, torch.float64))
    want = rule_output(fixture, key, net)
    assert same_bits(y.cpu().numpy(), want)
    # the front end on the same tensors: the same bits
    spec = _nets().mlp_spec(net)
    layers, input_relu, input_bn = R.spec_layers(spec, lambda t: t)
    mk = _ops().MlpLayer
    args = (x,) if key.endswith("_host") else (x["points"],)
    direct = _ops().mlp_forward(*args, [mk(*l) for l in layers], x1=None if key.endswith("_host") else x["coords"],
                                input_relu=input_relu, input_bn=None if input_bn is None else mk(*input_bn))
    assert torch.equal(direct, y)
    # within the measured distance of a float64 forward on the device (the margin: test_mlp_rules.py)
    e_gpu_torch, e_kernel = R.units(by_torch.cpu().numpy(), y64.cpu().numpy()), R.units(want, y64.cpu().numpy())
    print(f"{key}: E_gpu_torch {e_gpu_torch:.2f} E_kernel {e_kernel:.2f}")
    assert e_kernel <= 8 * max(e_gpu_torch, 1)
    assert R.units(want, fixture[f"{key}_y64"]) == float(fixture[f"{key}_e_rule"])


def test_torch_path_where_the_kernel_does_not_serve(fixture):
    nets = _nets()
    for key, prepare, reason in [
            ("test_host", lambda n: n, "gradients are on"),
            ("test_agent", lambda n: n.train(), "training mode"),
            ("plain_host", lambda n: n.double(), "float32"),
            ("residual_agent", lambda n: n, "ResidualBlock")]:
        net = prepare(fixture_net(fixture, key))
        dtype = next(net.parameters()).dtype
        x = fixture_input(fixture, key, dtype)
        grad = key == "test_host"
        with torch.set_grad_enabled(grad):
            assert reason in net.fused_reason, (key, net.fused_reason)
            state = copy.deepcopy(net.state_dict())
            y = net(x)
            net.load_state_dict(state)  # (training mode moved the running statistics)
            assert torch.equal(y, plain(net)(x)), key
            assert y.requires_grad == grad
    # a float64 input to a float32 net raises as nn.Sequential does; a switched-off module takes torch's path
    net = fixture_net(fixture, "plain_host")
    with torch.inference_mode():
        net.fused_enabled = False
        assert torch.equal(net(fixture_input(fixture, "plain_host")), plain(net)(fixture_input(fixture, "plain_host")))
        with pytest.raises(RuntimeError):
            net(fixture_input(fixture, "plain_host", torch.float64))


def test_serves_the_new_values(fixture):
    key = "test_agent"
    net = fixture_net(fixture, key)
    x = fixture_input(fixture, key)

    def served(n):
        layers, input_relu, input_bn = R.spec_layers(_nets().mlp_spec(n), lambda t: None if t is None else t.detach().cpu().numpy())
        want = R.forward(np.concatenate([fixture[f"{key}_points"].reshape(R.ROWS, -1), fixture[f"{key}_coords"]], axis=1),
                         layers, input_relu, input_bn)
        with torch.inference_mode():
            return same_bits(n(x).cpu().numpy(), want)
    assert served(net)
    # an in-place optimiser step: the same addresses, new values
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    plain(net)(x).square().mean().backward()
    opt.step()
    net.eval()
    assert served(net)
    # replaced tensors: .to() and back, a deepcopy, a loaded state
    moved = net.cpu().cuda()
    assert served(moved)
    clone = copy.deepcopy(net)
    with torch.no_grad():
        for p in clone.parameters():
            p.mul_(1.5)
    assert served(clone) and served(net)
    with torch.inference_mode():
        assert not torch.equal(clone(x), net(x))
    net.load_state_dict(clone.state_dict())
    with torch.inference_mode():
        assert torch.equal(clone(x), net(x))
    fused = _nets().fuse(plain(net))
    assert [id(m) for m in fused.children()] == [id(m) for m in net.children()] and served(fused.eval())
    # tensor OBJECTS that are swapped for others while the old ones stay alive: a parameter and a running buffer
    # assigned anew, a state loaded with assign=True; then the stack itself changes: another eps, a ReLU taken out
    held = [net[2].weight, net[3].running_mean]  # (alive here, as they are in the old table)
    net[2].weight = nn.Parameter(net[2].weight.detach() * 0.5)
    assert served(net)
    net[3].running_mean = net[3].running_mean + 0.25
    assert served(net)
    spare = {k: (v * 1.25).clone() if v.is_floating_point() else v.clone() for k, v in clone.state_dict().items()}
    net.load_state_dict(spare, assign=True)
    assert served(net) and net[2].weight.data_ptr() == spare["2.weight"].data_ptr()
    with torch.inference_mode():
        before = net(x).clone()
    net[3].eps = 0.5
    assert served(net)
    with torch.inference_mode():
        assert not torch.equal(net(x), before)
    relu_at = [i for i, m in enumerate(net) if isinstance(m, nn.ReLU)][-1]
    del net[relu_at]
    assert served(net) and len(held) == 2
    net[3] = nn.BatchNorm1d(net[3].num_features).cuda().eval()
    assert served(net)
    # the batch norm on the input is part of the table as well
    front = fixture_net(fixture, "doubled_bn_agent")
    with torch.inference_mode():
        first = front(x).clone()
        front[1].running_var = front[1].running_var * 4
        assert not torch.equal(front(x), first) and torch.allclose(front(x), plain(front)(x), rtol=1e-4, atol=1e-5)


def _top_two_gap_units(q64, allowed=None):
    """the distance of the two largest Q-values of a row (among the allowed actions) in units of max |Q| * 2^-24"""
    unit = q64.abs().max() * R.UNIT
    if allowed is not None:
        q64 = torch.where(allowed, q64, torch.full_like(q64, -float("inf")))
    top = torch.topk(q64, 2, dim=1).values
    return (top[:, 0] - top[:, 1]) / unit


def test_fused_game_plays_the_same_moves(fixture):
    """FusedGame with create_mlp's nets against the same modules as plain nn.Sequential: 5 steps at (20, 3) x 257, each
    from one state, torch.manual_seed reset before each call, exploration rate 0.2.  Rows whose float64 top-two
    Q-values (of the actions the move may take) lie closer than 64 units may differ and are left out; at most 5 % of
    the rows may be left out."""
    from hironaka_amd.core import HipPoints
    from hironaka_amd.fused_game import FusedGame
    host, agent = fixture_net(fixture, "example_host"), fixture_net(fixture, "example_agent")
    with torch.inference_mode():
        assert host.fused_reason is None and agent.fused_reason is None
    games = FusedGame(host, agent, log_time=False), FusedGame(plain(host), plain(agent), log_time=False)
    assert games[0].host_net is host and isinstance(games[0].agent_net, _nets().FusedSequential)
    host64, agent64 = copy.deepcopy(plain(host)).double(), copy.deepcopy(plain(agent)).double()
    b, m, d = 257, 20, 3
    start = torch.randint(0, 20, (b, m, d), generator=torch.Generator().manual_seed(7)).float()
    pts = HipPoints(start.clone())
    pts.get_newton_polytope()
    left_out = 0
    for t in range(5):
        other = HipPoints(pts.points.clone())
        feats = [p.get_features() for p in (pts, other)]
        assert torch.equal(*feats)
        moves = []
        for game, p, f in zip(games, (pts, other), feats):
            torch.manual_seed(100 + t)
            moves.append(game.host_move(p, exploration_rate=0.2, features=f))
        with torch.inference_mode():
            sure = _top_two_gap_units(host64(feats[0].double())) >= 64
        assert torch.equal(moves[0][1][sure], moves[1][1][sure]), t
        host_moves = moves[1][0]  # both agents answer the same host
        actions = []
        for game, p, f in zip(games, (pts, other), feats):
            torch.manual_seed(200 + t)
            actions.append(game.agent_move(p, host_moves, exploration_rate=0.2, features=f))
        with torch.inference_mode():
            q = agent64({"points": feats[0].double(), "coords": host_moves.double()})
            sure_agent = _top_two_gap_units(q, host_moves.bool()) >= 64
        assert torch.equal(actions[0][sure_agent], actions[1][sure_agent]), t
        same = actions[0] == actions[1]
        assert torch.equal(pts.points[same], other.points[same]), t
        left_out = max(left_out, int((~sure).sum()), int((~sure_agent).sum()))
    assert left_out <= 0.05 * b, left_out


def test_a_fused_forward_replays_from_a_graph(fixture):
    key = "example_agent"
    net = fixture_net(fixture, key)
    x = fixture_input(fixture, key)
    static = {k: v.clone() for k, v in x.items()}
    with torch.inference_mode():
        eager = net(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(static)
        graph.replay()
        assert torch.equal(out, eager)
        static["points"].copy_(x["points"].flip(0))
        static["coords"].copy_(x["coords"].flip(0))
        graph.replay()
        assert torch.equal(out, eager.flip(0))


@pytest.mark.parametrize("role", ["host", "agent"])
def test_a_fused_step_replays_from_a_graph(fixture, role):
    """one whole FusedGame.collect with create_mlp's nets -- features, both nets, the torch.rand draws, the argmax, the
    move, the push into the replay buffer -- captured and replayed: the state and the buffer of an eager collect from
    the same state under the same seed, exploration rate 0.2"""
    from hironaka_amd.core import HipPoints
    from hironaka_amd.fused_game import FusedGame
    from hironaka_amd.replay_buffer import ReplayBuffer
    host, agent = fixture_net(fixture, "test_host"), fixture_net(fixture, "test_agent")
    game = FusedGame(host, agent, log_time=False)
    b, m, d = 257, 20, 3
    start = torch.randint(0, 20, (b, m, d), generator=torch.Generator().manual_seed(9)).float()
    shape = (m, d) if role == "host" else {"points": (m, d), "coords": (d,)}
    outputs = 2 ** d - d - 1 if role == "host" else d

    def fresh():
        pts = HipPoints(start.clone())
        pts.get_newton_polytope()
        return pts, ReplayBuffer(shape, outputs, 1024, "cuda")

    pts, buf = fresh()
    first = pts.points.clone()
    torch.manual_seed(31)
    game.collect(pts, role, buf, exploration_rate=0.2)  # (also the warm-up: the encoder and the kernels exist now)
    with torch.inference_mode():
        assert host.fused_last_reason is None and agent.fused_last_reason is None
    g_pts, g_buf = fresh()
    assert torch.equal(g_pts.points, first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        game.collect(g_pts, role, g_buf, exploration_rate=0.2)
    assert not bool(g_buf.cursor.any())  # capturing runs nothing
    torch.manual_seed(31)
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(g_pts.points, first)
    assert torch.equal(g_pts.points, pts.points)
    assert torch.equal(g_buf.cursor, buf.cursor)
    for k, (x, y) in enumerate(zip(g_buf._rings(), buf._rings())):
        assert torch.equal(x, y), k
