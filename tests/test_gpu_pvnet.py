"""hk_pvnet_forward and hironaka_amd.net on the device against tests/pvnet_rules.py (which test_pvnet_rules.py pins by hand
and, within torch's own distance of float64, to torch).

Everything the kernel writes is compared with the rule bit for bit under HK_PVNET_RAW_VALUE (NaNs have to sit in the same
places); every case runs with each row tile forced and with the tile the library picks.  The shapes are the smallest that
reach every path: normed widths 32 / 64 / 128 / 256 (1, 2, 4, 8 columns per group), input widths on both sides of the
MFMA's 16 and up to the limit, blocks with and without a projection, batches on both sides of the 16- and 64-row tiles,
1 to 32 blocks."""
import copy
import itertools
import pickle

import numpy as np
import pytest
import torch

import pvnet_rules as R
from hironaka_amd import _abi as A
from test_gpu_mlp import SENTINEL, Guarded, dev, inputs  # noqa: F401  (the same inputs and guarded layouts)

pytestmark = pytest.mark.gpu
same_bits = R.same_bits
F32 = np.float32
TILES = (None, A.HK_MLP_TILE_SMALL, A.HK_MLP_TILE_LARGE)
# |tanhf(z) - tanh(z)| in units of 2^-24 over test_the_tanh's inputs, measured on the MI355X (profiles/pvnet_probe.json
# "tanh_max_units"); the bound is twice that: another seed may land on another pattern of last bits
TANH_MEASURED_UNITS = 0.917
TANH_BOUND_UNITS = 2 * TANH_MEASURED_UNITS


def _ops():
    from hironaka_amd import ops
    return ops


def _net():
    from hironaka_amd import net
    return net


def device_plan(net):
    ops = _ops()
    dn = lambda d: None if d is None else ops.PvnetDense(*(dev(t) for t in d))  # noqa: E731
    return ops.PvnetPlan([ops.PvnetBlock(b.kind, dn(b.dense1), dn(b.dense2), dn(b.proj), b.eps) for b in net.blocks],
                         tuple(dev(t) for t in net.policy), tuple(dev(t) for t in net.value))


def check(x, net, where=None, tiles=TILES, want=None):
    """the kernel's (policy, raw value) on x against the rule's, with every tile"""
    plan = device_plan(net)
    want = R.forward(x, net) if want is None else want
    for tile in tiles:
        p, v = _ops().pvnet_forward(dev(x), plan, tile=tile, raw_value=True)
        assert p.shape == (len(x), net.policy[0].shape[0]) and v.shape == (len(x),)
        assert same_bits(p.cpu().numpy(), want[0]), (where, tile, "policy")
        assert same_bits(v.cpu().numpy(), want[1]), (where, tile, "value")
    return want


@pytest.mark.parametrize("n", [32, 64, 128, 256])
def test_cross_of_normed_and_input_widths(n):
    """one residue block of every normed width behind every input width: 256 -> 256 is the block without a projection at
    the limit; 19 rows (one full MFMA tile and a tail)"""
    rng = np.random.default_rng(n)
    for k0 in (1, 15, 18, 60, 63, 255, 256):
        net = R.random_net(rng, k0, [n], 4)
        assert (net.blocks[0].proj is None) == (k0 == n)
        check(inputs(rng, 19, k0), net, (k0, n))


def test_residue_blocks_with_and_without_projection():
    rng = np.random.default_rng(20)
    for k0, arch in ((60, [64, 128, 128, 32]), (64, [64, 64]), (32, [32, 256, 32, 32]), (18, [128, 64])):
        net = R.random_net(rng, k0, arch, 4)
        assert [b.proj is None for b in net.blocks] == [k == n for k, n in zip([k0] + arch[:-1], arch)]
        check(inputs(rng, 21, k0), net, (k0, arch))


def test_dense_blocks():
    """dense blocks of widths 1, 17, 33 and 256, alone and between residue blocks"""
    rng = np.random.default_rng(21)
    for k0, arch in ((63, [17, 33, 256, 1, 64]), (15, [1]), (256, [256, 33]), (18, [17])):
        check(inputs(rng, 21, k0), R.random_net(rng, k0, arch, 3, "dense"), (k0, arch))
    for k0, arch, kinds in ((18, [64, 33, 128], ["residue", "dense", "residue"]), (60, [17, 32, 1], ["dense", "residue", "dense"])):
        check(inputs(rng, 21, k0), R.random_net(rng, k0, arch, 3, kinds), (k0, arch, kinds))


def test_policy_widths():
    rng = np.random.default_rng(22)
    for actions in (1, 3, 4, 15, 16, 255):
        for k0, arch, kind in ((18, [64], "residue"), (33, [17], "dense")):
            check(inputs(rng, 18, k0), R.random_net(rng, k0, arch, actions, kind), (actions, kind))


@pytest.mark.parametrize("tile", TILES[1:])
def test_a_dense_trunk_is_mlp_forward(tile):
    """a trunk of dense blocks is `Linear -> ReLU` per block and the two heads are one Linear of actions + 1 columns, so
    pvnet_forward (raw value) and mlp_forward, with the policy and value weights stacked as its last layer, run the one
    Dense loop with and without the value row and must give the same bits: column j < A the policy, column A the value.
    Batches one row past a tile; k0 = 15 (weights float by float, a padded chunk) and 60 (16-byte loads, no multiple of
    16); a width that pads and two layers; the value row inside the first column tile (3 actions), as its last column
    (15) and alone in a second one (16)."""
    ops = _ops()
    rng = np.random.default_rng(20261020)
    for batch, k0, arch, actions in itertools.product((17, 65), (15, 60), ([33], [32, 48]), (3, 15, 16)):
        net = R.random_net(rng, k0, arch, actions, "dense")
        x = dev(inputs(rng, batch, k0))
        layers = [ops.MlpLayer(dev(b.dense1.weight), dev(b.dense1.bias), relu=True) for b in net.blocks]
        layers.append(ops.MlpLayer(dev(np.concatenate([net.policy[0], net.value[0]])),
                                   dev(np.concatenate([net.policy[1], net.value[1]]))))
        p, v = ops.pvnet_forward(x, device_plan(net), tile=tile, raw_value=True)
        out = ops.mlp_forward(x, layers, tile=tile).cpu().numpy()
        assert out.shape == (batch, actions + 1) and np.abs(out).max(axis=0).min() > 0
        where = (batch, k0, arch, actions)
        assert same_bits(p.cpu().numpy(), out[:, :actions]), (where, "policy")
        assert same_bits(v.cpu().numpy(), out[:, actions]), (where, "value")


@pytest.mark.parametrize("tile", TILES[1:])
def test_every_batch_around_the_tiles(tile):
    rng = np.random.default_rng(23)
    net = R.random_net(rng, 37, [64, 17], 5, ["residue", "dense"])
    x = inputs(rng, 3 * tile + 1, 37)
    want = R.forward(x, net)
    for batch in sorted({1, 2, 15, 16, 17, 63, 64, 65, 3 * tile + 1}):
        check(x[:batch], net, batch, tiles=(None, tile), want=(want[0][:batch], want[1][:batch]))
    p, v = _ops().pvnet_forward(dev(x[:0]), device_plan(net), tile=tile)
    assert p.shape == (0, 5) and v.shape == (0,)


def test_row_tile_crossover():
    """the batch on either side of the crossover, with the tile the library picks itself"""
    rng = np.random.default_rng(24)
    net = R.random_net(rng, 5, [32], 3)
    rows = rng.integers(0, 64, A.HK_MLP_TILE_CROSSOVER + 1)
    few = inputs(rng, 64, 5)
    x, few_want = few[rows], R.forward(few, net)
    want = few_want[0][rows], few_want[1][rows]
    plan = device_plan(net)
    for batch in (len(x) - 1, len(x)):
        p, v = _ops().pvnet_forward(dev(x[:batch]), plan, raw_value=True)
        assert same_bits(p.cpu().numpy(), want[0][:batch]) and same_bits(v.cpu().numpy(), want[1][:batch]), batch


@pytest.mark.parametrize("nblocks", [1, 2, 18, 32])
def test_block_counts(nblocks):
    rng = np.random.default_rng(nblocks)
    arch = [int(w) for w in rng.choice([64, 128], nblocks)]  # (groups of one column give the bias: other tests)
    kinds = ["dense" if nblocks == 18 and i % 3 == 2 else "residue" for i in range(nblocks)]
    net = R.random_net(rng, 60, arch, 4, kinds)
    x = inputs(rng, 33, 60)
    want = check(x, net, nblocks)
    # the last block still sees rows that are not zero, and the outputs differ from row to row
    before_last = R.trunk(x, net.blocks[:-1])
    assert (np.abs(before_last).max(axis=1) > 0).all() and (np.abs(R.trunk(x, net.blocks)).max(axis=1) > 0).all()
    assert len(np.unique(want[1])) == len(x)


def test_options():
    """every Dense with and without its bias, every group norm with and without its scale and its bias"""
    rng = np.random.default_rng(25)
    x = inputs(rng, 21, 19)
    for bias, scale, shift in itertools.product((False, True), repeat=3):
        net = R.random_net(rng, 19, [64, 64], 6, bias=bias)
        strip = lambda d: None if d is None else d._replace(gn_scale=d.gn_scale if scale else None,  # noqa: E731
                                                            gn_bias=d.gn_bias if shift else None)
        net = net._replace(blocks=[b._replace(dense1=strip(b.dense1), dense2=strip(b.dense2), proj=strip(b.proj)) for b in net.blocks])
        check(x, net, (bias, scale, shift))


@pytest.mark.parametrize("tile", TILES[1:])
def test_layouts_and_guards(tile):
    """x at an element offset and row stride, policy at a row stride, value at an element stride, between sentinels
    that must stay"""
    rng = np.random.default_rng(26)
    batch, k0, a = 37, 60, 4
    net = R.random_net(rng, k0, [64, 33], a, ["residue", "dense"])
    xs = inputs(rng, batch, k0)
    want = R.forward(xs, net)
    plan = device_plan(net)
    for case, (ox, sx, op, sp, ov, sv) in enumerate([(0, k0, 0, a, 0, 1), (1, k0, 1, a, 3, 1), (2, k0 + 5, 3, a + 7, 1, 3)]):
        x, p, v = Guarded(batch, k0, ox, sx, xs), Guarded(batch, a, op, sp), Guarded(batch, 1, ov, sv)
        got = _ops().pvnet_forward(x.view, plan, tile=tile, raw_value=True, policy=p.view, value=v.view[:, 0])
        assert got[0] is p.view and got[1].data_ptr() == v.view.data_ptr() and got[1].stride() == (sv,)
        assert p.holds(want[0]) and v.holds(want[1]) and x.holds(), case
    # policy and value as columns of one record [policy | value | 2 spare]
    rec = torch.full((batch, a + 3), SENTINEL, dtype=torch.float32, device="cuda")
    _ops().pvnet_forward(dev(xs), plan, tile=tile, raw_value=True, policy=rec[:, :a], value=rec[:, a])
    expect = np.full((batch, a + 3), SENTINEL, F32)
    expect[:, :a], expect[:, a] = want
    assert same_bits(rec.cpu().numpy(), expect)
    # a broadcast row (stride 0) and a 3-d input that the front end flattens
    one = _ops().pvnet_forward(dev(xs[:1]).expand(batch, k0), plan, tile=tile, raw_value=True)
    assert same_bits(one[0].cpu().numpy(), np.repeat(want[0][:1], batch, 0)) and same_bits(one[1].cpu().numpy(), np.repeat(want[1][:1], batch))
    cube = _ops().pvnet_forward(dev(xs).view(batch, 20, 3), plan, tile=tile, raw_value=True)
    assert same_bits(cube[0].cpu().numpy(), want[0]) and same_bits(cube[1].cpu().numpy(), want[1])


def test_the_tanh():
    """without the raw flag the policy's bits are the same and the value is tanhf of the rule's pre-activation: within
    TANH_BOUND_UNITS * 2^-24 of float64's tanh (pre-activations spread over +-4 and beyond)"""
    rng = np.random.default_rng(27)
    net = R.random_net(rng, 60, [128, 128], 4, value_gain=4.0)
    x = inputs(rng, 257, 60)
    want = R.forward(x, net)
    assert (np.abs(want[1]) < 4).mean() > 0.5 and want[1].min() < -3 and want[1].max() > 3
    plan = device_plan(net)
    worst = 0.0
    for tile in TILES:
        p, v = _ops().pvnet_forward(dev(x), plan, tile=tile)
        assert same_bits(p.cpu().numpy(), want[0]), tile
        v = v.cpu().numpy()
        assert (np.abs(v) <= 1).all()
        worst = max(worst, float(np.abs(v.astype(np.float64) - np.tanh(want[1].astype(np.float64))).max() / R.M.UNIT))
    print(f"tanh: max deviation {worst:.3f} units of 2^-24 (bound {TANH_BOUND_UNITS})")
    assert worst <= TANH_BOUND_UNITS


def test_front_end_refuses():
    ops = _ops()
    rng = np.random.default_rng(28)
    net = R.random_net(rng, 6, [32], 2)
    plan, x = device_plan(net), dev(inputs(rng, 4, 6))
    with pytest.raises(TypeError):
        ops.pvnet_forward(x.cpu(), plan)
    with pytest.raises(TypeError):
        ops.pvnet_forward(x.double(), plan)
    with pytest.raises(TypeError):
        ops.pvnet_forward(x, [net])
    with pytest.raises(ValueError):
        ops.pvnet_forward(x[:, :5], plan)
    with pytest.raises(ValueError):
        ops.pvnet_forward(x, plan, tile=32)
    with pytest.raises(ValueError):
        ops.pvnet_forward(x, plan, policy=torch.empty(4, 3, device="cuda"))
    with pytest.raises(ValueError):
        ops.pvnet_forward(x, plan, value=torch.empty(4, 1, device="cuda"))
    dn = lambda d: ops.PvnetDense(*(dev(t) for t in d))  # noqa: E731
    b = net.blocks[0]
    heads = (tuple(dev(t) for t in net.policy), tuple(dev(t) for t in net.value))
    with pytest.raises(ValueError, match="normed width"):
        wide = R.random_net(rng, 6, [96], 2, "dense").blocks[0]
        ops.PvnetPlan([ops.PvnetBlock("residue", dn(wide.dense1), dn(wide.dense1), dn(wide.dense1))], *heads)
    with pytest.raises(ValueError, match="proj"):
        ops.PvnetPlan([ops.PvnetBlock("residue", dn(b.dense1), dn(b.dense2))], *heads)
    with pytest.raises(ValueError, match="kind"):
        ops.PvnetPlan([ops.PvnetBlock("conv", dn(b.dense1))], *heads)
    with pytest.raises(TypeError):
        ops.PvnetPlan([ops.PvnetBlock("residue", dn(b.dense1), dn(b.dense2), dn(b.proj)._replace(bias=dev(b.proj.bias).cpu()))], *heads)
    with pytest.raises(ValueError):
        ops.PvnetPlan([ops.PvnetBlock("residue", dn(b.dense1), dn(b.dense2), dn(b.proj))], heads[0], heads[0])
    from hironaka_amd._lib import HironakaHipError
    with pytest.raises(HironakaHipError) as e:  # an output overlapping a parameter: the library's own status
        ops.pvnet_forward(x[:1], plan, policy=plan.tensors[1][:2].view(1, 2))
    assert e.value.status == A.HK_ERR_UNSUPPORTED


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_parameters_packed_in_a_flat_buffer(start):
    """[64, 128] behind k0 = 64 (K % 4 == 0 in every Dense and both heads: the 16-byte loads of the weights hang on the
    address alone) with every parameter a view into one flat buffer from element `start`; 19 rows, every tile.  The
    rule's bits, and the buffer -- sentinels and parameters -- as it was.  Then blocks of other widths one sentinel
    apart: every boundary at once."""
    from test_gpu_mlp import Packed
    ops = _ops()
    rng = np.random.default_rng(40 + start)
    for k0, arch, kinds, actions, gap in ((64, [64, 128], "residue", 4, 0), (60, [17, 64, 128], ["dense", "residue", "residue"], 15, 1)):
        net = R.random_net(rng, k0, arch, actions, kinds)
        x = inputs(rng, 19, k0)
        want = R.forward(x, net)
        denses = [d for b in net.blocks for d in (b.dense1, b.dense2, b.proj)]
        packed = Packed([a for d in denses for a in (d if d is not None else (None,) * 4)] + list(net.policy + net.value),
                        start, gap)
        assert len({p % 4 for p in packed.at if p is not None}) == (4 if gap else 1)
        v = iter(packed.views)

        def dn(d):  # (an absent Dense has four absent views)
            views = [next(v) for _ in range(4)]
            return None if d is None else ops.PvnetDense(*views)
        blocks = [ops.PvnetBlock(b.kind, dn(b.dense1), dn(b.dense2), dn(b.proj), b.eps) for b in net.blocks]
        plan = ops.PvnetPlan(blocks, (next(v), next(v)), (next(v), next(v)))
        assert plan.tensors[0].data_ptr() % 16 == 4 * start
        for tile in TILES:
            policy, value = Guarded(19, actions, 1, actions + 2), Guarded(19, 1, 3, 1)
            ops.pvnet_forward(dev(x), plan, tile=tile, raw_value=True, policy=policy.view, value=value.view[:, 0])
            assert policy.holds(want[0]) and value.holds(want[1]) and packed.holds(), (arch, tile)


def test_a_module_whose_parameters_are_views_of_one_flat_tensor():
    """a DenseResNet re-pointed at one flat tensor (a flattened parameter vector): the kernel's path, the rule's bits, a
    new table (every data_ptr changed), and the flat tensor as it was"""
    from test_gpu_mlp import repoint
    net = randomised(_net().DenseResNet(4, [64, 128], input_dim=64), 41).cuda()
    x = dev(inputs(np.random.default_rng(42), 19, 64))
    assert served(net, x)
    for start in (1, 2, 3, 0):
        plan = net.__dict__["_fused_plan"]
        flat, where = repoint(net, start)
        before = flat.clone()
        assert next(net.parameters()).data_ptr() == flat.data_ptr() + 4 * start
        assert served(net, x) and net.__dict__["_fused_plan"] is not plan, start
        assert torch.equal(flat, before) and bool((flat[:start] == SENTINEL).all()) and bool((flat[-8:] == SENTINEL).all())


@pytest.mark.parametrize("tile", TILES[1:])
def test_a_nan_stays_in_its_row(tile):
    rng = np.random.default_rng(29)
    net = R.random_net(rng, 20, [64, 48, 128], 3, ["residue", "dense", "residue"])
    x = inputs(rng, 70, 20)
    plan = device_plan(net)
    clean = [t.cpu().numpy() for t in _ops().pvnet_forward(dev(x), plan, tile=tile, raw_value=True)]
    x[5, 7], x[66, 0] = np.nan, np.inf
    got = [t.cpu().numpy() for t in _ops().pvnet_forward(dev(x), plan, tile=tile, raw_value=True)]
    want = R.forward(x, net)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert np.isnan(got[0][5]).all() and np.isnan(got[1][5]) and not np.isfinite(got[0][66]).any()
    rest = np.delete(np.arange(70), [5, 66])
    assert same_bits(got[0][rest], clean[0][rest]) and same_bits(got[1][rest], clean[1][rest])


# ---- through hironaka_amd.net -----------------------------------------------------------------------------------------

def to_numpy(t):
    return None if t is None else t.detach().cpu().numpy()


def randomised(net, seed):
    """biases, scales and shifts away from flax's zeros and ones"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(torch.rand(p.shape, generator=g) - 0.5)
    return net


def served(net, x):
    """the module's call under no_grad took the kernel's path and gave the rule's bits on the module's own parameters"""
    rule = R.module_net(net, to_numpy)
    want = R.forward(x.flatten(1).cpu().numpy(), rule)
    with torch.no_grad():
        p, v = net(x)
        raw = _ops().pvnet_forward(x, net._cached_plan(), raw_value=True)
    tanh = np.tanh(want[1].astype(np.float64))
    return (net.fused_last_reason is None and p.shape == (len(x), net.output_size) and v.shape == (len(x), 1)
            and same_bits(p.cpu().numpy(), want[0]) and same_bits(raw[0].cpu().numpy(), want[0])
            and same_bits(raw[1].cpu().numpy(), want[1])
            and float(np.abs(v[:, 0].cpu().numpy() - tanh).max()) <= TANH_BOUND_UNITS * R.M.UNIT)


@pytest.mark.parametrize("make", [lambda N: N.DenseResNet(4, [64, 128, 128, 32], spec=(20, 3), role="host", seed=1),
                                  lambda N: N.DenseNet(3, [17, 33], spec=(20, 3), role="agent", seed=2),
                                  lambda N: N.DResNetMini(3, spec=(5, 3), role="agent", seed=3)])
def test_the_module_takes_the_kernels_path(make):
    net = randomised(make(_net()), 4).cuda()
    x = dev(inputs(np.random.default_rng(30), 37, net.input_dim))
    with torch.no_grad():
        assert net.fused_reason is None
    assert served(net, x) and served(net, x.view(37, -1, 3))
    # with gradients on: the plain composition, and the module says so
    p, v = net(x)
    assert net.fused_last_reason == "gradients are on" and p.requires_grad and v.requires_grad
    plain = net.plain_forward(x)
    assert torch.equal(p, plain[0]) and torch.equal(v, plain[1])
    with torch.no_grad():
        net.fused_enabled = False
        off = net(x)
        assert net.fused_last_reason == "fused_enabled is False" and torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
        net.fused_enabled = True
        with pytest.raises(RuntimeError):  # an input of another dtype raises as the children do
            net(x.double())
        assert "float32" in net.fused_last_reason


def test_the_module_serves_the_new_values():
    N = _net()
    net = randomised(N.DenseResNet(4, [64, 64], spec=(20, 3), role="host", seed=5), 6).cuda()
    x = dev(inputs(np.random.default_rng(31), 33, 60))
    assert served(net, x)
    plan = net.__dict__["_fused_plan"]
    with torch.no_grad():
        before = net(x)[0].clone()
    # an in-place optimiser step: the same addresses, new values, the same table
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    p, v = net(x)
    (p.square().mean() + v.mean()).backward()
    opt.step()
    assert served(net, x) and net.__dict__["_fused_plan"] is plan
    with torch.no_grad():
        assert not torch.equal(net(x)[0], before)
    # replaced tensors: .to() and back, a parameter assigned anew -- a new table
    moved = net.cpu().cuda()
    assert served(moved, x) and moved.__dict__["_fused_plan"] is not plan
    plan = net.__dict__["_fused_plan"]
    held = net.blocks[1].Dense_0.weight  # (alive here, as it is in the old table)
    net.blocks[1].Dense_0.weight = torch.nn.Parameter(held.detach() * 0.5)
    assert served(net, x) and net.__dict__["_fused_plan"] is not plan and held is not None
    net.blocks[0].GroupNorm_1.bias = torch.nn.Parameter(net.blocks[0].GroupNorm_1.bias.detach() + 0.25)
    assert served(net, x)
    # copies build their own tables
    clone = copy.deepcopy(net)
    assert "_fused_plan" not in clone.__dict__
    with torch.no_grad():
        for q in clone.parameters():
            q.mul_(1.5)
    assert served(clone, x) and served(net, x)
    with torch.no_grad():
        assert not torch.equal(clone(x)[0], net(x)[0])
    loaded = pickle.loads(pickle.dumps(net))
    assert "_fused_plan" not in loaded.__dict__ and served(loaded, x)
    with torch.no_grad():
        assert torch.equal(loaded(x)[0], net(x)[0])
    net.load_state_dict(clone.state_dict())
    with torch.no_grad():
        assert torch.equal(clone(x)[0], net(x)[0]) and torch.equal(clone(x)[1], net(x)[1])
    # flax parameters travel through the host and back
    other = N.DenseResNet(4, [64, 64], spec=(20, 3), role="host", seed=7).cuda().load_flax_params(net.flax_params())
    assert served(other, x)
    with torch.no_grad():
        assert torch.equal(other(x)[0], net(x)[0])


def test_a_forward_replays_from_a_graph():
    net = randomised(_net().DenseResNet(3, [128] * 3, spec=(20, 3), role="agent", seed=8), 9).cuda()
    x = dev(inputs(np.random.default_rng(32), 96, 63))
    static = x.clone()
    with torch.no_grad():
        eager = [t.clone() for t in net(x)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(static)
        assert net.fused_last_reason is None
        graph.replay()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        static.copy_(x.flip(0))
        graph.replay()
        assert torch.equal(out[0], eager[0].flip(0)) and torch.equal(out[1], eager[1].flip(0))


# ---- through HipTrainer -----------------------------------------------------------------------------------------------

def trainer_config(net_type, net_arch):
    from test_gpu_trainer import CONFIG
    return dict(CONFIG, net_type=net_type, host={"net_arch": list(net_arch)}, agent={"net_arch": list(net_arch)})


@pytest.mark.parametrize("net_type,net_arch", [("dense_resnet", [32, 32]), ("dense_resnet", [64, 64]), ("dense", [32, 32])])
def test_trainer_builds_its_networks_from_the_config(net_type, net_arch):
    from hironaka_amd.functional import rollout_sanity_tests
    from hironaka_amd.trainer_api import HipTrainer
    N = _net()
    t = HipTrainer(42, trainer_config(net_type, net_arch))
    block = N.DenseResidueBlock if net_type == "dense_resnet" else N.DenseBlock
    for role, (k, a) in {"host": (60, 4), "agent": (63, 3)}.items():
        net = t.built_nets[role]
        assert isinstance(net, N.DenseResNet) and all(type(b) is block for b in net.blocks)
        assert (net.input_dim, net.output_size, net.net_arch) == (k, a, net_arch) and net.Dense_0.weight.is_cuda
        assert t.models[role].module is net
    assert not torch.equal(t.built_nets["host"].Dense_1.weight, t.built_nets["agent"].Dense_1.weight)
    b, T, m, d = t.eval_batch_size, t.max_length_game, t.max_num_points, t.dimension
    for role in ("host", "agent"):
        obs, policy, value = exp = t.simulate(7, role)
        assert obs.shape == (b * T, t.input_dim[role]) and policy.shape == (b * T, t.output_dim[role]) and value.shape == (b * T,)
        assert rollout_sanity_tests(exp, (m, d))
        assert torch.isfinite(value).all() and bool((value.abs() <= 1.0 + 1e-6).all())
        assert not obs.requires_grad and not policy.requires_grad
    assert t.built_nets["host"].fused_last_reason is None and t.built_nets["agent"].fused_last_reason is None


def test_trainer_keeps_what_it_is_given_and_refuses_custom():
    from hironaka_amd.trainer_api import HipTrainer, standin_mlp
    for net_type in ("custom", "custom_dense"):
        with pytest.raises(ValueError, match="CustomNet"):
            HipTrainer(42, trainer_config(net_type, [32, 32]))
    with pytest.raises(ValueError, match="net_type"):
        HipTrainer(42, trainer_config("transformer", [32, 32]))
    # a net that is given stays the caller's, called as it is; the other one is built
    host_net, host_params = standin_mlp(60, 4, 3, width=64)
    t = HipTrainer(42, trainer_config("dense_resnet", [32, 32]), host_net=host_net, host_params=host_params)
    assert t.models["host"] is host_net and list(t.built_nets) == ["agent"]
    cfg = trainer_config("dense_resnet", [32, 32])
    del cfg["agent"]
    with pytest.raises(ValueError, match="host_net and agent_net"):
        HipTrainer(42, cfg)
