"""hk_pv_loss and hironaka_amd.loss on the device against tests/pv_loss_rules.py (which test_pv_loss_rules.py pins to
torch's float64 operators and autograd).

TILE is the number of batch rows one workgroup owns: the batches below put a launch below, at and beyond one tile, with a
ragged last tile and a third workgroup; the action counts cover one lane per row up to four columns per lane (a row is
served by the power of two >= A lanes, at most 64).  The kernel evaluates a row in double and rounds every stored float32
once: loss, row_loss and dvalue lie within one float32 ulp of the rule's float64 value (the double arithmetic is good to
a few 2^-52, so the rounding can differ from the correctly rounded value at near-ties only), dlogits within one ulp plus
2^-40 * w / (A * B) absolute for the cancellation in p - q at double precision."""
import copy

import numpy as np
import pytest
import torch

import pv_loss_rules as R
from hironaka_amd import _abi as A

pytestmark = pytest.mark.gpu

TILE = A.HK_PVLOSS_TILE_ROWS
BATCHES = [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]
ACTIONS = [1, 3, 4, 26, 120, 255]
SENTINEL = -77.25
UNIT = 2.0 ** -24


def _ops():
    from hironaka_amd import ops
    return ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(a, stride, offset):
    """`a` [rows, A] as a view into a sentinel-filled block: rows `stride` elements apart, `offset` elements in"""
    rows, width = a.shape
    flat = torch.full((offset + rows * stride,), SENTINEL, dtype=torch.float32, device="cuda")
    view = flat[offset:].reshape(rows, stride)[:, :width]
    view.copy_(torch.from_numpy(a).cuda())
    return flat, view


def _weights(case):
    logits, _, _, _, w, idx = case
    B = logits.shape[0]
    r, _ = R.rows_of(idx, B, case[2].shape[0])
    return np.ones(B) if w is None else w.astype(np.float64)[r]


def _check(res, want, case, where, row_loss=True):
    B, A_ = case[0].shape
    w = np.abs(_weights(case))
    assert R.within(res.loss.cpu().numpy(), want.loss), (where, res.loss.item(), want.loss)
    assert R.within(res.dvalue.cpu().numpy().reshape(B), want.dvalue), where
    assert R.within(res.dlogits.cpu().numpy(), want.dlogits, extra=(2.0 ** -40 * w / (A_ * B))[:, None]), where
    if row_loss:
        assert R.within(res.row_loss.cpu().numpy(), want.row_loss), where
    else:
        assert res.row_loss is None
    assert int(res.status.item()) == want.status, where
    if case[4] is None:  # no weight: +-1 / B or 0, to the bit
        expect = (np.sign(want.dvalue) * (np.float32(1) / np.float32(B))).astype(np.float32)
        assert np.array_equal(res.dvalue.cpu().numpy().reshape(B), expect), where


@pytest.mark.parametrize("A_", ACTIONS)
def test_kernel_matches_rule(A_):
    """every batch at this action count, the combinations dealt round: weight and index each NULL and given, value as
    [B] and [B, 1], row_loss NULL and given, logits / dlogits contiguous and as columns of a wider record"""
    ops = _ops()
    rng = np.random.default_rng(100 + A_)
    for k, B in enumerate(BATCHES):
        for variant in (k, k + 3):
            weight, index = bool(variant & 1), bool(variant & 2)
            column, strided, row_loss = bool(variant & 4) != weight, variant % 3 == 0, variant % 2 == 0
            case = R.case(rng, B, A_, weight=weight, index=index)
            want = R.pv_loss(*case)
            logits, value, tp, tv, w, idx = (_dev(a) for a in case)
            out, flat = {}, None
            if strided:
                _, logits = _padded(case[0], A_ + 3, 1)
                flat, out["dlogits"] = _padded(np.zeros_like(case[0]), A_ + 2, 3)
                out["dlogits"].fill_(SENTINEL)
                _, tp = _padded(case[2], A_ + 1, 2)
            if column:
                value = value.reshape(B, 1)
            res = ops.pv_loss(logits, value, tp, tv, w, idx, out=out, want=("row_loss",) if row_loss else ())
            where = (B, A_, variant)
            assert res.dvalue.shape == value.shape and res.dlogits.shape == (B, A_) and res.loss.shape == ()
            _check(res, want, case, where, row_loss)
            if strided:  # what lies between the rows of dlogits survives
                assert res.dlogits is out["dlogits"]
                block = flat[3:].reshape(B, A_ + 2).cpu().numpy()
                assert (block[:, A_:] == SENTINEL).all() and (flat[:3].cpu().numpy() == SENTINEL).all(), where


def test_value_and_dvalue_as_columns_of_the_networks_record():
    """logits and value as the columns of one [B, A + 1] record, dlogits and dvalue likewise: element strides above 1"""
    ops = _ops()
    rng = np.random.default_rng(7)
    B, A_ = TILE + 2, 4
    case = R.case(rng, B, A_)
    want = R.pv_loss(*case)
    record = torch.full((B, A_ + 1), SENTINEL, device="cuda")
    record[:, :A_], record[:, A_] = _dev(case[0]), _dev(case[1])
    grad = torch.full((B, A_ + 2), SENTINEL, device="cuda")
    res = ops.pv_loss(record[:, :A_], record[:, A_:], *(_dev(a) for a in case[2:]),
                      out={"dlogits": grad[:, :A_], "dvalue": grad[:, A_:A_ + 1]})
    assert res.dvalue.shape == (B, 1) and res.dvalue.stride(0) == A_ + 2
    _check(res, want, case, "record")
    assert (grad[:, A_ + 1] == SENTINEL).all()


def test_same_bits_on_every_launch_and_from_a_larger_workspace():
    ops = _ops()
    rng = np.random.default_rng(8)
    for B, A_ in [(2 * TILE + 3, 26), (5 * TILE + 1, 4), (3, 255)]:
        case = R.case(rng, B, A_)
        dev = [_dev(a) for a in case]
        runs = [ops.pv_loss(*dev), ops.pv_loss(*dev),
                ops.pv_loss(*dev, workspace=ops.pv_loss_workspace(40 * TILE, "cuda"))]
        own = ops.pv_loss_workspace(B, "cuda")
        runs += [ops.pv_loss(*dev, workspace=own), ops.pv_loss(*dev, workspace=own)]  # the ticket is zero again
        assert not own.view(torch.int64)[0].item()
        first = [t.cpu().numpy().tobytes() for t in runs[0][:4]]
        for res in runs[1:]:
            assert [t.cpu().numpy().tobytes() for t in res[:4]] == first, (B, A_)
        _check(runs[0], R.pv_loss(*case), case, (B, A_))


def test_nan_stays_in_its_row():
    ops = _ops()
    rng = np.random.default_rng(9)
    B, A_ = TILE + 3, 26
    case = list(R.case(rng, B, A_))
    clean = R.pv_loss(*case)
    for where in ("logits", "target", "value"):
        dirty = [None if a is None else a.copy() for a in case]
        if where == "logits":
            dirty[0][5, 7] = np.nan
        elif where == "target":
            dirty[2][case[5][5], 3] = np.nan
            assert (case[5] == case[5][5]).sum() == 1  # the sample belongs to row 5 alone
        else:
            dirty[1][5] = np.nan
        want = R.pv_loss(*dirty)
        res = ops.pv_loss(*(_dev(a) for a in dirty))
        assert np.isnan(want.loss) and np.isnan(res.loss.item()) and np.isnan(res.row_loss[5].item()), where
        _check(res, want, dirty, where)
        keep = np.arange(B) != 5
        assert np.array_equal(want.dlogits[keep], clean.dlogits[keep])
        assert np.isfinite(res.dlogits.cpu().numpy()[keep]).all() and np.isfinite(res.dvalue.cpu().numpy()[keep]).all()


@pytest.mark.parametrize("bad", [-1, "N", 2 ** 40, -2 ** 62])
def test_bad_index_zeroes_its_row_and_writes_nothing_else(bad):
    """every output in a guard band of its own inside one sentinel block: the status bit, a zero row, nothing outside"""
    ops = _ops()
    rng = np.random.default_rng(10)
    B, A_, row = TILE + 2, 3, TILE
    case = list(R.case(rng, B, A_, hard=False))
    N = case[2].shape[0]
    good = R.pv_loss(*case)
    case[5] = case[5].copy()
    case[5][row] = N if bad == "N" else bad
    want = R.pv_loss(*case)
    assert want.status == R.BAD_INDEX and not want.dlogits[row].any() and np.array_equal(want.dlogits[:row], good.dlogits[:row])
    G = 64  # floats of guard on either side
    block = torch.full((4 * G + B * (A_ + 1) + B + B + 1 + G,), SENTINEL, device="cuda")
    at = G
    dlogits = block[at:at + B * (A_ + 1)].reshape(B, A_ + 1)[:, :A_]
    at += B * (A_ + 1) + G
    dvalue = block[at:at + B]
    at += B + G
    row_loss = block[at:at + B]
    at += B + G
    loss = block[at:at + 1].reshape(())
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    inputs = [_dev(a) for a in case]
    before = [t.clone() for t in inputs]
    res = ops.pv_loss(*inputs, out={"dlogits": dlogits, "dvalue": dvalue, "row_loss": row_loss, "loss": loss,
                                    "status": status})
    assert int(status.item()) == A.HK_PVLOSS_BAD_INDEX
    _check(res, want, case, bad)
    got = res.dlogits.cpu().numpy()
    assert not got[row].any() and res.dvalue[row].item() == 0 and res.row_loss[row].item() == 0
    assert got[np.arange(B) != row].all()  # exactly that row
    written = torch.zeros_like(block, dtype=torch.bool)
    for t in (dlogits, dvalue, row_loss, loss):
        written.view(torch.uint8).as_strided(t.shape, t.stride(), t.storage_offset()).fill_(1)
    assert written.sum().item() == B * A_ + 2 * B + 1
    assert (block[~written] == SENTINEL).all() and not (block[written] == SENTINEL).any()
    assert all(torch.equal(a, b) for a, b in zip(inputs, before))


def test_python_boundary_refusals():
    ops = _ops()
    from hironaka_amd._lib import HironakaHipError
    rng = np.random.default_rng(3)
    case = R.case(rng, 4, 3)
    logits, value, tp, tv, w, idx = (_dev(a) for a in case)
    with pytest.raises(TypeError):
        ops.pv_loss(logits.cpu(), value, tp, tv, w, idx)
    with pytest.raises(TypeError):
        ops.pv_loss(logits.double(), value, tp, tv, w, idx)
    with pytest.raises(TypeError):
        ops.pv_loss(logits, value, tp, tv, w, idx.int())
    with pytest.raises(TypeError):
        ops.pv_loss(logits, value[:3], tp, tv, w, idx)
    with pytest.raises(ValueError):
        ops.pv_loss(logits, value, tp[:, :2], tv, w, idx)
    with pytest.raises(ValueError):
        ops.pv_loss(logits, value, tp, tv, w, None)  # 9 samples, 4 rows, no index
    with pytest.raises(ValueError):
        ops.pv_loss(logits, value, tp, tv, w, idx, want=("target",))
    with pytest.raises(ValueError):
        ops.pv_loss(logits, value, tp, tv, w, idx, workspace=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(HironakaHipError):  # the gradient on top of the logits: refused on the host
        ops.pv_loss(logits, value, tp, tv, w, idx, out={"dlogits": logits})
    empty = ops.pv_loss(logits[:0], value[:0], tp, tv, w, idx[:0])
    assert empty.dlogits.shape == (0, 3) and np.isnan(empty.loss.item())


# ---- hironaka_amd.loss: the autograd function ---------------------------------------------------------------------------

def _units(g, g64, largest):
    """max |g - g64| in units of max |g64| * 2^-24 -- of the network's largest gradient where this tensor's own is zero in
    exact arithmetic and its float64 value is rounding noise (below 2^-24 of the largest): at a normed width of 32 a group
    is ONE column, the norm's output is its bias whatever comes in, and nothing in front of it has a gradient"""
    own = np.abs(g64).max()
    scale = (own if own > largest * UNIT else largest) * UNIT
    err = np.abs(g.astype(np.float64) - g64).max()
    return 0.0 if err == 0 else err / scale


NETS = [("dense_resnet_host", "DenseResNet", 60, 4), ("dense_resnet_agent", "DenseResNet", 63, 3),
        ("dense_host", "DenseNet", 60, 4), ("dense_agent", "DenseNet", 63, 3)]


@pytest.mark.parametrize("name,cls,in_dim,A_", NETS, ids=[n[0] for n in NETS])
def test_backward_through_a_network_lies_within_torchs_distance_of_float64(name, cls, in_dim, A_):
    """policy_value_loss(...).backward() through a [32] x 2 network at 32 rows (the test config: inputs 60 / 63, 4 / 3
    actions) against the same module through torch_policy_value_loss: E_fused <= 2 * max(E_torch, 1), E the largest over
    the parameters' gradients of max |g - g64| in units of max |g64| * 2^-24 against a float64 run of module and loss --
    the form and margin of test_pvnet_rules.py, one E per network (_units: a gradient that is zero in exact arithmetic in
    the units of the network's largest).  Both ways share the float32 forward and torch's backward through the network;
    they differ in the last bits of dlogits and dvalue alone.
    Recorded on an MI355X, E_torch / E_fused, and the worst E_fused : max(E_torch, 1) of a single tensor, which is NOT
    held to the factor 2 (errors of two to five units on either side: DenseResidueBlock_1.GroupNorm_1.bias of the host
    4.69 against 2.13, DenseResidueBlock_0.GroupNorm_1.weight of the agent 29.6 against 11.4):
        dense_resnet_host 2628.76 / 2628.76, 2.20    dense_resnet_agent 504.78 / 426.52, 2.59
        dense_host 3.54 / 3.54, 1.18                 dense_agent 3.98 / 3.13, 1.18
    """
    from hironaka_amd import loss as hkloss
    from hironaka_amd import net as hknet
    rng = np.random.default_rng(in_dim)
    module = getattr(hknet, cls)(A_, [32, 32], input_dim=in_dim, seed=5).cuda()
    with torch.no_grad():  # off the initial zeros and ones, so that every gradient is a sum of unlike terms
        for p in module.parameters():
            p.add_(0.1 * torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).cuda())
    B, N = 32, 40
    obs = _dev(rng.uniform(-1, 1, (B, in_dim)).astype(np.float32))
    _, _, tp, tv, w, idx = R.case(rng, B, A_, N=N)
    tp, tv, w, idx = (_dev(a) for a in (tp, tv, w, idx))

    def grads(mod, fn, dtype):
        mod.zero_grad()
        logits, value = mod(obs.to(dtype))
        loss = fn(logits, value, tp.to(dtype), tv.to(dtype), w.to(dtype), index=idx)
        loss.backward()
        return loss.item(), [p.grad.detach().cpu().numpy() for p in mod.parameters()]

    loss_fused, g_fused = grads(module, hkloss.policy_value_loss, torch.float32)
    assert module.fused_last_reason == "gradients are on"
    loss_torch, g_torch = grads(module, hkloss.torch_policy_value_loss, torch.float32)
    loss64, g64 = grads(copy.deepcopy(module).double(), hkloss.torch_policy_value_loss, torch.float64)
    assert abs(loss_fused - loss_torch) <= 32 * UNIT * abs(loss_torch)  # the same float32 outputs of the network go in
    assert abs(loss_fused - loss64) <= 1e-4 * abs(loss64)
    largest = max(np.abs(r).max() for r in g64)
    e_torch = [_units(g, r, largest) for g, r in zip(g_torch, g64)]
    e_fused = [_units(g, r, largest) for g, r in zip(g_fused, g64)]
    worst = max(f / max(t, 1) for f, t in zip(e_fused, e_torch))
    print(f"{name}: max E_torch {max(e_torch):.2f} max E_fused {max(e_fused):.2f} worst ratio {worst:.2f}")
    assert max(e_fused) <= 2 * max(max(e_torch), 1)


def test_autograd_function_scales_by_the_incoming_gradient_and_refuses_target_gradients():
    from hironaka_amd import loss as hkloss
    rng = np.random.default_rng(4)
    case = R.case(rng, 9, 4)
    want = R.pv_loss(*case)
    logits, value, tp, tv, w, idx = (_dev(a) for a in case)
    logits.requires_grad_()
    value = value.reshape(9, 1).requires_grad_()
    loss = hkloss.policy_value_loss(logits, value, tp, tv, w, index=idx, params=None)
    assert R.within(loss.detach().cpu().numpy(), want.loss)
    (3.0 * loss).backward()
    assert value.grad.shape == (9, 1)
    assert R.within(logits.grad.cpu().numpy() / 3, want.dlogits, extra=2.0 ** -30)
    assert R.within(value.grad.cpu().numpy().reshape(9) / 3, want.dvalue, extra=2.0 ** -30)
    with pytest.raises(ValueError):
        hkloss.policy_value_loss(logits, value, tp.clone().requires_grad_(), tv, w, index=idx)
    for wrong in (idx.cpu(), idx.int(), idx.tolist()):  # refused here, by name, not deep inside ops.pv_loss
        with pytest.raises(TypeError, match="index must be an int64 tensor"):
            hkloss.policy_value_loss(logits, value, tp, tv, w, index=wrong)
    # float64 on the device: the torch composition, differentiable in everything
    tp64 = tp.double().requires_grad_()
    hkloss.policy_value_loss(logits.detach().double(), value.detach().double(), tp64, tv.double(), w.double(),
                             index=idx).backward()
    assert tp64.grad is not None and torch.isfinite(tp64.grad).all()
