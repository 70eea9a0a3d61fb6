"""hk_dqn_td / hk_polyak_update and hironaka_amd.dqn on the device against tests/dqn_rules.py (which test_dqn_rules.py
pins to the reference's own DQNTrainer) and against tests/golden/dqn_fit.npz.

R is the number of batch rows one workgroup owns: the batches below are the smallest that put a launch below, at and
beyond one tile, with a ragged last tile; the action counts cover one lane per row up to several columns per lane (a row
is served by the power of two >= A lanes, at most 64).  Target, row_loss, dq and status are compared bit for bit (NaNs
have to sit in the same places: a NaN's payload is no rule); the loss within B eps64 + eps_T relative of the rules' double
sum (a double sum of non-negative terms in any order, then one rounding to T)."""
import os
import warnings

import numpy as np
import pytest
import torch

import dqn_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A

pytestmark = pytest.mark.gpu
same_bits = R.same_bits

TILE = A.HK_DQN_TILE_ROWS
BATCHES = [1, 5, TILE - 1, TILE, TILE + 1, 3 * TILE + 1]
ACTIONS = [1, 2, 7, 11, 26, 57, 63, 64, 65, 120, 300]
DTYPES = [np.float32, np.float64]
EPS64 = np.finfo(np.float64).eps
SENTINEL = -77.25


def _ops():
    from hironaka_amd import ops
    return ops


def _batch(rng, B, A_, dtype):
    """Q-values spread so that the TD errors lie on both sides of 1; the action at 0 and at A - 1 among the rows"""
    q = (2.0 * rng.standard_normal((B, A_))).astype(dtype)
    next_q = (2.0 * rng.standard_normal((B, A_))).astype(dtype)
    actions = rng.integers(0, A_, B).astype(np.int32)
    actions[0], actions[-1] = 0, A_ - 1
    rewards = rng.integers(-1, 2, B).astype(np.float32)
    dones = rng.integers(0, 2, B).astype(bool)
    if B > 1:  # at gamma 0.99: a small error in the first row, a large one in the last
        target = R.td_target(next_q, rewards, dones, 0.99)
        q[0, 0], q[-1, -1] = target[0] + dtype(0.25), target[-1] - dtype(5)
    return q, next_q, actions, rewards, dones


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _want(q, next_q, actions, rewards, dones, gamma):
    target = R.td_target(next_q, rewards, dones, gamma)
    return (target, R.td_loss_rows(q, target, actions), R.td_grad(q, target, actions), R.td_loss(q, target, actions),
            R.td_status(actions, q.shape[1]))


def _loss_ok(got, want, B, dtype):
    got, want = float(got), float(want)
    if np.isnan(want):
        return np.isnan(got)
    return abs(got - want) <= (B * EPS64 + np.finfo(dtype).eps) * abs(want)


def _check(res, want, B, dtype, where):
    target, rows, grad, loss, status = want
    assert same_bits(res.target.cpu().numpy(), target), where
    assert same_bits(res.row_loss.cpu().numpy(), rows), where
    assert same_bits(res.dq.cpu().numpy(), grad), where
    assert int(res.status.item()) == status, where
    assert res.loss.dtype == res.dq.dtype and res.loss.shape == () and _loss_ok(res.loss.item(), loss, B, dtype), \
        (where, res.loss.item(), loss)


@pytest.mark.parametrize("dtype", DTYPES)
def test_td_matches_rules(dtype):
    ops = _ops()
    rng = np.random.default_rng(5)
    for B in BATCHES:
        for A_ in ACTIONS:
            case = _batch(rng, B, A_, dtype)
            dev = _cuda(*case)
            res = ops.dqn_td(*dev, 0.99)
            _check(res, _want(*case, 0.99), B, dtype, (B, A_))
            again = ops.dqn_td(*dev, 0.99)
            assert res.loss.cpu().numpy().tobytes() == again.loss.cpu().numpy().tobytes(), (B, A_)
            x, _ = R.td_error(case[0], R.td_target(case[1], case[3], case[4], 0.99), case[2])
            if B > 1:
                assert np.abs(x).min() < 1 < np.abs(x).max()  # both branches of the loss


@pytest.mark.parametrize("dtype", DTYPES)
def test_td_nonfinite_rows(dtype):
    """a NaN in a row, an all-NaN row, +inf, all -inf, a done row whose max is inf (0 * inf: NaN), a lone finite value"""
    ops = _ops()
    inf, nan = np.inf, np.nan
    rng = np.random.default_rng(6)
    B, A_ = 70, 7
    q, next_q, actions, rewards, dones = _batch(rng, B, A_, dtype)
    next_q[0, 3] = nan
    next_q[1, :] = nan
    next_q[2, 6] = inf
    next_q[3, :] = -inf
    next_q[4, 0], dones[4] = inf, True
    next_q[5, :], dones[5] = -inf, True
    next_q[6, :] = -inf
    next_q[6, 5] = 0.5
    next_q[7, 0], next_q[7, 1] = nan, inf
    dones[[0, 1, 2, 3, 6, 7]] = [False, True, False, False, False, False]
    for rows in (slice(None), slice(8, None)):  # with the rows whose loss is NaN, and without: a finite loss
        case = tuple(a[rows].copy() for a in (q, next_q, actions, rewards, dones))
        res = ops.dqn_td(*_cuda(*case), 0.9)
        want = _want(*case, 0.9)
        _check(res, want, case[0].shape[0], dtype, rows)
        assert np.isnan(want[3]) == (rows == slice(None))
    target = R.td_target(next_q, rewards, dones, 0.9)
    assert np.isnan(target[[0, 1, 4, 5, 7]]).all() and target[2] == inf and target[3] == -inf and np.isfinite(target[6])


def _padded(a, stride, offset):
    """`a` [B, A] as a view into a sentinel-filled block: rows `stride` elements apart, `offset` elements in"""
    B, A_ = a.shape
    flat = torch.full((offset + B * stride,), SENTINEL, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = flat[offset:].reshape(B, stride)[:, :A_]
    view.copy_(torch.from_numpy(a).cuda())
    return flat, view


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("A_,strides,offsets", [(7, (9, 8, 12), (1, 0, 3)), (64, (65, 64, 67), (0, 1, 2)),
                                                (1, (2, 3, 1), (1, 1, 1))])
def test_td_strided_rows_and_null_outputs(dtype, A_, strides, offsets):
    """q, next_q and dq as slices of wider records that start off the allocation's alignment: what lies between the
    rows of dq survives; without target and row_loss the rest is the same"""
    ops = _ops()
    B = TILE + 5
    rng = np.random.default_rng(A_)
    case = _batch(rng, B, A_, dtype)
    want = _want(*case, 0.99)
    (_, q), (_, next_q) = _padded(case[0], strides[0], offsets[0]), _padded(case[1], strides[1], offsets[1])
    flat, dq = _padded(np.zeros_like(case[0]), strides[2], offsets[2])
    dq.fill_(SENTINEL)
    assert q.stride(0) == strides[0] and dq.data_ptr() % 16 == (offsets[2] * dq.element_size()) % 16
    rest = _cuda(*case[2:])
    res = ops.dqn_td(q, next_q, *rest, 0.99, out={"dq": dq})
    assert res.dq is dq
    _check(res, want, B, dtype, "strided")
    expect = np.full(flat.shape[0], SENTINEL, dtype=dtype)
    expect[offsets[2]:].reshape(B, strides[2])[:, :A_] = want[2]
    assert same_bits(flat.cpu().numpy(), expect)
    bare = ops.dqn_td(q, next_q, *rest, 0.99, want=())
    assert bare.target is None and bare.row_loss is None
    assert same_bits(bare.dq.cpu().numpy(), want[2]) and bare.loss.item() == res.loss.item()


@pytest.mark.parametrize("dtype", DTYPES)
def test_td_bad_actions(dtype):
    ops = _ops()
    B, A_ = TILE + 9, 11
    rng = np.random.default_rng(9)
    case = list(_batch(rng, B, A_, dtype))
    case[2][[3, TILE + 2]] = [-1, A_]
    case[2][[4, 5]] = [-(2 ** 31), 2 ** 31 - 1]
    want = _want(*case, 0.99)
    assert want[4] == A.HK_DQN_BAD_ACTION and not want[2][[3, 4, 5, TILE + 2]].any() and want[1][3] == 0
    q, next_q = _cuda(case[0], case[1])
    flat, dq = _padded(np.zeros_like(case[0]), A_ + 2, 1)
    dq.fill_(SENTINEL)
    res = ops.dqn_td(q, next_q, *_cuda(*case[2:]), 0.99, out={"dq": dq})
    _check(res, want, B, dtype, "bad actions")
    expect = np.full(flat.shape[0], SENTINEL, dtype=dtype)
    expect[1:].reshape(B, A_ + 2)[:, :A_] = want[2]
    assert same_bits(flat.cpu().numpy(), expect)  # nothing was written beside the rows
    from hironaka_amd import dqn
    with pytest.raises(IndexError):
        dqn.td_loss(q, next_q, *_cuda(*case[2:]), 0.99, check=True)
    case[2][[3, 4, 5, TILE + 2]] = 0
    assert int(ops.dqn_td(q, next_q, *_cuda(*case[2:]), 0.99).status.item()) == 0
    dqn.td_loss(q, next_q, *_cuda(*case[2:]), 0.99, check=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_td_many_workgroups_share_a_workspace(dtype):
    """41 workgroups hand their partial sums to the one that draws the last ticket; three launches of different inputs
    into the same workspace: a ticket that is not zeroed again, or a partial read stale, shows in the loss"""
    ops = _ops()
    B, A_ = 40 * TILE + 3, 3
    rng = np.random.default_rng(12)
    workspace = ops.dqn_td_workspace(B, "cuda")
    assert workspace.numel() == 16 + 41 * 8
    cases = [_batch(rng, B, A_, dtype) for _ in range(3)]
    cases[1][0][:] *= 40.0  # other partial sums in every slot than the launch before left there
    results = [ops.dqn_td(*_cuda(*case), 0.99, workspace=workspace, want=()) for case in cases]
    again = ops.dqn_td(*_cuda(*cases[0]), 0.99, workspace=workspace, want=())
    for case, res in zip(cases, results):
        target = R.td_target(case[1], case[3], case[4], 0.99)
        want = R.td_loss(case[0], target, case[2])
        assert _loss_ok(res.loss.item(), want, B, dtype), (res.loss.item(), want)
        assert same_bits(res.dq.cpu().numpy(), R.td_grad(case[0], target, case[2]))
    assert results[0].loss.item() == again.loss.item() != results[1].loss.item()
    assert int(workspace[:8].view(torch.int64).item()) == 0  # the ticket is zero between launches


@pytest.mark.parametrize("dtype", DTYPES)
def test_td_loss_autograd(dtype):
    from hironaka_amd import dqn
    B, A_ = 37, 11
    rng = np.random.default_rng(14)
    case = _batch(rng, B, A_, dtype)
    target = R.td_target(case[1], case[3], case[4], 0.99)
    grad = R.td_grad(case[0], target, case[2])
    q, next_q, actions, rewards, dones = _cuda(*case)
    columns = (actions.reshape(-1, 1), rewards.reshape(-1, 1), dones.reshape(-1, 1))  # as ReplayBuffer.sample returns
    leaf = q.clone().requires_grad_(True)
    loss = dqn.td_loss(leaf, next_q, *columns, 0.99)
    assert loss.shape == () and loss.requires_grad
    assert _loss_ok(loss.item(), R.td_loss(case[0], target, case[2]), B, dtype)
    loss.backward()
    assert same_bits(leaf.grad.cpu().numpy(), grad)
    leaf.grad = None
    (3 * dqn.td_loss(leaf, next_q, actions, rewards, dones, 0.99)).backward()
    assert same_bits(leaf.grad.cpu().numpy(), (grad * dtype(3)).astype(dtype))
    with pytest.raises(ValueError):
        dqn.td_loss(leaf, next_q.clone().requires_grad_(True), actions, rewards, dones, 0.99)
    assert same_bits(dqn.td_target(next_q, *columns[1:], 0.99).cpu().numpy(), target)
    import hironaka_amd
    assert hironaka_amd.td_loss is dqn.td_loss and hironaka_amd.fit_network is dqn.fit_network
    with pytest.raises(TypeError):
        dqn.td_loss(leaf.detach().cpu(), next_q.cpu(), actions.cpu(), rewards.cpu(), dones.cpu(), 0.99)


# ---- the fixture: the reference's own fit step --------------------------------------------------------------------

@pytest.fixture(scope="module")
def fit():
    return np.load(os.path.join(GOLDEN, "dqn_fit.npz"))


class _StubBuffer:
    def __init__(self, fit, k):
        self.batch = tuple(torch.from_numpy(fit[f"c{k}_{name}"]).cuda()
                           for name in ("obs", "actions", "rewards", "dones", "next_obs"))

    def sample(self, batch_size, device=None, clone=True):
        assert batch_size == self.batch[1].shape[0]
        return self.batch


def _net(fit, k, tag):
    dtype = torch.float64 if fit["case_f64"][k] else torch.float32
    net = R.build_net(R.NET_KINDS[int(fit["case_net"][k])], int(fit["case_A"][k]), dtype)
    with torch.no_grad():
        for name, t in R.net_state(net).items():
            t.copy_(torch.from_numpy(fit[f"c{k}_{tag}_{name}"]))
    return net.cuda()


def _torch_fit(q_net, q_net_target, optimizer, replay_buffer, batch_size, gamma, max_grad_norm):
    """the reference's formulation (dqn_trainer.py:62-98) in torch on the device: the yardstick of the end-to-end check"""
    observations, actions, rewards, dones, next_observations = replay_buffer.sample(batch_size)
    with torch.no_grad():
        next_q_values, _ = q_net_target(next_observations).max(dim=1)
        target_q_values = rewards + (~dones) * gamma * next_q_values.reshape(-1, 1)
    current_q_values = torch.gather(q_net(observations), dim=1, index=actions.long())
    loss = torch.nn.functional.smooth_l1_loss(current_q_values, target_q_values)
    optimizer.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(q_net.parameters(), max_grad_norm)
    optimizer.step()
    return loss


def _distance(net, fit, k, tag):
    """the largest |parameter - recorded| over a tensor's largest recorded magnitude, in units of eps_T"""
    worst = 0.0
    for name, t in R.net_state(net).items():
        want = fit[f"c{k}_{tag}_{name}"]
        scale = max(float(np.abs(want).max()), np.finfo(want.dtype).tiny)
        worst = max(worst, float(np.abs(t.detach().cpu().numpy() - want).max()) / scale / float(np.finfo(want.dtype).eps))
    return worst


def fit_distances(fit):
    """per case: how far the parameters after one step lie from the recorded ones, (torch formulation, fit_network)"""
    from hironaka_amd import dqn
    out = []
    for k in range(len(fit["case_B"])):
        pair = []
        for step in (_torch_fit, dqn.fit_network):
            q_net, target = _net(fit, k, "q0"), _net(fit, k, "t0")
            optimizer = torch.optim.SGD(q_net.parameters(), lr=float(fit["lr"]))
            loss = step(q_net, target, optimizer, _StubBuffer(fit, k), int(fit["case_B"][k]),
                        float(fit["case_gamma"][k]), float(fit["case_max_grad_norm"][k]))
            assert loss.shape == ()
            pair.append(max(_distance(q_net, fit, k, "q1"), _distance(target, fit, k, "t1")))
        out.append(tuple(pair))
    return out


def test_fixture_kernel_on_recorded_q_values(fit):
    """the recorded next_q / current_q straight into hk_dqn_td: the reference's target bit for bit, its gradient with
    respect to current_q within 2 eps_T (either side rounds at most twice after x), the loss within B eps_T"""
    ops = _ops()
    for k in range(len(fit["case_B"])):
        q, next_q = fit[f"c{k}_current_q"], fit[f"c{k}_next_q"]
        eps, B = np.finfo(q.dtype).eps, q.shape[0]
        res = ops.dqn_td(*_cuda(q, next_q, fit[f"c{k}_actions"], fit[f"c{k}_rewards"], fit[f"c{k}_dones"]),
                         float(fit["case_gamma"][k]))
        assert same_bits(res.target.cpu().numpy(), fit[f"c{k}_target"]), k
        got, want = res.dq.cpu().numpy().astype(np.float64), fit[f"c{k}_dq"].astype(np.float64)
        assert ((got == 0) == (want == 0)).all(), k
        nz = want != 0
        assert (np.abs(got[nz] - want[nz]) <= 2 * eps * np.abs(want[nz])).all(), k
        ref = float(fit[f"c{k}_loss"])
        assert abs(res.loss.item() - ref) <= B * eps * abs(ref), k
        assert int(res.status.item()) == 0


def test_fixture_fit_network_end_to_end(fit):
    """every case through fit_network on the device, from the recorded parameters and batch.  The matmuls are not ours
    and differ between CPU and GPU, so the bound is measured: twice the largest distance that the reference's own
    formulation, run in torch on this device, shows from the fixture over all cases"""
    distances = fit_distances(fit)
    yardstick = max(t for t, _ in distances)
    ours = max(o for _, o in distances)
    print(f"parameters after one step, distance from the fixture in eps_T: torch on device {yardstick:.3f}, "
          f"fit_network {ours:.3f}; per case {distances}")
    assert ours <= 2 * yardstick, distances


# ---- hk_polyak_update ------------------------------------------------------------------------------------------------

def _polyak_pairs(rng, sizes, dtype, offsets=(0, 1)):
    """(src, dst) views of `sizes` elements at every offset of `offsets` into sentinel-padded storages, and the
    storages"""
    pairs, stores = [], []
    for k, n in enumerate(sizes):
        for off in offsets:
            so = off if k % 2 == 0 else 1 - off if len(offsets) == 2 else off  # src and dst agree or disagree
            src_store = torch.full((n + 3,), SENTINEL, dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device="cuda")
            dst_store = torch.full((n + 3,), SENTINEL, dtype=src_store.dtype, device="cuda")
            src, dst = src_store[so:so + n], dst_store[off:off + n]
            src.copy_(torch.from_numpy(rng.standard_normal(n).astype(dtype)))
            dst.copy_(torch.from_numpy(rng.standard_normal(n).astype(dtype)))
            pairs.append((src, dst))
            stores.append((src_store, dst_store, so, off))
    return pairs, stores


def _polyak_check(pairs, stores, tau, dtype, where):
    ops = _ops()
    want = [R.polyak(s.cpu().numpy(), d.cpu().numpy(), tau) for s, d in pairs]
    before = [s.cpu().numpy().copy() for s, _ in pairs]
    ops.polyak_update([s for s, _ in pairs], [d for _, d in pairs], tau)
    for k, ((src, dst), (src_store, dst_store, so, off), w) in enumerate(zip(pairs, stores, want)):
        n = src.numel()
        expect = np.full(n + 3, SENTINEL, dtype=dtype)
        expect[off:off + n] = w
        assert same_bits(dst_store.cpu().numpy(), expect), (where, k, n)  # the sentinel on both sides survives
        expect[:] = SENTINEL
        expect[so:so + n] = before[k]
        assert same_bits(src_store.cpu().numpy(), expect), (where, k, n)
        if tau == 1.0:
            assert torch.equal(dst, src)


CHUNK = A.HK_POLYAK_CHUNK_BYTES // 16  # 16-byte transfers per workgroup


@pytest.mark.parametrize("tau", R.TAUS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_polyak_sizes_and_offsets(dtype, tau):
    """every size at element offsets 0 and 1 of a larger storage, src and dst at the same offset (16-byte transfers
    with single elements in front and behind) and at different ones (element by element); 4 * 256 * 4 + 1 float32
    elements are one chunk of 16-byte transfers and one element more"""
    rng = np.random.default_rng(21)
    sizes = [0, 1, 3, 4, 5, 255, 1025, 4 * CHUNK + 1]
    pairs, stores = _polyak_pairs(rng, sizes, dtype)
    pairs2, stores2 = _polyak_pairs(rng, sizes[::-1], dtype)  # the other pairing of agreeing and disagreeing offsets
    _polyak_check(pairs + pairs2, stores + stores2, tau, dtype, "sizes")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [1, 2, 64, 65, 130])
def test_polyak_many_tensors(count, dtype):
    """lists up to and beyond HK_POLYAK_MAX_TENSORS tensors of mixed sizes, empty ones among them, in one call"""
    rng = np.random.default_rng(count)
    sizes = [(7 * k * k + 3 * k) % 41 if k % 9 else (CHUNK * 4 + 5 if k == 9 else 0) for k in range(1, count + 1)]
    pairs, stores = _polyak_pairs(rng, sizes, dtype, offsets=(1,))
    assert len(pairs) == count
    _polyak_check(pairs, stores, 0.3 if count % 2 else 0.005, dtype, count)


def test_polyak_refuses_what_it_cannot_serve():
    ops = _ops()
    from hironaka_amd import dqn
    a, b = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(TypeError):
        ops.polyak_update([a.cpu()], [b], 0.5)
    with pytest.raises(TypeError):
        ops.polyak_update([a], [b.double()], 0.5)
    with pytest.raises(TypeError):
        ops.polyak_update([a[::2]], [b[::2]], 0.5)
    with pytest.raises(TypeError):
        ops.polyak_update([a.half()], [b.half()], 0.5)
    with pytest.raises(ValueError):
        ops.polyak_update([a], [b[:4]], 0.5)
    from hironaka_amd._lib import HironakaHipError
    with pytest.raises(HironakaHipError):
        ops.polyak_update([a], [a], 0.5)  # src == dst: refused on the host
    with pytest.raises(HironakaHipError):
        ops.polyak_update([a[:6]], [a[2:]], 0.5)
    with pytest.raises(ValueError):
        dqn.polyak_update([a, a], [b], 0.5)
    with pytest.raises(ValueError):
        list(dqn.zip_equal([1, 2], [1]))
    assert list(dqn.zip_equal([1, 2], [3, 4])) == [(1, 3), (2, 4)]
    ops.polyak_update([], [], 0.5)
    assert not a.any() and not b.any()


def test_fixture_update_target_net(fit):
    """the recorded nets after the step through update_target_net: the reference's target parameters and BatchNorm
    statistics, bit for bit, at every tau"""
    from hironaka_amd import dqn
    seen_buffers = False
    for k in range(len(fit["case_B"])):
        q_net = _net(fit, k, "q1")
        for j, tau in enumerate(R.TAUS):
            target = _net(fit, k, "t1")
            dqn.update_target_net(q_net, target, tau)
            for name, t in R.net_state(target).items():
                assert same_bits(t.detach().cpu().numpy(), fit[f"c{k}_tau{j}_{name}"]), (k, tau, name)
                seen_buffers |= "running_var" in name
            if tau == 1.0:
                for (name, t), s in zip(R.net_state(target).items(), R.net_state(q_net).values()):
                    assert torch.equal(t, s), (k, name)
        for name, t in R.net_state(q_net).items():
            assert same_bits(t.detach().cpu().numpy(), fit[f"c{k}_q1_{name}"])  # the source is left alone
    assert seen_buffers


# ---- no synchronisation, graph capture ---------------------------------------------------------------------------------

def test_fit_step_does_not_synchronise():
    from hironaka_amd import dqn
    rng = np.random.default_rng(30)
    q, next_q, actions, rewards, dones = _cuda(*_batch(rng, TILE + 3, 11, np.float32))
    leaf = q.requires_grad_(True)
    srcs = [torch.randn(n, device="cuda") for n in (5, 1025, 64)]
    dsts = [torch.randn(n, device="cuda") for n in (5, 1025, 64)]
    dqn.td_loss(leaf, next_q, actions, rewards, dones, 0.99).backward()  # the stream's workspace exists now
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "a prototype feature"
        torch.cuda.set_sync_debug_mode("error")  # a synchronising torch call raises
        try:
            dqn.td_loss(leaf, next_q, actions, rewards, dones, 0.99).backward()
            dqn.polyak_update(srcs, dsts, 0.005)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert leaf.grad is not None


def test_sample_td_and_polyak_replay_from_a_graph():
    """replay_sample -> dqn_td -> polyak_update on one stream, captured: three replays == three eager calls (the cursor,
    the ticket and the target parameters are device state that every replay moves on)"""
    ops = _ops()
    capacity, n, A_ = 3 * TILE, TILE + 40, 7
    rng = np.random.default_rng(31)
    q, next_q, actions, rewards, dones = _cuda(*_batch(rng, capacity, A_, np.float32))
    rings = [q, next_q, actions.reshape(-1, 1), rewards.reshape(-1, 1), dones.reshape(-1, 1)]
    src = [torch.randn(k, device="cuda") for k in (300, 5)]
    start = [torch.randn(k, device="cuda") for k in (300, 5)]

    def fresh():
        cursor = ops.replay_cursor("cuda")
        cursor[A.HK_REPLAY_FULL] = 1
        return cursor, [t.clone() for t in start], [torch.zeros((n,) + tuple(r.shape[1:]), dtype=r.dtype,
                                                                  device="cuda") for r in rings]

    def step(cursor, dst, out, workspace):
        cols, _ = ops.replay_sample(rings, cursor, n, seed=4, out=out)
        res = ops.dqn_td(*cols, 0.99, workspace=workspace)
        ops.polyak_update(src, dst, 0.3)
        return res

    cursor, dst, out = fresh()
    workspace = ops.dqn_td_workspace(n, "cuda")
    eager = []
    for _ in range(3):
        res = step(cursor, dst, out, workspace)
        eager.append((res.loss.clone(), res.dq.clone(), res.target.clone(), [t.clone() for t in dst]))
    assert eager[0][0].item() != eager[1][0].item()
    cursor, dst, out = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step(cursor, dst, out, workspace)
    assert int(cursor[A.HK_REPLAY_SAMPLES_DRAWN]) == 0  # capturing runs nothing
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert res.loss.item() == eager[k][0].item(), k
        assert torch.equal(res.dq, eager[k][1]) and torch.equal(res.target, eager[k][2]), k
        for x, y in zip(dst, eager[k][3]):
            assert torch.equal(x, y), k
    assert int(res.status.item()) == 0 and int(cursor[A.HK_REPLAY_SAMPLES_DRAWN]) == 3
