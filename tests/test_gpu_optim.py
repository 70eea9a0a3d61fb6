"""hk_optim_prepare / hk_optim_apply and hironaka_amd.optim on the device against tests/optim_rules.py (which
test_optim_rules.py pins to torch's own clip_grad_norm_, Adam and SGD) and against tests/golden/optim_step.npz.

PER is the number of elements of one 16 KiB chunk: the sizes below are the smallest that put a tensor below, at and
beyond one chunk and beyond two, with the single elements in front of and behind the 16-byte transfers.  Everything the
kernels write is compared with the rules bit for bit (NaNs have to sit in the same places): parameters, state, clipped
gradients, the state block's doubles.  Against torch: bits wherever the rules are torch's bits, and the fixture's
measured tolerance for Adam's parameters."""
import collections
import copy
import os
import re
import warnings

import numpy as np
import pytest
import torch

import dqn_rules as D
import optim_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A

pytestmark = pytest.mark.gpu
same_bits = R.same_bits

DTYPES = [np.float32, np.float64]
SENTINEL = -77.25
PAD = 8  # elements of sentinel around every view
KINDS = {"scale": R.SCALE, "sgd": R.SGD, "adam": R.ADAM}
FIELDS = ("p", "g", "m", "v")


def _ops():
    from hironaka_amd import ops
    return ops


def _per(dtype):
    return A.HK_OPTIM_CHUNK_BYTES // np.dtype(dtype).itemsize


def _sizes(dtype):
    per = _per(dtype)
    return [0, 1, 3, 4, 5, 1023, per, per + 1, 2 * per + 3]


def _tdtype(dtype):
    return torch.float32 if dtype == np.float32 else torch.float64


class Tensors:
    """n-element views p, g, m, v per size at element offsets into sentinel-padded storages: `together` puts the four of
    an entry at one odd offset (16-byte transfers with single elements in front and behind), otherwise at four different
    ones (element by element)"""

    def __init__(self, rng, sizes, dtype, together=True, scale=1.0):
        self.dtype, self.sizes = dtype, list(sizes)
        self.host, self.store, self.view, self.offset = [], [], [], []
        for k, n in enumerate(sizes):
            offs = {f: (1 + k % 3 if together else j + (k % 2)) for j, f in enumerate(FIELDS)}
            host = {"p": rng.standard_normal(n), "g": scale * rng.standard_normal(n), "m": 0.1 * rng.standard_normal(n),
                    "v": 0.01 * rng.random(n)}
            host = {f: x.astype(dtype) for f, x in host.items()}
            store = {f: torch.full((n + 2 * PAD,), SENTINEL, dtype=_tdtype(dtype), device="cuda") for f in FIELDS}
            view = {f: store[f][offs[f]:offs[f] + n] for f in FIELDS}
            for f in FIELDS:
                view[f].copy_(torch.from_numpy(host[f]))
            self.host.append(host), self.store.append(store), self.view.append(view), self.offset.append(offs)

    def column(self, f):
        return [v[f] for v in self.view]

    def chain(self, kind, state, uses_m=True, **kw):
        ops = _ops()
        cols = {"scale": (None, None, None), "sgd": (self.column("p"), self.column("m") if uses_m else None, None),
                "adam": (self.column("p"), self.column("m"), self.column("v"))}[kind]
        return ops.OptimChain(kind, self.column("g"), *cols, state=state, **kw)

    def check(self, where):
        """the storages hold what self.host holds, between untouched sentinels"""
        for k, n in enumerate(self.sizes):
            for f in FIELDS:
                expect = np.full(n + 2 * PAD, SENTINEL, dtype=self.dtype)
                off = self.offset[k][f]
                expect[off:off + n] = self.host[k][f]
                assert same_bits(self.store[k][f].cpu().numpy(), expect), (where, k, n, f)


def _rule_step(t, kind, st, hyper, max_norm, lr, keep=False):
    """one step of the rules over the host copies of `t`; returns the new state block"""
    b1, b2 = hyper.get("betas", (0.0, 0.0))
    st = R.prepare(st, [h["g"] for h in t.host], t.dtype, max_norm=max_norm, lr=lr, beta1=b1, beta2=b2,
                   advance=kind != "scale")
    for h in t.host:
        if kind == "scale":
            g = R.scale(h["g"], st["clip_coef"])
        elif kind == "sgd":
            mom = hyper.get("momentum", 0.0)
            h["p"], g, buf = R.sgd(h["p"], h["g"], h["m"] if mom else None, st,
                                   **{k: v for k, v in hyper.items() if k != "betas"})
            if mom:
                h["m"] = buf
        else:
            h["p"], g, h["m"], h["v"] = R.adam(h["p"], h["g"], h["m"], h["v"], st, beta1=b1, beta2=b2,
                                               eps=hyper.get("eps", 1e-8), weight_decay=hyper.get("weight_decay", 0.0))
        if not keep:
            h["g"] = g
    return st


def _device_step(chain, kind, hyper, max_norm, lr, keep=False):
    ops = _ops()
    b1, b2 = hyper.get("betas", (0.0, 0.0))
    ops.optim_prepare(chain, max_norm=max_norm, lr=lr, beta1=b1, beta2=b2, advance=kind != "scale")
    if kind == "scale":
        ops.optim_apply(chain)
    elif kind == "sgd":
        ops.optim_apply(chain, keep_grads=keep, **{k: v for k, v in hyper.items() if k != "betas"})
    else:
        ops.optim_apply(chain, keep_grads=keep, beta1=b1, beta2=b2, eps=hyper.get("eps", 1e-8),
                        weight_decay=hyper.get("weight_decay", 0.0))


def _same_state(block, st, where):
    got = _ops().optim_state_read(block)
    for name, want in st.items():
        assert same_bits(np.float64(got[name]), np.float64(want)), (where, name, got[name], want)


HYPER = {"scale": {}, "adam": dict(betas=(0.9, 0.999), weight_decay=0.01),
         "sgd": dict(momentum=0.9, weight_decay=0.01, nesterov=True)}


@pytest.mark.parametrize("together", [True, False])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_sizes_and_offsets(dtype, kind, together):
    """every size at odd element offsets, the arrays of an entry at one offset and at four; two steps, so that SGD's
    first-step rule and the running one are both met; clipping bites (the norm is in the hundreds)"""
    ops = _ops()
    t = Tensors(np.random.default_rng(41), _sizes(dtype), dtype, together)
    block = ops.optim_state("cuda")
    chain = t.chain(kind, block)
    assert chain.total_workgroups == R.workgroups(t.sizes, dtype) == 0 + 5 + 1 + 2 + 3
    st = R.new_state()
    for step in range(2):
        st = _rule_step(t, kind, st, HYPER[kind], 1.5, 0.05)
        _device_step(chain, kind, HYPER[kind], 1.5, 0.05)
        _same_state(block, st, step)
        t.check((kind, together, step))
    assert 0.0 < st["clip_coef"] < 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [1, 64, 65, 130])
def test_many_tensors(count, dtype):
    """lists up to and beyond HK_OPTIM_MAX_TENSORS: chains of one, two and three launches, empty tensors among them and
    a tensor of several chunks in the second table"""
    ops = _ops()
    per = _per(dtype)
    sizes = [(7 * k * k + 3 * k) % 41 if k % 9 else (2 * per + 5 if k == 72 else 0) for k in range(1, count + 1)]
    t = Tensors(np.random.default_rng(count), sizes, dtype)
    block = ops.optim_state("cuda")
    chain = t.chain("adam", block)
    assert len(chain.descs) == (count + 63) // 64
    st = _rule_step(t, "adam", R.new_state(), HYPER["adam"], 2.0, 0.01)
    _device_step(chain, "adam", HYPER["adam"], 2.0, 0.01)
    _same_state(block, st, count)
    t.check(count)


def test_a_chain_whose_last_table_is_empty():
    """65 tensors of which the last has no element: the last launch owns no chunk and still adds the slots"""
    ops = _ops()
    t = Tensors(np.random.default_rng(3), [5] * 64 + [0], np.float32)
    block = ops.optim_state("cuda")
    st = _rule_step(t, "scale", R.new_state(), {}, 1.0, 0.0)
    _device_step(t.chain("scale", block), "scale", {}, 1.0, 0.0)
    _same_state(block, st, "empty tail")
    t.check("empty tail")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_clipping_and_keep_grads(kind, dtype):
    """max_norm below the norm, above it and inf; the clipped gradient written back or not"""
    ops = _ops()
    seen = set()
    for max_norm in (0.25, 1e6, float("inf")):
        for keep in (False, True):
            t = Tensors(np.random.default_rng(7), [37, 1030, 4], dtype)
            before = [h["g"].copy() for h in t.host]
            block = ops.optim_state("cuda")
            st = _rule_step(t, kind, R.new_state(), HYPER[kind], max_norm, 0.05, keep)
            _device_step(t.chain(kind, block), kind, HYPER[kind], max_norm, 0.05, keep)
            _same_state(block, st, (max_norm, keep))
            t.check((max_norm, keep))
            seen.add(st["clip_coef"] < 1.0)
            changed = any(not same_bits(h["g"], b) for h, b in zip(t.host, before))
            assert changed == (not keep and max_norm == 0.25)
    assert seen == {True, False}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_gradient(bad, dtype):
    """a NaN or an inf among the gradients: the norm, the coefficient and every element are the rules'"""
    ops = _ops()
    for kind in ("scale", "adam", "sgd"):
        t = Tensors(np.random.default_rng(8), [9, 600], dtype)
        t.host[1]["g"][17] = bad
        t.view[1]["g"][17] = float(bad)
        block = ops.optim_state("cuda")
        st = _rule_step(t, kind, R.new_state(), HYPER[kind], 1.0, 0.05)
        _device_step(t.chain(kind, block), kind, HYPER[kind], 1.0, 0.05)
        _same_state(block, st, (kind, bad))
        t.check((kind, bad))
        assert not np.isfinite(st["total_norm"]) and (np.isnan(st["clip_coef"]) or st["clip_coef"] == 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_launches_give_the_same_bits(dtype):
    ops = _ops()
    results = []
    for _ in range(2):
        t = Tensors(np.random.default_rng(9), [3 * _per(dtype) + 11, 77] * 8, dtype)
        block = ops.optim_state("cuda")
        _device_step(t.chain("adam", block), "adam", HYPER["adam"], 1.0, 0.05)
        results.append((block.cpu().numpy().tobytes(), [s[f].cpu().numpy().tobytes() for s in t.store for f in FIELDS]))
    assert results[0] == results[1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_block_and_learning_rate_over_three_steps(dtype):
    """step, the running powers and the step's scalars after every step; lr from the host, then from the device, changed
    between the steps, through a workspace of the caller's own"""
    ops = _ops()
    t = Tensors(np.random.default_rng(10), [50, 1025], dtype)
    block = ops.optim_state("cuda")
    chain = t.chain("adam", block, workspace=ops.optim_workspace(R.workgroups(t.sizes, dtype), "cuda"))
    hyper = dict(betas=(0.4, 0.9))
    lr_dev = torch.tensor([0.0], dtype=torch.float64, device="cuda")
    st = R.new_state()
    for step, (lr, on_device) in enumerate([(0.05, False), (0.02, True), (0.007, True)]):
        st = _rule_step(t, "adam", st, hyper, 0.5, lr)
        lr_dev.fill_(lr)
        _device_step(chain, "adam", hyper, 0.5, lr_dev if on_device else lr)
        _same_state(block, st, step)
        t.check(step)
    assert st["step"] == 3 and st["beta1_pow"] == 0.4 * 0.4 * 0.4 and st["lr"] == 0.007
    lr32 = torch.tensor(0.25, dtype=torch.float32, device="cuda")  # any one-element tensor on the device serves
    st = _rule_step(t, "adam", st, hyper, 0.5, 0.25)
    _device_step(chain, "adam", hyper, 0.5, lr32)
    _same_state(block, st, "float32 lr")


@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_grad_norm(dtype):
    """optim.clip_grad_norm_ against the rule to the bit, and within a reasoned bound of torch's own on the device"""
    from hironaka_amd import optim
    rng = np.random.default_rng(11)
    sizes = [12, 0, 1025, _per(dtype) + 1]
    for max_norm in (0.5, 1e9):
        host = [rng.standard_normal(n).astype(dtype) for n in sizes]
        params = [torch.nn.Parameter(torch.zeros(n, dtype=_tdtype(dtype), device="cuda")) for n in sizes] + \
                 [torch.nn.Parameter(torch.zeros(3, dtype=_tdtype(dtype), device="cuda"))]  # one without a gradient
        theirs = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for p, q, h in zip(params, theirs, host):
            p.grad = torch.from_numpy(h).cuda()
            q.grad = p.grad.clone()
        norm = optim.clip_grad_norm_(params, max_norm)
        want = R.total_norm(host, dtype)
        assert norm.dtype == _tdtype(dtype) and norm.shape == () and same_bits(norm.cpu().numpy(), np.array(want))
        coef = R.clip_coef(want, max_norm, dtype)
        for p, h in zip(params, host):
            assert same_bits(p.grad.cpu().numpy(), R.scale(h, coef))
        assert params[-1].grad is None
        ref = float(torch.nn.utils.clip_grad_norm_(theirs, max_norm))
        n = sum(sizes)
        # torch's float32 tree over n squares: log2(n) roundings of the sum, half of that in the root, and two roundings
        bound = (2 + np.log2(n) / 2) * float(np.spacing(np.float32(ref))) if dtype == np.float32 else n * 2.0 ** -52 * ref
        assert abs(float(norm) - ref) <= bound
    assert float(optim.clip_grad_norm_([torch.nn.Parameter(torch.zeros(3, device="cuda"))], 1.0)) == 0.0


# ---- the optimizer objects against the fixture and against torch ----------------------------------------------------

@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "optim_step.npz"))


def _make(kind, params, hyper, lr, ours):
    from hironaka_amd import optim
    if kind == R.ADAM:
        return optim.Adam(params, lr=lr, **hyper) if ours else torch.optim.Adam(params, lr=lr, **hyper)
    return optim.SGD(params, lr=lr, **hyper) if ours else torch.optim.SGD(params, lr=lr, **hyper)


def _params(flat, shapes, dtype):
    return [torch.nn.Parameter(torch.from_numpy(x.copy()).cuda()) for x in R.split(flat, shapes)]


def _flat(tensors):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors])


def _torch_state_dict(opt, kind, hyper, s, s1, s2, shapes):
    """the state_dict that torch's optimizer would hold before step s of a fixture case"""
    sd = opt.state_dict()
    if s == 0:
        return sd
    state = {}
    for k, (m, v) in enumerate(zip(R.split(s1, shapes) if s1 is not None else [None] * len(shapes),
                                   R.split(s2, shapes) if s2 is not None else [None] * len(shapes))):
        if kind == R.ADAM:
            state[k] = {"step": torch.tensor(float(s)), "exp_avg": torch.from_numpy(m.copy()),
                        "exp_avg_sq": torch.from_numpy(v.copy())}
        else:
            state[k] = {"momentum_buffer": torch.from_numpy(m.copy()) if m is not None else None}
    sd["state"] = state
    return sd


def test_fixture_cases_through_the_optimizer_objects(fix):
    """every step of every case from torch's recorded parameters, state and gradients (loaded through
    load_state_dict) through clip_and_step.  The kernels' norm is within the CPU test's bound of torch's; where its
    clipping coefficient is torch's to the bit (torch adds the squares in another order: a third of the steps differ in
    the norm's last bit) the clipped gradients, Adam's exp_avg and exp_avg_sq and all of SGD are torch's bits; Adam's
    parameters lie within the fixture's measured tolerance of the reference evaluation everywhere"""
    tolerance = float(fix["adam_p_tolerance"])
    lr = float(fix["lr"])
    exact_steps = steps = 0
    worst = 0.0
    for key, _, kind, hyper, dtype, net in R.case_keys():
        shapes = [tuple(p.shape) for p in D.build_net(net, R.NUM_ACTIONS, torch.float32).parameters()]
        max_norm = float(fix[f"{key}_max_norm"])
        has1, has2 = f"{key}_s1" in fix, f"{key}_s2" in fix
        for s in range(R.STEPS):
            params = _params(fix[f"{key}_p"][s], shapes, dtype)
            opt = _make(kind, params, hyper, lr, ours=True)
            opt.load_state_dict(_torch_state_dict(opt, kind, hyper, s, fix[f"{key}_s1"][s - 1] if has1 and s else None,
                                                  fix[f"{key}_s2"][s - 1] if has2 and s else None, shapes))
            for p, g in zip(params, R.split(fix[f"{key}_grad"][s], shapes)):
                p.grad = torch.from_numpy(g.copy()).cuda()
            opt.clip_and_step(max_norm)
            norm = float(opt.total_norm())
            want = float(fix[f"{key}_norm"][s])
            bound = float(np.spacing(np.float32(want))) if dtype == np.float32 else \
                fix[f"{key}_grad"].shape[1] * 2.0 ** -52 * want
            assert abs(norm - want) <= bound, (key, s)
            steps += 1
            p1 = _flat(params)
            if kind == R.ADAM:
                n = p1.size
                m0 = fix[f"{key}_s1"][s - 1] if s else np.zeros(n, dtype)
                v0 = fix[f"{key}_s2"][s - 1] if s else np.zeros(n, dtype)
                block = _ops().optim_state_read(opt._blocks[0])
                ref = R.adam_reference(fix[f"{key}_p"][s], _flat([p.grad for p in params]), m0, v0, block,
                                       hyper["betas"], weight_decay=hyper.get("weight_decay", 0.0))
                dist = R.adam_distance(p1, ref, fix[f"{key}_p"][s], dtype)
                worst = max(worst, dist)
                assert dist <= tolerance, (key, s, dist, tolerance)
            if R.clip_coef(dtype(norm), max_norm, dtype) != R.clip_coef(fix[f"{key}_norm"][s], max_norm, dtype):
                continue
            exact_steps += 1
            assert same_bits(_flat([p.grad for p in params]), fix[f"{key}_clipped"][s]), (key, s)
            if has1:
                name = "exp_avg" if kind == R.ADAM else "momentum_buffer"
                assert same_bits(_flat([opt.state[p][name] for p in params]), fix[f"{key}_s1"][s]), (key, s)
            if has2:
                assert same_bits(_flat([opt.state[p]["exp_avg_sq"] for p in params]), fix[f"{key}_s2"][s]), (key, s)
            if kind == R.SGD:
                assert same_bits(p1, fix[f"{key}_p"][s + 1]), (key, s)
    print(f"{exact_steps} of {steps} steps with torch's clipping coefficient to the bit; Adam's parameters at most "
          f"{worst:.3f} units from the reference (tolerance {tolerance:.3f})")
    assert steps == len(R.case_keys()) * R.STEPS and exact_steps >= steps // 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_one_step_against_torch_on_the_device(name, dtype, fix):
    """one step from identical state next to torch's own optimizer on the device: SGD bit for bit where the norms agree
    to the bit, Adam's parameters within the measured tolerance, both after a first step that builds the state"""
    _, kind, hyper = next(c for c in R.CASES if c[0] == name)
    tolerance = float(fix["adam_p_tolerance"])
    rng = np.random.default_rng(12)
    shapes = [(33, 7), (7,), (1030,)]
    start = [rng.standard_normal(s).astype(dtype) for s in shapes]
    ours_p = [torch.nn.Parameter(torch.from_numpy(x.copy()).cuda()) for x in start]
    theirs_p = [torch.nn.Parameter(torch.from_numpy(x.copy()).cuda()) for x in start]
    ours, theirs = _make(kind, ours_p, hyper, 0.05, True), _make(kind, theirs_p, hyper, 0.05, False)
    for step in range(2):
        grads = [rng.standard_normal(s).astype(dtype) for s in shapes]
        for p, q, g in zip(ours_p, theirs_p, grads):
            p.grad, q.grad = torch.from_numpy(g.copy()).cuda(), torch.from_numpy(g.copy()).cuda()
        with torch.no_grad():  # identical state: torch's becomes ours
            for p, q in zip(ours_p, theirs_p):
                q.copy_(p)
                for k, v in ours.state[p].items():
                    if isinstance(v, torch.Tensor) and k != "step":
                        theirs.state[q][k].copy_(v)
        before = _flat(ours_p)
        ours.clip_and_step(5.0)
        ref_norm = torch.nn.utils.clip_grad_norm_(theirs_p, 5.0)
        theirs.step()
        got, want = _flat(ours_p), _flat(theirs_p)
        if kind == R.SGD:
            if float(ours.total_norm()) == float(ref_norm):
                assert same_bits(got, want), step
            else:
                assert np.abs(got - want).max() <= 4 * np.finfo(dtype).eps * np.abs(want).max()
        else:
            unit = np.maximum(R.ulp(want, dtype), R.ulp(want.astype(np.longdouble) - before, dtype))
            dist = float((np.abs(got.astype(np.longdouble) - want) / unit).max())
            print(f"{name} {np.dtype(dtype).name} step {step}: {dist:.3f} units from torch on the device")
            assert dist <= tolerance, (step, dist)


def test_state_dict_round_trips_with_torch():
    from hironaka_amd import optim
    rng = np.random.default_rng(13)
    for kind, hyper in ((R.ADAM, dict(betas=(0.9, 0.999))), (R.SGD, dict(momentum=0.9))):
        start = [rng.standard_normal(s).astype(np.float32) for s in ((5, 3), (40,))]
        grads = [[rng.standard_normal(x.shape).astype(np.float32) for x in start] for _ in range(4)]

        def run(opt, params, steps):
            for g in steps:
                for p, x in zip(params, g):
                    p.grad = torch.from_numpy(x.copy()).cuda()
                opt.step()

        make = lambda: [torch.nn.Parameter(torch.from_numpy(x.copy()).cuda()) for x in start]  # noqa: E731
        a_p, b_p = make(), make()
        a = _make(kind, a_p, hyper, 0.05, True)
        run(a, a_p, grads[:2])
        sd = copy.deepcopy(a.state_dict())  # as a checkpoint would be: load_state_dict does not copy tensors that fit
        if kind == R.ADAM:
            assert all(float(e["step"]) == 2.0 for e in sd["state"].values())
        b = _make(kind, b_p, hyper, 0.05, False)  # ours -> torch's
        with torch.no_grad():
            for p, q in zip(a_p, b_p):
                q.copy_(p)
        b.load_state_dict(sd)
        run(b, b_p, grads[2:3])
        c = optim.from_torch(b)  # torch's -> ours, over the same parameters
        assert type(c) is (optim.Adam if kind == R.ADAM else optim.SGD) and c.param_groups[0]["params"][0] is b_p[0]
        run(c, b_p, grads[3:])
        run(a, a_p, grads[2:])  # ours all the way
        if kind == R.ADAM:
            assert _ops().optim_state_read(c._blocks[0])["step"] == 4
            assert float(c.state_dict()["state"][0]["step"]) == 4.0
        got, want = _flat(b_p), _flat(a_p)
        assert np.abs(got - want).max() <= 64 * np.finfo(np.float32).eps * np.abs(want).max()


def test_refusals():
    from hironaka_amd import optim
    from hironaka_amd._lib import HironakaHipError
    ops = _ops()
    p = torch.nn.Parameter(torch.zeros(8, device="cuda"))
    q = torch.nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.float64))
    for name in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError):
            optim.Adam([p], **{name: True})
    with pytest.raises(NotImplementedError):
        optim.SGD([p], lr=0.1, maximize=True)
    with pytest.raises(NotImplementedError):
        optim.from_torch(torch.optim.Adam([p], amsgrad=True))
    with pytest.raises(NotImplementedError):
        optim.from_torch(torch.optim.AdamW([p]))
    mixed = optim.Adam([p, q])
    p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
    with pytest.raises(TypeError):
        mixed.step()
    half = torch.nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.float16))
    half.grad = torch.ones_like(half)
    with pytest.raises(TypeError):
        optim.Adam([half]).step()
    block = ops.optim_state("cuda")
    a = torch.zeros(16, device="cuda")
    with pytest.raises(HironakaHipError):  # the parameter on top of its gradient: refused on the host
        ops.optim_apply(ops.OptimChain("sgd", [a[:8]], [a[4:12]], state=block))
    with pytest.raises(HironakaHipError):
        ops.optim_apply(ops.OptimChain("adam", [a[:4]], [a[4:8]], [a[8:12]], [a[10:14]], state=block))
    with pytest.raises(TypeError):
        ops.OptimChain("scale", [a.cpu()], state=block)
    with pytest.raises(TypeError):
        ops.OptimChain("scale", [a[::2]], state=block)
    with pytest.raises(ValueError):
        ops.OptimChain("sgd", [a[:8]], [a[8:12]], state=block)
    with pytest.raises(ValueError):
        ops.OptimChain("lamb", [a], state=block)
    none = optim.Adam([torch.nn.Parameter(torch.ones(3, device="cuda"))])
    none.step()  # no gradient anywhere: nothing happens, as in torch
    assert not none._blocks and float(none.param_groups[0]["params"][0].detach().sum()) == 3.0
    assert not a.any()


# ---- fit_network, no synchronisation, graph capture -----------------------------------------------------------------

class _Buffer:
    def __init__(self, rng, B, obs_dim, num_actions):
        self.batch = (torch.from_numpy(rng.standard_normal((B, obs_dim)).astype(np.float32)).cuda(),
                      torch.from_numpy(rng.integers(0, num_actions, (B, 1)).astype(np.int32)).cuda(),
                      torch.from_numpy(rng.integers(-1, 2, (B, 1)).astype(np.float32)).cuda(),
                      torch.from_numpy(rng.integers(0, 2, (B, 1)).astype(bool)).cuda(),
                      torch.from_numpy(rng.standard_normal((B, obs_dim)).astype(np.float32)).cuda())

    def sample(self, batch_size, device=None, clone=True):
        return self.batch


def test_fit_network_runs_clip_and_step_and_does_not_synchronise():
    from hironaka_amd import dqn, optim
    torch.manual_seed(5)
    q_net = D.build_net("three_layer", 4, torch.float32).cuda()
    target = D.build_net("three_layer", 4, torch.float32).cuda()
    buffer = _Buffer(np.random.default_rng(14), 40, D.OBS_DIM, 4)
    calls = []

    class Counting(optim.Adam):
        def clip_and_step(self, max_grad_norm, keep_grads=False):
            calls.append(max_grad_norm)
            return super().clip_and_step(max_grad_norm, keep_grads)

    opt = Counting(q_net.parameters(), lr=1e-2)
    for _ in range(2):  # the stream's workspaces, the state and the descriptors exist now
        dqn.fit_network(q_net, target, opt, buffer, 40, 0.99, 0.5)
    before = _flat(q_net.parameters())
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "a prototype feature"
        torch.cuda.set_sync_debug_mode("error")  # a synchronising torch call raises
        try:
            loss = dqn.fit_network(q_net, target, opt, buffer, 40, 0.99, 0.5)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert calls == [0.5] * 3 and loss.shape == ()
    # fit_network's zero_grad() drops the gradients and backward allocates new ones: the descriptors of the step before
    # serve all the same, with the new gradients' addresses written into them
    chain = opt._chains[0][1]
    dqn.fit_network(q_net, target, opt, buffer, 40, 0.99, 0.5)
    assert opt._chains[0][1] is chain
    calls.pop()
    assert not same_bits(_flat(q_net.parameters()), before)
    assert _ops().optim_state_read(opt._blocks[0])["step"] == 4
    # the step is the two lines it replaces: torch's clip_grad_norm_ and our step() from the same start agree
    clipped_norm = float(np.sqrt((_flat([p.grad for p in q_net.parameters()]).astype(np.float64) ** 2).sum()))
    assert clipped_norm <= 0.5 * (1 + 1e-5)


def test_clip_and_step_is_a_step_to_hooks_and_schedulers():
    from hironaka_amd import optim
    p = torch.nn.Parameter(torch.ones(8, device="cuda"))
    opt = optim.SGD([p], lr=0.5)
    seen = []
    opt.register_step_post_hook(lambda *a, **k: seen.append(1))
    scheduler = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # "lr_scheduler.step() before optimizer.step()" would raise
        for _ in range(2):
            p.grad = torch.ones_like(p)
            opt.clip_and_step(1e9)
            scheduler.step()
    assert seen == [1, 1] and opt.param_groups[0]["lr"] == 0.125
    assert same_bits(p.detach().cpu().numpy(), np.full(8, 1.0 - 0.5 - 0.25, np.float32))  # lr is read on every call


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_alone_meets_a_nonfinite_gradient_in_its_element_alone(dtype):
    """HK_OPTIM_NO_CLIP: the coefficient is 1 whatever the norm is, the block still has the norm; through the objects,
    step() with one infinite gradient leaves every other element what torch's step() leaves"""
    ops = _ops()
    from hironaka_amd import optim
    for kind in ("adam", "sgd"):
        t = Tensors(np.random.default_rng(16), [9, 600], dtype)
        t.host[1]["g"][17] = np.inf
        t.view[1]["g"][17] = float("inf")
        block = ops.optim_state("cuda")
        chain = t.chain(kind, block)
        b1, b2 = HYPER[kind].get("betas", (0.0, 0.0))
        st = R.prepare(R.new_state(), [h["g"] for h in t.host], dtype, lr=0.05, beta1=b1, beta2=b2, advance=True,
                       clip=False)
        ops.optim_prepare(chain, lr=0.05, beta1=b1, beta2=b2, advance=True, clip=False)
        _same_state(block, st, kind)
        assert st["clip_coef"] == 1.0 and st["total_norm"] == np.inf
    for make, theirs in ((optim.Adam, torch.optim.Adam), (optim.SGD, torch.optim.SGD)):
        start = np.random.default_rng(17).standard_normal(40).astype(dtype)
        grad = np.random.default_rng(18).standard_normal(40).astype(dtype)
        grad[7] = np.inf
        p, q = (torch.nn.Parameter(torch.from_numpy(start.copy()).cuda()) for _ in range(2))
        p.grad, q.grad = torch.from_numpy(grad.copy()).cuda(), torch.from_numpy(grad.copy()).cuda()
        make([p], lr=0.05).step()
        theirs([q], lr=0.05).step()
        got, want = p.detach().cpu().numpy(), q.detach().cpu().numpy()
        finite = np.arange(40) != 7
        assert np.isfinite(got[finite]).all() and not np.isfinite(got[7]) and not np.isfinite(want[7])
        assert np.abs(got[finite] - want[finite]).max() <= 8 * np.finfo(dtype).eps * np.abs(want[finite]).max()
        assert same_bits(p.grad.cpu().numpy(), grad)  # step() alone leaves .grad as it was


def _graph_edges(dot):
    """(nodes, edges) of a graph as the runtime prints it in dot: `a -> b` lines are edges, `a [...]` lines nodes"""
    edges = re.findall(r'^\s*"?([\w.]+)"?\s*->\s*"?([\w.]+)"?', dot, flags=re.M)
    nodes = set(re.findall(r'^\s*"?([\w.]+)"?\s*\[', dot, flags=re.M)) - {"node", "edge", "graph"}
    return nodes | {n for e in edges for n in e}, edges


def test_fit_step_replays_from_a_graph(tmp_path, monkeypatch):
    """sample -> TD -> backward -> clip_and_step -> Polyak captured into one graph and replayed three times equals three
    eager steps bit for bit; the learning rate is a tensor on the device that changes between the steps.  The graph is a
    linear chain.  Where the runtime writes its own dump of the captured graph (CUDAGraph.debug_dump), every node of it
    has at most one predecessor and one successor; torch 2.10 on ROCm returns from debug_dump without a file, so what is
    always asserted is what makes the chain linear: the capture is of ONE stream, and every stream that this package's
    launches ask for while capturing (they all ask torch.cuda.current_stream) is that stream.  Which stream torch's own
    kernels of the forward and backward passes take cannot be observed from here."""
    from hironaka_amd import dqn, optim
    rng = np.random.default_rng(15)
    buffer = _Buffer(rng, 64, D.OBS_DIM, 5)
    lrs = [0.05, 0.02, 0.01]

    def fresh():
        torch.manual_seed(6)
        q_net = D.build_net("three_layer", 5, torch.float32).cuda()
        target = D.build_net("three_layer", 5, torch.float32).cuda()
        lr = torch.tensor([lrs[0]], dtype=torch.float64, device="cuda")
        opt = optim.Adam(q_net.parameters(), lr=lr)
        for p in q_net.parameters():  # static gradients, as a captured step needs them
            p.grad = torch.zeros_like(p)
        return q_net, target, opt, lr

    def step(q_net, target, opt):
        observations, actions, rewards, dones, next_observations = buffer.sample(64)
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
        eager.append((loss.item(), _flat(q_net.parameters()), _flat(target.parameters())))
    assert eager[0][0] != eager[1][0]
    q_net, target, opt, lr = fresh()
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    state = [p.detach().clone() for p in list(q_net.parameters()) + list(target.parameters())]
    with torch.cuda.stream(warm):  # one step on the side stream builds state, descriptors and workspaces
        step(q_net, target, opt)
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    with torch.no_grad():  # and is undone: parameters, Adam's state and the count
        for p, s in zip(list(q_net.parameters()) + list(target.parameters()), state):
            p.copy_(s)
        for p in q_net.parameters():
            opt.state[p]["exp_avg"].zero_()
            opt.state[p]["exp_avg_sq"].zero_()
        opt._blocks[0].copy_(_ops().optim_state("cuda"))
    graph = torch.cuda.CUDAGraph()
    graph.enable_debug_mode()  # keeps the captured graph for debug_dump
    asked = []
    current_stream = torch.cuda.current_stream

    def recording(device=None):
        stream = current_stream(device)
        asked.append(stream.cuda_stream)
        return stream

    with torch.cuda.graph(graph, stream=warm):
        monkeypatch.setattr(torch.cuda, "current_stream", recording)
        loss = step(q_net, target, opt)
        monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    # replay_sample is not part of this step (the stub buffer serves fixed rows); TD, two prepare / apply launches and
    # Polyak each ask once or more
    assert len(asked) >= 4 and set(asked) == {warm.cuda_stream}, (len(asked), set(asked), warm.cuda_stream)
    dot_path = str(tmp_path / "fit_step.dot")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "DEBUG: calling debug_dump()"
        graph.debug_dump(dot_path)
    if os.path.exists(dot_path):
        with open(dot_path) as f:
            dot = f.read()
        nodes, edges = _graph_edges(dot)
        assert len(nodes) >= 10, (len(nodes), dot[:500])  # two network calls, TD, backward, two launches, Polyak
        assert len(edges) == len(nodes) - 1 and len(set(edges)) == len(edges), (len(nodes), len(edges))
        assert max(collections.Counter(a for a, _ in edges).values()) == 1  # at most one successor
        assert max(collections.Counter(b for _, b in edges).values()) == 1  # at most one predecessor
    for k in range(3):
        lr.fill_(lrs[k])
        graph.replay()
        torch.cuda.synchronize()
        assert loss.item() == eager[k][0], k
        assert same_bits(_flat(q_net.parameters()), eager[k][1]), k
        assert same_bits(_flat(target.parameters()), eager[k][2]), k
    assert _ops().optim_state_read(opt._blocks[0])["step"] == 3
