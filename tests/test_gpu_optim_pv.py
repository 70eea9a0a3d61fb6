"""The MCTS trainer's additions to hironaka_amd.optim on the device, against something other than themselves:
safe_clip_grads_ against the reference's formula (hironaka/jax/util.py:426-430) in float64, and AdamW against
torch.optim.AdamW on the same parameters and gradients."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4), (5,), (2, 2, 2), (700,)]


def _grads(rng, scale, dtype):
    """parameters on the device whose gradients have the 2-norm `scale` (to rounding), and one without a gradient"""
    raw = [rng.standard_normal(s) for s in SHAPES]
    norm = np.sqrt(sum((g ** 2).sum() for g in raw))
    ps = [torch.nn.Parameter(torch.zeros(s, dtype=dtype, device="cuda")) for s in SHAPES]
    for p, g in zip(ps, raw):
        p.grad = torch.from_numpy(g * (scale / norm)).to(dtype).cuda()
    return ps + [torch.nn.Parameter(torch.zeros(3, dtype=dtype, device="cuda"))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_safe_clip_grads_on_the_device_is_the_reference_formula(dtype):
    """g where norm < max_norm (to the bit), else g * max_norm / (norm + 1e-9), the norm being the float64 2-norm of the
    gradients as they lie on the device.  The norm: within hk_optim_prepare's bound of the float64 value (the bound
    test_gpu_optim.py holds clip_grad_norm_ to); a clipped gradient: the coefficient rounded to the gradients' dtype, then
    one rounded product -- two roundings plus the norm's error, 4 eps of the largest element."""
    from hironaka_amd import optim
    rng = np.random.default_rng(31)
    eps = float(torch.finfo(dtype).eps)
    n = sum(int(np.prod(s)) for s in SHAPES)
    for scale, max_norm in [(0.5, 1.0), (0.999, 1.0), (1.001, 1.0), (3.0, 1.0), (40.0, 0.5), (2.0, 2.5)]:
        ps = _grads(rng, scale, dtype)
        before = [p.grad.double().cpu().numpy().copy() for p in ps[:-1]]
        bits = [p.grad.cpu().numpy().tobytes() for p in ps[:-1]]
        norm = float(np.sqrt(sum((g ** 2).sum() for g in before)))
        got = optim.safe_clip_grads_(ps, max_norm)
        assert got.is_cuda and got.shape == () and got.dtype == dtype and ps[-1].grad is None
        bound = (2 + np.log2(n) / 2) * float(np.spacing(np.float32(norm))) if dtype == torch.float32 else n * 2.0 ** -52 * norm
        assert abs(float(got) - norm) <= bound, (scale, max_norm)
        assert (norm < max_norm) == (scale < max_norm)  # no case sits on the edge by accident
        for p, g, b in zip(ps[:-1], before, bits):
            if norm < max_norm:
                assert p.grad.cpu().numpy().tobytes() == b, (scale, max_norm)
            else:
                want = g * max_norm / (norm + 1e-9)
                assert np.abs(p.grad.double().cpu().numpy() - want).max() <= 4 * eps * np.abs(want).max(), (scale, max_norm)
    # norm == max_norm exactly (3-4-5): not `<`, so the rule applies; in float64 the 1e-9 shows, in float32 the
    # coefficient 5 / (5 + 1e-9) rounds to 1
    p = torch.nn.Parameter(torch.zeros(2, dtype=dtype, device="cuda"))
    p.grad = torch.tensor([3.0, 4.0], dtype=dtype, device="cuda")
    assert float(optim.safe_clip_grads_(p, 5.0)) == 5.0
    want = np.array([3.0, 4.0]) * 5.0 / (5.0 + 1e-9)
    assert np.abs(p.grad.double().cpu().numpy() - want).max() <= 4 * eps * 4.0
    if dtype == torch.float64:
        assert bool((p.grad.cpu() < torch.tensor([3.0, 4.0], dtype=dtype)).all())
    q = torch.nn.Parameter(torch.zeros(2, dtype=dtype, device="cuda"))
    q.grad = torch.tensor([3.0, 4.0], dtype=dtype, device="cuda")
    optim.safe_clip_grads_(q, 2.5)  # and a different rule from torch's min(1, max_norm / (norm + 1e-6)) is visible in float64
    assert np.abs(q.grad.double().cpu().numpy() - np.array([1.5, 2.0]) * (1 / (1 + 2e-10))).max() <= 4 * eps * 2.0


def test_adamw_steps_match_torch_adamw():
    """four steps of optim.AdamW against torch.optim.AdamW on the same start and gradients, within the tolerance
    test_gpu_optim.py holds Adam to over four steps (64 eps of the largest parameter); the decay (lr 0.05, weight_decay
    0.2: a factor 0.99 per step) moves the parameters a thousand times further than that, and the coupled decay of
    optim.Adam lands elsewhere"""
    from hironaka_amd import optim
    rng = np.random.default_rng(32)
    start = [(3.0 * rng.standard_normal(s)).astype(np.float32) for s in ((5, 3), (40,), (300,))]
    grads = [[rng.standard_normal(x.shape).astype(np.float32) for x in start] for _ in range(4)]
    hyper = dict(lr=0.05, betas=(0.8, 0.95), eps=1e-6)

    def run(make):
        params = [torch.nn.Parameter(torch.from_numpy(x.copy()).cuda()) for x in start]
        opt = make(params)
        for step in grads:
            for p, g in zip(params, step):
                p.grad = torch.from_numpy(g.copy()).cuda()
            opt.step()
        return np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in params]), opt

    ours, opt = run(lambda ps: optim.AdamW(ps, weight_decay=0.2, **hyper))
    theirs, _ = run(lambda ps: torch.optim.AdamW(ps, weight_decay=0.2, **hyper))
    plain, _ = run(lambda ps: optim.Adam(ps, **hyper))
    coupled, _ = run(lambda ps: optim.Adam(ps, weight_decay=0.2, **hyper))
    scale = np.abs(theirs).max()
    tolerance = 64 * np.finfo(np.float32).eps * scale
    assert np.abs(ours - theirs).max() <= tolerance
    assert np.abs(ours - plain).max() > 1000 * tolerance and np.abs(ours - coupled).max() > 1000 * tolerance
    assert float(opt.state_dict()["state"][0]["step"]) == 4.0
    # max_grad_norm goes through: clipped to the same norm, the two still agree
    ours_c, _ = run(lambda ps: _Clipped(optim.AdamW(ps, weight_decay=0.2, **hyper), ps))
    theirs_c, _ = run(lambda ps: _Clipped(torch.optim.AdamW(ps, weight_decay=0.2, **hyper), ps))
    assert np.abs(ours_c - theirs_c).max() <= tolerance


class _Clipped:
    """step() behind torch's clip_grad_norm_ at 0.5 (ours: clip_and_step, the same rule in the kernels)"""

    def __init__(self, opt, params):
        self.opt, self.params = opt, params

    def step(self):
        if hasattr(self.opt, "clip_and_step"):
            self.opt.clip_and_step(0.5)
        else:
            torch.nn.utils.clip_grad_norm_(self.params, 0.5)
            self.opt.step()

    def state_dict(self):
        return self.opt.state_dict()
