"""
Generate tests/golden/optim_step.npz by RUNNING torch's own ``nn.utils.clip_grad_norm_``, ``torch.optim.Adam`` and
``torch.optim.SGD`` on the CPU (``foreach=False``): the two lines of ``DQNTrainer._fit_network``
(hironaka/trainer/dqn_trainer/dqn_trainer.py:95-98) that hk_optim_prepare / hk_optim_apply replace.  The .npz is what
travels, and it holds data only.

One case per (optimiser variant of tests/optim_rules.py CASES) x (float32, float64) x (the three nets of
dqn_rules.build_net).  A case runs STEPS steps: a forward pass of the net on a random batch, a mean squared error
against a random target scaled by 1, 0.01 and 1 in turn, backward, clip_grad_norm_(max_grad_norm), step.  max_grad_norm is
half the first step's norm, so that clipping bites in the first step, not in the second (whose loss is scaled down) and,
as it happens, again in the third; main() asserts that every case sees both.

Layout, for case key K (optim_rules.case_keys(); every tensor list flattened into one vector in named_parameters order):
    K_p        [STEPS + 1, n]   the parameters before the first step and after every step
    K_grad     [STEPS, n]       the gradients as backward left them
    K_clipped  [STEPS, n]       .grad after clip_grad_norm_
    K_s1       [STEPS, n]       exp_avg / momentum_buffer after every step (absent without momentum)
    K_s2       [STEPS, n]       exp_avg_sq after every step (Adam)
    K_p64      [STEPS, n]       float32 Adam cases: the parameters after one step of torch's float64 Adam from the float32
                                parameters, state and clipped gradient before that step (float64)
    K_norm     [STEPS]          what clip_grad_norm_ returned
    K_max_norm []
and the yardstick of Adam's last line, which no scalar formulation reproduces to the bit (torch's addcdiv_ is
vectorised):
    adam_p_yardstick   the largest distance of torch's float32 Adam from torch's float64 Adam run from the SAME float32
                       state and clipped gradient (re-synchronised every step), over all float32 Adam cases, in units of
                       max(ulp(p), ulp(update)) of float32
    adam_p_tolerance   twice that: what the rule may lie from the float64 result (the factor 2: the one rounding that a
                       differently ordered addcdiv adds)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_optim_golden.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dqn_rules as D  # noqa: E402
import optim_rules as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LOSS_SCALES = (1.0, 0.01, 1.0)


def flat(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors]).copy()


def make_optimizer(kind, params, hyper, lr=R.LR):
    if kind == R.ADAM:
        return torch.optim.Adam(params, lr=lr, foreach=False, **hyper)
    return torch.optim.SGD(params, lr=lr, foreach=False, **hyper)


def float64_step(params, clipped, state, hyper, step):
    """one step of torch's float64 Adam from the float32 parameters, state and clipped gradient"""
    ps = [torch.nn.Parameter(p.detach().double().clone()) for p in params]
    opt = make_optimizer(R.ADAM, ps, hyper)
    for p64, g, st in zip(ps, clipped, state):
        p64.grad = g.double().clone()
        opt.state[p64] = {"step": torch.tensor(float(step)), "exp_avg": st["exp_avg"].double().clone(),
                          "exp_avg_sq": st["exp_avg_sq"].double().clone()}
    opt.step()
    return flat(ps)


def run_case(key, kind, hyper, dtype, net_kind, seed, rec):
    torch.manual_seed(seed)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    net = D.build_net(net_kind, R.NUM_ACTIONS, tdt)
    net.train()
    params = list(net.parameters())
    opt = make_optimizer(kind, params, hyper)
    ps, grads, clipped, s1, s2, norms, p64 = [flat(params)], [], [], [], [], [], []
    max_norm, worst = None, 0.0
    for step in range(R.STEPS):
        obs = torch.randn(R.BATCH, D.OBS_DIM, dtype=tdt)
        target = torch.randn(R.BATCH, R.NUM_ACTIONS, dtype=tdt)
        opt.zero_grad()
        loss = ((net(obs) - target) ** 2).mean() * LOSS_SCALES[step]
        loss.backward()
        grads.append(flat([p.grad for p in params]))
        if max_norm is None:
            max_norm = 0.5 * float(np.sqrt((grads[0].astype(np.float64) ** 2).sum()))
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)))
        clipped.append(flat([p.grad for p in params]))
        if kind == R.ADAM and dtype == np.float32:
            before = flat(params).astype(np.float64)
            state = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in opt.state[p].items()}
                     if opt.state[p] else {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
                     for p in params]
            want = float64_step(params, [p.grad for p in params], state, hyper, step)
            p64.append(want)
        opt.step()
        ps.append(flat(params))
        if kind == R.ADAM:
            s1.append(flat([opt.state[p]["exp_avg"] for p in params]))
            s2.append(flat([opt.state[p]["exp_avg_sq"] for p in params]))
            if dtype == np.float32:
                unit = np.maximum(R.ulp(want, dtype), R.ulp(want - before, dtype))
                worst = max(worst, float((np.abs(ps[-1].astype(np.longdouble) - want) / unit).max()))
        elif hyper.get("momentum"):
            s1.append(flat([opt.state[p]["momentum_buffer"] for p in params]))
    bites = [n + 1e-6 > max_norm for n in norms]
    assert any(bites) and not all(bites), (key, norms, max_norm)
    rec[f"{key}_p"], rec[f"{key}_grad"], rec[f"{key}_clipped"] = np.stack(ps), np.stack(grads), np.stack(clipped)
    if s1:
        rec[f"{key}_s1"] = np.stack(s1)
    if s2:
        rec[f"{key}_s2"] = np.stack(s2)
    if p64:
        rec[f"{key}_p64"] = np.stack(p64)
    rec[f"{key}_norm"] = np.array(norms, dtype=dtype)
    rec[f"{key}_max_norm"] = np.array(max_norm)
    return worst


def main():
    rec, worst = {}, 0.0
    for k, (key, _, kind, hyper, dtype, net_kind) in enumerate(R.case_keys()):
        worst = max(worst, run_case(key, kind, hyper, dtype, net_kind, 7000 + k, rec))
    assert worst > 0.0
    rec["adam_p_yardstick"] = np.array(worst)
    rec["adam_p_tolerance"] = np.array(2.0 * worst)
    rec["lr"] = np.array(R.LR)
    path = os.path.join(OUT, "optim_step.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {len(R.case_keys())} cases, {len(rec)} arrays, {os.path.getsize(path)} bytes; "
          f"torch float32 Adam lies up to {worst:.4f} units from torch float64 Adam")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
