"""Writes tests/golden/mlp_train.npz: per case of mlp_train_rules.CASES the seeds the net and the inputs are drawn from
(mlp_rules.seeded_state: seeds, not weights), torch's own CPU training forward and backward in float32 and float64 --
every result to the byte for the small `test` config, by its distance E to the float64 run otherwise -- and the
distance of the rule of mlp_train_rules.py.  Run from the repository root: python tests/golden/make_mlp_train_golden.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import mlp_train_rules as T  # noqa: E402

SEED = 20240


def main():
    out = {}
    for i, key in enumerate(T.CASES):
        seed = SEED + 10 * i
        net = T.seeded_net(T.CASES[key][0], "host", seed)
        points, grad = T.case_inputs(key, seed + 1)
        r64 = T.torch_run(net, points, grad, torch.float64)
        r32 = T.torch_run(net, points, grad, torch.float32)
        rule = T.rule_run(net, points, grad)
        out[f"{key}_seed"] = seed
        out[f"{key}_names"] = np.array([k for k, _ in r64])
        out[f"{key}_e_torch"] = np.array(T.case_units(r32, r64))
        out[f"{key}_e_rule"] = np.array(T.case_units(rule, r64))
        if key == "test_256":
            for (k, v32), (_, v64) in zip(r32, r64):
                out[f"{key}_32_{k}"], out[f"{key}_64_{k}"] = v32, v64
        worst = max(r / max(t, 1) for r, t in zip(out[f"{key}_e_rule"], out[f"{key}_e_torch"]))
        print(f"{key}: max E_torch {out[f'{key}_e_torch'].max():.2f} max E_rule {out[f'{key}_e_rule'].max():.2f} "
              f"worst E_rule / max(E_torch, 1) {worst:.2f}")
    np.savez_compressed(os.path.join(HERE, "mlp_train.npz"), **out)


if __name__ == "__main__":
    main()
