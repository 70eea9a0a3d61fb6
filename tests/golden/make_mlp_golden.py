"""
Generate tests/golden/mlp_nets.npz by RUNNING the reference's own ``create_mlp`` (hironaka/trainer/nets.py:27-73) with
its two feature extractors on torch CPU.  Runs only where the reference checkout exists; the .npz is what travels, and it
holds data only.

For every net of mlp_rules.NET_ARCHS and both heads (key K = "<net>_<head>"):
    K_arch       the net_arch, as JSON
    K_children   the class names of the Sequential's children, as JSON
    K_shapes     [(state_dict key, shape), ...], as JSON
    K_seed       the seed of mlp_rules.seeded_state, which gives the state_dict (the weights are NOT stored: the example
                 config's alone are 5 MB), and of mlp_rules.seeded_inputs
    K_points     [96, 20, 3] features in [-0.2, 1];  K_coords [96, 3] (agent)
    K_y32, K_y64 the reference net's eval-mode outputs in float32 and, recast with .double(), in float64
    K_e_torch    max |y32 - y64| in units of max |y64| * 2^-24
    K_e_rule     the same distance for tests/mlp_rules.py's forward (NaN for the residual net, which the rule lacks)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mlp_golden.py
"""
import copy
import json
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from make_golden import OUT, REF, _load  # noqa: E402
import mlp_rules as R  # noqa: E402
from hironaka_amd import nets  # noqa: E402


def load_state(net, state):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return net.eval()


def main():
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not present: fixtures can only be regenerated next to the reference")
    ref = _load("reference_nets", "hironaka/trainer/nets.py")
    out = {}
    seed = 20260
    for name, arch in R.NET_ARCHS.items():
        for head, (input_dim, output_dim) in R.HEADS.items():
            seed += 1
            key = f"{name}_{head}"
            extractor = ref.HostFeatureExtractor if head == "host" else ref.AgentFeatureExtractor
            net = ref.create_mlp(extractor(input_dim), arch, input_dim, output_dim)
            shapes = [(k, list(v.shape)) for k, v in net.state_dict().items()]
            state = R.seeded_state(shapes, seed)
            load_state(net, state)
            points, coords = R.seeded_inputs(seed)
            t = torch.from_numpy
            with torch.no_grad():
                if head == "host":
                    y32 = net(t(points)).numpy()
                    y64 = copy.deepcopy(net).double()(t(points).double()).numpy()
                else:
                    y32 = net({"points": t(points), "coords": t(coords)}).numpy()
                    y64 = copy.deepcopy(net).double()({"points": t(points).double(), "coords": t(coords).double()}).numpy()
            e_rule = float("nan")
            if name not in R.RESIDUAL:
                mine_head = nets.HostFeatureExtractor if head == "host" else nets.AgentFeatureExtractor
                mine = load_state(nets.create_mlp(mine_head(input_dim), arch, input_dim, output_dim), state)
                layers, input_relu, input_bn = R.spec_layers(nets.mlp_spec(mine), lambda x: None if x is None
                                                             else x.detach().numpy())
                x = points.reshape(R.ROWS, -1)
                x = x if head == "host" else np.concatenate([x, coords], axis=1)
                e_rule = R.units(R.forward(x, layers, input_relu, input_bn), y64)
            out.update({f"{key}_arch": json.dumps(arch), f"{key}_shapes": json.dumps(shapes), f"{key}_seed": seed,
                        f"{key}_children": json.dumps([type(m).__name__ for m in net.children()]),
                        f"{key}_points": points, f"{key}_y32": y32, f"{key}_y64": y64,
                        f"{key}_e_torch": R.units(y32, y64), f"{key}_e_rule": e_rule})
            if head == "agent":
                out[f"{key}_coords"] = coords
            print(f"{key}: E_torch {out[key + '_e_torch']:.2f}  E_rule {e_rule:.2f}  "
                  f"argmax equal {bool((y32.argmax(1) == y64.argmax(1)).all())}")
    np.savez_compressed(os.path.join(OUT, "mlp_nets.npz"), **out)


if __name__ == "__main__":
    main()
