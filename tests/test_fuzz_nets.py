"""tests/fuzz_nets.py without a GPU: what the slice that tests/test_gpu_fuzz_nets.py commits reaches, how many of its cases
are degenerate (by the rule alone), that the comparison can fail on each kind of deviation, and that a seed gives the same
cases and the rule the same bits."""
import copy
import itertools

import numpy as np
import pytest

import fuzz_nets as F
from test_gpu_fuzz_nets import COUNT, SEED

FAMILIES = list(COUNT)
DEGENERATE_CAP, NONFINITE_CAP = 0.05, 0.10


@pytest.fixture(scope="module")
def slices():
    return {family: [F.case_at(family, SEED, i) for i in range(COUNT[family])] for family in FAMILIES}


def _blocks(case):
    """(kind, k, n) of every block of a pvnet case"""
    return [(kind, k, n) for kind, k, n in zip(case["kinds"], case["widths"][:-1], case["widths"][1:])]


def missing(family, cases):
    """what the issue asks a slice to reach and this one does not"""
    want = {}

    def need(name, hit):
        want[name] = want.get(name, False) or bool(hit)
    for c in cases:
        opts, batch = c["options"], c["batch"]
        if family != "train":
            for tile in (16, 64):
                for name, b in (("below", tile - 1), ("at", tile), ("one past", tile + 1)):
                    need(f"forced tile {tile} with a batch {name} the tile", c["tile"] == tile and batch == b)
            need("the library's own tile", c["tile"] is None)
        if family == "pvnet":
            blocks = _blocks(c)
            for n in F.NORMED:
                need(f"normed width {n} with a projection", ("residue", n) in [(kd, w) for kd, k, w in blocks if k != w])
                need(f"normed width {n} without a projection", ("residue", n, n) in blocks)
            need("a dense block narrower than 16", any(kd == "dense" and n < 16 for kd, _, n in blocks))
            need("a dense block of width 256", any(kd == "dense" and n == 256 for kd, _, n in blocks))
            need("255 actions", c["actions"] == 255)
            names = ("bias", "scale_on", "scale_off", "shift_on", "shift_off")
            need("no bias", not opts["bias"])
            for name in names:
                need(f"option {name}", opts[name])
        else:
            for name in ("bias", "bn", "input_relu", "last_relu") + (("input_bn",) if family == "mlp" else ()):
                need(f"option {name} on", opts[name])
                need(f"option {name} off", not opts[name])
            need("option affine on", opts["bn"] and opts["affine"])
            need("option affine off", opts["bn"] and not opts["affine"])
            if family == "mlp":
                need("option input affine on", opts["input_bn"] and opts["input_affine"])
                need("option input affine off", opts["input_bn"] and not opts["input_affine"])
            else:
                for m in (0.1, 0.5, 0.01):
                    need(f"momentum {m}", opts["bn"] and opts["momentum"] == m)
                need("a batch of 1 without batch norm", batch == 1)
                need("the cap of 1024 rows", batch == F.TRAIN_CAP)
                need("k0 + k1 no multiple of 4 at 1024 rows", batch == F.TRAIN_CAP and c["k1"] and (c["k0"] + c["k1"]) % 4)
            need("one input segment", c["k1"] == 0)
            need("two input segments", c["k1"] > 0)
        for k, misaligned in c["weights"]:
            need("K % 4 != 0", k % 4)
            need("K % 4 == 0 with a weight that is not 16-byte aligned", k % 4 == 0 and misaligned)
            need("K % 4 == 0 with an aligned weight", k % 4 == 0 and not misaligned)
        # (hk_pvnet_forward takes policy and value as columns of one record, but no input next to an output)
        for kind in F.INPUT_KINDS + (("record",) if family != "pvnet" else ()):
            need(f"an input laid out as {kind}", any(c["layout"][name].kind == kind for name in c["inputs"]))
        for kind in F.OUTPUT_KINDS + ("record",):
            if c["outputs"]:
                need(f"an output laid out as {kind}", any(c["layout"][name].kind == kind for name in c["outputs"]))
        for kind in ("fresh", "flat"):
            need(f"parameters {kind}", c["params"] == kind)
        for start in range(4):
            need(f"a flat buffer from element {start}", c["params"] == "flat" and c["start"] == start)
        need(f"depth {F.DEEP}", len(c["widths"]) - 1 == F.DEEP)
        need("a NaN", c["nonfinite"] is not None and c["nonfinite"][2] == "nan")
        need("an Inf", c["nonfinite"] is not None and c["nonfinite"][2] == "inf")
    return sorted(name for name, hit in want.items() if not hit)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_committed_slice_reaches_every_path(slices, family):
    assert missing(family, slices[family]) == []


def test_a_thin_slice_is_told_what_it_misses(slices):
    """the coverage list can fail: ten cases do not reach everything, and the list says what"""
    for family in FAMILIES:
        gaps = missing(family, slices[family][:10])
        assert gaps and all(isinstance(g, str) for g in gaps), family


@pytest.mark.parametrize("family", FAMILIES)
def test_degenerate_and_non_finite_shares(slices, family):
    """a net whose last hidden activations are all zero in some row tests nothing behind that point: at most 5 % of the
    slice, by the rule alone; cases with a NaN or an Inf are left out of that count and are at most 10 % themselves"""
    cases = slices[family]
    nonfinite = [c for c in cases if c["nonfinite"] is not None]
    finite = [c for c in cases if c["nonfinite"] is None]
    dead = [c["index"] for c in finite if F.degenerate(c)]
    print(f"{family}: {len(dead)} degenerate of {len(cases)} ({100 * len(dead) / len(cases):.2f} %): {dead}; "
          f"{len(nonfinite)} non-finite ({100 * len(nonfinite) / len(cases):.2f} %)")
    assert len(dead) <= DEGENERATE_CAP * len(cases), dead
    assert 0 < len(nonfinite) <= NONFINITE_CAP * len(cases)


# ---- the comparator can fail ---------------------------------------------------------------------------------------------

def _main(case):
    return "policy" if case["family"] == "pvnet" else "out"


def planted_case(family):
    """the first case of another seed with flat parameters, three rows or more and a NaN that the rule keeps to some rows
    of the output and not others; train's has a batch norm-free net (a batch norm spreads the NaN over the batch)"""
    for index in itertools.count():
        case = F.case_at(family, SEED + 1, index)
        if case["params"] != "flat" or case["batch"] < 3 or case["nonfinite"] is None or case["nonfinite"][2] != "nan":
            continue
        if family == "train" and case["options"]["bn"]:
            continue
        want = F.rule(case)
        out = want[_main(case)]
        rows = np.isnan(out).any(axis=1)
        if rows.any() and len({out[r].tobytes() for r in np.flatnonzero(np.isfinite(out).all(axis=1))}) >= 2:
            return case, want


def _flip_last_bit(case, got):
    out = got[_main(case)]
    at = tuple(np.argwhere(np.isfinite(out))[0])
    out.view(np.uint32)[at] ^= 1


def _swap_rows(case, got):
    out = got[_main(case)]
    rows = [r for r in range(len(out)) if np.isfinite(out[r]).all()]
    a, b = next((a, b) for a, b in itertools.combinations(rows, 2) if out[a].tobytes() != out[b].tobytes())
    out[[a, b]] = out[[b, a]]


def _sentinel(name):
    def plant(case, got):
        assert got[name][-1] == F.SENTINEL
        got[name][-1] = 0.0
    return plant


def _neighbour(case, got):
    flat = got["params"]
    first = F.leaves(case)[0].size
    assert flat[case["start"] + first - 1] != F.SENTINEL
    flat[case["start"] + first - 1] += 1.0  # the last element of the first tensor: the one before its neighbour


def _gradient_slot(case, got):
    g = got["grad0"].reshape(-1)
    i = next(i for i in range(len(g) - 1) if g[i] != g[i + 1] and np.isfinite(g[i:i + 2]).all())
    g[i + 1], g[i] = g[i], 0.0


def _gradient_slot_in_buffer(case, got):
    stats = F.leaves(case, True)
    at = F.positions([a.size for a in stats] + [int(np.prod(s)) for s in F.grad_shapes(case)], case["start2"], case["gaps2"])[0]
    g = got["written"][at[len(stats)]:]
    i = next(i for i in range(len(g) - 1) if g[i] != g[i + 1] and np.isfinite(g[i:i + 2]).all())
    g[i + 1], g[i] = g[i], 0.0


def _move_nan(case, got):
    out = got[_main(case)]
    rows = np.isnan(out).any(axis=1)
    src, dst = int(np.argmax(rows)), int(np.argmax(~rows))
    cols = np.isnan(out[src])
    out[src, cols], out[dst, cols] = 0.0, np.nan


@pytest.mark.parametrize("family", FAMILIES)
def test_the_comparator_fails_on_each_planted_deviation(family, tmp_path, monkeypatch):
    monkeypatch.setattr(F, "DUMP", str(tmp_path))
    case, want = planted_case(family)
    for name, a in want.items():
        a.setflags(write=False)
    F.compare(case, copy.deepcopy(want), want)  # the untouched copy passes
    stores = [k for k in want if k.endswith(".store")] + ["params"] + (["written"] if family == "train" else [])
    plants = [_flip_last_bit, _swap_rows, _neighbour, _move_nan] + [_sentinel(k) for k in stores]
    if family == "train":
        plants += [_gradient_slot, _gradient_slot_in_buffer]
    for plant in plants:
        got = {k: v.copy() for k, v in want.items()}
        plant(case, got)
        with pytest.raises(F.Mismatch) as e:
            F.compare(case, got, want)
        assert family.upper() in str(e.value) and f"case {case['index']} of seed {SEED + 1}" in str(e.value)
        assert "'batch'" in str(e.value) and (tmp_path / f"fuzz_nets_mismatch_{family}.npz").exists()
    # a name that one side lacks is a mismatch too
    with pytest.raises(F.Mismatch):
        F.compare(case, {k: v for k, v in want.items() if k != "params"}, want)


# ---- determinism -----------------------------------------------------------------------------------------------------------

def _arrays(obj, out):
    if isinstance(obj, np.ndarray):
        out.append(obj)
    elif isinstance(obj, dict):
        for k in obj:
            _arrays(obj[k], out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _arrays(v, out)
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_a_seed_gives_the_same_cases_and_the_rule_the_same_bits(slices, family):
    for index in (0, 1, 2, 3, COUNT[family] - 1):
        first, again = slices[family][index], F.case_at(family, SEED, index)
        assert repr(F.scalars(first)) == repr(F.scalars(again))
        a, b = _arrays(first, []), _arrays(again, [])
        assert len(a) == len(b) and all(F.same_bits(x, y) for x, y in zip(a, b))
        want, twice = F.rule(first), F.rule(again)
        assert list(want) == list(twice) and all(F.same_bits(want[k], twice[k]) for k in want)
    # ... the generator-taking form as well, and another seed gives other cases
    one, two = (F.draw(np.random.default_rng(5), family) for _ in range(2))
    assert repr(F.scalars(one)) == repr(F.scalars(two)) and F.same_bits(one["x"], two["x"])
    assert not F.same_bits(one["x"], F.draw(np.random.default_rng(6), family)["x"])
