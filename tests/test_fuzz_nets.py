"""tests/fuzz_nets.py without a GPU, for all five families: what the slice that tests/test_gpu_fuzz_nets.py commits reaches,
how many of its cases are degenerate (by the rule alone), that the comparison can fail on each kind of deviation, and that
a seed gives the same cases and the rule the same bits."""
import copy
import itertools

import numpy as np
import pytest

import customnet_rules as C
import fuzz_nets as F
from test_gpu_fuzz_nets import COUNT, SEED

FAMILIES = list(COUNT)
DEGENERATE_CAP, NONFINITE_CAP = 0.05, 0.10


@pytest.fixture(scope="module")
def slices():
    return {family: [F.case_at(family, SEED, i) for i in range(COUNT[family])] for family in FAMILIES}


def _blocks(case):
    """(kind, k, n) of every block of a pvnet, pvgrad or customnet case (customnet: of the last tower)"""
    return [(kind, k, n) for kind, k, n in zip(case["kinds"], case["widths"][:-1], case["widths"][1:])]


def _non_finite(case):
    """what the case planted that is no finite number"""
    planted = case["nonfinite"]
    if planted is None or case["family"] != "customnet":
        return [] if planted is None else [planted]
    return [p for p in planted if p[2] in ("nan", "+inf", "-inf")]


def missing(family, cases):
    """what the issue asks a slice to reach and this one does not"""
    want = {}

    def need(name, hit):
        want[name] = want.get(name, False) or bool(hit)
    for c in cases:
        opts, batch = c["options"], c["batch"]
        if family in ("mlp", "pvnet"):
            for tile in (16, 64):
                for name, b in (("below", tile - 1), ("at", tile), ("one past", tile + 1)):
                    need(f"forced tile {tile} with a batch {name} the tile", c["tile"] == tile and batch == b)
        if family in ("mlp", "pvnet", "customnet"):
            need("the library's own tile", c["tile"] is None)
        if family in ("pvnet", "pvgrad", "customnet"):
            blocks = _blocks(c)
            need("255 actions", c["actions"] == 255)
            need("no bias", not opts["bias"])
            for name in ("bias", "scale_on", "scale_off", "shift_on", "shift_off"):
                need(f"option {name}", opts[name])
        if family in ("pvnet", "pvgrad"):
            for n in F.NORMED:
                # (pvgrad: in front of a 32-wide block with a projection every gradient is zero by the rule -- such a case
                # is degenerate, drawn seldom and not asked for)
                if (family, n) != ("pvgrad", 32):
                    need(f"normed width {n} with a projection", ("residue", n) in [(kd, w) for kd, k, w in blocks if k != w])
                need(f"normed width {n} without a projection", ("residue", n, n) in blocks)
            need("a dense block narrower than 16", any(kd == "dense" and n < 16 for kd, _, n in blocks))
            need("a dense block of width 256", any(kd == "dense" and n == 256 for kd, _, n in blocks))
        if family in ("pvgrad", "customnet"):
            need("a group norm with a scale and no shift", opts["scale_alone"])
            need("a group norm with a shift and no scale", opts["shift_alone"])
            for eps in (F.P.EPS, 1e-5):
                need(f"eps {eps}", c["eps"] == eps and "residue" in c["kinds"])
        if family == "pvgrad":
            for b in F.PVGRAD_BATCHES:
                need(f"a batch of {b}", batch == b)
            need(f"{F.PVGRAD_TABLE} Denses: the parameter table full", c["denses"] == F.PVGRAD_TABLE)
            need(f"{F.PVGRAD_TABLE + 1} Denses: one in the second launch", c["denses"] == F.PVGRAD_TABLE + 1)
            need("more than two launches of the parameter table", c["denses"] > 2 * F.PVGRAD_TABLE)
            for kind in ("mean", "sparse"):
                need(f"gradients at the outputs: {kind}", c["grad_kind"] == kind)
            for kind in ("own", "flat"):
                need(f"gradients written to a buffer: {kind}", c["grads"] == kind)
            for start in range(4):
                need(f"the gradients' flat buffer from element {start}", c["grads"] == "flat" and c["start2"] == start)
            for name in ("grad_policy", "grad_value"):
                for kind in F.OUTPUT_KINDS + ("record",):
                    need(f"{name} laid out as {kind}", c["layout"][name].kind == kind)
            lay = c["layout"]["x0"]
            need("a strided x whose stride is not its width", lay.kind in ("stride", "record") and lay.stride != c["k0"] and batch > 1)
            need("a strided x at more than 1 000 rows", lay.kind in ("stride", "record") and lay.stride != c["k0"] and batch > 1000)
        elif family == "customnet":
            m, d, e = c["m"], c["d"], c["e"]
            for v in F.POINTS:
                need(f"m = {v}", m == v)
            for v in F.DIMS:
                need(f"d = {v}", d == v)
            need("e == 0", e == 0)
            need("e > 0", e > 0)
            for s in F.STRUCTURES:
                need(f"counts: {s}", c["structure"] == s)
            need("holes among the points", c["holes"])
            planted = c["nonfinite"] or ()
            for kind in F.EDGES:
                need(f"coordinate 0 of a point slot is {kind}", planted and planted[0][2] == kind)
            need("a NaN or an Inf in another column as well", len(planted) > 1)
            groups = np.bincount(C.counts(c["x"], m, d), minlength=m + 1)  # the rows of every count, by the rule
            for tile in (16, 64):
                for name, b in (("one below", tile - 1), ("at", tile), ("one past", tile + 1)):
                    need(f"forced tile {tile} with a group {name} the tile", c["tile"] == tile and b in groups)
            need("more than 1 024 rows", batch > 1024)
            need("empty groups between full ones", (np.diff(np.flatnonzero(groups)) > 1).any())
            for kind in ("residue", "dense"):
                need(f"a {kind} block", kind in c["kinds"])
            need("a dense block of a width that is no multiple of 16", any(kd == "dense" and n % 16 for kd, _, n in blocks))
            need("a head width that is no multiple of 16", (c["widths"][-1] + e) % 16)
        elif family != "pvnet":
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
        # (hk_pvnet_forward and hk_customnet_forward take policy and value as columns of one record, but no input next to
        # an output)
        for kind in F.INPUT_KINDS + (("record",) if family not in ("pvnet", "customnet") else ()):
            need(f"an input laid out as {kind}", any(c["layout"][name].kind == kind for name in c["inputs"]))
        for kind in F.OUTPUT_KINDS + ("record",):
            if c["outputs"]:
                need(f"an output laid out as {kind}", any(c["layout"][name].kind == kind for name in c["outputs"]))
        for kind in ("fresh", "flat"):
            need(f"parameters {kind}", c["params"] == kind)
        for start in range(4):
            need(f"a flat buffer from element {start}", c["params"] == "flat" and c["start"] == start)
        if family != "customnet":  # (a tower has one to three blocks)
            need(f"depth {F.DEEP}", len(c["widths"]) - 1 == F.DEEP)
        if family != "pvgrad":  # (finite only)
            need("a NaN", any(p[2] == "nan" for p in _non_finite(c)))
            need("an Inf", any(p[2] in ("inf", "+inf", "-inf") for p in _non_finite(c)))
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
    """a net whose last hidden activations are all zero in some row tests nothing behind that point (customnet: a row with
    a tower; pvgrad as well: a first block whose weight gets a gradient of zeros): at most 5 % of the slice, by the rule
    alone; cases with a NaN or an Inf are left out of that count and are at most 10 % themselves -- pvgrad has none"""
    cases = slices[family]
    nonfinite = [c for c in cases if _non_finite(c)]
    finite = [c for c in cases if not _non_finite(c)]
    dead = [c["index"] for c in finite if F.degenerate(c)]
    print(f"{family}: {len(dead)} degenerate of {len(cases)} ({100 * len(dead) / len(cases):.2f} %): {dead}; "
          f"{len(nonfinite)} non-finite ({100 * len(nonfinite) / len(cases):.2f} %)")
    assert len(dead) <= DEGENERATE_CAP * len(cases), dead
    if family == "pvgrad":
        assert not nonfinite and all(c["nonfinite"] is None and np.isfinite(c["x"]).all() for c in cases)
    else:
        assert 0 < len(nonfinite) <= NONFINITE_CAP * len(cases)
    if family == "customnet":  # rows without a tower are zero by design: the structure that has no others stays a small share
        assert sum(c["structure"] == "no tower" for c in cases) <= DEGENERATE_CAP * len(cases)


# ---- the comparator can fail ---------------------------------------------------------------------------------------------

def _main(case):
    return "out" if case["family"] in ("mlp", "train") else "policy"


def planted_case(family):
    """the first case of another seed with flat parameters, three rows or more and a NaN that the rule keeps to some rows
    of the output and not others; train's has a batch norm-free net (a batch norm spreads the NaN over the batch);
    pvgrad's has no NaN, its gradients in a flat buffer and rows that differ"""
    for index in itertools.count():
        case = F.case_at(family, SEED + 1, index)
        if case["params"] != "flat" or case["batch"] < 3:
            continue
        if family == "pvgrad":
            if case["grads"] != "flat" or case["layout"]["x0"].kind == "broadcast":
                continue
            return case, F.rule(case)
        if not any(p[2] == "nan" for p in _non_finite(case)):
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


def _moved_slot(g):
    i = next(i for i in range(len(g) - 1) if g[i] != g[i + 1] and np.isfinite(g[i:i + 2]).all())
    g[i + 1], g[i] = g[i], 0.0


def _gradient_slot(case, got):
    # (the first gradient that is not all alike: a 32-wide residue block's weight gets zeros)
    _moved_slot(next(g for g in (got[f"grad{j}"].reshape(-1) for j in itertools.count()) if len(set(g.tolist())) > 1))


def _gradient_slot_in_buffer(case, got):
    stats = F.leaves(case, True)
    at = F.positions([a.size for a in stats] + [int(np.prod(s)) for s in F.grad_shapes(case)], case["start2"], case["gaps2"])[0]
    _moved_slot(got["written"][at[len(stats)]:])


def _move_nan(case, got):
    out = got[_main(case)]
    rows = np.isnan(out).any(axis=1)
    src, dst = int(np.argmax(rows)), int(np.argmax(~rows))
    cols = np.isnan(out[src])
    out[src, cols], out[dst, cols] = 0.0, np.nan


def _workspace_counter(case, got):
    got["workspace"][1 + case["m"]] = 1  # the histogram's word of the rows without a tower


@pytest.mark.parametrize("family", FAMILIES)
def test_the_comparator_fails_on_each_planted_deviation(family, tmp_path, monkeypatch):
    monkeypatch.setattr(F, "DUMP", str(tmp_path))
    case, want = planted_case(family)
    for name, a in want.items():
        a.setflags(write=False)
    F.compare(case, copy.deepcopy(want), want)  # the untouched copy passes
    stores = [k for k in want if k.endswith(".store")] + ["params"] + (["written"] if family in ("train", "pvgrad") else [])
    plants = [_flip_last_bit, _swap_rows, _neighbour] + [_sentinel(k) for k in stores]
    if family != "pvgrad":
        plants.append(_move_nan)
    if family in ("train", "pvgrad"):
        plants += [_gradient_slot, _gradient_slot_in_buffer]
    if family == "customnet":
        plants.append(_workspace_counter)
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


# sha256 over the dtype, shape and bytes of every array of every case of the slices of the first three families, taken at
# the commit before pvgrad and customnet were added (250, 160 and 95 cases of SEED)
BEFORE = {"mlp": "93e6178336540be238adba461faa35e6aa8d167f51a70ea36446f5972315ef29",
          "train": "8f93f5ef318c820a1e68ab6b988608ca58082d4f9985262a1d285792066ea7d2",
          "pvnet": "dc92be7a38ae1d3dfdcc382c71c2888a5e8214c5bcd70bf6158b5348b69d8be1"}


def test_the_families_before_these_keep_their_cases(slices):
    """case_rng seeds by a family's index in FAMILIES: the new ones stand behind the three whose slices were committed
    before them, and those draw what they drew"""
    import hashlib
    assert F.FAMILIES[:3] == ("mlp", "train", "pvnet") and (COUNT["mlp"], COUNT["train"], COUNT["pvnet"]) == (250, 160, 95)
    for family, before in BEFORE.items():
        h = hashlib.sha256()
        for case in slices[family]:
            for a in _arrays(case, []):
                h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
        assert h.hexdigest() == before, family
