"""Which kernel serves a request, pinned without a GPU.

The selection -- the family (`pick`), the family's instantiation (its `*_variant`) and the grid (its `*_grid`) -- is
pure host code in headers: tests/kernel_selection.hip includes them, links nothing of the library and prints one line
per request of a fixed table.  Every family gives bit-identical results, so no parity test notices when a request
reaches another instantiation; this does."""
import os
import re
import subprocess

import level_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hironaka_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_selection.txt")


def test_selection_matches_the_golden_table(tmp_path):
    exe = str(tmp_path / "kernel_selection")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function",
                           "-I", CSRC, os.path.join(ROOT, "tests", "kernel_selection.hip"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # the table is the MI355X's: 1024 SIMDs
    proc = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    got = proc.stdout.splitlines()
    failed = [line for line in got if line.startswith("FAILED")]
    assert not failed, failed  # the program's own invariants: variant, grid, workspace bound
    assert proc.returncode == 0, proc.stderr
    want = open(GOLDEN).read().splitlines()
    changed = [(w, g) for w, g in zip(want, got) if w != g]
    assert not changed, changed[:10]
    assert len(got) == len(want)


def _macro_table(header, macro):
    text = open(os.path.join(CSRC, header)).read()
    body = re.search(r"#define %s\(X\)(.*)" % macro, text).group(1)
    return [(int(m), int(d)) for m, d in re.findall(r"X\((\d+), (\d+)\)", body)]


def _makefile_table(var):
    text = open(os.path.join(CSRC, "Makefile")).read()
    return [tuple(int(v) for v in s.split("_")) for s in re.search(r"^%s := (.*)$" % var, text, flags=re.M).group(1).split()]


def test_the_three_copies_of_the_spec_tables_agree():
    fast = _macro_table("hk_fast_kernel.h", "HK_FAST_SPECS")
    quad = _macro_table("hk_quad_kernel.h", "HK_QUAD_SPECS")
    assert len(fast) == 7 and len(quad) == 4
    assert _makefile_table("FAST_SPECS") == fast
    assert _makefile_table("QUAD_SPECS") == quad
    assert level_cases.ROLLOUT_SHAPES["one"] == fast
    assert level_cases.ROLLOUT_SHAPES["four"] == quad
    # the two-lane kernels are those of the one-lane table of at most 32 rows (hk_duo_kernel.h: duo_supported)
    assert set(level_cases.ROLLOUT_SHAPES["two"]) <= {s for s in fast if s[0] <= 32}
