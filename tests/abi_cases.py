"""What the CPU-side boundary tests share: reading a header of include/, the entry points it declares, and the layout
of its descriptors as the C compiler sees them."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

# the entry points a header declares: `int hk_...(`, `uint64_t hk_...(`, `const char* hk_...(` at the start of a line
DECLARED = re.compile(r"^(?:int|uint64_t|const char\*)\s+(hk_\w+)\(", flags=re.M)


def header(name="hironaka_hip.h"):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def declared(name="hironaka_hip.h"):
    return set(DECLARED.findall(header(name)))


def assert_layouts_match_c(structs, tmp_path):
    """sizeof/offsetof of every {struct name: ctypes class} as gcc sees them on include/hironaka_hip.h (as strict C,
    without a warning) == ctypes"""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "hironaka_hip.h"', 'int main(){']
    for s, cls in structs.items():
        src.append(f'printf("{s}.size %zu\\n", sizeof({s}));')
        src += [f'printf("{s}.{f[0]} %zu\\n", offsetof({s}, {f[0]}));' for f in cls._fields_]
    src.append('return 0;}')
    c, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(c, "w") as f:
        f.write("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert len(got) == sum(len(cls._fields_) + 1 for cls in structs.values())
    for s, cls in structs.items():
        assert int(got[f"{s}.size"]) == ctypes.sizeof(cls), s
        for f in cls._fields_:
            assert int(got[f"{s}.{f[0]}"]) == getattr(cls, f[0]).offset, (s, f[0])
