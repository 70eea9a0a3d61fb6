"""
Generate tests/golden/cpputil_newton_approx.npz: the inputs of tests/test_oracle.py::test_native_reference_cpputil
and what the reference's native getNewtonPolytope_approx (hironaka/cpp/cppUtil.cpp:58-61, built by
`make -C oracle ref` into oracle/_ref/cppUtil.so) returns for them.  The .npz holds plain input/output
arrays, so the test runs wherever the repository is, with or without the reference tree.

Usage:  python tests/golden/make_cpputil_golden.py
"""
import ctypes
import os

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))


def inputs():
    """games with >= 2 points and no duplicate rows (where the routine is right), rows shuffled"""
    rng = np.random.default_rng(5)
    b, m, d = 200, 8, 3
    pts = np.full((b, m, d), -1, dtype=np.int64)
    for g in range(b):
        n = int(rng.integers(2, m + 1))
        rows = set()
        while len(rows) < n:
            rows.add(tuple(rng.integers(0, 9, d).tolist()))
        pts[g, :n] = np.array(sorted(rows, key=lambda _: rng.random()))
    return pts


def run_native(path, pts):
    ref = ctypes.CDLL(path)
    ref.getNewtonPolytope_approx.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    ref.getNewtonPolytope_approx.restype = None
    b, m, d = pts.shape
    out = np.full_like(pts, -1)
    ref.getNewtonPolytope_approx(pts.ctypes.data, b, m, d, out.ctypes.data)
    return out


def main():
    path = os.path.join(ROOT, "oracle", "_ref", "cppUtil.so")
    if not os.path.exists(path):
        raise SystemExit(f"{path} missing: build it next to the reference with `make -C oracle ref`")
    pts = inputs()
    np.savez_compressed(os.path.join(OUT, "cpputil_newton_approx.npz"), points=pts, out=run_native(path, pts))
    print("wrote cpputil_newton_approx.npz")


if __name__ == "__main__":
    main()
