"""Time of an off-grid array build: 64 discs of 5 mm diameter on a 256^3 grid at dx = 0.2 mm, built
by arrays.offgrid_elements on the GPU, beside the float64 NumPy reference of the tests for ONE of those elements on the
same box.  Prints one JSON line.

    python tools/offgrid_build_time.py [--elements 64] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kwave_amd  # noqa: E402,F401
from kwave_amd import arrays, capi  # noqa: E402
from offgrid_reference import reference_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    n, dx = 256, 2.0e-4
    grid = arrays.Grid(n, n, n, dx, dx, dx)
    side = int(np.ceil(np.sqrt(a.elements)))
    pitch = 6.0e-3                                       # 5 mm discs on a 6 mm lattice in the plane z = 0.13 mm
    shapes = []
    for e in range(a.elements):
        cx, cy = ((e % side) - (side - 1) / 2) * pitch, ((e // side) - (side - 1) / 2) * pitch
        shapes.append(arrays.disc_element(grid, (cx + 0.3e-4, cy - 0.7e-4, 1.3e-4), 2.5e-3, (0.1, 0.2, 1.0)))
    points = sum(len(s[0]) for s in shapes)
    dev = capi.Device()
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        els = arrays.offgrid_elements(dev, grid, shapes)
        times.append(time.perf_counter() - t0)
    # the device call alone (the Python layer converts coordinates before it and slices the rows after it)
    coords = np.concatenate([arrays.grid_units(grid, s[0]) for s in shapes])
    ptr = np.concatenate([[0], np.cumsum([len(s[0]) for s in shapes])]).astype(np.uint64)
    scale = np.array([s[1] / dx ** 2 / len(s[0]) for s in shapes], dtype=np.float32)
    call = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        capi.offgrid_build(dev, coords, ptr, scale, (n, n, n))
        call.append(time.perf_counter() - t0)
    nnz = sum(i.size for i, _ in els)
    stencil = 15 ** 3
    out = {"grid": n, "elements": a.elements, "points": points, "entries": nnz, "contributions": points * stencil,
           "offgrid_elements_s": [round(t, 4) for t in times], "kw_offgrid_build_s": [round(t, 4) for t in call],
           "contributions_per_s_best_call": round(points * stencil / min(call), 0)}
    if not a.no_reference:
        one = arrays.grid_units(grid, shapes[0][0])
        t0 = time.perf_counter()
        W, _ = reference_weights(one, [0, len(one)], scale[:1], (n, n, n), 0.05)
        out["numpy_reference_one_element_s"] = round(time.perf_counter() - t0, 3)
        idx, w = els[0]
        out["one_element_max_abs_diff"] = float(np.max(np.abs(W[0, idx] - w)))
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
