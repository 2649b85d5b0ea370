#!/usr/bin/env python3
"""The delayed element kernels against the undelayed ones, on the 256^3 array of tools/velocity_element_compare.py
(128 elements, each a 10 x 14 x 14 block of about 2 000 grid points, 250 880 entries).

Kernels (same library, same device buffers, the forms alternating, HIP events around `--calls` back-to-back calls,
`--rounds` rounds; the median round in microseconds per call, with the minimum and maximum):

  sample   kw_sample_elements_multi(3)  against  kw_sample_elements_delayed(3) at max delay 0, 16 and 256
  source   kw_element_source_rows       against  kw_element_source_rows_delayed (max delay 16)

The delays focus the array at a point: d = round(max delay * (r_max - r) / (r_max - r_min)) with r the distance of the
entry's grid point from the focus, so an element's delays are as smooth as those of arrays.focus_delays.

Sizes, from the datasets themselves: the device bytes of the rings (R * E * fields * 4), and the input and output of a
focused array driven from one signal and read as one scan line (one element holding every point, per-point delays)
against its expanded form (one series per point, -p over every point).  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from element_array_compare import array_elements  # noqa: E402
from velocity_element_compare import _summary, _time_calls  # noqa: E402

FOCUS = (128.0, 128.0, 200.0)   # grid units


def focus_like_delays(els, n: int, top: int):
    """one int64 array per element: 0 at the farthest point of the array, `top` at the nearest"""
    if top == 0:
        return [np.zeros(len(i), np.int64) for i, _ in els]
    r = [np.sqrt((i % n - FOCUS[0]) ** 2 + (i // n % n - FOCUS[1]) ** 2 + (i // (n * n) - FOCUS[2]) ** 2) for i, _ in els]
    lo, hi = min(x.min() for x in r), max(x.max() for x in r)
    return [np.round(top * (hi - x) / (hi - lo)).astype(np.int64) for x in r]


def regroup(ptr, delays):
    """the regrouping of the header: (order, group_ptr, group_delay, element_group_ptr)"""
    order, gptr, gdelay, egp = [], [0], [], [0]
    for r in range(len(ptr) - 1):
        d = delays[ptr[r]:ptr[r + 1]]
        o = np.argsort(d, kind="stable")
        order.append(ptr[r] + o)
        ends = np.nonzero(np.diff(d[o], append=-1))[0]
        gdelay += d[o][ends].tolist()
        gptr += (ptr[r] + ends + 1).tolist()
        egp.append(len(gdelay))
    return np.concatenate(order), np.array(gptr, np.int64), np.array(gdelay, np.int64), np.array(egp, np.int64)


def kernels(capi, arrays, n: int, els, calls: int, rounds: int) -> dict:
    rng = np.random.default_rng(2)
    n_el, nt = len(els), 8
    d = capi.Device()
    keep = []

    def up(a, dtype):
        b = d.empty(int(np.asarray(a).size), dtype)
        b.upload(np.ascontiguousarray(a, dtype=dtype).reshape(-1))
        keep.append(b)
        return b.ptr

    def ptrs(v):
        return (C.c_void_p * len(v))(*v)
    try:
        sen = arrays.weighted_sensor(els)
        sp = sen["sensor_element_ptr"].reshape(-1).astype(np.int64)
        cols = sen["sensor_element_index"].reshape(-1).astype(np.int64) - 1
        w = sen["sensor_element_weight"].reshape(-1)
        nnz = int(sp[-1])
        fields = [up(rng.standard_normal(n ** 3).astype(np.float32), np.float32) for _ in range(3)]
        outs = [up(np.zeros(n_el, np.float32), np.float32) for _ in range(3)]
        outs_p, fields_p = ptrs(outs), ptrs(fields)
        cp = capi.element_chunk_ptr(sp)
        s_ptr, s_cp, s_ent = up(sp, np.uint32), up(cp, np.uint32), up(capi.csr_entries(cols, w), np.uint32)
        part = up(np.zeros(3 * int(cp[-1]), np.float32), np.float32)

        def sample_multi():
            capi.check(d.L.kw_sample_elements_multi(d.ctx, 3, outs_p, fields_p, s_ptr, s_ent, n_el, nnz, s_cp, int(cp[-1]), part))

        forms = {"multi": sample_multi}
        out = {"nnz_sensor": nnz, "chunks": int(cp[-1]), "calls": calls, "rounds": rounds, "sample": {}, "ring_bytes": {}}
        for top in (0, 16, 256):
            delays = np.concatenate(focus_like_delays(els, n, top))
            order, gptr, gdelay, egp = regroup(sp, delays)
            gcp = capi.element_chunk_ptr(gptr)
            rows = top + 1
            g = [up(gptr, np.uint32), up(capi.csr_entries(cols[order], w[order]), np.uint32), up(gdelay, np.uint32),
                 up(egp, np.uint32), up(gcp, np.uint32), up(np.zeros(3 * int(gcp[-1]), np.float32), np.float32)]
            rings = ptrs([up(np.zeros(rows * n_el, np.float32), np.float32) for _ in range(3)])
            step = [0]

            def sample_delayed(g=g, rings=rings, rows=rows, groups=len(gdelay), chunks=int(gcp[-1]), step=step):
                capi.check(d.L.kw_sample_elements_delayed(d.ctx, 3, outs_p, fields_p, g[0], g[1], g[2], g[3], n_el, groups, nnz,
                                                          g[4], chunks, g[5], rings, rows, step[0]))
                step[0] += 1
            forms[f"delayed_{top}"] = sample_delayed
            out["sample"][f"delayed_{top}"] = {"groups": len(gdelay), "chunks": int(gcp[-1])}
            out["ring_bytes"][str(top)] = rows * n_el * 3 * 4
        times = {name: [] for name in forms}
        for fn in forms.values():          # warm-up: code objects loaded, caches in their steady state
            _time_calls(capi, d, fn, calls)
        for _ in range(rounds):            # alternating
            for name, fn in forms.items():
                times[name].append(_time_calls(capi, d, fn, calls))
        for name in forms:
            out["sample"].setdefault(name, {}).update(_summary(times[name]))

        # source side: the three components, delays up to 16
        sig = [rng.standard_normal((nt, n_el)).astype(np.float32) for _ in range(3)]
        src = arrays.weighted_velocity_source(els, *sig, delays=focus_like_delays(els, n, 16))
        up_ptr = src["u_source_element_ptr"].reshape(-1).astype(np.int64)
        n_pts = up_ptr.size - 1
        u_ptr = up(up_ptr, np.uint32)
        u_ent = up(capi.csr_entries(src["u_source_element_index"].reshape(-1).astype(np.int64) - 1,
                                    src["u_source_element_weight"].reshape(-1)), np.uint32)
        u_del = up(src["u_source_element_delay"].reshape(-1), np.uint32)
        sigs_p = ptrs([up(s, np.float32) for s in sig])
        rows_p = ptrs([up(np.zeros(n_pts, np.float32), np.float32) for _ in range(3)])
        steps3 = (C.c_uint64 * 3)(nt, nt, nt)

        def source_rows():
            capi.check(d.L.kw_element_source_rows(d.ctx, rows_p, sigs_p, u_ptr, u_ent, n_pts, n_el, 3))

        def source_delayed():   # time index 12: part of the entries inside the signals, part before or past them
            capi.check(d.L.kw_element_source_rows_delayed(d.ctx, rows_p, sigs_p, steps3, u_ptr, u_ent, u_del, n_pts, n_el, 12))
        for fn in (source_rows, source_delayed):
            _time_calls(capi, d, fn, calls)
        t_rows, t_del = [], []
        for _ in range(rounds):
            t_rows.append(_time_calls(capi, d, source_rows, calls))
            t_del.append(_time_calls(capi, d, source_delayed, calls))
        out["source"] = {"points": n_pts, "nnz": int(up_ptr[-1]), "rows": _summary(t_rows), "delayed_16": _summary(t_del)}
        return out
    finally:
        d.close()


def sizes(arrays, n: int, els, nt_src: int, top: int) -> dict:
    """one element holding every point of the array, driven from one signal and read as one scan line"""
    pts = np.unique(np.concatenate([i for i, _ in els]))
    one = [(pts, np.ones(pts.size, np.float32))]
    delays = focus_like_delays(one, n, top)
    src = arrays.weighted_source(one, np.zeros((nt_src, 1), np.float32), delays=delays)
    sen = arrays.weighted_sensor(one, delays=delays)
    exp = arrays.expand_source(src)
    return {"points": int(pts.size), "signal_steps": nt_src, "max_delay": top,
            "focused_input_bytes": int(sum(v.nbytes for k, v in src.items() if "_source_element_" in k)),
            "expanded_input_bytes": int(exp.nbytes),
            "sensor_bytes": int(sum(v.nbytes for v in sen.values())),
            "focused_output_bytes_per_step": 4, "expanded_output_bytes_per_step": int(pts.size) * 4,
            "ring_bytes": (top + 1) * 1 * 1 * 4}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=("kernels", "sizes"))
    a = ap.parse_args()
    import kwave_amd  # noqa: F401
    from kwave_amd import arrays, capi

    n = 256
    els = array_elements(n, np.random.default_rng(1))
    out = {"grid": n, "elements": len(els)}
    if a.only in (None, "sizes"):
        out["sizes"] = sizes(arrays, n, els, 128, 256)
    if a.only in (None, "kernels"):
        out["kernels"] = kernels(capi, arrays, n, els, a.calls, a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
