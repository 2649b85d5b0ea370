#!/usr/bin/env python3
"""Weighted velocity transducer array against its expanded form, and the multi-field kernels against the one-field calls
they replace, on one 256^3 heterogeneous absorbing problem.

The array is the one of tools/element_array_compare.py: 128 elements, each a 10 x 14 x 14 block of about 2 000 grid points
with random weights.  It drives ux, uy and uz (additive, k-space corrected) and is recorded:

  expanded  ux/uy/uz_source_input = one series per point and component (u_source_many = 1), -u over every point
  weighted  u_source_element_* (CSR weights) + ux/uy/uz_source_element_input (128 signals each), --u_elements

Kernels (same library, same device buffers, the two forms alternating, HIP events around `--calls` back-to-back calls,
`--rounds` rounds; reported as the median round in microseconds per call, with the minimum and maximum):

  sample   kw_sample_elements_multi(3)  against  3 x kw_sample_elements
  source   kw_element_source_rows       against  3 x kw_element_source_row

Steps: ms/step from HIP events on the solver's stream over the timed steps (the source is active in every one), the bytes
of the source input datasets and the output bytes per step, from the datasets themselves.  Prints one JSON line.
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


def _time_calls(capi, d, fn, calls: int) -> float:
    """microseconds per call of fn(), `calls` of them between two events on the context's stream"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    capi.check(d.L.kw_event_create(d.ctx, C.byref(e0)))
    capi.check(d.L.kw_event_create(d.ctx, C.byref(e1)))
    capi.check(d.L.kw_event_record(d.ctx, e0))
    for _ in range(calls):
        fn()
    capi.check(d.L.kw_event_record(d.ctx, e1))
    capi.check(d.L.kw_event_synchronize(d.ctx, e1))
    ms = C.c_float()
    capi.check(d.L.kw_event_elapsed_ms(d.ctx, e0, e1, C.byref(ms)))
    d.L.kw_event_destroy(d.ctx, e0)
    d.L.kw_event_destroy(d.ctx, e1)
    return 1000.0 * float(ms.value) / calls


def _summary(us):
    us = sorted(us)
    return {"median_us": us[len(us) // 2], "min_us": us[0], "max_us": us[-1]}


def kernels(capi, arrays, n: int, els, calls: int, rounds: int) -> dict:
    rng = np.random.default_rng(2)
    n_el, nt = len(els), 8
    sig = [rng.standard_normal((nt, n_el)).astype(np.float32) for _ in range(3)]
    src = arrays.weighted_velocity_source(els, *sig)
    sen = arrays.weighted_sensor(els)
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
        # sensor side
        sp = sen["sensor_element_ptr"].reshape(-1).astype(np.int64)
        cp = capi.element_chunk_ptr(sp)
        n_chunks, nnz = int(cp[-1]), int(sp[-1])
        s_ptr, s_cp = up(sp, np.uint32), up(cp, np.uint32)
        s_ent = up(capi.csr_entries(sen["sensor_element_index"].reshape(-1).astype(np.int64) - 1,
                                    sen["sensor_element_weight"].reshape(-1)), np.uint32)
        fields = [up(rng.standard_normal(n ** 3).astype(np.float32), np.float32) for _ in range(3)]
        outs = [up(np.zeros(n_el, np.float32), np.float32) for _ in range(3)]
        part = up(np.zeros(3 * n_chunks, np.float32), np.float32)
        outs_p, fields_p = ptrs(outs), ptrs(fields)

        def sample_multi():
            capi.check(d.L.kw_sample_elements_multi(d.ctx, 3, outs_p, fields_p, s_ptr, s_ent, n_el, nnz, s_cp, n_chunks, part))

        def sample_three():
            for f in range(3):
                capi.check(d.L.kw_sample_elements(d.ctx, outs[f], fields[f], s_ptr, s_ent, n_el, nnz, s_cp, n_chunks, part))
        # source side
        up_ptr = src["u_source_element_ptr"].reshape(-1).astype(np.int64)
        n_pts = up_ptr.size - 1
        u_ptr = up(up_ptr, np.uint32)
        u_ent = up(capi.csr_entries(src["u_source_element_index"].reshape(-1).astype(np.int64) - 1,
                                    src["u_source_element_weight"].reshape(-1)), np.uint32)
        sigs = [up(s, np.float32) for s in sig]
        rows = [up(np.zeros(n_pts, np.float32), np.float32) for _ in range(3)]
        rows_p, sigs_p = ptrs(rows), ptrs(sigs)

        def source_multi():
            capi.check(d.L.kw_element_source_rows(d.ctx, rows_p, sigs_p, u_ptr, u_ent, n_pts, n_el, 3))

        def source_three():
            for c in range(3):
                capi.check(d.L.kw_element_source_row(d.ctx, rows[c], sigs[c], u_ptr, u_ent, n_pts, n_el, 3))
        out = {"points": n_pts, "nnz_source": int(up_ptr[-1]), "nnz_sensor": nnz, "chunks": n_chunks, "calls": calls,
               "rounds": rounds}
        for name, multi, three in (("sample", sample_multi, sample_three), ("source", source_multi, source_three)):
            for fn in (multi, three):      # warm-up: code objects loaded, caches in their steady state
                _time_calls(capi, d, fn, calls)
            t_multi, t_three = [], []
            for _ in range(rounds):        # alternating
                t_multi.append(_time_calls(capi, d, multi, calls))
                t_three.append(_time_calls(capi, d, three, calls))
            out[name] = {"multi": _summary(t_multi), "three_calls": _summary(t_three)}
        return out
    finally:
        d.close()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=("kernels", "steps"))
    a = ap.parse_args()
    import kwave_amd  # noqa: F401
    from kwave_amd import arrays, capi, synthetic
    from kwave_amd.solver import HostSolver

    n, nt = 256, a.warmup + a.steps
    rng = np.random.default_rng(1)
    els = array_elements(n, rng)
    out = {"grid": n, "elements": len(els), "steps": a.steps}
    if a.only in (None, "kernels"):
        out["kernels"] = kernels(capi, arrays, n, els, a.calls, a.rounds)
    if a.only in (None, "steps"):
        base = synthetic.make_problem(n, heterogeneous=True, nonlinear=True, absorbing=True, source="none", nt=nt, pml_size=10)
        t = np.arange(nt)[:, None]
        sig = [(1.0e-2 * np.sin(2 * np.pi * 0.05 * t + 0.1 * np.arange(len(els))[None, :] + c)).astype(np.float32)
               for c in range(3)]
        src = arrays.weighted_velocity_source(els, *sig)
        sen = arrays.weighted_sensor(els)
        npts = int(src["u_source_index"].size)
        out["points"] = npts
        mode = {"u_source_mode": np.array([[[2]]], dtype=np.uint64)}
        expanded = dict(base)
        expanded.update({k: v for k, v in src.items() if "_source_element_" not in k})
        expanded.update(arrays.expand_velocity_source(src))
        expanded.update(mode)
        expanded["sensor_mask_index"] = src["u_source_index"]
        weighted = dict(base)
        weighted.update(src)
        weighted.update(sen)
        weighted.update(mode)
        in_exp = sum(expanded[f"u{c}_source_input"].nbytes for c in "xyz")
        in_wtd = sum(src[k].nbytes for k in src if "_source_element_" in k)
        runs = {"expanded": (expanded, dict(u_raw=1), in_exp, 3 * npts * 4),
                "weighted": (weighted, dict(u_elements=1), in_wtd, 3 * len(els) * 4)}
        res = {name: [] for name in runs}
        for _ in range(2):                 # alternating, two runs of each form
            for name, (pr, flags, _, _) in runs.items():
                g = HostSolver(pr, **flags)
                g.run(a.warmup)
                g.sync()
                res[name].append(g.time_steps(a.steps) / a.steps)
                g.finish()
                fused = g.scalar("fused_pipeline")
                g.close()
                out.setdefault("fused_pipeline", fused)
        for name, (_, _, in_bytes, row_bytes) in runs.items():
            out[name] = {"ms_per_step": res[name], "source_input_bytes": int(in_bytes), "output_bytes_per_step": int(row_bytes)}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
