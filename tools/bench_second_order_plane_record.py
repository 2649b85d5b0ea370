#!/usr/bin/env python3
"""Plane-sensor record of the 3-D exact k-space propagator on one GPU: SecondOrder.plane_record(times) against run(times)
with sensor_index set to the same plane — the only way to the same numbers without the record — and the record's parts
alone:

    python tools/bench_second_order_plane_record.py [--sides 128 256] [--times 256] [--reps 7] [--warmup 2]

--sides: the domain's side N and the expanded side E, in pairs (128 256 256 512: two points).  One JSON line per point and
medium (absorbing y = 1.5 at 0.75 dB/(MHz^1.5 cm), lossless): a domain N^3 in E^3 at 0.1 mm, the output times n dt with
dt = dx / c0, plane 0.  The two forms run in one process and alternate rep by rep after the warm-up rounds; figures are
medians with their range.

  record / run       the C entries kwh_second_order_plane_record (dst = NULL) and kwh_second_order_run, host clock around the
                     call and a synchronise of the context: the device work, no copy of the record
  record_copy / run_copy   plane_record(times) and run(times) of the Python class: the same with the record (n_times Ny Nx
                     floats either way) copied into a NumPy array
  set_p0 / set_p0_plain    set_p0 with the plane set (the fused forward, one 3-D rocFFT and the prepare) and without
  prepare, kernel, c2r_crop   kw_second_order_plane_prepare, kw_second_order_plane_record and, on a second context
                     (Ex, Ey, n_times), kw_fft_c2r_frames with kw_plane_recon_crop through the C ABI, device events
  kernel_gfma_s, kernel_gh_s   the record kernel's rate against its own counts: 2 Ey (Ex/2 + 1) (Ez/2 + 1) n_times fused
                     multiply-adds on complex values, and (Ex/2 + 1) (Ey/2 + 1) (Ez/2 + 1) n_times evaluations of H
  max_rel_diff       |plane_record - run| over max |run| on this run's data (the tests hold the 2e-5 bound in relative L2)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_second_order import ALPHA_COEFF, ALPHA_POWER, C0, DX, F32, capi, constants  # noqa: E402
from kwave_amd import second_order  # noqa: E402


def summary(name, v):
    return {name + "_ms": round(float(np.median(v)), 4), name + "_ms_min_max": [round(min(v), 4), round(max(v), 4)]}


def class_case(n, e, coeff, times, reps, warmup):
    """the two forms through SecondOrder, alternating"""
    p0 = np.random.default_rng(n).standard_normal((n, n, n)).astype(F32)
    kw = dict(alpha_coeff=coeff, alpha_power=ALPHA_POWER, expanded=(e, e, e), sensor_index=np.arange(n * n))
    p = second_order.SecondOrder((n, n, n), (DX, DX, DX), C0, plane=0, **kw)
    L, sync = second_order._lib(), lambda: capi.check(capi.load().kw_sync(p.ctx))
    tp = times.ctypes.data_as(C.POINTER(C.c_double))
    forms = {
        "record": lambda: second_order._check(L.kwh_second_order_plane_record(p._h, tp, times.size, None)),
        "run": lambda: second_order._check(L.kwh_second_order_run(p._h, tp, times.size)),
        "record_copy": lambda: p.plane_record(times),
        "run_copy": lambda: p.run(times),
        "set_p0": lambda: p.set_p0(p0),
    }
    out = {k: [] for k in forms}
    try:
        fused = p.fused
        p.set_p0(p0)
        rec, raw = p.plane_record(times), p.run(times).reshape(times.size, n, n)
        diff = float(np.abs(rec - raw).max() / np.abs(raw).max())
        for rep in range(warmup + reps):
            for name, fn in forms.items():
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                if rep >= warmup:
                    out[name].append((time.perf_counter() - t0) * 1e3)
        chunk = p.plane_chunk_times
    finally:
        p.close()
    plain = second_order.SecondOrder((n, n, n), (DX, DX, DX), C0, **kw)   # no plane: set_p0 as it was
    try:
        out["set_p0_plain"] = []
        for rep in range(warmup + reps):
            t0 = time.perf_counter()
            plain.set_p0(p0)
            capi.check(capi.load().kw_sync(plain.ctx))
            if rep >= warmup:
                out["set_p0_plain"].append((time.perf_counter() - t0) * 1e3)
    finally:
        plain.close()
    res = {"fused": fused, "plane_chunk_times": chunk, "max_rel_diff": float(f"{diff:.3e}")}
    for name, v in out.items():
        res.update(summary(name, v))
    res["run_over_record"] = round(res["run_ms"] / res["record_ms"], 1)
    res["run_copy_over_record_copy"] = round(res["run_copy_ms"] / res["record_copy_ms"], 1)
    return res


def parts_case(n, e, coeff, times, reps, warmup):
    """prepare, the record kernel, and the C2R with the crop, each alone, device events"""
    nxc, mf, nt = e // 2 + 1, e // 2 + 1, times.size
    vol_h = np.zeros((e, e, e), F32)
    vol_h[:n, :n, :n] = np.random.default_rng(n).standard_normal((n, n, n))
    op = capi.SecondOrderOp()
    op.dx = op.dy = op.dz = DX
    op.c0 = C0
    op.a = coeff * 100.0 * (1.0e-6 / (2.0 * np.pi)) ** ALPHA_POWER / (20.0 * np.log10(np.e))
    op.alpha_power, op.absorbing = ALPHA_POWER, int(coeff > 0.0)
    dev, d2 = capi.Device(), capi.Device()
    try:
        dev.set_constants(constants(e, e, e))
        dev.call("fft_create_plans_3d")
        vol, spec = dev.array(vol_h), dev.empty(2 * nxc * e * e)
        dev.call("fft_r2c_3d", vol, spec)
        q, g = dev.empty(2 * e * nxc * mf), dev.empty(2 * nt * e * nxc)
        tdev = dev.array(times)
        d2.set_constants(constants(e, e, nt))
        d2.call("fft_create_plans_frames")
        planes, crop = d2.empty(e * e * nt), d2.empty(n * n * nt)

        def c2r_crop():
            d2.call("fft_c2r_frames", g, planes)
            d2.call("plane_recon_crop", crop, planes, e, e, nt, n, n, nt, 0)

        parts = {"prepare": (dev, lambda: dev.call("second_order_plane_prepare", q, spec, 0)),
                 "kernel": (dev, lambda: dev.call("second_order_plane_record", g, q, C.byref(op), tdev, nt)),
                 "c2r_crop": (d2, c2r_crop)}
        ev = {k: (d.event(), d.event()) for k, (d, _) in parts.items()}
        out = {k: [] for k in parts}
        for rep in range(warmup + reps):
            for name, (d, fn) in parts.items():
                dev.sync()
                d2.sync()
                e0, e1 = ev[name]
                d.record(e0)
                fn()
                d.record(e1)
                d.sync()
                if rep >= warmup:
                    out[name].append(d.elapsed_ms(e0, e1))
    finally:
        dev.close()
        d2.close()
    res = {}
    for name, v in out.items():
        res.update(summary(name, v))
    fma, h = 2 * e * nxc * mf * nt, nxc * (e // 2 + 1) * mf * nt
    res.update({"kernel_fma": fma, "kernel_h": h, "kernel_gfma_s": round(fma / res["kernel_ms"] / 1e6, 1),
                "kernel_gh_s": round(h / res["kernel_ms"] / 1e6, 2)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--times", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts-only", action="store_true", help="the record's parts alone (no propagator)")
    args = ap.parse_args()
    if len(args.sides) % 2:
        ap.error("--sides takes pairs N E")
    times = np.ascontiguousarray(DX / C0 * np.arange(args.times), dtype=np.float64)
    for n, e in zip(args.sides[0::2], args.sides[1::2]):
        for coeff in (ALPHA_COEFF, 0.0):
            res = {"domain": n, "expanded": e, "n_times": args.times, "alpha_coeff": coeff, "reps": args.reps}
            if not args.parts_only:
                res.update(class_case(n, e, coeff, times, args.reps, args.warmup))
            res.update(parts_case(n, e, coeff, times, args.reps, args.warmup))
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
