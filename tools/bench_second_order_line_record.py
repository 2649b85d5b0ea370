#!/usr/bin/env python3
"""Line-sensor record of the batched 2-D exact k-space propagator on one GPU: SecondOrderFrames.line_record(times) against
run(times) with sensor_index set to the same row — the only way to the same numbers without the record — and the record's
parts alone:

    python tools/bench_second_order_line_record.py [--frames 64 8 1] [--times 1024] [--reps 7] [--warmup 2]

One JSON line per frame count and medium (absorbing y = 1.5 at 0.75 dB/(MHz^1.5 cm), lossless): frames of 256 x 256 in
512 x 512 at 0.1 mm, the output times n dt with dt = dx / c0, row 0.  The two forms run in one process and alternate rep by
rep after the warm-up rounds; figures are medians with their range.

  record / run       the C entries kwh_second_order_frames_line_record (dst = NULL) and kwh_second_order_frames_run, host
                     clock around the call and a synchronise of the context: the device work, no copy of the record
  record_copy / run_copy   line_record(times) and run(times) of the Python class: the same with the record (F n_times Nx
                     floats either way) copied into a NumPy array
  prepare, kernel, c2r_crop   kw_second_order_line_prepare, kw_second_order_line_record and, on a second context
                     (Ex, 1, F n_times), kw_fft_c2r_frames with kw_plane_recon_crop through the C ABI, device events
  kernel_gfma_s, kernel_gh_s   the record kernel's rate against its own counts: 2 F (Ex/2 + 1) (Ey/2 + 1) n_times fused
                     multiply-adds, and (Ex/2 + 1) (Ey/2 + 1) n_times ceil(F / 64) evaluations of H
  max_rel_diff       |line_record - run| over max |run| on this run's data (the tests hold the 2e-5 bound in relative L2)
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

N, E = (256, 256), (512, 512)


def summary(name, v):
    return {name + "_ms": round(float(np.median(v)), 4), name + "_ms_min_max": [round(min(v), 4), round(max(v), 4)]}


def class_case(nf, coeff, times, reps, warmup):
    """the two forms through SecondOrderFrames, alternating"""
    p0 = np.random.default_rng(nf).standard_normal((nf, N[1], N[0])).astype(F32)
    p = second_order.SecondOrderFrames(N, (DX, DX), C0, nf, alpha_coeff=coeff, alpha_power=ALPHA_POWER, expanded=E,
                                       sensor_index=np.arange(N[0]), line_row=0)
    L, sync = second_order._lib(), lambda: capi.check(capi.load().kw_sync(p.ctx))
    tp = times.ctypes.data_as(C.POINTER(C.c_double))
    forms = {
        "record": lambda: second_order._check(L.kwh_second_order_frames_line_record(p._h, tp, times.size, None)),
        "run": lambda: second_order._check(L.kwh_second_order_frames_run(p._h, tp, times.size)),
        "record_copy": lambda: p.line_record(times),
        "run_copy": lambda: p.run(times),
    }
    out = {k: [] for k in forms}
    try:
        assert p.fused
        p.set_p0(p0)
        rec, raw = p.line_record(times), p.run(times).transpose(1, 0, 2)
        diff = float(np.abs(rec - raw).max() / np.abs(raw).max())
        for rep in range(warmup + reps):
            for name, fn in forms.items():
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                if rep >= warmup:
                    out[name].append((time.perf_counter() - t0) * 1e3)
        chunk = p.line_chunk_times
    finally:
        p.close()
    res = {"line_chunk_times": chunk, "max_rel_diff": float(f"{diff:.3e}")}
    for name, v in out.items():
        res.update(summary(name, v))
    res["run_over_record"] = round(res["run_ms"] / res["record_ms"], 1)
    res["run_copy_over_record_copy"] = round(res["run_copy_ms"] / res["record_copy_ms"], 1)
    return res


def parts_case(nf, coeff, times, reps, warmup):
    """prepare, the record kernel, and the C2R with the crop, each alone, device events"""
    ex, ey = E
    nxc, mf, nt = ex // 2 + 1, ey // 2 + 1, times.size
    vol_h = np.zeros((nf, ey, ex), F32)
    vol_h[:, :N[1], :N[0]] = np.random.default_rng(nf).standard_normal((nf, N[1], N[0]))
    op = capi.SecondOrderOp()
    op.dx = op.dy = DX
    op.c0 = C0
    op.a = coeff * 100.0 * (1.0e-6 / (2.0 * np.pi)) ** ALPHA_POWER / (20.0 * np.log10(np.e))
    op.alpha_power, op.absorbing = ALPHA_POWER, int(coeff > 0.0)
    dev, d2 = capi.Device(), capi.Device()
    try:
        dev.set_constants(constants(ex, ey, nf))
        dev.call("fft_create_plans_frames")
        vol, spec = dev.array(vol_h), dev.empty(2 * nxc * ey * nf)
        dev.call("fft_r2c_frames", vol, spec)
        q, g = dev.empty(2 * nxc * mf * nf), dev.empty(2 * nf * nt * nxc)
        tdev = dev.array(times)
        d2.set_constants(constants(ex, 1, nf * nt))
        d2.call("fft_create_plans_frames")
        rows, crop = d2.empty(ex * nf * nt), d2.empty(N[0] * nf * nt)

        def c2r_crop():
            d2.call("fft_c2r_frames", g, rows)
            d2.call("plane_recon_crop", crop, rows, ex, nf * nt, 1, N[0], nf * nt, 1, 0)

        parts = {"prepare": (dev, lambda: dev.call("second_order_line_prepare", q, spec, 0)),
                 "kernel": (dev, lambda: dev.call("second_order_line_record", g, q, C.byref(op), tdev, nt)),
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
    fma, h = 2 * nf * nxc * mf * nt, nxc * mf * nt * ((nf + 63) // 64)
    res.update({"kernel_fma": fma, "kernel_h": h, "kernel_gfma_s": round(fma / res["kernel_ms"] / 1e6, 1),
                "kernel_gh_s": round(h / res["kernel_ms"] / 1e6, 2)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[64, 8, 1])
    ap.add_argument("--times", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    times = np.ascontiguousarray(DX / C0 * np.arange(args.times), dtype=np.float64)
    for nf in args.frames:
        for coeff in (ALPHA_COEFF, 0.0):
            res = {"frames": nf, "plane": list(N), "expanded": list(E), "n_times": args.times, "alpha_coeff": coeff, "reps": args.reps}
            res.update(class_case(nf, coeff, times, args.reps, args.warmup))
            res.update(parts_case(nf, coeff, times, args.reps, args.warmup))
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
