#!/usr/bin/env python3
"""CW field propagator on one GPU: the pair stage kw_fused_cw_pair against the same result composed from the older entry
points, and a whole FieldPropagator.run, on cubic expanded grids:

    python tools/bench_cw.py [--sizes 256 512] [--reps 20] [--warmup 3] [--split512 both|on|off]

One JSON line per case.  Times are HIP events on the context's stream; the two forms alternate rep by rep.

  pair      one kw_fused_cw_pair: x- and y-forward of two arrays, the pair z-pass, y- and x-inverse of two arrays
  composed  what the entry points before it allow: Gr Sr, Gi Sr, Gi Si, Gr Si as four kw_fused_scale_source calls (in place,
            so Sr and Si are copied once each first) and two combining passes.  The combining passes are timed as plain
            device copies (one read, one write per point; the real ones read two arrays), so `composed_ms` is a lower bound.
  bytes     pass_bytes: what the five passes of the pair stage must move — per pass every array once in and once out, the
            z-pass also the two operators: 84 B per point of the expanded grid with R = E / 2 bins; io_bytes: the pair in,
            the pair out and the operators, 20 B per point.  pass_fraction = pass_bytes / pair time over the device-copy
            bandwidth measured at the volume of one real array.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kwave_amd  # noqa: E402,F401
from kwave_amd import capi, cw  # noqa: E402

F32 = np.float32
C0, DX = 1500.0, 0.25e-3


def constants(n):
    k = capi.Constants()
    k.nx = k.ny = k.nz = n
    k.n_elements = n ** 3
    k.nx_complex, k.ny_complex, k.nz_complex = n // 2 + 1, n, n
    k.n_elements_complex = (n // 2 + 1) * n * n
    k.fft_divider = 1.0 / n ** 3
    k.fft_divider_x = k.fft_divider_y = k.fft_divider_z = 1.0 / n
    k.dt, k.dt_by_2 = 1.0, 0.5
    return k


def stage_case(n, split512, reps, warmup):
    dev = capi.Device()
    hip = dev.L
    if not split512:
        capi.check(hip.kw_set_tuning(dev.ctx, C.byref(capi.make_tuning({"split512": 0}))))
    dev.set_constants(constants(n))
    dev.call("fused_create")
    nr, np_ = (n // 2 + 1) * n * n, C.c_size_t()
    dev.call("fused_reduced_elems", C.byref(np_))
    f0 = C0 / (6.0 * DX)
    g = [dev.empty(nr), dev.empty(nr)]
    dk = C.c_double(2.0 * np.pi / (n * DX))
    dev.call("cw_operator", g[0], g[1], C.c_double(C0), C.c_double(2.0 * np.pi * f0), C.c_double(0.6 * n * DX / C0), dk, dk, dk)
    gp = [dev.empty(np_.value), dev.empty(np_.value)]
    for a, b in zip(gp, g):
        dev.call("fused_import_reduced", a, b)
    rng = np.random.default_rng(n)
    host = rng.standard_normal(n ** 3).astype(F32)
    re, im = dev.array(host), dev.array(host[::-1].copy())
    tmp = [dev.empty(n ** 3) for _ in range(4)]
    nbytes = 4 * n ** 3

    def pair():
        dev.call("fused_cw_pair", re, im, gp[0], gp[1])

    def composed():
        dev.call("memcpy_d2d", tmp[0], re, nbytes)      # Sr and Si once more each: the stage works in place
        dev.call("memcpy_d2d", tmp[1], im, nbytes)
        dev.call("fused_scale_source", re, gp[0])       # Gr Sr
        dev.call("fused_scale_source", tmp[0], gp[1])   # Gi Sr
        dev.call("fused_scale_source", im, gp[0])       # Gr Si
        dev.call("fused_scale_source", tmp[1], gp[1])   # Gi Si
        dev.call("memcpy_d2d", tmp[2], re, nbytes)      # stand-ins for Pr = Gr Sr - Gi Si and Pi = Gi Sr + Gr Si
        dev.call("memcpy_d2d", tmp[3], im, nbytes)

    e0, e1 = dev.event(), dev.event()
    times = {"pair": [], "composed": []}
    for _ in range(warmup):
        pair()
        composed()
    for _ in range(reps):
        for name, fn in (("pair", pair), ("composed", composed)):
            dev.record(e0)
            fn()
            dev.record(e1)
            times[name].append(dev.elapsed_ms(e0, e1))
        re.upload(host)                                   # keep the values finite over many passes
        im.upload(host)
    copy = C.c_double()
    capi.check(hip.kw_measure_copy_bandwidth(dev.ctx, C.c_size_t(nbytes), 20, C.byref(copy)))
    pair_ms, comp_ms = float(np.median(times["pair"])), float(np.median(times["composed"]))
    pass_bytes, io_bytes = 84 * n ** 3, 20 * n ** 3
    out = {"expanded": n, "split512": bool(split512), "reps": reps, "pair_ms": round(pair_ms, 4),
           "pair_ms_min_max": [round(min(times["pair"]), 4), round(max(times["pair"]), 4)],
           "composed_ms": round(comp_ms, 4), "composed_over_pair": round(comp_ms / pair_ms, 3),
           "pass_bytes": pass_bytes, "io_bytes": io_bytes, "pass_gbs": round(pass_bytes / pair_ms / 1e6, 1),
           "copy_gbs": round(copy.value, 1), "pass_fraction": round(pass_bytes / pair_ms / 1e6 / copy.value, 3)}
    dev.call("fused_destroy")
    dev.close()
    return out


def run_case(n, reps):
    """a whole FieldPropagator.run (host source in, complex field out) and its FFT round trip alone"""
    dom = int((n - 2) / (1.0 + np.sqrt(3.0)))             # the largest cubic domain whose default expanded side is <= n
    f0 = C0 / (6.0 * DX)
    p = cw.FieldPropagator((dom,) * 3, (DX,) * 3, C0, f0, expanded=(n,) * 3)
    amp = np.zeros((dom,) * 3, F32)
    amp[dom // 2, dom // 4: 3 * dom // 4, dom // 4: 3 * dom // 4] = 1.0
    phase = np.zeros_like(amp)
    p.run(amp, phase)
    t0 = time.perf_counter()
    for _ in range(reps):
        p.run(amp, phase)
    run_ms = (time.perf_counter() - t0) / reps * 1e3
    hip, ctx = capi.load(), p.ctx
    e0, e1 = C.c_void_p(), C.c_void_p()
    capi.check(hip.kw_event_create(ctx, C.byref(e0)))
    capi.check(hip.kw_event_create(ctx, C.byref(e1)))
    capi.check(hip.kw_event_record(ctx, e0))
    for _ in range(reps):
        p.propagate()
    capi.check(hip.kw_event_record(ctx, e1))
    capi.check(hip.kw_event_synchronize(ctx, e1))
    ms = C.c_float()
    capi.check(hip.kw_event_elapsed_ms(ctx, e0, e1, C.byref(ms)))
    out = {"expanded": n, "domain": dom, "fused_pipeline": p.fused, "run_ms": round(run_ms, 3),
           "round_trip_ms": round(ms.value / reps, 4)}
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split512", choices=("both", "on", "off"), default="both")
    args = ap.parse_args()
    for n in args.sizes:
        modes = [True] if n != 512 else {"both": [True, False], "on": [True], "off": [False]}[args.split512]
        for split in modes:
            print(json.dumps(stage_case(n, split, args.reps, args.warmup)), flush=True)
        print(json.dumps(run_case(n, max(3, args.reps // 4))), flush=True)


if __name__ == "__main__":
    main()
