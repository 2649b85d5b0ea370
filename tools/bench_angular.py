#!/usr/bin/env python3
"""Angular-spectrum projector on one GPU: the fused stage kw_fused_angular_planes against its rocFFT twin, the plane-chunk
size, and a whole AngularSpectrum.run, on square expanded grids:

    python tools/bench_angular.py [--sizes 256 512] [--reps 20] [--warmup 3] [--chunks 16 32 64] [--chunk-grids 512]
                                  [--run-domain 256]

One JSON line per case.  Times are HIP events on the context's stream; the two forms alternate rep by rep.

  stage   one kw_fused_angular_planes on a chunk of Zc planes: k_yinv_angular and the x-inverse of two arrays
  twin    the same planes on rocFFT: kw_angular_mix and 2 Zc two-dimensional C2R transforms
  bytes   pass_bytes: what the two passes of the stage must move — the y-inverse writes two spectra, the x-inverse reads
          them and writes two real arrays: 24 B per expanded point and plane with R = E / 2 bins, plus the source's spectra
          and the tables once (18 B per point).  pass_fraction = pass_bytes / stage time over the device-copy bandwidth
          measured at the volume of one real array of the chunk.
  chunk   AngularSpectrum.project() of 128 planes with chunk_planes 16 / 32 / 64: time per plane, crop included
  run     a whole AngularSpectrum.run (host plane in, complex volume out) and its project() alone; beside it, for
          orientation only (the two solve different problems), a FieldPropagator.run from tools/bench_cw.py
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
from kwave_amd import angular, capi  # noqa: E402

F32 = np.float32
C0, DX = 1500.0, 0.25e-3
F0 = C0 / (3.0 * DX)
K = 2.0 * np.pi * F0 / C0


def constants(n, nz):
    k = capi.Constants()
    k.nx = k.ny = n
    k.nz = nz
    k.n_elements = n * n * nz
    k.nx_complex, k.ny_complex, k.nz_complex = n // 2 + 1, n, nz
    k.n_elements_complex = (n // 2 + 1) * n * nz
    k.fft_divider = 1.0 / (n * n)
    k.fft_divider_x = k.fft_divider_y = 1.0 / n
    k.fft_divider_z = 1.0
    k.dt, k.dt_by_2 = 1.0, 0.5
    return k


def operator(dev, tab, imported, nz):
    dev.call("angular_operator", tab, imported, C.c_double(DX), C.c_double(DX), C.c_double(K), C.c_double(20.0), C.c_double(0.0),
             C.c_double(DX), nz, 1)


def stage_case(n, zc, reps, warmup):
    rng = np.random.default_rng(n)
    plane = rng.standard_normal((n, n)).astype(F32)
    nr = (n // 2 + 1) * n
    # the fused stage
    dev = capi.Device()
    dev.set_constants(constants(n, zc))
    dev.call("fused_create")
    ne = C.c_size_t()
    dev.call("fused_angular_elems", C.byref(ne))
    tab, imported = dev.empty(5 * nr, np.uint32), dev.empty(5 * ne.value, np.uint32)
    operator(dev, tab, imported, 4096)
    chunk = np.zeros((zc, n, n), F32)
    chunk[0] = plane
    re, im = dev.array(chunk), dev.array(chunk[:, ::-1].copy())
    spr, spi = dev.empty(2 * ne.value), dev.empty(2 * ne.value)
    dev.call("fused_angular_forward", re, im, spr, spi)
    # the twin
    d2 = capi.Device()
    d2.set_constants(constants(n, 1))
    d2.call("fft_create_plans_3d")
    tab2 = d2.empty(5 * nr, np.uint32)
    operator(d2, tab2, None, 4096)
    s2r, s2i = d2.array(plane), d2.array(plane[::-1].copy())
    sp2r, sp2i = d2.empty(2 * nr), d2.empty(2 * nr)
    d2.call("fft_r2c_3d", s2r, sp2r)
    d2.call("fft_r2c_3d", s2i, sp2i)
    mr, mi = d2.empty(2 * nr * zc), d2.empty(2 * nr * zc)
    o2r, o2i = d2.empty(n * n * zc), d2.empty(n * n * zc)

    def stage():
        dev.call("fused_angular_planes", spr, spi, imported, 64, re, im)

    def twin():
        d2.call("angular_mix", mr, mi, sp2r, sp2i, tab2, nr, zc, 64, 1.0 / (n * n))
        for z in range(zc):
            d2.call("fft_c2r_3d", mr.ptr + 8 * nr * z, o2r.ptr + 4 * n * n * z)
            d2.call("fft_c2r_3d", mi.ptr + 8 * nr * z, o2i.ptr + 4 * n * n * z)

    times = {"stage": [], "twin": []}
    ev = {"stage": (dev, dev.event(), dev.event()), "twin": (d2, d2.event(), d2.event())}
    for _ in range(warmup):
        stage()
        twin()
    dev.sync()
    d2.sync()
    for _ in range(reps):
        for name, fn in (("stage", stage), ("twin", twin)):
            d, e0, e1 = ev[name]
            d.record(e0)
            fn()
            d.record(e1)
            times[name].append(d.elapsed_ms(e0, e1))
    copy = C.c_double()
    capi.check(dev.L.kw_measure_copy_bandwidth(dev.ctx, C.c_size_t(4 * n * n * zc), 20, C.byref(copy)))
    st, tw = float(np.median(times["stage"])), float(np.median(times["twin"]))
    pass_bytes = 24 * n * n * zc + 18 * n * n
    out = {"expanded": n, "chunk_planes": zc, "reps": reps, "stage_ms": round(st, 4),
           "stage_ms_min_max": [round(min(times["stage"]), 4), round(max(times["stage"]), 4)], "twin_ms": round(tw, 4),
           "twin_over_stage": round(tw / st, 3), "pass_bytes": pass_bytes, "pass_gbs": round(pass_bytes / st / 1e6, 1),
           "copy_gbs": round(copy.value, 1), "pass_fraction": round(pass_bytes / st / 1e6 / copy.value, 3)}
    dev.call("fused_destroy")
    dev.close()
    d2.close()
    return out


def timed_project(p, reps):
    hip, ctx = capi.load(), p.ctx
    e0, e1 = C.c_void_p(), C.c_void_p()
    capi.check(hip.kw_event_create(ctx, C.byref(e0)))
    capi.check(hip.kw_event_create(ctx, C.byref(e1)))
    p.project()
    out = []
    for _ in range(reps):
        capi.check(hip.kw_event_record(ctx, e0))
        p.project()
        capi.check(hip.kw_event_record(ctx, e1))
        capi.check(hip.kw_event_synchronize(ctx, e1))
        ms = C.c_float()
        capi.check(hip.kw_event_elapsed_ms(ctx, e0, e1, C.byref(ms)))
        out.append(ms.value)
    return out


def chunk_case(n, chunks, reps, planes=128):
    """project() of `planes` planes on an n x n expanded grid with each chunk size, alternating rep by rep"""
    dom = n // 2
    amp = np.zeros((dom, dom), F32)
    amp[dom // 4: 3 * dom // 4, dom // 4: 3 * dom // 4] = 1.0
    ps = {zc: angular.AngularSpectrum((dom, dom), (DX, DX), C0, F0, 0.0, DX, planes, alpha_np=20.0, expanded=(n, n), chunk_planes=zc)
          for zc in chunks}
    for p in ps.values():
        p.run(amp, np.zeros_like(amp))
    times = {zc: [] for zc in chunks}
    for _ in range(reps):
        for zc, p in ps.items():
            times[zc] += timed_project(p, 1)
    out = {"expanded": n, "planes": planes, "reps": reps, "default_chunk_planes": angular.plan((dom, dom), (DX, DX), C0, F0, 0.0, DX, planes)[1]}
    for zc in chunks:
        out[f"chunk_{zc}_us_per_plane"] = round(float(np.median(times[zc])) / planes * 1e3, 2)
    for p in ps.values():
        p.close()
    return out


def run_case(dom, planes, reps, fused=True):
    p = angular.AngularSpectrum((dom, dom), (DX, DX), C0, F0, 0.0, DX, planes, alpha_np=20.0, fused_kernels=fused)
    amp = np.zeros((dom, dom), F32)
    amp[dom // 4: 3 * dom // 4, dom // 4: 3 * dom // 4] = 1.0
    phase = np.zeros_like(amp)
    p.run(amp, phase)
    t0 = time.perf_counter()
    for _ in range(reps):
        p.run(amp, phase)
    run_ms = (time.perf_counter() - t0) / reps * 1e3
    proj = timed_project(p, reps)
    out = {"domain": [dom, dom, planes], "expanded": list(p.expanded), "chunk_planes": p.chunk_planes, "fused_pipeline": p.fused,
           "run_ms": round(run_ms, 3), "project_ms": round(float(np.median(proj)), 4)}
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunks", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--chunk-grids", type=int, nargs="*", default=[512], help="expanded sides of the chunk-size comparison")
    ap.add_argument("--run-domain", type=int, default=256)
    ap.add_argument("--field-propagator", type=int, default=512, help="expanded side of the FieldPropagator.run beside it; 0: none")
    args = ap.parse_args()
    for n in args.sizes:
        zc = angular.plan((n // 2, n // 2), (DX, DX), C0, F0, 0.0, DX, 128)[1]
        print(json.dumps(stage_case(n, zc, args.reps, args.warmup)), flush=True)
    for n in args.chunk_grids if args.chunks else []:
        print(json.dumps(chunk_case(n, args.chunks, max(5, args.reps // 2))), flush=True)
    if args.run_domain:
        for fused in (True, False):
            print(json.dumps(run_case(args.run_domain, args.run_domain, max(3, args.reps // 4), fused)), flush=True)
        if args.field_propagator:
            from bench_cw import run_case as cw_run_case
            out = cw_run_case(args.field_propagator, 3)
            out["what"] = "cw.FieldPropagator.run, for orientation"
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
