#!/usr/bin/env python3
"""Batched k-space line reconstruction on one GPU: frames per second of the fused stage kw_fused_line_recon against its
rocFFT twin, and the launch times of the stage's three kernels:

    python tools/bench_line_recon.py [--cases 128x512x1 128x512x16 128x512x64 128x512x1024 256x512x256] [--reps 20] [--warmup 3]

One JSON line per case Ny x Nt x F (Ey = Ny; Lt = the fast-path length at or above 2 Nt - 1).  The forms alternate rep by
rep; figures are medians, with the range beside them.

  stage    one kw_fused_line_recon over the F frames: the x-forward, k_yfused_line_recon (forward along t, weight, gather,
           inverse along t, each frame apart), the storing x-inverse, in place on t-even planes
  twin     the same on rocFFT: F batched 2-D R2C transforms, kw_line_recon_mix (an out-of-place gather over the
           half-spectra) and F batched 2-D C2R transforms (HIP events on each context's stream)
  fps      frames per second of each form: F / time
  kernels  the three launches of the stage alone, from the library's per-kernel timing (kw_profile_*)
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kwave_amd  # noqa: E402,F401
from kwave_amd import capi, recon  # noqa: E402

F32 = np.float32
C0, DY = 1500.0, 0.25e-3
DT = DY / (C0 * np.pi)


def constants(ey, lt, nf):
    k = capi.Constants()
    k.nx, k.ny, k.nz = ey, lt, nf
    k.n_elements = ey * lt * nf
    k.nx_complex, k.ny_complex, k.nz_complex = ey // 2 + 1, lt, nf
    k.n_elements_complex = (ey // 2 + 1) * lt * nf
    k.fft_divider = 1.0 / (ey * lt)
    k.fft_divider_x, k.fft_divider_y, k.fft_divider_z = 1.0 / ey, 1.0 / lt, 1.0
    k.dt, k.dt_by_2 = 1.0, 0.5
    return k


def make_op(interp):
    op = capi.PlaneReconOp()
    op.dx = op.dy = DY
    op.dt, op.c0 = DT, C0
    op.interp, op.reserved = interp, 0
    return op


def even_frames(nf, lt, ey):
    rng = np.random.default_rng(nf + lt + ey)
    v = rng.standard_normal((nf, lt, ey)).astype(F32)
    half = (lt - 1) // 2
    v[:, lt - half:] = v[:, half:0:-1]
    return v


def case(ny, nt, nf, reps, warmup):
    ey, lt, _depth, chunk, fast = recon.plan_line_recon(ny, DY, DT, nt, C0, frames=nf)
    if not fast or chunk != nf:
        return {"case": [ny, nt, nf], "skipped": f"Ey = {ey}, Lt = {lt}, chunk = {chunk}: not one fused chunk"}
    vol_h = even_frames(nf, lt, ey)
    nr = (ey // 2 + 1) * lt * nf
    op = make_op(0)
    dev = capi.Device()
    dev.set_constants(constants(ey, lt, nf))
    dev.call("fused_set_frames", 1)
    dev.call("fused_create")
    src, vol = dev.array(vol_h), dev.empty(ey * lt * nf)
    d2 = capi.Device()
    d2.set_constants(constants(ey, lt, nf))
    d2.call("fft_create_plans_frames")
    src2, spec2, mixed2, out2 = d2.array(vol_h), d2.empty(2 * nr), d2.empty(2 * nr), d2.empty(ey * lt * nf)

    def stage():
        dev.call("fused_line_recon", src, C.byref(op), vol)

    def twin():
        d2.call("fft_r2c_frames", src2, spec2)
        d2.call("line_recon_mix", mixed2, spec2, C.byref(op), C.c_float(2.0 / (ey * lt)))
        d2.call("fft_c2r_frames", mixed2, out2)

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
    # the three launches of the stage, per-kernel timing
    capi.check(dev.L.kw_profile_enable(dev.ctx, 1))
    capi.profile_collect(dev.ctx)
    kern = {}
    for _ in range(reps):
        stage()
        for name, (calls, total) in capi.profile_collect(dev.ctx).items():
            if name.startswith("k_"):
                kern.setdefault(name, []).append(total)   # (a masked last tile is a second launch of the same name)
    capi.check(dev.L.kw_profile_enable(dev.ctx, 0))
    st, tw = float(np.median(times["stage"])), float(np.median(times["twin"]))
    out = {"case": [ny, nt, nf], "grid": [ey, lt, nf], "reps": reps, "stage_ms": round(st, 4),
           "stage_ms_min_max": [round(min(times["stage"]), 4), round(max(times["stage"]), 4)], "twin_ms": round(tw, 4),
           "twin_ms_min_max": [round(min(times["twin"]), 4), round(max(times["twin"]), 4)],
           "twin_over_stage": round(tw / st, 3), "stage_fps": round(nf / st * 1e3, 1), "twin_fps": round(nf / tw * 1e3, 1),
           "kernel_us": {name: round(float(np.median(v)) * 1e3, 2) for name, v in sorted(kern.items())}}
    dev.call("fused_destroy")
    dev.close()
    d2.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["128x512x1", "128x512x16", "128x512x64", "128x512x1024", "256x512x256"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for g in args.cases:
        ny, nt, nf = (int(v) for v in g.split("x"))
        print(json.dumps(case(ny, nt, nf, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
