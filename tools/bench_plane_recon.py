#!/usr/bin/env python3
"""k-space plane reconstruction on one GPU: the fused round trip kw_fused_plane_recon against its rocFFT twin, and the stage's
z-pass k_zfused_recon against the pipeline's plain z-fused multiply, on the same grids:

    python tools/bench_plane_recon.py [--grids 256x256x256 512x512x512 512x512x1024] [--reps 20] [--warmup 3]

One JSON line per grid (Ex x Ey x Lt).  The forms alternate rep by rep; figures are medians, with the range beside them.

  stage    one kw_fused_plane_recon: x- and y-forward, k_zfused_recon (weight, gather from w to kz along the line in LDS),
           the y-inverse and the storing x-inverse, in place on a t-even volume
  twin     the same on rocFFT: one 3-D R2C transform, kw_plane_recon_mix (an out-of-place gather over the half-spectrum)
           and one 3-D C2R transform (HIP events on each context's stream)
  zpass    k_zfused_recon alone against kw_fused_probe(which = 2), the z-fused pass that multiplies by an operator array
           read from memory: the price of two float64 square roots per bin, two barriers and the gather from LDS.  Both
           from the library's per-kernel timing (kw_profile_*), both interpolants, on the same context and scratch array.
  bytes    zpass_bytes: the spectrum read and written once, 16 B per bin; zpass_gbs is that over the z-pass time, beside the
           device-copy bandwidth measured at the volume of one spectrum.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kwave_amd  # noqa: E402,F401
from kwave_amd import capi  # noqa: E402

F32 = np.float32
C0, DX = 1500.0, 0.25e-3
DT = DX / (C0 * np.pi)


def constants(ex, ey, lt):
    k = capi.Constants()
    k.nx, k.ny, k.nz = ex, ey, lt
    k.n_elements = ex * ey * lt
    k.nx_complex, k.ny_complex, k.nz_complex = ex // 2 + 1, ey, lt
    k.n_elements_complex = (ex // 2 + 1) * ey * lt
    k.fft_divider = 1.0 / (ex * ey * lt)
    k.fft_divider_x, k.fft_divider_y, k.fft_divider_z = 1.0 / ex, 1.0 / ey, 1.0 / lt
    k.dt, k.dt_by_2 = 1.0, 0.5
    return k


def make_op(interp):
    op = capi.PlaneReconOp()
    op.dx = op.dy = DX
    op.dt, op.c0 = DT, C0
    op.interp, op.reserved = interp, 0
    return op


def kernel_ms(dev, name):
    calls, total = capi.profile_collect(dev.ctx)[name]
    return total / calls


def even_volume(ex, ey, lt):
    rng = np.random.default_rng(ex + ey + lt)
    v = rng.standard_normal((lt, ey, ex)).astype(F32)
    half = (lt - 1) // 2
    v[lt - half:] = v[half:0:-1]
    return v


def grid_case(ex, ey, lt, reps, warmup):
    vol_h = even_volume(ex, ey, lt)
    nr = (ex // 2 + 1) * ey * lt
    ops = {"linear": make_op(0), "nearest": make_op(1)}
    # the fused stage
    dev = capi.Device()
    dev.set_constants(constants(ex, ey, lt))
    dev.call("fused_create")
    src, vol = dev.array(vol_h), dev.empty(ex * ey * lt)
    nred = C.c_size_t()
    dev.call("fused_reduced_elems", C.byref(nred))
    unit = dev.array(np.ones(nred.value, dtype=F32))
    # the twin
    d2 = capi.Device()
    d2.set_constants(constants(ex, ey, lt))
    d2.call("fft_create_plans_3d")
    src2, spec2, mixed2, out2 = d2.array(vol_h), d2.empty(2 * nr), d2.empty(2 * nr), d2.empty(ex * ey * lt)

    def stage():
        dev.call("fused_plane_recon", src, C.byref(ops["linear"]), vol)

    def twin():
        d2.call("fft_r2c_3d", src2, spec2)
        d2.call("plane_recon_mix", mixed2, spec2, C.byref(ops["linear"]), C.c_float(2.0 / (ex * ey * lt)))
        d2.call("fft_c2r_3d", mixed2, out2)

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
    # the z-pass alone against the plain z-fused multiply, per-kernel timing, alternating
    capi.check(dev.L.kw_profile_enable(dev.ctx, 1))
    capi.profile_collect(dev.ctx)
    zp = {"linear": [], "nearest": [], "plain": []}
    for _ in range(reps):
        for name in ("linear", "nearest"):
            dev.call("fused_plane_recon", src, C.byref(ops[name]), vol)
            zp[name].append(kernel_ms(dev, "k_zfused_recon"))
        dev.call("fused_probe", 2, unit)
        zp["plain"].append(kernel_ms(dev, "k_zfused_source"))
    capi.check(dev.L.kw_profile_enable(dev.ctx, 0))
    copy = C.c_double()
    capi.check(dev.L.kw_measure_copy_bandwidth(dev.ctx, C.c_size_t(8 * nr), 20, C.byref(copy)))
    st, tw = float(np.median(times["stage"])), float(np.median(times["twin"]))
    z0, z1, zpl = (float(np.median(zp[n])) for n in ("linear", "nearest", "plain"))
    zbytes = 16 * nr
    out = {"grid": [ex, ey, lt], "reps": reps, "stage_ms": round(st, 4),
           "stage_ms_min_max": [round(min(times["stage"]), 4), round(max(times["stage"]), 4)], "twin_ms": round(tw, 4),
           "twin_ms_min_max": [round(min(times["twin"]), 4), round(max(times["twin"]), 4)],
           "twin_over_stage": round(tw / st, 3), "zpass_linear_ms": round(z0, 4), "zpass_nearest_ms": round(z1, 4),
           "zpass_plain_ms": round(zpl, 4), "zpass_over_plain": round(z0 / zpl, 3), "zpass_bytes": zbytes,
           "zpass_gbs": round(zbytes / z0 / 1e6, 1), "copy_gbs": round(copy.value, 1)}
    dev.call("fused_destroy")
    dev.close()
    d2.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="*", default=["256x256x256", "512x512x512", "512x512x1024"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for g in args.grids:
        ex, ey, lt = (int(v) for v in g.split("x"))
        print(json.dumps(grid_case(ex, ey, lt, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
