#!/usr/bin/env python3
"""Batched 2-D exact k-space propagator on one GPU: one output time of F frames by the fused stage
kw_fused_second_order_frames_time against its rocFFT twin, and the stage's pass along y k_yfused_second_order beside the 3-D
propagator's z-pass k_zfused_second_order on a 3-D context of the same number of bins:

    python tools/bench_second_order_frames.py [--batches 64x512x512] [--reps 20] [--warmup 3] [--dp0dt]

One JSON line per batch (F x Ey x Ex, the expanded planes).  The forms alternate rep by rep; figures are medians with
their range.

  stage    one kw_fused_second_order_frames_time: k_yfused_second_order (H formed in registers) and the storing x-inverse —
           what one output time of the whole batch costs, absorbing medium (y = 1.5)
  twin     the same on rocFFT: kw_second_order_frames_mix on the kept half-spectra and the batched 2-D C2R transform
           (HIP events on each context's stream)
  ypass    k_yfused_second_order alone, absorbing, beside k_zfused_second_order on the 3-D context (Ex, Ey, F) — the same
           bins, the same H, lines of Ey along y against lines of F along z.  From the library's per-kernel timing.
           (F must be a fast-path line length for the 3-D context; otherwise the figure is left out.)

--dp0dt: instead of the above, on one frames context and alternating rep by rep, one kw_fused_second_order_frames_time
(single), one kw_fused_second_order_frames_time_pair (pair: both kept spectra through k_yfused_second_order_pair, one
x-inverse) and the two passes alone from the library's per-kernel timing (bench_second_order.dp0dt_case).  The comparison
that matters is pair against twice single.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_second_order import F32, capi, constants, dp0dt_case, kernel_ms, make_op  # noqa: E402


def batch_case(nf, ey, ex, reps, warmup):
    rng = np.random.default_rng(nf + ey + ex)
    vol_h = rng.standard_normal((nf, ey, ex)).astype(F32)
    nr = (ex // 2 + 1) * ey * nf
    op = make_op(True)
    dev = capi.Device()
    dev.set_constants(constants(ex, ey, nf))
    dev.call("fused_set_frames", 1)
    ok = C.c_int()
    dev.call("fused_supported", C.byref(ok))
    if ok.value != 1:
        raise SystemExit(f"the fused pipeline does not take a frames context of {ex} x {ey} x {nf}")
    dev.call("fused_create")
    ne = C.c_size_t()
    dev.call("fused_second_order_frames_elems", C.byref(ne))
    vol, kept = dev.array(vol_h), dev.empty(2 * ne.value)
    dev.call("fused_second_order_frames_forward", vol, kept)
    d2 = capi.Device()
    d2.set_constants(constants(ex, ey, nf))
    d2.call("fft_create_plans_frames")
    src2, spec2, mixed2, out2 = d2.array(vol_h), d2.empty(2 * nr), d2.empty(2 * nr), d2.empty(ex * ey * nf)
    d2.call("fft_r2c_frames", src2, spec2)

    def stage():
        dev.call("fused_second_order_frames_time", kept, C.byref(op), vol)

    def twin():
        d2.call("second_order_frames_mix", mixed2, spec2, C.byref(op), C.c_float(1.0 / (ex * ey)))
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
    d2.close()
    # the pass along y alone beside the 3-D z-pass on the same bins, per-kernel timing, alternating
    ok3 = C.c_int()
    d3 = capi.Device()
    d3.set_constants(constants(ex, ey, nf))
    d3.call("fused_supported", C.byref(ok3))
    passes = {"k_yfused_second_order": []}
    if ok3.value == 1:
        d3.call("fused_create")
        n3 = C.c_size_t()
        d3.call("fused_second_order_elems", C.byref(n3))
        vol3, kept3 = d3.array(vol_h), d3.empty(2 * n3.value)
        d3.call("fused_second_order_forward", vol3, kept3)
        capi.check(d3.L.kw_profile_enable(d3.ctx, 1))
        capi.profile_collect(d3.ctx)
        passes["k_zfused_second_order"] = []
    capi.check(dev.L.kw_profile_enable(dev.ctx, 1))
    capi.profile_collect(dev.ctx)
    for _ in range(reps):
        stage()
        passes["k_yfused_second_order"].append(kernel_ms(dev, "k_yfused_second_order"))
        if ok3.value == 1:
            d3.call("fused_second_order_time", kept3, C.byref(op), vol3)
            passes["k_zfused_second_order"].append(kernel_ms(d3, "k_zfused_second_order"))
    capi.check(dev.L.kw_profile_enable(dev.ctx, 0))
    copy = C.c_double()
    capi.check(dev.L.kw_measure_copy_bandwidth(dev.ctx, C.c_size_t(8 * nr), 20, C.byref(copy)))
    dev.call("fused_destroy")
    dev.close()
    if ok3.value == 1:
        d3.call("fused_destroy")
    d3.close()
    st, tw = float(np.median(times["stage"])), float(np.median(times["twin"]))
    yp = float(np.median(passes["k_yfused_second_order"]))
    out = {"batch": [nf, ey, ex], "reps": reps, "stage_ms": round(st, 4),
           "stage_ms_min_max": [round(min(times["stage"]), 4), round(max(times["stage"]), 4)], "twin_ms": round(tw, 4),
           "twin_ms_min_max": [round(min(times["twin"]), 4), round(max(times["twin"]), 4)], "twin_over_stage": round(tw / st, 3),
           "stage_us_per_frame": round(1e3 * st / nf, 3), "ypass_ms": round(yp, 4),
           "ypass_ms_min_max": [round(min(passes["k_yfused_second_order"]), 4), round(max(passes["k_yfused_second_order"]), 4)],
           "ypass_bytes": 16 * nr, "ypass_gbs": round(16 * nr / yp / 1e6, 1), "copy_gbs": round(copy.value, 1)}
    if ok3.value == 1:
        zp = float(np.median(passes["k_zfused_second_order"]))
        out.update({"zpass_3d_ms": round(zp, 4), "ypass_over_zpass_3d": round(yp / zp, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="*", default=["64x512x512"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dp0dt", action="store_true", help="time the single stage, the pair stage and the pair pass instead")
    args = ap.parse_args()
    for b in args.batches:
        nf, ey, ex = (int(v) for v in b.split("x"))
        if args.dp0dt:
            print(json.dumps(dp0dt_case(ex, ey, nf, args.reps, args.warmup, frames=True)), flush=True)
            continue
        print(json.dumps(batch_case(nf, ey, ex, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
