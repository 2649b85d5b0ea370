#!/usr/bin/env python3
"""Exact k-space propagator on one GPU: one output time by the fused stage kw_fused_second_order_time against its rocFFT
twin, the stage's z-pass k_zfused_second_order against k_zfused_time at the same length, and the time loop's step on the
same grid beside them:

    python tools/bench_second_order.py [--grids 256x256x256] [--reps 20] [--warmup 3] [--loop-steps 50] [--dp0dt]

One JSON line per grid (Ex x Ey x Ez).  The forms alternate rep by rep; figures are medians.

  stage    one kw_fused_second_order_time: k_zfused_second_order (H formed in registers), the y-inverse and the storing
           x-inverse — what one output time costs, absorbing medium (y = 1.5)
  twin     the same time on rocFFT: kw_second_order_mix on the kept half-spectrum and one 3-D C2R transform
           (HIP events on each context's stream)
  zpass    k_zfused_second_order alone — lossless, absorbing with y = 1.5 (|k|^(y-1) is a square root) and with y = 1.1 (the
           float64 power function) — against k_zfused_time (the time-domain projector's z-pass: one float64 square root,
           a sincosf and an exp2f per bin) on the same context and scratch array: what the float64 work of the absorbing
           H costs.  From the library's per-kernel timing.
  loop     ms per step of the time loop (HostSolver, heterogeneous, nonlinear, absorbing, p0 source: the flagship
           workload of bench.py) on a cube of the grid's x side, wall clock over --loop-steps steps after a warm-up.

--dp0dt: instead of the above, the stage with dp0/dt as a second initial condition on the same context, the forms
alternating rep by rep, absorbing medium (y = 1.5):
  single   one kw_fused_second_order_time (as `stage` above)
  pair     one kw_fused_second_order_time_pair: k_zfused_second_order_pair over both kept spectra, the y-inverse and the
           storing x-inverse.  The comparison that matters is pair against twice single: what two propagators and an
           addition cost.
  pass     k_zfused_second_order_pair and k_zfused_second_order alone, from the library's per-kernel timing
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
from kwave_amd import capi, synthetic  # noqa: E402
from kwave_amd.solver import HostSolver  # noqa: E402

F32 = np.float32
C0, DX = 1500.0, 1.0e-4
T = 40.0e-6
ALPHA_COEFF, ALPHA_POWER = 0.75, 1.5


def constants(ex, ey, ez):
    k = capi.Constants()
    k.nx, k.ny, k.nz = ex, ey, ez
    k.n_elements = ex * ey * ez
    k.nx_complex, k.ny_complex, k.nz_complex = ex // 2 + 1, ey, ez
    k.n_elements_complex = (ex // 2 + 1) * ey * ez
    k.fft_divider = 1.0 / (ex * ey * ez)
    k.fft_divider_x, k.fft_divider_y, k.fft_divider_z = 1.0 / ex, 1.0 / ey, 1.0 / ez
    k.dt, k.dt_by_2 = 1.0, 0.5
    return k


def make_op(absorbing, y=ALPHA_POWER):
    op = capi.SecondOrderOp()
    op.dx = op.dy = op.dz = DX
    op.c0, op.t = C0, T
    op.a = ALPHA_COEFF * 100.0 * (1.0e-6 / (2.0 * np.pi)) ** y / (20.0 * np.log10(np.e))
    op.alpha_power = y
    op.absorbing = int(absorbing)
    return op


def time_op():
    op = capi.AngularTimeOp()
    op.dx = op.dy = DX
    op.dt, op.c0, op.z = DX / (C0 * np.pi), C0, 40e-3
    op.ak = None
    op.restriction, op.retarded = 1, 1
    return op


def kernel_ms(dev, name):
    calls, total = capi.profile_collect(dev.ctx)[name]
    return total / calls


def loop_ms_per_step(n, steps, warmup):
    pr = synthetic.make_problem(n, heterogeneous=True, nonlinear=True, absorbing=True, source="p0", nt=warmup + steps + 8)
    sim = HostSolver(pr, p_raw=1, p_max=1)
    try:
        sim.run(warmup)
        sim.sync()
        t0 = time.perf_counter()
        sim.run(steps)
        sim.sync()
        return (time.perf_counter() - t0) * 1e3 / steps
    finally:
        sim.close()


def dp0dt_case(ex, ey, n3, reps, warmup, frames=False):
    """single stage, pair stage and the pair pass alone on one context (Ex, Ey, Ez), or with `frames` a frames context
    (Ex, Ey, F); shared with tools/bench_second_order_frames.py"""
    rng = np.random.default_rng(ex + ey + n3)
    shape = (n3, ey, ex)
    nr = (ex // 2 + 1) * ey * n3
    entry = "fused_second_order_frames_" if frames else "fused_second_order_"
    kernel = "k_yfused_second_order" if frames else "k_zfused_second_order"
    dev = capi.Device()
    dev.set_constants(constants(ex, ey, n3))
    if frames:
        dev.call("fused_set_frames", 1)
    ok = C.c_int()
    dev.call("fused_supported", C.byref(ok))
    if ok.value != 1:
        raise SystemExit(f"the fused pipeline does not take a context of {ex} x {ey} x {n3}")
    dev.call("fused_create")
    ne = C.c_size_t()
    dev.call(entry + "elems", C.byref(ne))
    vol, kept_p, kept_v = dev.array(rng.standard_normal(shape).astype(F32)), dev.empty(2 * ne.value), dev.empty(2 * ne.value)
    dev.call(entry + "forward", vol, kept_p)
    vol_v = dev.array((rng.standard_normal(shape) * C0 / DX).astype(F32))
    dev.call(entry + "forward", vol_v, kept_v)
    op = make_op(True)
    forms = {"single": lambda: dev.call(entry + "time", kept_p, C.byref(op), vol),
             "pair": lambda: dev.call(entry + "time_pair", kept_p, kept_v, C.byref(op), vol)}
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    dev.sync()
    e0, e1 = dev.event(), dev.event()
    times = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            dev.record(e0)
            fn()
            dev.record(e1)
            times[name].append(dev.elapsed_ms(e0, e1))
    capi.check(dev.L.kw_profile_enable(dev.ctx, 1))
    capi.profile_collect(dev.ctx)
    passes = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            fn()
            passes[name].append(kernel_ms(dev, kernel + ("_pair" if name == "pair" else "")))
    capi.check(dev.L.kw_profile_enable(dev.ctx, 0))
    copy = C.c_double()
    capi.check(dev.L.kw_measure_copy_bandwidth(dev.ctx, C.c_size_t(8 * nr), 20, C.byref(copy)))
    dev.call("fused_destroy")
    dev.close()
    med = lambda v: float(np.median(v))   # noqa: E731
    rng_of = lambda v: [round(min(v), 4), round(max(v), 4)]   # noqa: E731
    si, pa, ps, pp = med(times["single"]), med(times["pair"]), med(passes["single"]), med(passes["pair"])
    return {("batch" if frames else "grid"): ([n3, ey, ex] if frames else [ex, ey, n3]), "dp0dt": True, "reps": reps,
            "single_stage_ms": round(si, 4), "single_stage_ms_min_max": rng_of(times["single"]),
            "pair_stage_ms": round(pa, 4), "pair_stage_ms_min_max": rng_of(times["pair"]),
            "pair_over_twice_single": round(pa / (2.0 * si), 3), "single_pass_ms": round(ps, 4),
            "pair_pass_ms": round(pp, 4), "pair_pass_ms_min_max": rng_of(passes["pair"]), "pair_pass_over_single_pass": round(pp / ps, 3),
            "pair_pass_bytes": 24 * nr, "pair_pass_gbs": round(24 * nr / pp / 1e6, 1), "single_pass_gbs": round(16 * nr / ps / 1e6, 1),
            "copy_gbs": round(copy.value, 1)}


def grid_case(ex, ey, ez, reps, warmup, loop_steps):
    rng = np.random.default_rng(ex + ey + ez)
    vol_h = rng.standard_normal((ez, ey, ex)).astype(F32)
    nr = (ex // 2 + 1) * ey * ez
    dev = capi.Device()
    dev.set_constants(constants(ex, ey, ez))
    dev.call("fused_create")
    ne = C.c_size_t()
    dev.call("fused_second_order_elems", C.byref(ne))
    vol, kept = dev.array(vol_h), dev.empty(2 * ne.value)
    dev.call("fused_second_order_forward", vol, kept)
    ops = {"lossless": make_op(False), "absorbing": make_op(True), "general": make_op(True, 1.1)}
    top = time_op()
    d2 = capi.Device()
    d2.set_constants(constants(ex, ey, ez))
    d2.call("fft_create_plans_3d")
    src2, spec2, mixed2, out2 = d2.array(vol_h), d2.empty(2 * nr), d2.empty(2 * nr), d2.empty(ex * ey * ez)
    d2.call("fft_r2c_3d", src2, spec2)

    def stage():
        dev.call("fused_second_order_time", kept, C.byref(ops["absorbing"]), vol)

    def twin():
        d2.call("second_order_mix", mixed2, spec2, C.byref(ops["absorbing"]), C.c_float(1.0 / (ex * ey * ez)))
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
    # the z-pass alone against the time-domain projector's, per-kernel timing, alternating
    capi.check(dev.L.kw_profile_enable(dev.ctx, 1))
    capi.profile_collect(dev.ctx)
    zp = {"lossless": [], "absorbing": [], "general": [], "angular_time": []}
    for _ in range(reps):
        for name in ("lossless", "absorbing", "general"):
            dev.call("fused_second_order_time", kept, C.byref(ops[name]), vol)
            zp[name].append(kernel_ms(dev, "k_zfused_second_order"))
        dev.call("fused_angular_time_plane", kept, C.byref(top), vol)
        zp["angular_time"].append(kernel_ms(dev, "k_zfused_time"))
    capi.check(dev.L.kw_profile_enable(dev.ctx, 0))
    copy = C.c_double()
    capi.check(dev.L.kw_measure_copy_bandwidth(dev.ctx, C.c_size_t(8 * nr), 20, C.byref(copy)))
    dev.call("fused_destroy")
    dev.close()
    d2.close()
    st, tw = float(np.median(times["stage"])), float(np.median(times["twin"]))
    z0, z1, zg, zt = (float(np.median(zp[n])) for n in ("lossless", "absorbing", "general", "angular_time"))
    out = {"grid": [ex, ey, ez], "reps": reps, "stage_ms": round(st, 4),
           "stage_ms_min_max": [round(min(times["stage"]), 4), round(max(times["stage"]), 4)], "twin_ms": round(tw, 4),
           "twin_over_stage": round(tw / st, 3), "zpass_lossless_ms": round(z0, 4), "zpass_absorbing_ms": round(z1, 4),
           "zpass_general_power_ms": round(zg, 4), "zpass_angular_time_ms": round(zt, 4), "zpass_over_angular_time": round(z1 / zt, 3), "zpass_bytes": 16 * nr,
           "zpass_gbs": round(16 * nr / z1 / 1e6, 1), "copy_gbs": round(copy.value, 1)}
    if loop_steps > 0:
        loop = loop_ms_per_step(ex, loop_steps, warmup)
        out.update({"loop_grid": [ex, ex, ex], "loop_ms_per_step": round(loop, 4), "stage_over_loop_step": round(st / loop, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="*", default=["256x256x256"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-steps", type=int, default=50)
    ap.add_argument("--dp0dt", action="store_true", help="time the single stage, the pair stage and the pair pass instead")
    args = ap.parse_args()
    for g in args.grids:
        ex, ey, ez = (int(v) for v in g.split("x"))
        if args.dp0dt:
            print(json.dumps(dp0dt_case(ex, ey, ez, args.reps, args.warmup)), flush=True)
            continue
        print(json.dumps(grid_case(ex, ey, ez, args.reps, args.warmup, args.loop_steps)), flush=True)


if __name__ == "__main__":
    main()
