#!/usr/bin/env python3
"""Bioheat solver on one GPU: steps per second of the Laplacian and the flux form at 128^3 and 256^3, the update
kernel's algorithmic bytes over its time, and the device-copy bandwidth at the same byte volume:

    python tools/bench_thermal.py [--sizes 128 256] [--steps 200] [--warmup 5] [--rocfft]

One JSON line per case.  The update kernel's time comes from the device library's per-entry-point events
(kw_profile_enable) over a second set of steps; its algorithmic bytes are 4 B per point and array it reads or writes
(T and cem43 both ways, the divergence arrays, the coefficient arrays that are arrays, Q)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kwave_amd  # noqa: E402,F401
from kwave_amd import capi  # noqa: E402
from kwave_amd.thermal import ThermalSolver  # noqa: E402

F32, U64 = np.float32, np.uint64


def problem(n, flux):
    """soft tissue at body temperature with a Gaussian source; flux: K, rho C and the perfusion vary smoothly by +-20 %"""
    d = 0.25e-3
    pr = {k: np.array([[[n]]], U64) for k in ("Nx", "Ny", "Nz")}
    pr.update({k: np.array([[[d]]], F32) for k in ("dx", "dy", "dz")})
    r = np.arange(n) / n
    bump = np.exp(-np.sin(np.pi * (r - 0.5)) ** 2 / 0.1).astype(F32)
    g = bump[:, None, None] * bump[None, :, None] * bump[None, None, :]
    wave = (1 + 0.2 * np.sin(2 * np.pi * r)[:, None, None] * np.cos(2 * np.pi * r)[None, None, :] * np.ones((1, n, 1))).astype(F32)
    s = (lambda v: (v * wave).astype(F32)) if flux else (lambda v: np.array([[[v]]], F32))
    pr["thermal_conductivity"], pr["density"], pr["specific_heat"] = s(0.5), s(1000.0), np.array([[[3600.0]]], F32)
    pr["blood_density"], pr["blood_specific_heat"] = np.array([[[1060.0]]], F32), np.array([[[3600.0]]], F32)
    pr["blood_perfusion_rate"], pr["blood_ambient_temperature"] = s(0.01), np.array([[[37.0]]], F32)
    pr["T0"], pr["Q"] = np.array([[[37.0]]], F32), (2.0e7 * g).astype(F32)
    d_max = 0.5 * 1.2 / (1000.0 * 0.8 * 3600.0)
    pr["dt"] = np.array([[[2.0 / (d_max * 3 * (np.pi / d) ** 2)]]], F32)   # the explicit-Euler limit
    reads = 3 + (3 if flux else 1) + (2 if flux else 0) + 1   # T, cem43, T_max; the divergence arrays; a and P as arrays; Q
    return pr, reads + 3                                        # T, cem43 and T_max are written back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rocfft", action="store_true", help="fused_kernels off: rocFFT and the granular kernels")
    args = ap.parse_args()
    for n in args.sizes:
        for flux in (False, True):
            pr, arrays = problem(n, flux)
            s = ThermalSolver(pr, fused_kernels=not args.rocfft, t_max=True)
            s.run(args.warmup)
            ms = s.time_steps(args.steps)
            hip, ctx = capi.load(), s.ctx
            capi.check(hip.kw_profile_enable(ctx, 1))
            s.run(args.steps)
            prof = capi.profile_collect(ctx)
            capi.check(hip.kw_profile_enable(ctx, 0))
            calls, total_ms = prof["thermal_update"]
            update_ms = total_ms / calls
            nbytes = 4 * arrays * n ** 3
            copy = C.c_double()
            capi.check(hip.kw_measure_copy_bandwidth(ctx, C.c_size_t(nbytes // 2), 20, C.byref(copy)))
            stages = {k: round(v[1] / v[0], 4) for k, v in sorted(prof.items())}
            print(json.dumps({"grid": n, "form": "flux" if flux else "laplacian", "fused_pipeline": s.fused,
                              "steps_per_s": round(args.steps / ms * 1e3, 1), "ms_per_step": round(ms / args.steps, 4),
                              "update_ms": round(update_ms, 4), "update_arrays": arrays, "update_bytes": nbytes,
                              "update_gbs": round(nbytes / update_ms / 1e6, 1), "copy_gbs_same_volume": round(copy.value, 1),
                              "peak_T": round(float(s.T_max.max()), 3), "entry_ms": stages}))
            s.close()


if __name__ == "__main__":
    main()
