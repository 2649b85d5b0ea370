#!/usr/bin/env python3
"""One-term power-law absorption against the full power law and the lossless step on the bench workload (alpha_power = 1.5).

One heterogeneous nonlinear N^3 problem (p0 source, the sensor plane recorded as in bench.py), run four ways:

  power_law      absorbing_flag = 1   the absorbing pressure stage over two arrays
  no_dispersion  absorbing_flag = 3   the stage over one array: tau * F^-1{nabla1 F{rho0 sum du}}
  no_absorption  absorbing_flag = 4   the stage over one array: eta * F^-1{nabla2 F{sum rho}}
  lossless       absorbing_flag = 0   no absorption stage

Per mode: ms/step from HIP events on the solver's stream, as the median of --repeats timed blocks of --steps steps after
--warmup steps (and the spread (max - min) / median of the blocks: what a difference has to exceed), and the device
bytes the solver holds (free device memory before the solver is created minus after the warm-up).  The modes run in
one process in the order given by --modes, each in a fresh solver; run it twice with the order reversed to see what
the position in the process is worth.  To compare against an earlier build, run the same command from that build's
tree (--modes power_law,lossless: it does not know flags 3 and 4).  Per-kernel times come from a run of their own:

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/alpha_mode_compare.py --modes power_law --repeats 1

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def free_bytes(capi, ctx) -> int:
    info = capi.DeviceInfo()
    capi.check(capi.load().kw_device_info_get(ctx, C.byref(info)))
    return int(info.free_mem)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--modes", default="power_law,no_dispersion,no_absorption,lossless")
    a = ap.parse_args()
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, synthetic
    from kwave_amd.solver import HostSolver

    n, nt = a.size, a.warmup + a.repeats * a.steps + 8
    base = synthetic.make_problem(n, heterogeneous=True, nonlinear=True, absorbing=True, source="p0", nt=nt)
    flag = {"power_law": 1, "no_dispersion": 3, "no_absorption": 4, "lossless": 0}
    out = {"grid": n, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "order": a.modes.split(",")}
    probe = capi.Device()
    for mode in out["order"]:
        pr = dict(base)
        pr["absorbing_flag"] = np.array([[[flag[mode]]]], dtype=np.uint64)
        before = free_bytes(capi, probe.ctx)
        g = HostSolver(pr, p_raw=1, p_max=1)
        g.run(a.warmup)
        g.sync()
        held = before - free_bytes(capi, probe.ctx)
        blocks = [g.time_steps(a.steps) / a.steps for _ in range(a.repeats)]
        med = statistics.median(blocks)
        out[mode] = {"ms_per_step": med, "blocks_ms_per_step": blocks, "spread": (max(blocks) - min(blocks)) / med,
                     "device_bytes": int(held), "fused_pipeline": g.scalar("fused_pipeline")}
        g.close()
        del g
    probe.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
