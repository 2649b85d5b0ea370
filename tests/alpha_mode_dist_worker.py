"""Worker for tests/test_gpu_alpha_mode.py: P ranks share one MI355X (gloo all-to-all through the host) on a problem with
one-term power-law absorption and a pressure source that ends half way; rank 0 writes the gathered fields, the sensor
series and the exchange callbacks per chained step to --out — for this run and for a short run of
the full power law on the same ranks, whose step has 13 transposes."""
import argparse
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kwave_amd  # noqa: E402,F401
from kwave_amd import synthetic  # noqa: E402
from kwave_amd.dist import DistSolver, partition_problem  # noqa: E402


def chained_step_exchanges(sim):
    """exchange callbacks per step, from a run of 2 and a run of 4 steps: what a run() call adds once (the spectrum of p
    left by the previous call is not taken over) drops out of the difference"""
    c0 = sim.exchanges
    sim.run(2)
    c1 = sim.exchanges
    sim.run(4)
    return ((sim.exchanges - c1) - (c1 - c0)) / 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[32, 32, 32])
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--mode", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, P = dist.get_rank(), dist.get_world_size()
    nx, ny, nz = a.dims
    kw = dict(heterogeneous=True, nonlinear=True, absorbing=True, source="p_source", source_mode=1, source_many=1, nt=a.steps,
              nt_src=a.steps // 2, pml_size=4, sensor="random")
    pr = synthetic.make_problem(nx, ny, nz, alpha_mode=a.mode, **kw)
    loc, info = partition_problem(pr, rank, P)
    assert int(np.asarray(loc["absorbing_flag"]).ravel()[0]) == synthetic.ALPHA_MODE_FLAGS[a.mode]
    del pr
    sim = DistSolver(loc, rank, P, nz, device_index=0, p_raw=1)
    sim.run(a.steps - 6)  # the source ended at steps // 2: the steps from here on are chained end to end
    per_step = chained_step_exchanges(sim)
    sim.finish()
    fields = {k: sim.field(k) for k in ("p", "ux", "uz", "rhoy")}
    series = sim.stream("p") if info["sensor_positions"].size else np.zeros((a.steps, 0), dtype=np.float32)
    sim.close()
    # the full power law on the same ranks: 13 transposes per chained step, the unit the count above is read in
    full = partition_problem(synthetic.make_problem(nx, ny, nz, **dict(kw, nt_src=2)), rank, P)[0]
    ref = DistSolver(full, rank, P, nz, device_index=0, p_raw=1)
    ref.run(4)
    per_step_full = chained_step_exchanges(ref)
    ref.close()
    gathered = [None] * P if rank == 0 else None
    dist.gather_object({"fields": fields, "series": series, "pos": info["sensor_positions"]}, gathered, dst=0)
    if rank == 0:
        out = {k: np.concatenate([g["fields"][k] for g in gathered], axis=0) for k in fields}
        full = np.zeros((a.steps, sum(g["pos"].size for g in gathered)), dtype=np.float32)
        for g in gathered:
            if g["pos"].size:
                full[:, g["pos"]] = g["series"]
        out["series"] = full
        out["exchanges_per_step"] = np.array([per_step, per_step_full])
        np.savez(a.out, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
