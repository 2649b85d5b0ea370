"""Worker for tests/test_gpu_stokes.py: P ranks share one MI355X (gloo all-to-all through the host) on a Stokes-absorbing
problem with a pressure source that ends half way; rank 0 writes the gathered fields and the sensor series to --out."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[32, 32, 32])
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, P = dist.get_rank(), dist.get_world_size()
    nx, ny, nz = a.dims
    pr = synthetic.make_problem(nx, ny, nz, heterogeneous=True, nonlinear=True, absorbing=True, stokes=True, source="p_source",
                                source_mode=1, source_many=1, nt=a.steps, nt_src=a.steps // 2, pml_size=4, sensor="random")
    loc, info = partition_problem(pr, rank, P)
    assert int(np.asarray(loc["absorbing_flag"]).ravel()[0]) == 2
    del pr
    sim = DistSolver(loc, rank, P, nz, device_index=0, p_raw=1)
    sim.run(a.steps)
    sim.finish()
    fields = {k: sim.field(k) for k in ("p", "ux", "uz", "rhoy")}
    series = sim.stream("p") if info["sensor_positions"].size else np.zeros((a.steps, 0), dtype=np.float32)
    gathered = [None] * P if rank == 0 else None
    dist.gather_object({"fields": fields, "series": series, "pos": info["sensor_positions"]}, gathered, dst=0)
    if rank == 0:
        out = {k: np.concatenate([g["fields"][k] for g in gathered], axis=0) for k in fields}
        full = np.zeros((a.steps, sum(g["pos"].size for g in gathered)), dtype=np.float32)
        for g in gathered:
            if g["pos"].size:
                full[:, g["pos"]] = g["series"]
        out["series"] = full
        out["exchanges"] = np.array([sim.exchanges])
        np.savez(a.out, **out)
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
