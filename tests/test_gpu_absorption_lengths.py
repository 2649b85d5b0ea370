"""The Stokes and one-term power-law epilogues at every fast-path line length: kw_fused_density(terms = 4, 5, 6) and
kw_fused_absorption_pressure_one (EPI_PSUM1), short / long / masked-tile / whole-plane forms, on the grids of
test_gpu_stages.py (every length along x, y and z with the other sides 16; (n, 108, 1), whose 108 rows end every x-tile
size in a masked tile; three mixed grids; 32^3 and 64^3 with and without whole-plane kernels).

The bodies are those of test_gpu_stokes.test_density_stage_bits_and_fp64 and of test_gpu_alpha_mode.test_density_stage_terms
/ test_pressure_stage_bits_and_fp64, run on one Grid per test.  Per grid and combination they assert
  * form against form, bit for bit: plain and chained calls write the same rho, `first` and p;
    kw_fused_velocity(P_IN_SCRATCH) from the chained spectrum gives the bits of the call that reads p;
    kw_fused_absorption_pressure_one(TERMS_IN_SCRATCH) gives the bits of the unchained call;
  * epilogue against element-wise kernel, bit for bit: p equals kw_sum_pressure_stokes_* on the rho / du that the plain
    call stored, and kw_sum_pressure_terms_one_* on the stage's own inverse-transformed term.  Those kernels equal a numpy
    float32 formula exactly (test_gpu_unfused_kernels.py), so p is pinned to that formula with no tolerance;
  * t arrays a call must leave alone, read-only inputs and guard bands are unchanged;
  * fp64 (oracle/kwave_np.py, test_gpu_stages.metrics: whole array, worst line, upper half of the spectrum along the
    tested axes) for rho, stored du, `first`, the stored term and p of kw_fused_absorption_pressure_one, held to
    TOL_WHOLE, TOL_LINE and TOL_UPPER of test_gpu_stages.py: the same quantities through the same transforms those numbers
    were measured for (the one-term pressure stage sums one spectral term where the measured stage sums two).  p of the
    Stokes epilogue and p of the two composed one-term stages keep the whole-array 1e-5 of their own files.
Every reference norm is asserted > 0, except the z components of a 2-D grid, which must come out exactly 0.

Combinations: terms 4, 5 and 6 on every grid; (nonlinear, arrays) = (1, True) and (0, False) where x is the tested axis
and on the 2-D, mixed and whole-plane grids, one of the two (alternating with the grid's index) on the y and z axis grids.

These tests were not run on a GPU when they were written: no measured worst values are recorded here yet.  Each test
prints its worst (whole array / worst line / upper half) per quantity on a line that starts with ABSORPTION; the first run
on an MI355X should put the largest of them here, next to the tolerances 2.2e-6 / 5e-6 / 2.1e-6.
"""
import numpy as np
import pytest

from test_gpu_stages import AXIS_GRIDS, MIXED_GRIDS, TOL_LINE, TOL_UPPER, TOL_WHOLE, TWO_D_GRIDS, Checker, Grid
import test_gpu_alpha_mode as one_term
import test_gpu_stokes as stokes

pytestmark = pytest.mark.gpu

TOL_P = 1e-5  # whole-array bound of test_gpu_stokes.py / test_gpu_alpha_mode.py on p through two roundings of a stage
BOTH = ((1, True), (0, False))  # (nonlinear, media as arrays)
gid = lambda d: "x".join(map(str, d))  # noqa: E731


class Recorder(Checker):
    """Checker whose rows carry a reference norm > 0 — or, for the z components of a 2-D grid, an exact zero"""

    def __init__(self, axes, two_d):
        super().__init__(axes)
        self.two_d = two_d

    def __call__(self, label, got, ref):
        if self.two_d and label[-1] == "2" and (" rho" in label or " du" in label):
            assert not np.any(ref) and not np.any(got), f"{label}: not exactly zero on a 2-D grid"
            return
        assert np.linalg.norm(ref) > 0.0, f"{label}: zero reference"
        super().__call__(label, got, ref)


def check_grid(syn, dims, axes, combos, plane_kernels=1):
    g = Grid(syn, dims, plane_kernels)
    try:
        rec = Recorder(axes, g.two_d)
        loose = {}
        for nonlinear, arrays in combos:
            tag = f"nl={nonlinear} arrays={int(arrays)}"
            loose[f"stokes p {tag}"] = stokes.density_stage(g, nonlinear, arrays, rec)
            for which in (0, 1):
                errs = one_term.density_stage_terms(g, which, nonlinear, arrays, rec)
                loose[f"one-term which={which} p of both stages {tag}"] = errs["p"]
        for arrays in sorted({a for _, a in combos}):  # (the pressure stage has no nonlinear form)
            for which in (0, 1):
                err, err2, _ = one_term.pressure_stage(g, which, arrays, rec)
                loose[f"two-term entry which={which} arrays={int(arrays)}"] = err2
        g.check_readonly()
    finally:
        g.close()
    worst = {}
    for label, w, ln, up in rec.rows:
        fam = label.rstrip("012")
        worst[fam] = tuple(max(a, b) for a, b in zip(worst.get(fam, (0.0, 0.0, 0.0)), (w, ln, up)))
    print(f"\nABSORPTION {gid(dims)} plane={plane_kernels}: " +
          "; ".join(f"{k} {w:.2e}/{ln:.2e}/{up:.2e}" for k, (w, ln, up) in worst.items()) +
          f"; loose p {max(loose.values()):.2e}")
    bad = rec.failures()
    assert not bad, (dims, (TOL_WHOLE, TOL_LINE, TOL_UPPER), bad[:8])
    assert max(loose.values()) <= TOL_P, (dims, loose)


@pytest.mark.parametrize("dims", AXIS_GRIDS, ids=gid)
def test_absorption_epilogues_every_length(syn, dims):
    """every length along x, y and z with the other two sides 16.  The y and z lengths matter: the one-term stage sends
    a single array through the y-pass and Z_ABSORB, a form the two-term stages never use."""
    if dims == (16, 16, 16):
        check_grid(syn, dims, (0, 1, 2), BOTH)
        return
    tested = next(a for a in range(3) if dims[a] != 16)
    combos = BOTH if tested == 0 else (BOTH[AXIS_GRIDS.index(dims) % 2],)
    check_grid(syn, dims, (2 - tested,), combos)  # array axes are (z, y, x)


@pytest.mark.parametrize("dims", TWO_D_GRIDS, ids=gid)
def test_absorption_epilogues_masked_x_tiles_2d(syn, dims):
    """(n, 108, 1): the rows end in a partial x tile, the only way to the *_tail code objects on one GPU"""
    check_grid(syn, dims, (1, 2), BOTH)


@pytest.mark.parametrize("plane", [1, 0])
@pytest.mark.parametrize("n", [32, 64])
def test_absorption_epilogues_whole_plane_kernels(syn, n, plane):
    check_grid(syn, (n, n, n), (0, 1, 2), BOTH, plane)


@pytest.mark.parametrize("dims", MIXED_GRIDS, ids=gid)
def test_absorption_epilogues_mixed_grids(syn, dims):
    check_grid(syn, dims, (0, 1, 2), BOTH)
