"""The 256-point density and pressure-sum epilogues of k_xinv keep values in the real tile in LDS instead of in registers
(kw_fused.hip: LAST_IN_LDS, FW0_IN_LDS; switched on per line length by last_inverse_in_lds / psum_row_in_lds): the
density epilogue reads its third inverse out of the tile cell by cell, and both chained forms write the row they hand to
the forward transform into the cell they have just read.  Nothing in the arithmetic moves, so:

 (a) the chained stage gives the bits of its plain form — in what both store, and in what the consumer stage computes
     from the chained spectrum (TERMS_IN_SCRATCH / P_IN_SCRATCH) against what it computes from the plain form's stored
     arrays, which it sends through k_xfwd itself;
 (b) both forms hold the fp64 bounds of tests/test_gpu_stages.py (its Checker, its TOL_*), against the fp64 stage
     functions of oracle/kwave_np.py on the same float32 inputs.

Heterogeneous, nonlinear power-law medium (terms = 2, every medium array present), one stage call each through the
C ABI, white noise between guard bands as in test_gpu_stages.  Grids: (256, 16, 16) whole x tiles; 256 x 48 in 2-D, one
whole and one masked tile of 32 rows; (256, 100, 100), 10 000 rows = 312 whole tiles and a masked half tile, the smallest
3-D grid of supported lengths whose row count is no multiple of 32.
"""
import numpy as np
import pytest

from test_gpu_stages import (CHAIN_P, CHAIN_TERMS, P_IN_SCRATCH, TERMS_IN_SCRATCH, Checker, Grid)

pytestmark = pytest.mark.gpu

GRIDS = [(256, 16, 16), (256, 48, 1), (256, 100, 100)]


def _bits(a, b):
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


def density_and_pressure_sum(g, chk):
    """runs the stages on the Grid g, hands every output of both forms to chk with its fp64 reference and returns
    {label: number of elements whose bits differ between the chained and the plain form}"""
    rng = g.rng.bit_generator
    u = g.comps([g.noise() for _ in range(3)])
    rho = g.comps([g.noise(0.1) for _ in range(3)])
    u0 = g.comps([g.noise() for _ in range(3)])
    diff = {}

    # ---- density: plain, its consumer on the stored terms; chained, the consumer on the spectra in scratch
    s_density = rng.state
    plain, want, _ = g.density(u, rho, True, 2, True, False, 0)
    s_sum = rng.state
    p_dev, p_ref, _ = g.absorption(plain["t1"], plain["t2"], plain["t0"], True, 0)
    p_plain = p_dev.read()
    rng.state = s_density  # the same media and PML vectors
    chained, want_c, _ = g.density(u, rho, True, 2, True, False, CHAIN_TERMS)
    rng.state = s_sum
    p_dev, _, _ = g.absorption(chained["t1"], plain["t2"], plain["t0"], True, TERMS_IN_SCRATCH)
    p_scratch = p_dev.read()
    assert sorted(chained) == ["rho0", "rho1", "rho2", "t1"], sorted(chained)
    for k in plain:
        chk(f"density plain {k}", plain[k], want[k])
    for k in chained:
        chk(f"density chained {k}", chained[k], want_c[k])
        diff[f"density {k}"] = _bits(chained[k], plain[k])
    chk("pressure sum plain p", p_plain, p_ref)
    chk("pressure sum from the chained spectra p", p_scratch, p_ref)
    diff["p from the density's chained spectra"] = _bits(p_scratch, p_plain)

    # ---- pressure sum: chained; the consumer on its spectrum in scratch, then on the plain form's stored p
    rng.state = s_sum
    pc_dev, _, _ = g.absorption(plain["t1"], plain["t2"], plain["t0"], True, CHAIN_P)
    p_chained = pc_dev.read()
    chk("pressure sum chained p", p_chained, p_ref)
    diff["pressure sum p"] = _bits(p_chained, p_plain)
    s_velocity = rng.state
    u_scratch, u_ref, _ = g.velocity(p_plain, u0, True, P_IN_SCRATCH, p_dev=pc_dev)
    rng.state = s_velocity
    u_plain, _, _ = g.velocity(p_plain, u0, True, 0)
    for a in range(3):
        chk(f"velocity from the chained spectrum u{a}", u_scratch[a], u_ref[a])
        chk(f"velocity from the stored p u{a}", u_plain[a], u_ref[a])
        diff[f"u{a} from the pressure sum's chained spectrum"] = _bits(u_scratch[a], u_plain[a])
    return diff


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_chained_epilogues_give_the_bits_of_the_plain_forms_and_hold_fp64(syn, dims):
    g = Grid(syn, dims)
    try:
        chk = Checker((1, 2) if g.two_d else (2,))
        diff = density_and_pressure_sum(g, chk)
        g.check_readonly()
    finally:
        g.close()
    print("%s: worst whole %.3e line %.3e upper %.3e; elements that differ: %s" % ((dims,) + chk.worst()[:3] + (diff,)))
    assert not any(diff.values()), (dims, diff)
    bad = chk.failures()
    assert not bad, (dims, bad[:8])
