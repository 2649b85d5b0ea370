"""Angular-spectrum projector on the GPU: kw_angular_operator against float64, the fused stage (k_yinv_angular + x-inverse)
at every fast-path line length, the stage against its rocFFT twin, and kwave_amd.angular.AngularSpectrum end to end
against the float64 NumPy restatement of tests/angular_reference.py, against the exact field of a Gaussian-apodised
aperture and against cw.FieldPropagator.

Bounds.
  kw_angular_operator  phase words within +-1 modulo 2^32 (one rounding of a float64 value, two float64 libraries);
                       b0, b1 within 2^-24 relative plus 1e-12; alive counts exact, on inputs whose restriction_margin is at
                       least 1e-9 (asserted first: a condition on the inputs).
  stage, twin, AngularSpectrum   1e-5 relative L2, the project's parity bound, against float64 of the same float32 inputs.
  amplitude / phase / heat       test_gpu_cw.py's per-element bounds.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import angular_reference as ar  # noqa: E402
import cw_reference as cr  # noqa: E402
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
PARITY = 1e-5
LENGTHS = cr.fast_lengths()
LAM = 1.0e-3
K = 2.0 * np.pi / LAM


@pytest.fixture(scope="module")
def angular():
    import kwave_amd  # noqa: F401
    from kwave_amd import angular
    return angular


@pytest.fixture()
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def operator(dev, ex, ey, spacing, k, alpha, z0, dz, nz, restrict, imported=None):
    """kw_angular_operator on the grid of the context's constants: the five natural tables as a (5, ey, nxc) uint32 array"""
    nr = (ex // 2 + 1) * ey
    tab = Guarded(dev, np.full(5 * nr, 0xDEADBEEF, np.uint32), dtype=np.uint32)
    dev.call("angular_operator", tab.ptr, imported.ptr if imported is not None else None, C.c_double(spacing[0]),
             C.c_double(spacing[1]), C.c_double(k), C.c_double(alpha), C.c_double(z0), C.c_double(dz), nz, int(restrict))
    dev.sync()
    return tab


def plane_layout(ex, ey):
    """(P, side) of the fused pipeline's plane layout for rows of ex // 2 + 1 bins"""
    nxc = ex // 2 + 1
    side = nxc % 16 == 1 and nxc > 16
    return (nxc - 1 if side else (nxc + 15) // 16 * 16), side


# ---- 1. kw_angular_operator ---------------------------------------------------------------------------------------------
OPERATOR_CASE = dict(spacing=(LAM / 3, 0.8 * LAM / 3), k=K, alpha=25.0, z0=0.37 * LAM, dz=3.7 * LAM, nz=1024)


@pytest.mark.parametrize("ex,ey", [(48, 16), (16, 100), (512, 16)])
def test_operator_against_float64(dev, ex, ey):
    p = OPERATOR_CASE
    margin = ar.restriction_margin((ex, ey), p["spacing"], p["k"], p["z0"], p["dz"], p["nz"])
    assert margin >= 1e-9, margin                    # a condition on the inputs: no bin sits on a plane's cut-off
    set_constants(dev, ex, ey, 16)
    ok = C.c_int()
    dev.call("fused_supported", C.byref(ok))
    assert ok.value == 1
    dev.call("fused_create")
    n = C.c_size_t()
    dev.call("fused_angular_elems", C.byref(n))
    P, side = plane_layout(ex, ey)
    assert n.value == P * ey + (ey if side else 0)
    imported = Guarded(dev, np.full(5 * n.value, 0xDEADBEEF, np.uint32), dtype=np.uint32)
    nxc = ex // 2 + 1
    for restrict in (True, False):
        tab = operator(dev, ex, ey, p["spacing"], p["k"], p["alpha"], p["z0"], p["dz"], p["nz"], restrict, imported)
        got = tab.read().reshape(5, ey, nxc)
        a0, a1, b0, b1, alive = ar.tables((ex, ey), p["spacing"], p["k"], p["alpha"], p["z0"], p["dz"], p["nz"], restrict)
        for name, g, w in (("a0", got[0], a0), ("a1", got[1], a1)):
            d = (g.astype(np.int64) - w.astype(np.int64)) % (1 << 32)
            d = np.minimum(d, (1 << 32) - d)
            print(f"operator {ex}x{ey} restriction {restrict} {name}: worst difference {d.max()} of 2^32 turns")
            assert d.max() <= 1, name
        for name, g, w in (("b0", got[2].view(F32), b0), ("b1", got[3].view(F32), b1)):
            assert np.all(np.abs(g.astype(np.float64) - w) <= U * np.abs(w) + 1e-12), name
        assert np.array_equal(got[4], alive)
        if restrict:
            assert alive.min() == 0 and alive.max() == p["nz"] and np.unique(alive).size > 3  # the restriction does cut here
        # the imported copy: the same words in rows of P bins, the x-Nyquist column behind them
        imp = imported.read().reshape(5, -1)
        main = imp[:, :P * ey].reshape(5, ey, P)
        assert np.array_equal(main[:, :, :nxc - 1 if side else nxc], got[:, :, :nxc - 1 if side else nxc])
        assert not main[:, :, nxc:].any()
        if side:
            assert np.array_equal(imp[:, P * ey:], got[:, :, nxc - 1])
        tab.free()
    dev.call("fused_destroy")


# ---- 2. the fused stage -------------------------------------------------------------------------------------------------
def source_pair(rng, ex, ey):
    """a random smooth pair on the whole expanded plane, with a little white noise so that every bin (the x-Nyquist column
    among them) carries something"""
    y, x = np.meshgrid(np.arange(ey) / ey, np.arange(ex) / ex, indexing="ij")
    out = []
    for _ in range(2):
        c = rng.uniform(-1.0, 1.0, 6)
        s = (c[0] + c[1] * np.cos(2 * np.pi * x + c[2]) + c[3] * np.sin(4 * np.pi * y + c[4]) * np.cos(2 * np.pi * x) +
             c[5] * np.exp(-((x - 0.4) ** 2 + (y - 0.6) ** 2) / 0.02))
        out.append((s + 0.05 * rng.standard_normal((ey, ex))).astype(F32))
    return out


class Stage:
    """a fused context of (ex, ey, zc) with a source pair transformed once; planes(j0) runs one chunk"""

    def __init__(self, dev, ex, ey, zc, sr, si):
        self.dev, self.ex, self.ey, self.zc = dev, ex, ey, zc
        set_constants(dev, ex, ey, zc)
        ok = C.c_int()
        dev.call("fused_supported", C.byref(ok))
        assert ok.value == 1, (ex, ey, zc)
        dev.call("fused_create")
        n = C.c_size_t()
        dev.call("fused_angular_elems", C.byref(n))
        self.n = n.value
        self.imported = Guarded(dev, np.zeros(5 * self.n, np.uint32), dtype=np.uint32)
        chunk = np.zeros((zc, ey, ex), F32)
        chunk[0] = sr
        self.re = Guarded(dev, chunk)
        chunk[0] = si
        self.im = Guarded(dev, chunk)
        self.spr, self.spi = Guarded(dev, np.full(2 * self.n, np.nan, F32)), Guarded(dev, np.full(2 * self.n, np.nan, F32))
        dev.call("fused_angular_forward", self.re.ptr, self.im.ptr, self.spr.ptr, self.spi.ptr)
        self.outr = Guarded(dev, np.full((zc, ey, ex), np.nan, F32))
        self.outi = Guarded(dev, np.full((zc, ey, ex), np.nan, F32))

    def tables(self, spacing, k, alpha, z0, dz, nz, restrict):
        self.tab = operator(self.dev, self.ex, self.ey, spacing, k, alpha, z0, dz, nz, restrict, self.imported)

    def planes(self, j0):
        self.dev.call("fused_angular_planes", self.spr.ptr, self.spi.ptr, self.imported.ptr, j0, self.outr.ptr, self.outi.ptr)
        self.dev.sync()
        return self.outr.read(), self.outi.read()

    def close(self):
        self.dev.call("fused_destroy")


STAGE = dict(spacing=(LAM / 3, LAM / 3), k=K, z0=0.0, dz=3.7 * LAM, nz=1024)
ALPHA_STAGE = 2.0 / (1023 * 3.7 * LAM)   # exp(-2) along the axis at the last plane


def stage_errors(dev, ex, ey):
    rng = np.random.default_rng(ex * 1009 + ey)
    sr, si = source_pair(rng, ex, ey)
    s = Stage(dev, ex, ey, 16, sr, si)
    errs = []
    for alpha in (0.0, ALPHA_STAGE):
        s.tables(STAGE["spacing"], STAGE["k"], alpha, STAGE["z0"], STAGE["dz"], STAGE["nz"], False)
        for j0 in (0, 1008):   # the last plane is 1023: a float32 product q z is ~3e-4 rad off there
            gr, gi = s.planes(j0)
            wr, wi = ar.solve_pair(sr, si, (ex, ey), STAGE["spacing"], STAGE["k"], alpha, STAGE["z0"] + j0 * STAGE["dz"],
                                   STAGE["dz"], 16, False)
            errs.append(ar.rel_l2(gr + 1j * gi.astype(np.float64), wr + 1j * wi))
        s.tab.free()
    s.close()
    return errs


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length(dev, L):
    """L x 16 (the x-inverse of two arrays; where L is a multiple of 32 it reads the x-Nyquist column back from the side
    array, whose y-pass ran at length 16 only) and 16 x L (k_yinv_angular<L>, one column tile, no side array); lossless
    and absorbing, from plane 0 and from plane 1008.  The side array here covers the x-pass side only: k_yinv_angular<L>
    with a side block is in test_stage_at_every_line_length_with_side_array."""
    for ex, ey in ((L, 16), (16, L)):
        errs = stage_errors(dev, ex, ey)
        print(f"angular stage {ex}x{ey}x16: rel L2 lossless j0=0 {errs[0]:.3e} j0=1008 {errs[1]:.3e}; "
              f"absorbing j0=0 {errs[2]:.3e} j0=1008 {errs[3]:.3e}")
        assert max(errs) < PARITY, (ex, ey)


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length_with_side_array(dev, L):
    """96 x L: k_yinv_angular<L> on three main column tiles and on the side block of the x-Nyquist column, whose lanes are
    the planes of the chunk and whose tables are the compact column behind the rows; lossless and absorbing, from plane 0
    and from plane 1008.  Measured 1.4e-7 to 2.3e-7 from plane 0 and 3.4e-7 to 7.4e-7 from plane 1008 (worst at 900)."""
    errs = stage_errors(dev, 96, L)
    print(f"angular stage 96x{L}x16: rel L2 lossless j0=0 {errs[0]:.3e} j0=1008 {errs[1]:.3e}; "
          f"absorbing j0=0 {errs[2]:.3e} j0=1008 {errs[3]:.3e}")
    assert max(errs) < PARITY, L


# ---- 3. fused against twin --------------------------------------------------------------------------------------------------
TWIN = dict(spacing=(LAM / 3, 0.8 * LAM / 3), k=K, alpha=30.0, z0=0.4 * LAM, dz=1.3 * LAM, nz=40)


@pytest.mark.parametrize("ex,ey", [(32, 48), (48, 16)])
def test_fused_stage_and_rocfft_twin(dev, ex, ey):
    from kwave_amd import capi
    p = TWIN
    rng = np.random.default_rng(ex + ey)
    sr, si = source_pair(rng, ex, ey)
    j0, zc = 16, 16
    wr, wi = ar.solve_pair(sr, si, (ex, ey), p["spacing"], p["k"], p["alpha"], p["z0"] + j0 * p["dz"], p["dz"], zc, True)
    want = wr + 1j * wi
    s = Stage(dev, ex, ey, zc, sr, si)
    s.tables(p["spacing"], p["k"], p["alpha"], p["z0"], p["dz"], p["nz"], True)
    gr, gi = s.planes(j0)
    fused = ar.rel_l2(gr + 1j * gi.astype(np.float64), want)
    s.close()
    # the twin: 2-D plans of (ex, ey, 1), kw_angular_mix on the natural tables, one C2R transform per plane and part
    d2 = capi.Device()
    try:
        set_constants(d2, ex, ey, 1)
        d2.call("fft_create_plans_3d")
        nr = (ex // 2 + 1) * ey
        tab = operator(d2, ex, ey, p["spacing"], p["k"], p["alpha"], p["z0"], p["dz"], p["nz"], True)
        bre, bim = Guarded(d2, sr), Guarded(d2, si)
        spr, spi = Guarded(d2, np.zeros(2 * nr, F32)), Guarded(d2, np.zeros(2 * nr, F32))
        d2.call("fft_r2c_3d", bre.ptr, spr.ptr)
        d2.call("fft_r2c_3d", bim.ptr, spi.ptr)
        mr, mi = Guarded(d2, np.full(2 * nr * zc, np.nan, F32)), Guarded(d2, np.full(2 * nr * zc, np.nan, F32))
        d2.call("angular_mix", mr.ptr, mi.ptr, spr.ptr, spi.ptr, tab.ptr, nr, zc, j0, 1.0 / (ex * ey))
        outr, outi = Guarded(d2, np.full((zc, ey, ex), np.nan, F32)), Guarded(d2, np.full((zc, ey, ex), np.nan, F32))
        for z in range(zc):
            d2.call("fft_c2r_3d", mr.ptr + 8 * nr * z, outr.ptr + 4 * ex * ey * z)
            d2.call("fft_c2r_3d", mi.ptr + 8 * nr * z, outi.ptr + 4 * ex * ey * z)
        d2.sync()
        twin = ar.rel_l2(outr.read() + 1j * outi.read().astype(np.float64), want)
        d2.call("angular_mix", None, None, None, None, None, 0, 4, 0, 1.0)   # no bins: no pointer is looked at
    finally:
        d2.close()
    print(f"angular {ex}x{ey}: fused stage {fused:.3e}, rocFFT twin {twin:.3e} (rel L2 against float64)")
    assert fused < PARITY and twin < PARITY


def test_stage_refuses_two_d_and_slab_contexts(dev):
    from kwave_amd import capi
    a = Guarded(dev, np.zeros(32 * 32 * 16, F32))
    b = Guarded(dev, np.zeros(32 * 32 * 16, F32))
    t = Guarded(dev, np.zeros(5 * 32 * 32, np.uint32), dtype=np.uint32)
    set_constants(dev, 32, 32, 1)
    dev.call("fused_create")
    for entry, args in (("fused_angular_planes", (a.ptr, b.ptr, t.ptr, 0, a.ptr, b.ptr)),
                        ("fused_angular_forward", (a.ptr, b.ptr, a.ptr, b.ptr))):
        with pytest.raises(capi.KWaveError, match=r"no Z-slabs, no Nz == 1"):
            dev.call(entry, *args)
    dev.call("fused_destroy")
    # one rank with an exchange callback = the slab path against itself; the callback is never reached
    exchange = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)(lambda *args: 1)
    set_constants(dev, 32, 32, 16)
    dev.call("fused_set_slab", 1, 0, 16, C.cast(exchange, C.c_void_p), None)
    dev.call("fused_create")
    with pytest.raises(capi.KWaveError, match=r"no Z-slabs, no Nz == 1"):
        dev.call("fused_angular_planes", a.ptr, b.ptr, t.ptr, 0, a.ptr, b.ptr)
    dev.call("fused_destroy")


# ---- 4. AngularSpectrum end to end ------------------------------------------------------------------------------------------
C0 = 1500.0
E2E = dict(dims=(24, 20), spacing=(1.0e-3, 0.8e-3), f0=C0 / 3.0e-3, z0=0.5e-3, dz=1.1e-3, planes=20)


def e2e_source(seed):
    rng = np.random.default_rng(seed)
    shape = E2E["dims"][::-1]
    return rng.uniform(0.2, 1.0, shape).astype(F32), rng.uniform(-np.pi, np.pi, shape).astype(F32)


@functools.lru_cache(maxsize=None)
def e2e_reference(alpha, restrict, expanded, seed):
    amp, phase = e2e_source(seed)
    P0 = amp.astype(np.float64) * np.exp(1j * phase.astype(np.float64))
    k = 2.0 * np.pi * E2E["f0"] / C0
    return ar.project(P0, E2E["spacing"], k, alpha, E2E["z0"], E2E["dz"], E2E["planes"], expanded, restrict)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
@pytest.mark.parametrize("restrict", [True, False], ids=["restricted", "unrestricted"])
@pytest.mark.parametrize("alpha", [0.0, 30.0], ids=["lossless", "absorbing"])
def test_angular_spectrum_against_the_restatement(angular, alpha, restrict, fused):
    """20 planes in chunks of 16: two chunks, the second one partial"""
    expanded = (48, 48) if fused else (48, 40)
    p = angular.AngularSpectrum(E2E["dims"], E2E["spacing"], C0, E2E["f0"], E2E["z0"], E2E["dz"], E2E["planes"], alpha_np=alpha,
                                angular_restriction=restrict, chunk_planes=16, fused_kernels=fused)
    try:
        assert p.fused == fused and p.expanded == expanded and p.chunk_planes == 16
        got = p.run(*e2e_source(1))
        assert got.dtype == np.complex64 and got.shape == (20, 20, 24)
        err = ar.rel_l2(got, e2e_reference(alpha, restrict, expanded, 1))
        print(f"AngularSpectrum alpha {alpha} restriction {restrict} fused {fused}: rel L2 {err:.3e}")
        assert err < PARITY
        # a second run with another plane, handed in as parts, reuses the tables
        a2, ph2 = e2e_source(2)
        P2 = a2.astype(np.float64) * np.exp(1j * ph2.astype(np.float64))
        re2, im2 = P2.real.astype(F32), P2.imag.astype(F32)
        got2 = p.run_parts(re2, im2)
        k = 2.0 * np.pi * E2E["f0"] / C0
        want2 = ar.project(re2.astype(np.float64) + 1j * im2, E2E["spacing"], k, alpha, E2E["z0"], E2E["dz"], E2E["planes"],
                           expanded, restrict)
        assert p.runs == 2 and ar.rel_l2(got2, want2) < PARITY
        p.project()                                   # the chunks alone give the same planes again
        assert np.array_equal(p._result(), got2)
        amp, ph = p.amplitude(), p.phase()
        assert np.all(np.abs(amp - np.abs(got2)) <= 4 * U * np.abs(got2))
        assert np.all(np.abs(ph.astype(np.float64) - np.angle(got2.astype(np.complex128))) <= 2.0 ** -22)
        rho0 = 1000.0
        Q = p.heat(30.0, rho0)
        want_q = 30.0 / (rho0 * C0) * np.abs(got2.astype(np.complex128)) ** 2
        assert np.all(np.abs(Q - want_q) <= 6 * U * want_q)      # the float32 rounding of q itself on top of the kernel's 4
        assert np.array_equal(p.heat(np.full(p.shape, 30.0), rho0), Q)
    finally:
        p.close()


def test_chunk_size_does_not_change_a_plane(angular):
    """70 planes by the default chunk (64: one whole, one of six planes) and in chunks of 16, 32 and 48: H of a plane
    depends on its index alone, so every plane comes out bit for bit the same"""
    amp, phase = e2e_source(3)
    k = 2.0 * np.pi * E2E["f0"] / C0
    got = {}
    for zc in (None, 16, 32, 48):
        p = angular.AngularSpectrum(E2E["dims"], E2E["spacing"], C0, E2E["f0"], E2E["z0"], E2E["dz"], 70, alpha_np=30.0,
                                    chunk_planes=zc)
        try:
            assert p.fused and p.chunk_planes == (zc or 64)
            got[zc] = p.run(amp, phase)
        finally:
            p.close()
    P0 = amp.astype(np.float64) * np.exp(1j * phase.astype(np.float64))
    assert ar.rel_l2(got[None], ar.project(P0, E2E["spacing"], k, 30.0, E2E["z0"], E2E["dz"], 70, (48, 48))) < PARITY
    for zc in (16, 32, 48):
        assert np.array_equal(got[zc], got[None]), zc


# ---- 5. the exact aperture field ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restrict", [True, False], ids=["restricted", "unrestricted"])
def test_exact_aperture_field(angular, restrict):
    n, dx = 32, 1.0e-3
    f0 = C0 / (3.0 * dx)
    k = 2.0 * np.pi * f0 / C0
    P0 = ar.aperture_field(n, dx, k, 4 * dx)
    exact = np.stack([ar.aperture_field(n, dx, k, (4 + j) * dx) for j in range(13)])
    re, im = P0.real.astype(F32), P0.imag.astype(F32)
    own = ar.rel_l2(ar.project(re.astype(np.float64) + 1j * im, (dx, dx), k, 0.0, 0.0, dx, 13, (64, 64), restrict), exact)
    p = angular.AngularSpectrum((n, n), (dx, dx), C0, f0, 0.0, dx, 13, angular_restriction=restrict, expanded=(64, 64))
    try:
        assert p.fused and p.chunk_planes == 16
        got = p.run_parts(re, im)
    finally:
        p.close()
    err = ar.rel_l2(got, exact)
    print(f"aperture field, restriction {restrict}: GPU against exact {err:.3e}, restatement against exact {own:.3e}")
    assert err <= PARITY + own


# ---- 6. agreement with FieldPropagator ---------------------------------------------------------------------------------------
def test_agrees_with_field_propagator(angular):
    """32^3 at 4 points per wavelength, a Gaussian (sigma = 3 cells) source plane at z-index 4: FieldPropagator's plane 10
    projected over the 22 planes downstream.  The two float64 restatements differ by the lateral truncation of the plane
    (measured 3.6e-3); the GPU results must agree within twice that."""
    from kwave_amd import cw
    n, dx = 32, 1.0e-3
    f0 = C0 / (4.0 * dx)
    k = 2.0 * np.pi * f0 / C0
    c = (np.arange(n) - (n - 1) / 2.0)
    S = np.zeros((n, n, n), F32)
    S[4] = np.exp(-(c[None, :] ** 2 + c[:, None] ** 2) / (2.0 * 3.0 ** 2)).astype(F32)
    T, e = cr.plan((n, n, n), (dx, dx, dx), C0)
    vol = cr.propagate(S.astype(np.float64), (dx, dx, dx), C0, f0, T, e)
    figure = ar.rel_l2(ar.project(vol[10], (dx, dx), k, 0.0, 0.0, dx, 22, (64, 64)), vol[10:])
    fp = cw.FieldPropagator((n, n, n), (dx, dx, dx), C0, f0)
    try:
        assert fp.expanded == e
        field = fp.run_parts(S, np.zeros_like(S))
    finally:
        fp.close()
    p = angular.AngularSpectrum((n, n), (dx, dx), C0, f0, 0.0, dx, 22, expanded=(64, 64))
    try:
        got = p.run_parts(field[10].real, field[10].imag)
    finally:
        p.close()
    err = ar.rel_l2(got, field[10:])
    print(f"AngularSpectrum against FieldPropagator over 22 planes: GPU to GPU {err:.3e}, float64 restatements {figure:.3e}")
    assert figure < 1e-2
    assert err <= 2 * figure
