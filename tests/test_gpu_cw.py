"""CW field propagator on the GPU: each device entry point on its own against float64 of the same float32 inputs, the
fused pair stage at every fast-path line length, and kwave_amd.cw.FieldPropagator end to end against the float64 NumPy
restatement of tests/cw_reference.py and against the project's own time loop.

Bounds.
  kw_cw_operator   |g32 - g64| <= 2^-24 |g64| + 1e-12 max|G| per component: one float32 rounding of a float64 value, plus the
                   difference of two float64 libraries at arguments of up to thousands of radians.
  kw_cw_mix        3 * 2^-24 * (|gr x| + |gi y|) per element: two products and one sum, each rounded once, no contraction.
  kw_fused_cw_pair 1e-5 relative L2 on Re and on Im, the project's parity bound; the same for its rocFFT twin.
  kw_cw_embed      copies and the zero fill exact; scaled: 3 * 2^-24 * (|a sr| + |b si|) (two products, one sum);
                   amplitude / phase form: 6 * 2^-24 * |A| (sincosf within 2 units of the last place of a value <= 1, i.e.
                   4 * 2^-24, one product, one to spare).
  kw_cw_extract    copies exact; |P| and Q within 4 * 2^-24 relative (two squares, a sum, the root or the product with q);
                   the phase within 2^-22 rad where |P| is above 1e-3 of its maximum (float64 atan2 rounded once: half a
                   float32 spacing at pi is 2^-23).
  FieldPropagator  1e-5 relative L2 against the restatement fed the same float32 source.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import cw_reference as cr  # noqa: E402
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
PARITY = 1e-5
LENGTHS = cr.fast_lengths()
MIXED = [(16, 32, 48), (48, 16, 32), (32, 32, 16)]   # (nx, ny, nz); the last: whole-plane x kernels with two arrays


@pytest.fixture(scope="module")
def cw():
    import kwave_amd  # noqa: F401
    from kwave_amd import cw
    return cw


@pytest.fixture()
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


# ---- 1. kw_cw_operator ---------------------------------------------------------------------------------------------------
def test_operator_against_float64(dev):
    nx, ny, nz = 16, 32, 48
    spacing = (1.0e-3, 0.7e-3, 0.9e-3)
    c0, f0 = 1500.0, 400e3
    T = 40 * cr.default_time((nx, ny, nz), spacing, c0)      # a T up to ~1e3 rad
    set_constants(dev, nx, ny, nz)
    nr = (nx // 2 + 1) * ny * nz
    gre, gim = Guarded(dev, np.full(nr, np.nan, F32)), Guarded(dev, np.full(nr, np.nan, F32))
    dk = [2.0 * np.pi / (n * d) for n, d in zip((nx, ny, nz), spacing)]
    dev.call("cw_operator", gre.ptr, gim.ptr, C.c_double(c0), C.c_double(2.0 * np.pi * f0), C.c_double(T),
             C.c_double(dk[0]), C.c_double(dk[1]), C.c_double(dk[2]))
    dev.sync()
    want = cr.stored_operator((nx, ny, nz), spacing, c0, f0, T, half=True).reshape(-1)
    top = np.abs(want).max()
    assert c0 * cr.wavenumber_magnitude((nx, ny, nz), spacing, half=True).max() * T > 500.0
    for name, got, ref in (("re", gre.read(), want.real), ("im", gim.read(), want.imag)):
        err = np.abs(got.astype(np.float64) - ref)
        bound = U * np.abs(ref) + 1e-12 * top
        print(f"operator {name}: worst |g32 - g64| / bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound), name


# ---- 2. kw_cw_mix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,offset", [(1, 0), (2, 0), (5, 0), (1027, 0), (1027, 8), (1100001, 0)])
def test_mix_against_float64(dev, n, offset):
    rng = np.random.default_rng(n + offset)
    x, y = rng.standard_normal(2 * n).astype(F32), rng.standard_normal(2 * n).astype(F32)
    gr, gi = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    bx, by = Guarded(dev, x, offset), Guarded(dev, y, offset)
    bgr, bgi = Guarded(dev, gr, offset // 2), Guarded(dev, gi, offset // 2)
    dev.call("cw_mix", bx.ptr, by.ptr, bgr.ptr, bgi.ptr, n)
    dev.sync()
    x8, y8 = x.astype(np.float64), y.astype(np.float64)
    r8, i8 = np.repeat(gr.astype(np.float64), 2), np.repeat(gi.astype(np.float64), 2)
    for name, got, ref, M in (("re", bx.read(), r8 * x8 - i8 * y8, np.abs(r8 * x8) + np.abs(i8 * y8)),
                              ("im", by.read(), i8 * x8 + r8 * y8, np.abs(i8 * x8) + np.abs(r8 * y8))):
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 3 * U * M), name
    assert np.array_equal(bgr.read(), gr) and np.array_equal(bgi.read(), gi)
    dev.call("cw_mix", None, None, None, None, 0)   # n == 0 looks at no pointer


# ---- 3. kw_fused_cw_pair ------------------------------------------------------------------------------------------------
def smooth_operator(rng, nx, ny, nz):
    """a random smooth real pair on the reduced grid, symmetric under k -> -k on every axis (so that the half-spectrum
    products stay Hermitian), 1 / N folded in, float32"""
    ix, iy, iz = np.arange(nx // 2 + 1), np.arange(ny), np.arange(nz)
    out = []
    for _ in range(2):
        c = rng.uniform(-1.0, 1.0, 7)
        g = (c[0] + c[1] * np.cos(2 * np.pi * ix / nx)[None, None, :] + c[2] * np.cos(2 * np.pi * iy / ny)[None, :, None] +
             c[3] * np.cos(2 * np.pi * iz / nz)[:, None, None] + c[4] * np.cos(4 * np.pi * iy / ny)[None, :, None] *
             np.cos(2 * np.pi * ix / nx)[None, None, :] + c[5] * np.cos(4 * np.pi * iz / nz)[:, None, None] +
             c[6] * np.cos(6 * np.pi * iz / nz)[:, None, None] * np.cos(2 * np.pi * iy / ny)[None, :, None])
        out.append((g / (nx * ny * nz)).astype(F32))
    return out


def pair_case(dev, nx, ny, nz, twin):
    rng = np.random.default_rng(nx * 1000003 + ny * 1009 + nz)
    sr, si = rng.standard_normal((nz, ny, nx)).astype(F32), rng.standard_normal((nz, ny, nx)).astype(F32)
    gr, gi = smooth_operator(rng, nx, ny, nz)
    G = gr.astype(np.float64) + 1j * gi.astype(np.float64)
    wr, wi = cr.solve_pair(sr.astype(np.float64), si.astype(np.float64), G)   # unnormalised inverse, like the device's
    set_constants(dev, nx, ny, nz)
    ok = C.c_int()
    dev.call("fused_supported", C.byref(ok))
    assert ok.value == 1, (nx, ny, nz)
    dev.call("fused_create")
    n = C.c_size_t()
    dev.call("fused_reduced_elems", C.byref(n))
    bgr, bgi = Guarded(dev, gr), Guarded(dev, gi)
    pgr, pgi = Guarded(dev, np.full(n.value, np.nan, F32)), Guarded(dev, np.full(n.value, np.nan, F32))
    dev.call("fused_import_reduced", pgr.ptr, bgr.ptr)
    dev.call("fused_import_reduced", pgi.ptr, bgi.ptr)
    bre, bim = Guarded(dev, sr), Guarded(dev, si)
    dev.call("fused_cw_pair", bre.ptr, bim.ptr, pgr.ptr, pgi.ptr)
    dev.sync()
    errs = [cr.rel_l2(bre.read(), wr), cr.rel_l2(bim.read(), wi)]
    if twin:  # the rocFFT path on the same inputs
        nr = (nx // 2 + 1) * ny * nz
        dev.call("fft_create_plans_3d")
        tre, tim = Guarded(dev, sr), Guarded(dev, si)
        spr, spi = Guarded(dev, np.zeros(2 * nr, F32)), Guarded(dev, np.zeros(2 * nr, F32))
        dev.call("fft_r2c_3d", tre.ptr, spr.ptr)
        dev.call("fft_r2c_3d", tim.ptr, spi.ptr)
        dev.call("cw_mix", spr.ptr, spi.ptr, bgr.ptr, bgi.ptr, nr)
        dev.call("fft_c2r_3d", spr.ptr, tre.ptr)
        dev.call("fft_c2r_3d", spi.ptr, tim.ptr)
        dev.sync()
        errs += [cr.rel_l2(tre.read(), wr), cr.rel_l2(tim.read(), wi)]
    dev.call("fused_destroy")
    return errs


@pytest.mark.parametrize("L", LENGTHS)
def test_pair_stage_at_every_line_length(dev, L):
    """16 x 16 x L: the z kernel is the new code; a length whose factorisation or wave count it gets wrong shows here"""
    errs = pair_case(dev, 16, 16, L, twin=False)
    print(f"fused pair 16x16x{L}: rel L2 re {errs[0]:.3e} im {errs[1]:.3e}")
    assert max(errs) < PARITY


@pytest.mark.parametrize("L", LENGTHS)
def test_pair_stage_at_every_line_length_with_side_array(dev, L):
    """96 x 16 x L: k_zfused_pair<L> (k_zfused_pair_split for the 2 x 256 form of 512) on three main column tiles (two
    32-column ones, the second half valid, at 240 and 400) and on the side block of the x-Nyquist column, which reads both
    operator parts from the per-length side rows that kw_fused_import_reduced wrote.  White-noise sources: that column
    carries 1 / 96 of the energy.  Measured 2.0e-7 to 2.7e-7 (worst at 864)."""
    errs = pair_case(dev, 96, 16, L, twin=False)
    print(f"fused pair 96x16x{L}: rel L2 re {errs[0]:.3e} im {errs[1]:.3e}")
    assert max(errs) < PARITY


@pytest.mark.parametrize("dims", MIXED, ids=["x".join(map(str, d)) for d in MIXED])
def test_pair_stage_on_mixed_grids_and_its_rocfft_twin(dev, dims):
    errs = pair_case(dev, *dims, twin=True)
    print(f"fused pair {dims}: rel L2 re {errs[0]:.3e} im {errs[1]:.3e}; rocFFT twin re {errs[2]:.3e} im {errs[3]:.3e}")
    assert max(errs) < PARITY


def test_pair_stage_refuses_two_d(dev):
    from kwave_amd import capi
    set_constants(dev, 32, 32, 1)
    dev.call("fused_create")
    a, b = Guarded(dev, np.zeros(1024, F32)), Guarded(dev, np.zeros(1024, F32))
    with pytest.raises(capi.KWaveError, match="single GPU and 3-D only"):
        dev.call("fused_cw_pair", a.ptr, b.ptr, a.ptr, b.ptr)
    dev.call("fused_destroy")


# ---- 4. kw_cw_embed / kw_cw_extract -------------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 255, 256, 257, "n_big"]


def embed_dims(dev, n):
    """(ex, ey, ez, nx, ny, nz): a small 3-D corner for the small sizes; for n_big one row longer than the grid-stride span
    of the 16-byte kernels (CU count x 8 blocks x 256 lanes x 4 floats)"""
    if n == "n_big":
        n = dev.info().compute_units * 8 * 256 * 4 + 4
        return n + 4, 1, 2, n, 1, 1
    return n + 4, 3, 4, n, 2, 3


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "off_by_one_float"])
@pytest.mark.parametrize("n", SIZES)
def test_embed_against_numpy(dev, n, offset):
    ex, ey, ez, nx, ny, nz = embed_dims(dev, n)
    rng = np.random.default_rng(nx + offset)
    a, b = rng.standard_normal((nz, ny, nx)).astype(F32), rng.uniform(-4.0, 4.0, (nz, ny, nx)).astype(F32)
    a8, b8 = a.astype(np.float64), b.astype(np.float64)
    ba, bb = Guarded(dev, a, offset), Guarded(dev, b, offset)
    sr, si = 0.75, -1.25
    forms = [(1, 1.0, 0.0, a8, b8, None),
             (1, sr, si, a8 * sr - b8 * si, a8 * si + b8 * sr, (3 * U * (np.abs(a8 * sr) + np.abs(b8 * si)),
                                                                3 * U * (np.abs(a8 * si) + np.abs(b8 * sr)))),
             (0, 1.0, 0.0, a8 * np.cos(b8), a8 * np.sin(b8), (6 * U * np.abs(a8),) * 2)]
    if n == "n_big":
        forms = forms[:2]
    for parts, fr, fi, wr, wi, bound in forms:
        ere, eim = Guarded(dev, np.full((ez, ey, ex), np.nan, F32), offset), Guarded(dev, np.full((ez, ey, ex), np.nan, F32), offset)
        dev.call("cw_embed", ere.ptr, eim.ptr, ba.ptr, bb.ptr, parts, fr, fi, ex, ey, ez, nx, ny, nz)
        dev.sync()
        for got, want, bnd in ((ere.read(), wr, bound and bound[0]), (eim.read(), wi, bound and bound[1])):
            corner = got[:nz, :ny, :nx]
            outside = got.copy()
            outside[:nz, :ny, :nx] = 0.0
            assert not outside.any() and not np.signbit(outside).any()        # the zero fill: +0 everywhere
            if bnd is None:
                assert np.array_equal(corner.view(np.uint32), want.astype(F32).view(np.uint32))
            else:
                assert np.all(np.abs(corner.astype(np.float64) - want) <= bnd)
        ere.free()
        eim.free()
    assert np.array_equal(ba.read(), a) and np.array_equal(bb.read(), b)
    dev.call("cw_embed", None, None, None, None, 1, 1.0, 0.0, 0, 4, 4, 0, 2, 2)   # no points: no pointer is looked at


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "off_by_one_float"])
@pytest.mark.parametrize("n", SIZES)
def test_extract_against_numpy(dev, n, offset):
    ex, ey, ez, nx, ny, nz = embed_dims(dev, n)
    rng = np.random.default_rng(nx + 7 * offset)
    re, im = rng.standard_normal((ez, ey, ex)).astype(F32), rng.standard_normal((ez, ey, ex)).astype(F32)
    re[0, 0, 0], im[0, 0, 0] = -2.0, 0.0                                      # phase pi: the widest float32 spacing
    q = rng.uniform(0.5, 2.0, (nz, ny, nx)).astype(F32)
    bre, bim, bq = Guarded(dev, re, offset), Guarded(dev, im, offset), Guarded(dev, q, offset)
    outs = {k: Guarded(dev, np.full((nz, ny, nx), np.nan, F32), offset) for k in ("re", "im", "amp", "phase", "Q")}
    dev.call("cw_extract", bre.ptr, bim.ptr, ex, ey, ez, nx, ny, nz, outs["re"].ptr, outs["im"].ptr, outs["amp"].ptr,
             outs["phase"].ptr, outs["Q"].ptr, bq.ptr, 0.0)
    dev.sync()
    r8, i8 = re[:nz, :ny, :nx].astype(np.float64), im[:nz, :ny, :nx].astype(np.float64)
    assert np.array_equal(outs["re"].read().view(np.uint32), re[:nz, :ny, :nx].view(np.uint32))
    assert np.array_equal(outs["im"].read().view(np.uint32), im[:nz, :ny, :nx].view(np.uint32))
    amp = np.hypot(r8, i8)
    assert np.all(np.abs(outs["amp"].read() - amp) <= 4 * U * amp)
    Q = q.astype(np.float64) * amp ** 2
    assert np.all(np.abs(outs["Q"].read() - Q) <= 4 * U * Q)
    keep = amp > 1e-3 * amp.max()
    assert np.all(np.abs(outs["phase"].read().astype(np.float64) - np.arctan2(i8, r8))[keep] <= 2.0 ** -22)
    assert outs["phase"].read()[0, 0, 0] == F32(np.pi)
    # a scalar q, and every output but one left out
    only = Guarded(dev, np.full((nz, ny, nx), np.nan, F32), offset)
    dev.call("cw_extract", bre.ptr, bim.ptr, ex, ey, ez, nx, ny, nz, None, None, None, None, only.ptr, None, 1.5)
    dev.sync()
    assert np.all(np.abs(only.read() - 1.5 * amp ** 2) <= 4 * U * 1.5 * amp ** 2)
    assert np.array_equal(bre.read(), re) and np.array_equal(bim.read(), im)
    dev.call("cw_extract", None, None, 4, 4, 4, 0, 2, 2, None, None, None, None, None, None, 0.0)


# ---- 5. FieldPropagator end to end --------------------------------------------------------------------------------------
C0 = 1500.0
E2E = {  # name -> dims, spacing, expanded (None: default), fused_kernels, path the case is meant to take
    "fused": ((8, 12, 10), (1.0e-3, 0.7e-3, 0.9e-3), None, True, True),
    "rocfft_same_domain": ((8, 12, 10), (1.0e-3, 0.7e-3, 0.9e-3), None, False, False),
    "rocfft_side_22": ((6, 8, 8), (1.0e-3, 1.0e-3, 1.0e-3), (22, 24, 26), True, False),
}


def e2e_source(dims, seed):
    rng = np.random.default_rng(seed)
    shape = dims[::-1]
    return rng.uniform(0.2, 1.0, shape).astype(F32), rng.uniform(-np.pi, np.pi, shape).astype(F32)


@functools.lru_cache(maxsize=None)
def e2e_reference(name, seed):
    dims, spacing, expanded, fused, _ = E2E[name]
    f0 = C0 / (6.0 * max(spacing))
    T, e = cr.plan(dims, spacing, C0, fused=fused)
    e = expanded or e
    amp, phase = e2e_source(dims, seed)
    S = amp.astype(np.float64) * np.exp(1j * phase.astype(np.float64))
    return f0, T, e, cr.propagate(S, spacing, C0, f0, T, e)


@pytest.mark.parametrize("name", list(E2E))
def test_field_propagator_against_the_restatement(cw, name):
    dims, spacing, expanded, fused, fast = E2E[name]
    f0, T, e, want = e2e_reference(name, 1)
    p = cw.FieldPropagator(dims, spacing, C0, f0, expanded=expanded, fused_kernels=fused)
    try:
        assert p.fused == fast and p.expanded == e and p.t == T
        if name == "fused":
            assert p.expanded == (32, 48, 32)
        got = p.run(*e2e_source(dims, 1))
        assert got.dtype == np.complex64 and got.shape == dims[::-1]
        err = cr.rel_l2(got, want)
        print(f"FieldPropagator {name}: rel L2 {err:.3e}")
        assert err < PARITY
        # a second run with another source reuses the operator
        got2 = p.run(*e2e_source(dims, 2))
        assert p.runs == 2 and cr.rel_l2(got2, e2e_reference(name, 2)[3]) < PARITY
        # the other outputs belong to the last run
        amp, ph = p.amplitude(), p.phase()
        assert np.all(np.abs(amp - np.abs(got2)) <= 4 * U * np.abs(got2))
        assert np.all(np.abs(ph.astype(np.float64) - np.angle(got2.astype(np.complex128))) <= 2.0 ** -22)
        alpha, rho0 = 5.0, 1000.0
        Q = p.heat(alpha, rho0)
        want_q = alpha / (rho0 * C0) * np.abs(got2.astype(np.complex128)) ** 2
        assert np.all(np.abs(Q - want_q) <= 6 * U * want_q)      # the float32 rounding of q itself on top of the kernel's 4
        Qa = p.heat(np.full(dims[::-1], alpha), rho0)
        assert np.array_equal(Qa, Q)
    finally:
        p.close()


def test_run_elements_with_two_discs(cw):
    import kwave_amd  # noqa: F401
    from kwave_amd import arrays
    dims, spacing = (16, 16, 12), (1.0e-3, 1.0e-3, 1.0e-3)
    f0 = C0 / (6.0 * 1.0e-3)
    grid = arrays.Grid(*dims, *spacing)
    shapes = [arrays.disc_element(grid, (-2.2e-3, 0.3e-3, -1.0e-3), 2.0e-3), arrays.disc_element(grid, (2.4e-3, -0.6e-3, -1.0e-3), 2.0e-3)]
    elements = arrays.offgrid_elements(None, grid, shapes)
    amplitudes, phases = [1.0, 0.6], [0.3, -1.1]
    p = cw.FieldPropagator(dims, spacing, C0, f0)
    try:
        got = p.run_elements(elements, amplitudes, phases)
        T, e = p.t, p.expanded
    finally:
        p.close()
    # the reference, fed the expanded CSR
    drive = np.stack([np.array(amplitudes) * np.cos(phases), np.array(amplitudes) * np.sin(phases)]).astype(F32)
    ds = arrays.weighted_source(elements, drive)
    rows = arrays.expand_source(ds).reshape(2, -1).astype(np.float64)
    S = np.zeros(dims[0] * dims[1] * dims[2], dtype=np.complex128)
    S[ds["p_source_index"].reshape(-1).astype(np.int64) - 1] = rows[0] + 1j * rows[1]
    assert np.count_nonzero(S) > 20
    want = cr.propagate(S.reshape(dims[::-1]), spacing, C0, f0, T, e)
    err = cr.rel_l2(got, want)
    print(f"run_elements, two discs: rel L2 {err:.3e}")
    assert err < PARITY


# ---- 6. agreement with the time loop ------------------------------------------------------------------------------------
def time_loop_case():
    """32^3, homogeneous, lossless, linear, PML on: a 3 x 3 patch drives p_s sin(w t) as an additive source until steady;
    returns the problem, the patch, the comparison points and the frequency"""
    import kwave_amd  # noqa: F401
    from kwave_amd import synthetic
    n, pml, steps_per_period, periods, p_s = 32, 6, 27, 14, 1.0e5
    nt = steps_per_period * periods
    pr = synthetic.make_problem(n, heterogeneous=False, nonlinear=False, absorbing=False, source="p_source", source_mode=2,
                                source_many=0, nt=nt, pml_size=pml)
    dt, dx = float(pr["dt"].ravel()[0]), float(pr["dx"].ravel()[0])
    f0 = 1.0 / (steps_per_period * dt)
    xs, c = 12, n // 2
    patch = [(z, y, xs) for z in (c - 1, c, c + 1) for y in (c - 1, c, c + 1)]
    lin = np.sort(np.array([(z * n + y) * n + x for z, y, x in patch], dtype=np.uint64)) + np.uint64(1)
    t = np.arange(nt, dtype=np.float64) * dt
    # k-Wave's scaling of an additive pressure source: source.p * 2 dt / (N c0 dx), N = 3, per density component
    pr["p_source_input"] = (p_s * np.sin(2.0 * np.pi * f0 * t) * 2.0 * dt / (3.0 * C0 * dx)).astype(F32).reshape(1, nt, 1)
    pr["p_source_index"] = lin.reshape(1, 1, -1)
    pr["p_source_flag"] = np.array([[[nt]]], dtype=np.uint64)
    # comparison points: at least 4 cells from the PML and from the patch, every 2nd along y and z
    lo, hi = pml + 4, n - pml - 4
    pts = [(z, y, x) for z in range(lo, hi, 2) for y in range(lo, hi, 2) for x in range(lo, hi)
           if max(abs(z - c) - 1, abs(y - c) - 1, abs(x - xs), 0) >= 4]
    sensor = np.sort(np.array([(z * n + y) * n + x for z, y, x in pts], dtype=np.uint64)) + np.uint64(1)
    pr["sensor_mask_index"] = sensor.reshape(1, 1, -1)
    return pr, patch, sensor.astype(np.int64) - 1, f0, dt, dx, steps_per_period, periods, p_s


# the first measurement: 4.327e-4 relative L2 at 282 points, mean ratio 1.0002 — no constant factor, so the
# source scale and the extraction hold; the bound is twice that
TIME_LOOP_BOUND = 2 * 4.327e-4


def test_amplitude_agrees_with_the_time_loop(cw):
    """|P| from FieldPropagator(source_scale="kwave") against the amplitude of the time loop's steady state over its last
    whole periods.  The margin over the measured difference covers the PML's residual reflection and the period window."""
    from kwave_amd.solver import HostSolver
    pr, patch, points, f0, dt, dx, spp, periods, p_s = time_loop_case()
    assert points.size >= 150
    window = 3 * spp
    nt = spp * periods
    s = HostSolver(pr, p_raw=1, sampling_start=nt - window)
    s.run(nt)
    s.finish()
    series = s.stream("p").astype(np.float64).reshape(window, -1)
    s.close()
    assert series.shape[1] == points.size
    tt = np.arange(window) * dt
    amp_loop = np.abs(2.0 / window * (series * np.exp(-2j * np.pi * f0 * tt)[:, None]).sum(axis=0))
    n = 32
    src = np.zeros((n, n, n), dtype=F32)
    for z, y, x in patch:
        src[z, y, x] = p_s
    p = cw.FieldPropagator((n, n, n), (dx, dx, dx), C0, f0, source_scale="kwave")
    try:
        p.run(src, np.zeros_like(src))
        amp_cw = p.amplitude().reshape(-1)[points].astype(np.float64)
    finally:
        p.close()
    err = cr.rel_l2(amp_cw, amp_loop)
    ratio = float(np.mean(amp_cw / amp_loop))
    print(f"CW amplitude against the time loop at {points.size} points: rel L2 {err:.3e}, mean ratio {ratio:.4f}")
    assert err < TIME_LOOP_BOUND
