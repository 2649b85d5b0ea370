"""Time-domain angular-spectrum projector on the GPU: the fused stage (forward, k_zfused_time, y- and x-inverse) at every
fast-path line length, the stage against its rocFFT twin, kw_angular_time_embed / _reduce alone, and
kwave_amd.angular.AngularSpectrumTime end to end against the float64 NumPy restatement of tests/angular_time_reference.py,
against the CW projector and against the exact field of a pulsed aperture.

Bounds.
  stage, twin, AngularSpectrumTime   1e-5 relative L2, the project's parity bound, against float64 of the same float32
                                     inputs.  H has two discontinuities (the restriction's cut-off, the circle kr = k of an
                                     absorbing medium): every test that uses one asserts first that its inputs keep every bin
                                     1e-9 away from it (angular_time_reference.margins) — a condition on the inputs.
  embed, reduce                      exact: copies, zero fill, max and min of float32 values.
  against the CW projector           2e-5: two results, each within 1e-5 of the same float64 field.
  pulsed aperture                    1e-5 plus the restatement's own error on that plane.
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
import angular_time_reference as tr  # noqa: E402
import cw_reference as cr  # noqa: E402
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
PARITY = 1e-5
MARGIN = 1e-9
LENGTHS = cr.fast_lengths()
LAM = 1.0e-3
C0 = 1500.0


@pytest.fixture(scope="module")
def angular():
    import kwave_amd  # noqa: F401
    from kwave_amd import angular, capi
    assert "kw_fused_angular_time_plane" in capi._SIG
    return angular


@pytest.fixture()
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def coeff_for(alpha_np, f, y):
    """alpha_coeff [dB / (MHz^y cm)] that gives alpha_np [Np/m] at f [Hz]"""
    return alpha_np / ((f * 1e-6) ** y * 100.0 * tr.NEPER_PER_DB)


def make_op(dev, keep, spacing, dt, z, lt, alpha_coeff, alpha_power, restrict, retarded):
    """kw_angular_time_op for one plane; the absorption table goes to the device (kept alive in `keep`)"""
    from kwave_amd import capi
    op = capi.AngularTimeOp()
    op.dx, op.dy, op.dt, op.c0, op.z = spacing[0], spacing[1], dt, C0, z
    op.ak = None
    if alpha_coeff > 0.0:
        ak = Guarded(dev, tr.ak_table(lt, dt, C0, alpha_coeff, alpha_power), dtype=np.float64)
        keep.append(ak)
        op.ak = ak.ptr
    op.restriction, op.retarded = int(restrict), int(retarded)
    return op


def source_volume(rng, ex, ey, lt):
    """a smooth random record on the whole expanded volume plus 5 % white noise, so that every bin (the x-Nyquist column
    among them) carries something"""
    t, y, x = np.meshgrid(np.arange(lt) / lt, np.arange(ey) / ey, np.arange(ex) / ex, indexing="ij")
    c = rng.uniform(-1.0, 1.0, 8)
    s = (c[0] + c[1] * np.cos(2 * np.pi * x + c[2]) * np.sin(2 * np.pi * t + c[6]) +
         c[3] * np.sin(4 * np.pi * y + c[4]) * np.cos(2 * np.pi * x) * np.cos(4 * np.pi * t) +
         c[5] * np.exp(-((x - 0.4) ** 2 + (y - 0.6) ** 2 + (t - 0.5) ** 2) / 0.02) * np.cos(6 * np.pi * t + c[7]))
    return (s + 0.05 * rng.standard_normal((lt, ey, ex))).astype(F32)


class Stage:
    """a fused context of (ex, ey, lt) with a record transformed once and kept; plane(op) projects to one plane"""

    def __init__(self, dev, ex, ey, lt, vol):
        self.dev = dev
        set_constants(dev, ex, ey, lt)
        ok = C.c_int()
        dev.call("fused_supported", C.byref(ok))
        assert ok.value == 1, (ex, ey, lt)
        dev.call("fused_create")
        n = C.c_size_t()
        dev.call("fused_angular_time_elems", C.byref(n))
        assert n.value == (ex // 2 + 1 + 15) // 16 * 16 * ey * lt
        self.vol = Guarded(dev, vol)
        self.kept = Guarded(dev, np.full(2 * n.value, np.nan, F32))
        dev.call("fused_angular_time_forward", self.vol.ptr, self.kept.ptr)
        dev.sync()
        self.kept_bytes = self.kept.read().view(np.uint8)
        self.out = Guarded(dev, np.full((lt, ey, ex), np.nan, F32))

    def plane(self, op):
        self.dev.call("fused_angular_time_plane", self.kept.ptr, C.byref(op), self.out.ptr)
        self.dev.sync()
        return self.out.read()

    def close(self):
        assert np.array_equal(self.kept.read().view(np.uint8), self.kept_bytes)  # the kept spectrum survives every plane
        self.dev.call("fused_destroy")
        for g in (self.vol, self.kept, self.out):
            g.free()


# ---- 1. the fused stage at every line length ------------------------------------------------------------------------------
STAGE_SPACING = (LAM / 3, 0.8 * LAM / 3)
STAGE_DT = STAGE_SPACING[0] / (C0 * np.pi)
Z_NEAR, Z_FAR = 0.37 * LAM, 0.37 * LAM + 1023 * 3.7 * LAM
STAGE_COEFF = coeff_for(2.0 / Z_FAR, C0 / LAM, 1.5)   # exp(-2) along the axis at f = c0 / lambda on the far plane


def stage_errors(dev, ex, ey, lt):
    assert tr.margins((ex, ey), lt, STAGE_SPACING, STAGE_DT, C0, [Z_NEAR, Z_FAR])[1] >= MARGIN   # the absorbing variants
    rng = np.random.default_rng(ex * 1009 + ey * 31 + lt)
    vol = source_volume(rng, ex, ey, lt)
    X = np.fft.rfftn(vol.astype(np.float64))
    s = Stage(dev, ex, ey, lt, vol)
    keep, errs = [], []
    for coeff in (0.0, STAGE_COEFF):
        for z, retarded in ((Z_NEAR, False), (Z_FAR, True)):   # a float32 product q z is ~1e-3 rad off on the far plane
            op = make_op(dev, keep, STAGE_SPACING, STAGE_DT, z, lt, coeff, 1.5, False, retarded)
            got = s.plane(op)
            H = tr.H_time((ex, ey), lt, STAGE_SPACING, STAGE_DT, C0, z, coeff, 1.5, False, retarded, half=True)
            want = np.fft.irfftn(X * H, s=vol.shape, axes=(0, 1, 2))
            errs.append(tr.rel_l2(got, want))
    s.close()
    for g in keep:
        g.free()
    return errs


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length(dev, L):
    """(L, 16, 16): the x-passes at every length (where L is a multiple of 32 they write and read the side array, whose y-
    and z-passes ran at length 16 only); (16, 16, L): k_zfused_time<L> on one column tile, no side array.  Lossless and
    absorbing, 0.37 and 3785.47 wavelengths out (retarded time on the far plane), restriction off; the whole expanded
    output.  The side array here covers the x-pass side only: the y- and z-pass kernels at every length with a side block
    are in test_stage_at_every_line_length_with_side_array."""
    for ex, ey, lt in ((L, 16, 16), (16, 16, L)):
        errs = stage_errors(dev, ex, ey, lt)
        print(f"angular-time stage {ex}x{ey}x{lt}: rel L2 lossless near {errs[0]:.3e} far {errs[1]:.3e}; "
              f"absorbing near {errs[2]:.3e} far {errs[3]:.3e}")
        assert max(errs) < PARITY, (ex, ey, lt)


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length_with_side_array(dev, L):
    """(96, 16, L): k_zfused_time<L> on three main column tiles (two 32-column ones, the second half valid, at 240 and 400)
    and on the side block of the x-Nyquist column, which forms H at kx = Nx/2 for 16 rows ky.  The variants of the test
    above: lossless and absorbing, near plane and far plane with retarded time; the whole expanded output.  Measured
    1.9e-7 to 1.0e-6 on the near plane (worst at 300); on the far plane 1.8e-7 to 2.7e-6 lossless (worst at 540) and 1.3e-7
    to 6.5e-6 absorbing (worst at 768)."""
    errs = stage_errors(dev, 96, 16, L)
    print(f"angular-time stage 96x16x{L}: rel L2 lossless near {errs[0]:.3e} far {errs[1]:.3e}; "
          f"absorbing near {errs[2]:.3e} far {errs[3]:.3e}")
    assert max(errs) < PARITY, L


# ---- 2. fused against twin ------------------------------------------------------------------------------------------------
TWIN = dict(spacing=(LAM / 3, 0.8 * LAM / 3), coeff=coeff_for(30.0, C0 / LAM, 1.5), z=4.3 * LAM)


@pytest.mark.parametrize("ex,ey,lt", [(32, 48, 48), (48, 16, 64)])
def test_fused_stage_and_rocfft_twin(dev, ex, ey, lt):
    from kwave_amd import capi
    p = TWIN
    dt = p["spacing"][0] / (C0 * np.pi)
    first, second = tr.margins((ex, ey), lt, p["spacing"], dt, C0, [p["z"]])
    assert first >= MARGIN and second >= MARGIN
    vol = source_volume(np.random.default_rng(ex + ey + lt), ex, ey, lt)
    kw = dict(alpha_coeff=p["coeff"], alpha_power=1.5, restrict=True, retarded=True)
    want = tr.solve_expanded(vol, (ex, ey), lt, p["spacing"], dt, C0, p["z"], **kw)
    want_lossless = tr.solve_expanded(vol, (ex, ey), lt, p["spacing"], dt, C0, p["z"], restrict=True, retarded=True)
    keep = []
    s = Stage(dev, ex, ey, lt, vol)
    fused = tr.rel_l2(s.plane(make_op(dev, keep, p["spacing"], dt, p["z"], lt, p["coeff"], 1.5, True, True)), want)
    s.close()
    # the twin: 3-D plans, kw_angular_time_mix on the natural half-spectrum, one C2R transform
    d2 = capi.Device()
    try:
        d2.call("angular_time_mix", None, None, None, C.c_float(1.0))   # no constants, no bins: no pointer is looked at
        set_constants(d2, ex, ey, lt)
        d2.call("fft_create_plans_3d")
        nr = (ex // 2 + 1) * ey * lt
        src, spec = Guarded(d2, vol), Guarded(d2, np.zeros(2 * nr, F32))
        d2.call("fft_r2c_3d", src.ptr, spec.ptr)
        mixed, out = Guarded(d2, np.full(2 * nr, np.nan, F32)), Guarded(d2, np.full((lt, ey, ex), np.nan, F32))
        twins = []
        for coeff, ref in ((p["coeff"], want), (0.0, want_lossless)):   # the second one with a NULL ak
            op = make_op(d2, keep, p["spacing"], dt, p["z"], lt, coeff, 1.5, True, True)
            assert (op.ak is None) == (coeff == 0.0)
            d2.call("angular_time_mix", mixed.ptr, spec.ptr, C.byref(op), C.c_float(1.0 / (ex * ey * lt)))
            d2.call("fft_c2r_3d", mixed.ptr, out.ptr)
            d2.sync()
            twins.append(tr.rel_l2(out.read(), ref))
    finally:
        d2.close()
    print(f"angular-time {ex}x{ey}x{lt}: fused stage {fused:.3e}, rocFFT twin {twins[0]:.3e}, twin without ak {twins[1]:.3e} "
          f"(rel L2 against float64)")
    assert fused < PARITY and max(twins) < PARITY


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def test_stage_refuses_two_d_and_slab_contexts(dev):
    from kwave_amd import capi
    a = Guarded(dev, np.zeros(2 * 32 * 32 * 16, F32))
    b = Guarded(dev, np.zeros(2 * 32 * 32 * 16, F32))
    op = make_op(dev, [], (1e-3, 1e-3), 2e-7, 1e-3, 16, 0.0, 1.5, True, False)
    set_constants(dev, 32, 32, 1)
    dev.call("fused_create")
    for entry, args in (("fused_angular_time_plane", (a.ptr, C.byref(op), b.ptr)), ("fused_angular_time_forward", (a.ptr, b.ptr))):
        with pytest.raises(capi.KWaveError, match=entry + r": single GPU and 3-D only \(no Z-slabs, no Nz == 1\)"):
            dev.call(entry, *args)
    dev.call("fused_destroy")
    # one rank with an exchange callback = the slab path against itself; the callback is never reached
    exchange = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)(lambda *args: 1)
    set_constants(dev, 32, 32, 16)
    dev.call("fused_set_slab", 1, 0, 16, C.cast(exchange, C.c_void_p), None)
    dev.call("fused_create")
    for entry, args in (("fused_angular_time_plane", (a.ptr, C.byref(op), b.ptr)), ("fused_angular_time_forward", (a.ptr, b.ptr))):
        with pytest.raises(capi.KWaveError, match=r"no Z-slabs, no Nz == 1"):
            dev.call(entry, *args)
    dev.call("fused_destroy")


# ---- 4. embed and reduce alone ----------------------------------------------------------------------------------------------
EMBED_CASES = [  # (nx, ny, nt), (ex, ey, lt), byte offset of the device pointers
    ((23, 19, 37), (48, 40, 48), 0),       # scalar path
    ((24, 20, 40), (48, 48, 48), 0),       # 16-byte path
    ((24, 20, 40), (48, 48, 48), 4),       # the same sizes off 16-byte alignment: scalar path
    ((1, 19, 37), (48, 40, 48), 0),        # a domain of one column
    ((48, 40, 48), (48, 40, 48), 0),       # nothing to fill
    ((200, 180, 5), (256, 256, 40), 0),    # beyond one grid-stride round, 16-byte path
    ((201, 180, 5), (256, 256, 40), 0),    # ... and scalar
]


@pytest.mark.parametrize("dims,expanded,offset", EMBED_CASES)
def test_embed_and_reduce_are_exact(dev, dims, expanded, offset):
    (nx, ny, nt), (ex, ey, lt) = dims, expanded
    rng = np.random.default_rng(nx * 7 + ny * 3 + nt + offset)
    src = rng.standard_normal((nt, ny, nx)).astype(F32)
    gs = Guarded(dev, src, offset)
    vol = Guarded(dev, np.full((lt, ey, ex), np.nan, F32), offset)
    dev.call("angular_time_embed", vol.ptr, gs.ptr, ex, ey, lt, nx, ny, nt)
    dev.sync()
    got = vol.read()
    want = tr.embed(src, (ex, ey), lt)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(gs.read(), src)
    # reduce on a volume that is random everywhere: what lies outside the crop must not be looked at
    full = rng.standard_normal((lt, ey, ex)).astype(F32)
    vol.write(full)
    crop = full[:nt, :ny, :nx]
    pmax = Guarded(dev, np.full((ny, nx), np.nan, F32), offset)
    pmin = Guarded(dev, np.full((ny, nx), np.nan, F32), offset)
    ser = Guarded(dev, np.full((nt, ny, nx), np.nan, F32), offset)
    dev.call("angular_time_reduce", vol.ptr, ex, ey, lt, nx, ny, nt, pmax.ptr, pmin.ptr, ser.ptr)
    dev.sync()
    assert np.array_equal(pmax.read(), crop.max(axis=0))
    assert np.array_equal(pmin.read(), crop.min(axis=0))
    assert np.array_equal(ser.read(), crop)
    assert np.array_equal(vol.read(), full)
    # every output alone; the others NULL
    for which in range(3):
        outs = [Guarded(dev, np.full(g.shape, np.nan, F32), offset) for g in (pmax, pmin, ser)]
        ptrs = [outs[i].ptr if i == which else None for i in range(3)]
        dev.call("angular_time_reduce", vol.ptr, ex, ey, lt, nx, ny, nt, *ptrs)
        dev.sync()
        for i, w in enumerate((crop.max(axis=0), crop.min(axis=0), crop)):
            r = outs[i].read()
            assert np.array_equal(r, w) if i == which else np.isnan(r).all()
            outs[i].free()
    for g in (gs, vol, pmax, pmin, ser):
        g.free()


def test_embed_and_reduce_of_nothing(dev):
    vol = Guarded(dev, np.full((8, 8, 8), np.nan, F32))
    out = Guarded(dev, np.full((8, 8), np.nan, F32))
    dev.call("angular_time_reduce", vol.ptr, 8, 8, 8, 0, 8, 8, out.ptr, out.ptr, None)    # zero points
    dev.call("angular_time_reduce", vol.ptr, 8, 8, 8, 8, 8, 0, out.ptr, out.ptr, None)    # zero steps
    dev.call("angular_time_reduce", None, 8, 8, 8, 8, 8, 8, None, None, None)             # nothing asked for
    dev.call("angular_time_embed", None, None, 0, 8, 8, 0, 0, 0)                          # an empty volume
    dev.call("angular_time_embed", vol.ptr, None, 8, 8, 8, 0, 4, 4)                       # an empty record: all zeros
    dev.sync()
    assert np.isnan(out.read()).all()
    assert not vol.read().any()


# ---- 5. AngularSpectrumTime end to end ---------------------------------------------------------------------------------------
E2E = dict(dims=(24, 20), nt=40, spacing=(1.0e-3, 0.8e-3), z=(0.5e-3, 1.6e-3, 2.0e-3, 4.4e-3, 9.9e-3))
E2E_DT = E2E["spacing"][0] / (C0 * np.pi)
E2E_COEFF = 0.75


def e2e_record(seed):
    rng = np.random.default_rng(seed)
    nx, ny = E2E["dims"]
    t = np.arange(E2E["nt"])[:, None, None] / E2E["nt"]
    phase = rng.uniform(-np.pi, np.pi, (ny, nx))
    amp = rng.uniform(0.2, 1.0, (ny, nx))
    p = amp * np.sin(2 * np.pi * 4 * t + phase) * np.exp(-((t - 0.5) ** 2) / 0.03) + 0.05 * rng.standard_normal((E2E["nt"], ny, nx))
    return p.astype(F32)


@functools.lru_cache(maxsize=None)
def e2e_reference(coeff, restrict, retarded, expanded, lt, seed):
    return tr.project(e2e_record(seed), expanded, lt, E2E["spacing"], E2E_DT, C0, E2E["z"], alpha_coeff=coeff, alpha_power=1.5,
                      restrict=restrict, retarded=retarded)


def e2e_margins(expanded, lt, coeff, restrict):
    first, second = tr.margins(expanded, lt, E2E["spacing"], E2E_DT, C0, E2E["z"])
    assert not restrict or first >= MARGIN
    assert coeff == 0.0 or second >= MARGIN


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
@pytest.mark.parametrize("restrict", [True, False], ids=["restricted", "unrestricted"])
@pytest.mark.parametrize("coeff", [0.0, E2E_COEFF], ids=["lossless", "absorbing"])
def test_angular_spectrum_time_against_the_restatement(angular, coeff, restrict, fused):
    expanded, lt = ((48, 48), 48) if fused else ((48, 40), 40)
    retarded = coeff > 0.0
    e2e_margins(expanded, lt, coeff, restrict)
    p = angular.AngularSpectrumTime(E2E["dims"], E2E["spacing"], E2E_DT, E2E["nt"], C0, E2E["z"], alpha_coeff=coeff,
                                    alpha_power=1.5, angular_restriction=restrict, retarded_time=retarded, fused_kernels=fused)
    try:
        assert p.fused == fused and p.expanded == expanded and p.time_length == lt and p.runs == 0
        got = p.run(e2e_record(1))
        assert got.dtype == F32 and got.shape == (5, 20, 24)
        want = e2e_reference(coeff, restrict, retarded, expanded, lt, 1)
        e_max, e_min = tr.rel_l2(got, want.max(axis=1)), tr.rel_l2(p.p_min(), want.min(axis=1))
        assert np.array_equal(p.p_max(), got)
        worst = 0.0
        for j in range(5):
            s = p.series(j)
            assert s.dtype == F32 and s.shape == (40, 20, 24)
            worst = max(worst, tr.rel_l2(s, want[j]))
            assert np.array_equal(got[j], s.max(axis=0)) and np.array_equal(p.p_min()[j], s.min(axis=0))
        print(f"AngularSpectrumTime alpha_coeff {coeff} restriction {restrict} fused {fused}: rel L2 p_max {e_max:.3e}, "
              f"p_min {e_min:.3e}, worst series {worst:.3e}")
        assert max(e_max, e_min, worst) < PARITY
        # a second run with another record reuses everything
        got2 = p.run(e2e_record(2))
        want2 = e2e_reference(coeff, restrict, retarded, expanded, lt, 2)
        assert p.runs == 2 and tr.rel_l2(got2, want2.max(axis=1)) < PARITY
        p.project()                                   # the planes alone give the same maps again
        assert np.array_equal(p.p_max(), got2)
    finally:
        p.close()


# ---- 6. a plane does not depend on its neighbours ------------------------------------------------------------------------------
def test_a_plane_alone_is_the_plane_among_five(angular):
    rec = e2e_record(3)
    kw = dict(alpha_coeff=E2E_COEFF, alpha_power=1.5, retarded_time=True)
    p = angular.AngularSpectrumTime(E2E["dims"], E2E["spacing"], E2E_DT, E2E["nt"], C0, E2E["z"], **kw)
    try:
        five, five_min, s3 = p.run(rec), p.p_min(), p.series(3)
    finally:
        p.close()
    q = angular.AngularSpectrumTime(E2E["dims"], E2E["spacing"], E2E_DT, E2E["nt"], C0, (E2E["z"][3],), **kw)
    try:
        one = q.run(rec)
        assert one.shape == (1, 20, 24)
        assert np.array_equal(one[0], five[3]) and np.array_equal(q.p_min()[0], five_min[3])
        assert np.array_equal(q.series(0), s3)
    finally:
        q.close()


# ---- 7. agreement with the CW projector ------------------------------------------------------------------------------------------
def test_one_bin_sinusoid_agrees_with_the_cw_projector(angular):
    """Re(P0 exp(i w t)) with Nt = Lt = 48 on bin 5, 30 Np/m at that bin: series(j) against Re(P_j exp(i w t)) of
    AngularSpectrum on the same expanded sides, GPU to GPU"""
    dims, spacing, nt, m = E2E["dims"], E2E["spacing"], 48, 5
    dt = E2E_DT
    f = m / (nt * dt)
    w = 2.0 * np.pi * f
    z0, dz, planes = 0.5e-3, 1.1e-3, 5
    zs = z0 + dz * np.arange(planes)
    first, second = tr.margins((48, 48), nt, spacing, dt, C0, zs)
    assert first >= MARGIN and second >= MARGIN
    assert ar.restriction_margin((48, 48), spacing, w / C0, z0, dz, planes) >= MARGIN
    rng = np.random.default_rng(7)
    amp, phase = rng.uniform(0.2, 1.0, dims[::-1]).astype(F32), rng.uniform(-np.pi, np.pi, dims[::-1]).astype(F32)
    P0 = amp.astype(np.float64) * np.exp(1j * phase.astype(np.float64))
    carrier = np.exp(1j * w * np.arange(nt) * dt)[:, None, None]
    cwp = angular.AngularSpectrum(dims, spacing, C0, f, z0, dz, planes, alpha_np=30.0, expanded=(48, 48))
    try:
        P = cwp.run(amp, phase).astype(np.complex128)
    finally:
        cwp.close()
    p = angular.AngularSpectrumTime(dims, spacing, dt, nt, C0, zs, alpha_coeff=coeff_for(30.0, f, 1.5), alpha_power=1.5,
                                    expanded=(48, 48), time_length=48)
    try:
        assert p.fused and p.time_length == 48
        p.run(np.real(P0[None] * carrier).astype(F32))
        errs = [tr.rel_l2(p.series(j), np.real(P[j][None] * carrier)) for j in range(planes)]
    finally:
        p.close()
    print("one-bin sinusoid, AngularSpectrumTime against AngularSpectrum, GPU to GPU: " + " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) < 2e-5


# ---- 8. the pulsed aperture ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aperture():
    return tr.aperture_case()


@pytest.mark.parametrize("retarded", [False, True], ids=["absolute", "retarded"])
def test_pulsed_aperture_field(angular, aperture, retarded):
    c = aperture
    rec = c["p0"].astype(F32)
    spacing = (c["dx"], c["dx"])
    own = tr.project(rec, c["expanded"], c["lt"], spacing, c["dt"], c["c0"], c["zs"], restrict=True, retarded=retarded)
    p = angular.AngularSpectrumTime((c["n"], c["n"]), spacing, c["dt"], c["nt"], c["c0"], c["zs"], retarded_time=retarded,
                                    expanded=c["expanded"], time_length=c["lt"])
    try:
        assert p.fused and p.time_length == 256
        p.run(rec)
        for j, z in enumerate(c["zs"]):
            exact = tr.aperture_exact(c, z, retarded)
            err, figure = tr.rel_l2(p.series(j), exact), tr.rel_l2(own[j], exact)
            print(f"pulsed aperture, retarded {retarded}, z = {z / c['dx']:.0f} dx: GPU against exact {err:.3e}, restatement "
                  f"against exact {figure:.3e}")
            assert err <= PARITY + figure
    finally:
        p.close()
