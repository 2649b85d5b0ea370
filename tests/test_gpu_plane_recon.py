"""k-space plane reconstruction on the GPU: the fused stage (forward, k_zfused_recon, y- and x-inverse) at every fast-path
line length, the stage against its rocFFT twin, the twin at an odd Lt, kw_plane_recon_embed / _crop alone, and
kwave_amd.recon.PlaneRecon end to end against the float64 NumPy restatement of tests/plane_recon_reference.py, on a record
of t alone and on the phantom of the CPU tests.

Bounds.
  stage, twin, PlaneRecon   1e-5 relative L2, the project's parity bound, against float64 of the same float32 inputs.  G has
                            two discontinuities (f = M, the end of the line; a = 1/2 for the nearest neighbour): every test
                            asserts first that its inputs keep every bin 1e-9 away from them
                            (plane_recon_reference.margins) — a condition on the inputs.  All use dt = dx / (c0 pi).
  stage against twin        2e-5: two results, each within 1e-5 of the same float64 field.
  embed, crop               exact: copies, zero fill, a clamp of float32 values.
  phantom                   the relative error against the phantom within 1e-4 (absolute) of the restatement's own figure.
  repeatability             bit-equal.
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
import plane_recon_reference as pr  # noqa: E402
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
PARITY = 1e-5
MARGIN = 1e-9
LENGTHS = cr.fast_lengths()
C0 = 1500.0
DX = 1.0e-4
SPACING = (DX, DX)
DT = DX / (C0 * np.pi)


@pytest.fixture(scope="module")
def recon():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, recon
    assert "kw_fused_plane_recon" in capi._SIG
    return recon


@pytest.fixture()
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def make_op(spacing, dt, interp):
    from kwave_amd import capi
    op = capi.PlaneReconOp()
    op.dx, op.dy, op.dt, op.c0 = spacing[0], spacing[1], dt, C0
    op.interp, op.reserved = pr.INTERPS.index(interp), 0
    return op


def assert_margins(ex, ey, lt, spacing=SPACING, dt=DT):
    first, second = pr.margins((ex, ey), lt, spacing, dt, C0)
    assert first >= MARGIN and second >= MARGIN, (ex, ey, lt, first, second)


def fused_stage(dev, vol, spacing, dt, interps, in_place=False):
    """kw_fused_plane_recon of the volume [lt][ey][ex] on a fused context of its own, per interpolant"""
    lt, ey, ex = vol.shape
    set_constants(dev, ex, ey, lt)
    ok = C.c_int()
    dev.call("fused_supported", C.byref(ok))
    assert ok.value == 1, (ex, ey, lt)
    dev.call("fused_create")
    src = Guarded(dev, vol)
    out = Guarded(dev, np.full(vol.shape, np.nan, F32))
    got = []
    for interp in interps:
        op = make_op(spacing, dt, interp)
        if in_place:
            src.write(vol)
            dev.call("fused_plane_recon", src.ptr, C.byref(op), src.ptr)
            dev.sync()
            got.append(src.read())
        else:
            dev.call("fused_plane_recon", src.ptr, C.byref(op), out.ptr)
            dev.sync()
            got.append(out.read())
            assert np.array_equal(src.read().view(np.uint32), vol.view(np.uint32))   # the input is not written
    dev.call("fused_destroy")
    src.free()
    out.free()
    return got


def twin_stage(vol, spacing, dt, interps):
    """kw_fft_r2c_3d, kw_plane_recon_mix, kw_fft_c2r_3d on a context of its own, per interpolant"""
    from kwave_amd import capi
    lt, ey, ex = vol.shape
    d2 = capi.Device()
    got = []
    try:
        d2.call("plane_recon_mix", None, None, None, C.c_float(1.0))   # no constants, no bins: no pointer is looked at
        set_constants(d2, ex, ey, lt)
        d2.call("fft_create_plans_3d")
        nr = (ex // 2 + 1) * ey * lt
        src, spec = Guarded(d2, vol), Guarded(d2, np.zeros(2 * nr, F32))
        d2.call("fft_r2c_3d", src.ptr, spec.ptr)
        d2.sync()
        spec_bytes = spec.read().view(np.uint8)
        mixed, out = Guarded(d2, np.full(2 * nr, np.nan, F32)), Guarded(d2, np.full(vol.shape, np.nan, F32))
        for interp in interps:
            op = make_op(spacing, dt, interp)
            d2.call("plane_recon_mix", mixed.ptr, spec.ptr, C.byref(op), C.c_float(2.0 / (ex * ey * lt)))
            d2.call("fft_c2r_3d", mixed.ptr, out.ptr)
            d2.sync()
            got.append(out.read())
        assert np.array_equal(spec.read().view(np.uint8), spec_bytes)   # the mix is out of place
        for g in (src, spec, mixed, out):
            g.free()
    finally:
        d2.close()
    return got


# ---- 1. the fused stage at every line length ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length(dev, L):
    """t-even random volumes.  (16, 16, L): k_zfused_recon<L>, the gather along a line of every length, both interpolants;
    (L, 16, 16): the column addressing and the x-passes at every length, linear (where L is a multiple of 32 they write and
    read the side array, whose y- and z-passes ran at length 16 only).  The whole expanded output is compared.  Measured
    1.7e-7 to 2.5e-7 (worst at 756): white noise needed no smoother input.  The side array here covers the x-pass side
    only: k_zfused_recon<L> with a side block is in test_stage_at_every_line_length_with_side_array."""
    for (ex, ey, lt), interps in (((16, 16, L), pr.INTERPS), ((L, 16, 16), ("linear",))):
        assert_margins(ex, ey, lt)
        vol = pr.even_volume((lt, ey, ex), ex * 1009 + ey * 31 + lt)
        got = fused_stage(dev, vol, SPACING, DT, interps)
        for interp, g in zip(interps, got):
            err = pr.rel_l2(g, pr.stage(vol, SPACING, DT, C0, interp))
            print(f"plane-recon stage {ex}x{ey}x{lt} {interp}: rel L2 {err:.3e}")
            assert err < PARITY, (ex, ey, lt, interp)


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length_with_side_array(dev, L):
    """t-even random volumes of (96, 16, L): k_zfused_recon<L> on three main column tiles (two 32-column ones, the second
    half valid, at 240 and 400) and on the side block of the x-Nyquist column, which forms the re-gridding weight at
    kx = Nx/2 for 16 rows ky; both interpolants, the whole expanded output.  Measured 1.9e-7 to 2.8e-7 (worst at 648)."""
    ex, ey, lt = 96, 16, L
    assert_margins(ex, ey, lt)
    vol = pr.even_volume((lt, ey, ex), ex * 1009 + ey * 31 + lt)
    got = fused_stage(dev, vol, SPACING, DT, pr.INTERPS)
    for interp, g in zip(pr.INTERPS, got):
        err = pr.rel_l2(g, pr.stage(vol, SPACING, DT, C0, interp))
        print(f"plane-recon stage {ex}x{ey}x{lt} {interp}: rel L2 {err:.3e}")
        assert err < PARITY, (ex, ey, lt, interp)


# ---- 2. fused against twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ex,ey,lt", [(32, 48, 64), (48, 16, 96)])
def test_fused_stage_and_rocfft_twin(dev, ex, ey, lt):
    """the stage in place and the twin against the restatement and against each other.  Measured 2.1e-7 to 2.5e-7 and
    2.7e-7 to 2.8e-7."""
    spacing = (DX, 0.8 * DX)
    assert_margins(ex, ey, lt, spacing)
    vol = pr.even_volume((lt, ey, ex), ex + ey + lt)
    fused = fused_stage(dev, vol, spacing, DT, pr.INTERPS, in_place=True)
    twin = twin_stage(vol, spacing, DT, pr.INTERPS)
    for interp, f, t in zip(pr.INTERPS, fused, twin):
        want = pr.stage(vol, spacing, DT, C0, interp)
        ef, et, eb = pr.rel_l2(f, want), pr.rel_l2(t, want), pr.rel_l2(f, t)
        print(f"plane-recon {ex}x{ey}x{lt} {interp}: fused stage {ef:.3e}, rocFFT twin {et:.3e} (rel L2 against float64), "
              f"fused against twin {eb:.3e}")
        assert ef < PARITY and et < PARITY and eb < 2 * PARITY


def test_twin_at_odd_time_length():
    """(20, 24, 79): k-Wave's own grid Lt = 2 Nt - 1 for Nt = 40; M = 39, and the bins M and M + 1 mirror each other"""
    ex, ey, lt = 20, 24, 79
    assert_margins(ex, ey, lt)
    vol = pr.even_volume((lt, ey, ex), 79)
    for interp, t in zip(pr.INTERPS, twin_stage(vol, SPACING, DT, pr.INTERPS)):
        err = pr.rel_l2(t, pr.stage(vol, SPACING, DT, C0, interp))
        print(f"plane-recon twin {ex}x{ey}x{lt} {interp}: rel L2 {err:.3e}")
        assert err < PARITY


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def test_stage_refuses_two_d_and_slab_contexts(dev):
    from kwave_amd import capi
    a = Guarded(dev, np.zeros(32 * 32 * 16, F32))
    b = Guarded(dev, np.zeros(32 * 32 * 16, F32))
    op = make_op(SPACING, DT, "linear")
    set_constants(dev, 32, 32, 1)
    dev.call("fused_create")
    with pytest.raises(capi.KWaveError, match=r"kw_fused_plane_recon: single GPU and 3-D only \(no Z-slabs, no Nz == 1\)"):
        dev.call("fused_plane_recon", a.ptr, C.byref(op), b.ptr)
    dev.call("fused_destroy")
    # one rank with an exchange callback = the slab path against itself; the callback is never reached
    exchange = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)(lambda *args: 1)
    set_constants(dev, 32, 32, 16)
    dev.call("fused_set_slab", 1, 0, 16, C.cast(exchange, C.c_void_p), None)
    dev.call("fused_create")
    with pytest.raises(capi.KWaveError, match=r"no Z-slabs, no Nz == 1"):
        dev.call("fused_plane_recon", a.ptr, C.byref(op), b.ptr)
    dev.call("fused_destroy")
    assert not a.read().any() and not b.read().any()
    a.free()
    b.free()


# ---- 4. embed and crop alone ------------------------------------------------------------------------------------------------
EMBED_CASES = [  # (nx, ny, nt), (ex, ey, lt), byte offset of the device pointers
    ((23, 19, 20), (48, 40, 48), 0),       # scalar path
    ((24, 20, 24), (48, 48, 48), 0),       # 16-byte path
    ((24, 20, 24), (48, 48, 48), 4),       # the same sizes off 16-byte alignment: scalar path
    ((1, 19, 20), (48, 40, 39), 0),        # a domain of one column, Lt = 2 Nt - 1
    ((48, 40, 24), (48, 40, 47), 0),       # k-Wave's grid: nothing to fill but the mirror image
    ((8, 8, 1), (8, 8, 1), 0),             # one sample: no mirror image at all
    ((200, 180, 5), (256, 256, 40), 0),    # beyond one grid-stride round, 16-byte path
    ((201, 180, 5), (256, 256, 40), 0),    # ... and scalar
    ((256, 256, 5), (256, 256, 40), 0),    # the crop's 16-byte path beyond one grid-stride round
]


@pytest.mark.parametrize("dims,expanded,offset", EMBED_CASES)
def test_embed_and_crop_are_exact(dev, dims, expanded, offset):
    (nx, ny, nt), (ex, ey, lt) = dims, expanded
    rng = np.random.default_rng(nx * 7 + ny * 3 + nt + offset)
    src = rng.standard_normal((nt, ny, nx)).astype(F32)
    gs = Guarded(dev, src, offset)
    vol = Guarded(dev, np.full((lt, ey, ex), np.nan, F32), offset)
    dev.call("plane_recon_embed", vol.ptr, gs.ptr, ex, ey, lt, nx, ny, nt)
    dev.sync()
    got = vol.read()
    want = pr.embed(src, (ex, ey), lt)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for n in range(1, lt):
        assert np.array_equal(got[lt - n], got[n])
    assert np.array_equal(gs.read(), src)
    # crop on a volume that is random everywhere: what lies outside the crop must not be looked at
    full = rng.standard_normal((lt, ey, ex)).astype(F32)
    full[0, 0, 0] = -0.0
    vol.write(full)
    for planes in (lt, max(1, nt - 1)):
        for positivity in (0, 1):
            out = Guarded(dev, np.full((planes, ny, nx), np.nan, F32), offset)
            dev.call("plane_recon_crop", out.ptr, vol.ptr, ex, ey, lt, nx, ny, planes, positivity)
            dev.sync()
            want = pr.crop(full, (nx, ny), planes, bool(positivity))
            assert np.array_equal(out.read().view(np.uint32), want.view(np.uint32)), (planes, positivity)
            out.free()
    assert np.array_equal(vol.read().view(np.uint32), full.view(np.uint32))
    gs.free()
    vol.free()


def test_embed_and_crop_of_nothing(dev):
    vol = Guarded(dev, np.full((8, 8, 8), np.nan, F32))
    out = Guarded(dev, np.full((8, 8), np.nan, F32))
    dev.call("plane_recon_crop", out.ptr, vol.ptr, 8, 8, 8, 0, 8, 8, 0)     # zero points
    dev.call("plane_recon_crop", out.ptr, vol.ptr, 8, 8, 8, 8, 8, 0, 1)     # zero planes
    dev.call("plane_recon_crop", None, None, 8, 8, 8, 8, 0, 8, 0)
    dev.call("plane_recon_embed", None, None, 0, 8, 8, 0, 0, 0)             # an empty volume
    dev.sync()
    assert np.isnan(out.read()).all() and np.isnan(vol.read()).all()
    dev.call("plane_recon_embed", vol.ptr, None, 8, 8, 8, 0, 4, 4)          # an empty record: all zeros
    dev.sync()
    assert not vol.read().any()
    vol.free()
    out.free()


def test_embed_refuses_a_volume_shorter_than_the_mirrored_record(dev):
    from kwave_amd import capi
    vol = Guarded(dev, np.full((8, 8, 8), np.nan, F32))
    src = Guarded(dev, np.zeros((5, 8, 8), F32))
    with pytest.raises(capi.KWaveError):
        dev.call("plane_recon_embed", vol.ptr, src.ptr, 8, 8, 8, 8, 8, 5)   # 2 * 5 - 1 = 9 > 8
    dev.sync()
    assert np.isnan(vol.read()).all()
    vol.free()
    src.free()


# ---- 5. PlaneRecon end to end ------------------------------------------------------------------------------------------------
E2E = dict(dims=(24, 20), nt=30, spacing=(DX, 0.8 * DX), expanded=(32, 32))


def e2e_record(seed):
    rng = np.random.default_rng(seed)
    nx, ny = E2E["dims"]
    t = np.arange(E2E["nt"])[:, None, None] / E2E["nt"]
    phase = rng.uniform(-np.pi, np.pi, (ny, nx))
    amp = rng.uniform(0.2, 1.0, (ny, nx))
    p = amp * np.sin(2 * np.pi * 4 * t + phase) * np.exp(-((t - 0.5) ** 2) / 0.03) + 0.05 * rng.standard_normal((E2E["nt"], ny, nx))
    return p.astype(F32)


@functools.lru_cache(maxsize=None)
def e2e_reference(lt, interp, positivity, seed):
    return pr.reconstruct(e2e_record(seed), E2E["expanded"], lt, E2E["spacing"], DT, C0, interp=interp, positivity=positivity)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
@pytest.mark.parametrize("positivity", [False, True], ids=["signed", "positive"])
@pytest.mark.parametrize("interp", pr.INTERPS)
def test_plane_recon_against_the_restatement(recon, interp, positivity, fused):
    """Nt = 30, 24 x 20 in 32 x 32; Lt = 64 on the fused path and 59 (k-Wave's grid) on rocFFT.  Measured 2.0e-7 to 2.1e-7
    fused, 3.8e-7 to 4.0e-7 rocFFT."""
    lt = 64 if fused else 59
    assert_margins(*E2E["expanded"], lt, E2E["spacing"])
    kw = dict(interp=interp, positivity=positivity, expanded=E2E["expanded"], fused_kernels=fused)
    if fused:
        kw["time_length"] = 64
    p = recon.PlaneRecon(E2E["dims"], E2E["spacing"], DT, E2E["nt"], C0, **kw)
    try:
        assert p.fused == fused and p.expanded == E2E["expanded"] and p.time_length == lt and p.runs == 0
        assert p.dz == pytest.approx(C0 * DT, rel=1e-15) and p.planes == 30
        got = p.run(e2e_record(1))
        assert got.dtype == F32 and got.shape == (30, 20, 24)
        want = e2e_reference(lt, interp, positivity, 1)
        err = pr.rel_l2(got, want)
        assert not positivity or got.min() >= 0.0
        # a second run with another record reuses everything
        got2 = p.run(e2e_record(2))
        err2 = pr.rel_l2(got2, e2e_reference(lt, interp, positivity, 2))
        print(f"PlaneRecon {interp} positivity {positivity} fused {fused}: rel L2 {err:.3e}, second record {err2:.3e}")
        assert p.runs == 2 and max(err, err2) < PARITY
    finally:
        p.close()


def test_fewer_planes_are_the_first_planes(recon):
    rec = e2e_record(3)
    kw = dict(expanded=E2E["expanded"], time_length=64)
    p = recon.PlaneRecon(E2E["dims"], E2E["spacing"], DT, E2E["nt"], C0, **kw)
    q = recon.PlaneRecon(E2E["dims"], E2E["spacing"], DT, E2E["nt"], C0, planes=7, **kw)
    try:
        full, few = p.run(rec), q.run(rec)
        assert few.shape == (7, 20, 24) and np.array_equal(few, full[:7])
    finally:
        p.close()
        q.close()


def test_record_of_t_alone_gives_back_its_profile(recon):
    """the identity of the CPU tests on the GPU, fused (16 x 16 x 80) and rocFFT (16 x 16 x 79): rho2 = 0 on the only bins
    that carry anything, so both interpolants return g(z).  Measured 9.8e-8 fused, 1.7e-7 rocFFT."""
    nt = 40
    rec, g = pr.identity_record(nt, 16, 16, C0, DT)
    for fused, lt in ((True, 80), (False, 79)):
        for interp in pr.INTERPS:
            p = recon.PlaneRecon((16, 16), SPACING, DT, nt, C0, interp=interp, fused_kernels=fused)
            try:
                assert p.fused == fused and p.time_length == lt
                got = p.run(rec.astype(F32))
            finally:
                p.close()
            want = np.broadcast_to(2.0 * rec.astype(F32).astype(np.float64), got.shape)   # g of the float32 record
            err = pr.rel_l2(got, want)
            print(f"identity record, fused {fused} {interp}: rel L2 against g {err:.3e}")
            assert err < PARITY
            assert np.max(np.abs(want[:, 0, 0] - g)) < 1e-7


def test_phantom_lands_at_the_restatements_figure(recon):
    """the phantom of the CPU tests, Lt = 256 on the fused path (16 x 16 x 256): the error against the phantom is the
    interpolation error of the method, 2.14e-2; the GPU lands within 1e-4 of the restatement's own figure (measured:
    2.1393e-2 both)"""
    rec, p0 = pr.phantom_case()
    rec32 = rec.astype(F32)
    own = pr.rel_l2(pr.reconstruct(rec32, (16, 16), 256, (1.0, 1.0), 1.0, 1.0, planes=64), p0[:64])
    p = recon.PlaneRecon((16, 16), (1.0, 1.0), 1.0, 100, 1.0, planes=64, time_length=256)
    try:
        assert p.fused and p.expanded == (16, 16) and p.time_length == 256
        got = p.run(rec32)
    finally:
        p.close()
    err = pr.rel_l2(got, p0[:64])
    print(f"phantom, Lt = 256: GPU against the phantom {err:.4e}, restatement against the phantom {own:.4e}")
    assert abs(err - own) <= 1e-4


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
def test_two_runs_are_bit_equal(recon, fused):
    rec = e2e_record(4)
    p = recon.PlaneRecon(E2E["dims"], E2E["spacing"], DT, E2E["nt"], C0, expanded=E2E["expanded"], fused_kernels=fused)
    try:
        a = p.run(rec)
        b = p.run(rec)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        p.close()
