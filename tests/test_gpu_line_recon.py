"""Batched k-space line reconstruction on the GPU: the fused stage of a frames context (x-forward, k_yfused_line_recon,
x-inverse) at every fast-path line length, with masked x tiles, the x-Nyquist side array and dead side blocks; the stage
against its rocFFT twin, the twin at an odd Lt; the refusals of the frames mode; kw_line_recon_embed / _crop alone; and
kwave_amd.recon.LineRecon end to end against the float64 NumPy restatement of tests/line_recon_reference.py — chunked,
against PlaneRecon, on a record of t alone and on the 2-D phantom of the CPU tests.

Bounds.
  stage, twin, LineRecon    1e-5 relative L2, the project's parity bound, against float64 of the same float32 inputs.  G has
                            two discontinuities (f = M, the end of the line; a = 1/2 for the nearest neighbour): every test
                            asserts first that its inputs keep every bin 1e-9 away from them
                            (line_recon_reference.margins) — a condition on the inputs.  All use dt = dx / (c0 pi).
  two device results        2e-5: each within 1e-5 of the same float64 field.
  embed, crop               exact: copies, zero fill, a clamp of float32 values.
  chunking (fused)          bit-equal: a frame's arithmetic does not depend on its neighbours.
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
import line_recon_reference as lr  # noqa: E402
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
PARITY = 1e-5
MARGIN = 1e-9
LENGTHS = cr.fast_lengths()
C0 = 1500.0
DX = 1.0e-4
DT = DX / (C0 * np.pi)


@pytest.fixture(scope="module")
def recon():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, recon
    assert "kw_fused_line_recon" in capi._SIG and hasattr(recon, "LineRecon")
    return recon


@pytest.fixture()
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def make_op(dy, dt, interp):
    """kw_plane_recon_op of a line reconstruction: dx = the sensor pitch; dy = 0, which the plane stage refuses and the
    line stage must not look at"""
    from kwave_amd import capi
    op = capi.PlaneReconOp()
    op.dx, op.dy, op.dt, op.c0 = dy, 0.0, dt, C0
    op.interp, op.reserved = lr.INTERPS.index(interp), 0
    return op


def assert_margins(ey, lt, dy=DX, dt=DT):
    first, second = lr.margins(ey, lt, dy, dt, C0)
    assert first >= MARGIN and second >= MARGIN, (ey, lt, first, second)


def fused_stage(dev, vol, dy, dt, interps, in_place=False):
    """kw_fused_line_recon of the frames [F][lt][ey] on a frames context of its own, per interpolant"""
    nf, lt, ey = vol.shape
    set_constants(dev, ey, lt, nf)
    dev.call("fused_set_frames", 1)
    ok = C.c_int()
    dev.call("fused_supported", C.byref(ok))
    assert ok.value == 1, (ey, lt, nf)
    dev.call("fused_create")
    src = Guarded(dev, vol)
    out = Guarded(dev, np.full(vol.shape, np.nan, F32))
    got = []
    for interp in interps:
        op = make_op(dy, dt, interp)
        if in_place:
            src.write(vol)
            dev.call("fused_line_recon", src.ptr, C.byref(op), src.ptr)
            dev.sync()
            got.append(src.read())
        else:
            dev.call("fused_line_recon", src.ptr, C.byref(op), out.ptr)
            dev.sync()
            got.append(out.read())
            assert np.array_equal(src.read().view(np.uint32), vol.view(np.uint32))   # the input is not written
    dev.call("fused_destroy")
    src.free()
    out.free()
    return got


def twin_stage(vol, dy, dt, interps):
    """kw_fft_r2c_frames, kw_line_recon_mix, kw_fft_c2r_frames on a context of its own, per interpolant"""
    from kwave_amd import capi
    nf, lt, ey = vol.shape
    d2 = capi.Device()
    got = []
    try:
        d2.call("line_recon_mix", None, None, None, C.c_float(1.0))   # no constants, no bins: no pointer is looked at
        set_constants(d2, ey, lt, nf)
        d2.call("fft_create_plans_frames")
        nr = (ey // 2 + 1) * lt * nf
        src, spec = Guarded(d2, vol), Guarded(d2, np.zeros(2 * nr, F32))
        d2.call("fft_r2c_frames", src.ptr, spec.ptr)
        d2.sync()
        spec_bytes = spec.read().view(np.uint8)
        mixed, out = Guarded(d2, np.full(2 * nr, np.nan, F32)), Guarded(d2, np.full(vol.shape, np.nan, F32))
        for interp in interps:
            op = make_op(dy, dt, interp)
            d2.call("line_recon_mix", mixed.ptr, spec.ptr, C.byref(op), C.c_float(2.0 / (ey * lt)))
            d2.call("fft_c2r_frames", mixed.ptr, out.ptr)
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
    """t-even random frames.  [3][L][16]: k_yfused_line_recon<L>, the gather along a line of every length, both
    interpolants, three frames whose 3 L rows end in a masked x tile (32 rows per tile at Ey = 16) wherever 3 L is no
    multiple of 32; [2][16][L]: the column addressing and the x passes at every length, linear — where L is a multiple of 32
    they write and read the side array [2][16], whose one side block runs with 2 of its 16 positions valid.  The whole
    expanded output is compared.  Measured 1.4e-7 to 2.2e-7 for [3][L][16] (worst at 1024) and 1.5e-7 to 2.4e-7 for
    [2][16][L] (worst at 756)."""
    for (nf, lt, ey), interps in (((3, L, 16), lr.INTERPS), ((2, 16, L), ("linear",))):
        assert_margins(ey, lt)
        vol = lr.even_frames((nf, lt, ey), ey * 1009 + lt * 31 + nf)
        got = fused_stage(dev, vol, DX, DT, interps)
        for interp, g in zip(interps, got):
            err = lr.rel_l2(g, lr.stage(vol, DX, DT, C0, interp))
            print(f"line-recon stage [{nf}][{lt}][{ey}] {interp}: rel L2 {err:.3e}")
            assert err < PARITY, (nf, lt, ey, interp)


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length_with_side_blocks(dev, L):
    """t-even random frames [17][L][96]: k_yfused_line_recon<L> on three main column tiles (two 32-column ones, the second
    half valid, at 240 and 400) and on the blocks of the x-Nyquist side array [17][L]: one full block of 16 frames and one
    with a single valid frame (at 240 and 400, 32 frames per block: one block with 17 valid, none dead); the other blocks of
    that tile index, past the last frame, return.  Both interpolants, the whole expanded output: frame 16 comes out right,
    and the guard bands show that nothing past it is stored.  Measured 1.7e-7 to 2.6e-7 (worst at 648), frame 16 alone
    1.6e-7 to 2.6e-7."""
    nf, lt, ey = 17, L, 96
    assert_margins(ey, lt)
    vol = lr.even_frames((nf, lt, ey), ey * 1009 + lt * 31 + nf)
    got = fused_stage(dev, vol, DX, DT, lr.INTERPS)
    for interp, g in zip(lr.INTERPS, got):
        want = lr.stage(vol, DX, DT, C0, interp)
        err, last = lr.rel_l2(g, want), lr.rel_l2(g[16], want[16])
        print(f"line-recon stage [{nf}][{lt}][{ey}] {interp}: rel L2 {err:.3e}, frame 16 {last:.3e}")
        assert err < PARITY and last < PARITY, (nf, lt, ey, interp)


# ---- 2. fused against twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,lt,ey", [(5, 64, 32), (3, 96, 48)])
def test_fused_stage_and_rocfft_twin(dev, nf, lt, ey):
    """the stage in place and the twin against the restatement and against each other, dy = 0.8 dx.  Measured 1.8e-7 to
    2.0e-7 (fused), 1.9e-7 to 2.1e-7 (twin) and 2.2e-7 to 2.5e-7."""
    dy = 0.8 * DX
    assert_margins(ey, lt, dy)
    vol = lr.even_frames((nf, lt, ey), nf + lt + ey)
    fused = fused_stage(dev, vol, dy, DT, lr.INTERPS, in_place=True)
    fused_out = fused_stage(dev, vol, dy, DT, ("linear",))        # out of place: the input is not written
    assert np.array_equal(fused_out[0].view(np.uint32), fused[0].view(np.uint32))
    twin = twin_stage(vol, dy, DT, lr.INTERPS)
    for interp, f, t in zip(lr.INTERPS, fused, twin):
        want = lr.stage(vol, dy, DT, C0, interp)
        ef, et, eb = lr.rel_l2(f, want), lr.rel_l2(t, want), lr.rel_l2(f, t)
        print(f"line-recon [{nf}][{lt}][{ey}] {interp}: fused stage {ef:.3e}, rocFFT twin {et:.3e} (rel L2 against float64), "
              f"fused against twin {eb:.3e}")
        assert ef < PARITY and et < PARITY and eb < 2 * PARITY


def test_twin_at_odd_time_length():
    """[3][79][20]: k-Wave's own grid Lt = 2 Nt - 1 for Nt = 40; M = 39, and the bins M and M + 1 mirror each other.
    Measured 2.6e-7 and 2.5e-7."""
    nf, lt, ey = 3, 79, 20
    assert_margins(ey, lt)
    vol = lr.even_frames((nf, lt, ey), 79)
    for interp, t in zip(lr.INTERPS, twin_stage(vol, DX, DT, lr.INTERPS)):
        err = lr.rel_l2(t, lr.stage(vol, DX, DT, C0, interp))
        print(f"line-recon twin [{nf}][{lt}][{ey}] {interp}: rel L2 {err:.3e}")
        assert err < PARITY


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def test_frames_context_refuses_the_other_stages_and_the_line_stage_refuses_other_contexts(dev):
    from kwave_amd import capi
    a = Guarded(dev, np.zeros(32 * 32 * 16, F32))
    b = Guarded(dev, np.zeros(32 * 32 * 16, F32))
    op = make_op(DX, DT, "linear")
    op.dy = DX
    # a frames context: every other stage is refused, by the mode's name
    set_constants(dev, 32, 32, 16)
    dev.call("fused_set_frames", 1)
    dev.call("fused_create")
    with pytest.raises(capi.KWaveError, match=r"kw_fused_set_frames: must be called before kw_fused_create"):
        dev.call("fused_set_frames", 0)
    with pytest.raises(capi.KWaveError, match=r"kw_fused_scale_source: .*frames mode"):
        dev.call("fused_scale_source", a.ptr, b.ptr)
    with pytest.raises(capi.KWaveError, match=r"kw_fused_plane_recon: .*frames mode"):
        dev.call("fused_plane_recon", a.ptr, C.byref(op), b.ptr)
    n = C.c_size_t()
    with pytest.raises(capi.KWaveError, match=r"frames mode"):
        dev.call("fused_reduced_elems", C.byref(n))
    dev.call("fused_destroy")
    # the line stage on a 3-D and on a 2-D context (the destroy above has ended the frames mode)
    for nz in (16, 1):
        set_constants(dev, 32, 32, nz)
        dev.call("fused_create")
        with pytest.raises(capi.KWaveError, match=r"kw_fused_line_recon: needs a context in frames mode"):
            dev.call("fused_line_recon", a.ptr, C.byref(op), b.ptr)
        dev.call("fused_destroy")
    # the plane stage keeps its own refusal of Nz == 1
    set_constants(dev, 32, 32, 1)
    dev.call("fused_create")
    with pytest.raises(capi.KWaveError, match=r"kw_fused_plane_recon: single GPU and 3-D only \(no Z-slabs, no Nz == 1\)"):
        dev.call("fused_plane_recon", a.ptr, C.byref(op), b.ptr)
    dev.call("fused_destroy")
    dev.sync()
    assert not a.read().any() and not b.read().any()   # nothing is written by a refused call
    a.free()
    b.free()


def test_frames_context_support_rule(dev):
    """no transform along z: any F up to 65535 (the frame is a block index); the ten x lengths without masked x kernels
    need whole x tiles of 16 rows; the padded bins P Lt F of one scratch array stay below 2^29, because the pass along t
    addresses a frame's lines by 32-bit byte offsets (80 x 1024 x 6553 bins end below 4 GiB, 6554 frames do not).  Only the
    query: nothing of that size is allocated."""
    ok = C.c_int()
    for (ey, lt, nf), want in (((32, 64, 5), 1), ((32, 64, 1), 1), ((32, 59, 4), 0), ((30, 64, 4), 0),
                               ((672, 100, 1), 0), ((672, 100, 4), 1), ((640, 100, 1), 1),
                               ((128, 1024, 6553), 1), ((128, 1024, 6554), 0), ((1024, 1024, 992), 1), ((1024, 1024, 993), 0),
                               ((16, 16, 65535), 1), ((16, 16, 65536), 0)):
        set_constants(dev, ey, lt, nf)
        dev.call("fused_set_frames", 1)
        dev.call("fused_supported", C.byref(ok))
        assert ok.value == want, (ey, lt, nf)
    dev.call("fused_set_frames", 0)
    set_constants(dev, 32, 64, 5)
    dev.call("fused_supported", C.byref(ok))
    assert ok.value == 0   # as a 3-D grid, 5 is no line length


# ---- 4. embed and crop alone ------------------------------------------------------------------------------------------------
EMBED_CASES = [  # (F, nt, ny), (lt, ey), byte offset of the device pointers
    ((5, 20, 23), (48, 40), 0),        # scalar path
    ((5, 24, 24), (48, 48), 0),        # 16-byte path
    ((5, 24, 24), (48, 48), 4),        # the same sizes off 16-byte alignment: scalar path
    ((1, 24, 24), (48, 48), 0),        # one frame
    ((5, 20, 1), (39, 40), 0),         # one sensor, Lt = 2 Nt - 1
    ((3, 24, 40), (47, 40), 0),        # k-Wave's grid: nothing to fill but the mirror image
    ((4, 1, 8), (1, 8), 0),            # one sample per sensor: no mirror image at all
    ((40, 5, 200), (64, 1024), 0),     # beyond one grid-stride round (2^19 threads), 16-byte path
    ((40, 5, 201), (64, 1024), 0),     # ... and scalar
    ((40, 40, 1024), (80, 1024), 0),   # the crop's 16-byte path beyond one grid-stride round
]


@pytest.mark.parametrize("dims,expanded,offset", EMBED_CASES)
def test_embed_and_crop_are_exact(dev, dims, expanded, offset):
    (nf, nt, ny), (lt, ey) = dims, expanded
    rng = np.random.default_rng(nf * 7 + ny * 3 + nt + offset)
    src = rng.standard_normal((nf, nt, ny)).astype(F32)
    gs = Guarded(dev, src, offset)
    vol = Guarded(dev, np.full((nf, lt, ey), np.nan, F32), offset)
    dev.call("line_recon_embed", vol.ptr, gs.ptr, ey, lt, nf, ny, nt)
    dev.sync()
    got = vol.read()
    want = lr.embed(src, ey, lt)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for n in range(1, lt):
        assert np.array_equal(got[:, lt - n], got[:, n])
    assert np.array_equal(gs.read(), src)
    # crop on a volume that is random everywhere: what lies outside the crop must not be looked at
    full = rng.standard_normal((nf, lt, ey)).astype(F32)
    full[0, 0, 0] = -0.0
    vol.write(full)
    for depth in (lt, max(1, nt - 1)):
        for positivity in (0, 1):
            for frames in sorted({nf, max(1, nf - 2)}):   # fewer frames than the volume holds: a padded last chunk
                out = Guarded(dev, np.full((frames, depth, ny), np.nan, F32), offset)
                dev.call("line_recon_crop", out.ptr, vol.ptr, ey, lt, frames, ny, depth, positivity)
                dev.sync()
                want = lr.crop(full[:frames], ny, depth, bool(positivity))
                assert np.array_equal(out.read().view(np.uint32), want.view(np.uint32)), (depth, positivity, frames)
                out.free()
    assert np.array_equal(vol.read().view(np.uint32), full.view(np.uint32))
    gs.free()
    vol.free()


def test_embed_and_crop_of_nothing(dev):
    vol = Guarded(dev, np.full((2, 8, 8), np.nan, F32))
    out = Guarded(dev, np.full((2, 8, 8), np.nan, F32))
    dev.call("line_recon_crop", out.ptr, vol.ptr, 8, 8, 2, 0, 8, 0)     # zero sensors
    dev.call("line_recon_crop", out.ptr, vol.ptr, 8, 8, 2, 8, 0, 1)     # zero rows
    dev.call("line_recon_crop", out.ptr, vol.ptr, 8, 8, 0, 8, 8, 1)     # zero frames
    dev.call("line_recon_crop", None, None, 8, 8, 2, 0, 8, 0)
    dev.call("line_recon_embed", None, None, 0, 8, 2, 0, 0)             # an empty volume
    dev.call("line_recon_embed", None, None, 8, 8, 0, 8, 4)             # no frames
    dev.sync()
    assert np.isnan(out.read()).all() and np.isnan(vol.read()).all()
    dev.call("line_recon_embed", vol.ptr, None, 8, 8, 2, 0, 4)          # empty records: all zeros
    dev.sync()
    assert not vol.read().any()
    vol.free()
    out.free()


def test_embed_refuses_a_volume_shorter_than_the_mirrored_record(dev):
    from kwave_amd import capi
    vol = Guarded(dev, np.full((2, 8, 8), np.nan, F32))
    src = Guarded(dev, np.zeros((2, 5, 8), F32))
    with pytest.raises(capi.KWaveError):
        dev.call("line_recon_embed", vol.ptr, src.ptr, 8, 8, 2, 8, 5)   # 2 * 5 - 1 = 9 > 8
    dev.sync()
    assert np.isnan(vol.read()).all()
    vol.free()
    src.free()


# ---- 5. LineRecon end to end ------------------------------------------------------------------------------------------------
E2E = dict(ny=24, nt=30, dy=0.8 * DX, expanded=32, frames=4)


def e2e_record(seed, frames=E2E["frames"]):
    rng = np.random.default_rng(seed)
    ny, nt = E2E["ny"], E2E["nt"]
    t = np.arange(nt)[None, :, None] / nt
    phase = rng.uniform(-np.pi, np.pi, (frames, 1, ny))
    amp = rng.uniform(0.2, 1.0, (frames, 1, ny))
    p = amp * np.sin(2 * np.pi * 4 * t + phase) * np.exp(-((t - 0.5) ** 2) / 0.03) + 0.05 * rng.standard_normal((frames, nt, ny))
    return p.astype(F32)


@functools.lru_cache(maxsize=None)
def e2e_reference(lt, interp, positivity, seed, frames=E2E["frames"]):
    return lr.reconstruct(e2e_record(seed, frames), E2E["expanded"], lt, E2E["dy"], DT, C0, interp=interp, positivity=positivity)


def make_recon(recon, fused, frames=E2E["frames"], **kw):
    kw.setdefault("expanded", E2E["expanded"])
    if fused:
        kw.setdefault("time_length", 64)
    return recon.LineRecon(E2E["ny"], E2E["dy"], DT, E2E["nt"], C0, frames=frames, fused_kernels=fused, **kw)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
@pytest.mark.parametrize("positivity", [False, True], ids=["signed", "positive"])
@pytest.mark.parametrize("interp", lr.INTERPS)
def test_line_recon_against_the_restatement(recon, interp, positivity, fused):
    """Nt = 30, Ny = 24 in Ey = 32, four frames; Lt = 64 on the fused path and 59 (k-Wave's grid) on rocFFT.  Measured
    1.7e-7 to 1.9e-7 fused, 3.5e-7 to 3.6e-7 rocFFT."""
    lt = 64 if fused else 59
    assert_margins(E2E["expanded"], lt, E2E["dy"])
    p = make_recon(recon, fused, interp=interp, positivity=positivity)
    q = make_recon(recon, fused, interp=interp, positivity=positivity, order="yt")
    try:
        assert p.fused == fused and p.expanded == 32 and p.time_length == lt and p.runs == 0 and p.chunk_frames == 4
        assert p.dx == pytest.approx(C0 * DT, rel=1e-15) and p.depth == 30
        rec = e2e_record(1)
        got = p.run(rec)
        assert got.dtype == F32 and got.shape == (4, 30, 24)
        err = lr.rel_l2(got, e2e_reference(lt, interp, positivity, 1))
        assert not positivity or got.min() >= 0.0
        # a second run with other records reuses everything
        got2 = p.run(e2e_record(2))
        err2 = lr.rel_l2(got2, e2e_reference(lt, interp, positivity, 2))
        print(f"LineRecon {interp} positivity {positivity} fused {fused}: rel L2 {err:.3e}, second records {err2:.3e}")
        assert p.runs == 2 and max(err, err2) < PARITY
        # the transposed records give the same bits
        got3 = q.run(np.ascontiguousarray(rec.transpose(0, 2, 1)))
        assert np.array_equal(got3.view(np.uint32), got.view(np.uint32))
    finally:
        p.close()
        q.close()


def test_one_frame_as_a_two_d_array_and_fewer_rows(recon):
    rec = e2e_record(3, 1)
    p = make_recon(recon, True, frames=1)
    q = make_recon(recon, True, frames=1, depth=7)
    try:
        full, few = p.run(rec[0]), q.run(rec)
        assert full.shape == (30, 24) and few.shape == (1, 7, 24) and np.array_equal(few[0], full[:7])
        with pytest.raises(ValueError, match="p must be"):
            p.run(rec[0, :-1])
    finally:
        p.close()
        q.close()


# ---- 6. chunking --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
def test_chunks_give_every_frame_its_own_result(recon, fused):
    """seven frames in chunks of three (the last chunk filled up with two zero records), in one chunk, and one by one.  On the
    fused path the three are bit-equal: the x passes pair the rows t, t + 1 of one frame (Lt is even) and the pass along t
    takes each frame's lines apart.  On rocFFT (whose plans differ with the batch) each is within the parity bound.
    Measured 1.7e-7 fused (worst frame 2.0e-7) and 3.7e-7 on rocFFT (worst frame 4.0e-7), the same at every chunking."""
    lt = 64 if fused else 59
    assert_margins(E2E["expanded"], lt, E2E["dy"])
    rec = e2e_record(5, 7)
    results = {}
    for chunk in (3, 7):
        p = make_recon(recon, fused, frames=7, chunk_frames=chunk)
        try:
            assert p.fused == fused and p.chunk_frames == chunk
            results[chunk] = p.run(rec)
        finally:
            p.close()
    p = make_recon(recon, fused, frames=1)
    try:
        results[1] = np.stack([p.run(rec[f]) for f in range(7)])
        assert p.runs == 7
    finally:
        p.close()
    want = e2e_reference(lt, "linear", False, 5, 7)
    for chunk, got in results.items():
        err = lr.rel_l2(got, want)
        worst = max(lr.rel_l2(got[f], want[f]) for f in range(7))
        print(f"LineRecon fused {fused}, 7 frames in chunks of {chunk}: rel L2 {err:.3e}, worst frame {worst:.3e}")
        assert got.shape == (7, 30, 24) and err < PARITY and worst < PARITY
    if fused:
        assert np.array_equal(results[3].view(np.uint32), results[7].view(np.uint32))
        assert np.array_equal(results[1].view(np.uint32), results[7].view(np.uint32))


# ---- 7. against the plane reconstruction --------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", lr.INTERPS)
def test_plane_recon_of_a_record_constant_along_x_is_the_line_recon(recon, interp):
    """PlaneRecon on a 16 x Ny record that is constant along its x axis (kx = 0 on the only bins that carry anything: the
    plane's rho2 is the line's) against LineRecon on one row: new code against old code through different kernels
    (x-forward, y-pass, k_zfused_recon, ... against x-forward, k_yfused_line_recon, x-inverse on another layout).
    Measured 1.6e-7 and 1.7e-7."""
    assert_margins(E2E["expanded"], 64, E2E["dy"])
    rec = e2e_record(6, 1)[0]                                            # [nt][ny]
    plane_rec = np.ascontiguousarray(np.repeat(rec[:, :, None], 16, axis=2))   # [nt][ny][16]
    pl = recon.PlaneRecon((16, E2E["ny"]), (1.3 * DX, E2E["dy"]), DT, E2E["nt"], C0, interp=interp,
                          expanded=(16, E2E["expanded"]), time_length=64)
    ln = make_recon(recon, True, frames=1, interp=interp)
    try:
        assert pl.fused and ln.fused
        a, b = pl.run(plane_rec), ln.run(rec)
    finally:
        pl.close()
        ln.close()
    worst = max(lr.rel_l2(a[:, :, ix], b) for ix in range(16))
    print(f"PlaneRecon on a record constant along x against LineRecon, {interp}: worst column {worst:.3e}")
    assert worst < 2 * PARITY


# ---- 8. identity, phantom, repeatability ------------------------------------------------------------------------------------
def test_record_of_t_alone_gives_back_its_profile(recon):
    """the identity of the CPU tests on the GPU, fused (Ey = 16, Lt = 80) and rocFFT (Lt = 79): rho2 = 0 on the only bins
    that carry anything, so both interpolants return g(x).  Measured 9.8e-8 fused, 1.7e-7 rocFFT."""
    nt = 40
    rec, g = lr.identity_record(nt, 16)
    for fused, lt in ((True, 80), (False, 79)):
        for interp in lr.INTERPS:
            p = recon.LineRecon(16, DX, DT, nt, C0, interp=interp, fused_kernels=fused)
            try:
                assert p.fused == fused and p.time_length == lt
                got = p.run(rec.astype(F32))
            finally:
                p.close()
            want = np.broadcast_to(2.0 * rec.astype(F32).astype(np.float64), got.shape)   # g of the float32 record
            err = lr.rel_l2(got, want)
            print(f"identity record, fused {fused} {interp}: rel L2 against g {err:.3e}")
            assert err < PARITY
            assert np.max(np.abs(want[:, 0] - g)) < 1e-7


def test_phantom_lands_at_the_restatements_figure(recon):
    """the 2-D phantom of the CPU tests, Lt = 256 on the fused path (Ey = 16): the error against the phantom is the
    interpolation error of the method, 1.94e-2; the GPU lands within 1e-4 of the restatement's own figure (measured:
    1.9399e-2 both)"""
    rec, p0 = lr.phantom_case()
    rec32 = rec.astype(F32)
    own = lr.rel_l2(lr.reconstruct(rec32, 16, 256, 1.0, 1.0, 1.0, depth=64), p0[:64])
    p = recon.LineRecon(16, 1.0, 1.0, 100, 1.0, depth=64, time_length=256)
    try:
        assert p.fused and p.expanded == 16 and p.time_length == 256
        got = p.run(rec32)
    finally:
        p.close()
    err = lr.rel_l2(got, p0[:64])
    print(f"phantom, Lt = 256: GPU against the phantom {err:.4e}, restatement against the phantom {own:.4e}")
    assert abs(err - own) <= 1e-4


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
def test_two_runs_are_bit_equal(recon, fused):
    rec = e2e_record(4)
    p = make_recon(recon, fused)
    try:
        a = p.run(rec)
        b = p.run(rec)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        p.close()
