"""Batched 2-D exact k-space propagator on the GPU: the fused stage of a frames context (x-forward kept,
k_yfused_second_order, x-inverse) at every fast-path line length, with and without the side array's blocks, the stage
against its rocFFT twin, the refusals, kwave_amd.second_order.SecondOrderFrames end to end against the float64 restatement
of tests/second_order_frames_reference.py, next to the 3-D class, and the wrap-around rule.

Bounds.
  stage, twin, SecondOrderFrames   1e-5 relative L2, the project's parity bound (PARITY of the sibling tests), against float64
                             of the same float32 inputs, over the whole expanded output.  The absorbing variants assert
                             first that B >= 1/4 on every bin of their grid, and every stage case that the expected result
                             has not vanished — conditions on the inputs.
  fused against twin, frames against the 3-D class   2e-5: two results within 1e-5 of the same float64 field.
  field(0)                   1e-6: H = 1, the forward and inverse pipeline alone.
  p_max, p_min, a frame alone or in a batch, a second set_p0, interleaved propagators   exact.
  wrap-around                2e-5 plus the restatement's own difference between the two expansions.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import cw_reference as cr  # noqa: E402
import second_order_frames_reference as fr  # noqa: E402
import second_order_reference as sr  # noqa: E402
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
PARITY = 1e-5
LENGTHS = cr.fast_lengths()
C0 = 1500.0
ENTRIES = ("kw_fused_second_order_frames_elems", "kw_fused_second_order_frames_forward", "kw_fused_second_order_frames_time",
           "kw_second_order_frames_mix")


@pytest.fixture(scope="module")
def second_order():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, second_order
    for name in ENTRIES:
        assert name in capi._SIG
    assert hasattr(second_order, "SecondOrderFrames")
    return second_order


@pytest.fixture()
def dev(second_order):
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def make_op(d, c0, t, coeff, y):
    """kw_second_order_op of a plane: dz = 0, which the 3-D entries refuse and the frames entries must not look at"""
    from kwave_amd import capi
    op = capi.SecondOrderOp()
    op.dx, op.dy, op.dz, op.c0, op.t = d[0], d[1], 0.0, c0, t
    op.a, op.alpha_power = sr.neper(coeff, y), y
    op.absorbing = int(coeff > 0.0)
    return op


def source_frames(rng, nf, ey, ex):
    """every frame its own smooth random field on the whole expanded plane plus 5 % white noise, so that every bin (the
    x-Nyquist column among them) carries something"""
    y, x = np.meshgrid(np.arange(ey) / ey, np.arange(ex) / ex, indexing="ij")
    out = np.empty((nf, ey, ex), F32)
    for f in range(nf):
        c = rng.uniform(-1.0, 1.0, 8)
        s = (c[0] + c[1] * np.cos(2 * np.pi * x + c[2]) * np.sin(2 * np.pi * y + c[6]) +
             c[3] * np.sin(4 * np.pi * y + c[4]) * np.cos(2 * np.pi * x) +
             c[5] * np.exp(-((x - 0.4) ** 2 + (y - 0.6) ** 2) / 0.02) * np.cos(6 * np.pi * y + c[7]))
        out[f] = s + 0.05 * rng.standard_normal((ey, ex))
    return out


class Stage:
    """a frames context of (ex, ey, F) with a batch transformed once and kept; time(op) gives every frame at one time"""

    def __init__(self, dev, vol):
        nf, ey, ex = vol.shape
        self.dev = dev
        set_constants(dev, ex, ey, nf)
        dev.call("fused_set_frames", 1)
        ok = C.c_int()
        dev.call("fused_supported", C.byref(ok))
        assert ok.value == 1, (ex, ey, nf)
        dev.call("fused_create")
        n = C.c_size_t()
        dev.call("fused_second_order_frames_elems", C.byref(n))
        assert n.value == (ex // 2 + 1 + 15) // 16 * 16 * ey * nf
        self.vol = Guarded(dev, vol)
        self.kept = Guarded(dev, np.full(2 * n.value, np.nan, F32))
        dev.call("fused_second_order_frames_forward", self.vol.ptr, self.kept.ptr)
        dev.sync()
        assert np.array_equal(self.vol.read().view(np.uint32), vol.view(np.uint32))   # the input is not written
        self.kept_bytes = self.kept.read().view(np.uint8)
        self.out = Guarded(dev, np.full(vol.shape, np.nan, F32))

    def time(self, op):
        self.dev.call("fused_second_order_frames_time", self.kept.ptr, C.byref(op), self.out.ptr)
        self.dev.sync()
        return self.out.read()   # (the guard bands: nothing is stored outside the batch)

    def close(self):
        assert np.array_equal(self.kept.read().view(np.uint8), self.kept_bytes)  # the kept spectrum survives every time
        self.dev.call("fused_destroy")
        for g in (self.vol, self.kept, self.out):
            g.free()


# ---- 1. the fused stage at every line length ------------------------------------------------------------------------------
def stage_errors(dev, ex, ey, nf, frame=None):
    """lossless near and far, absorbing near and far (second_order_reference.stage_case on the plane); the whole expanded
    output of every frame, and where asked for that of one frame alone"""
    d = sr.STAGE_D[:2]
    cases = fr.stage_case((ex, ey))
    assert fr.b_margins((ex, ey), d, sr.STAGE_C0, cases[3][0], sr.STAGE_Y)[0] >= 0.25
    vol = source_frames(np.random.default_rng(ex * 1009 + ey * 31 + nf), nf, ey, ex)
    X = np.fft.rfftn(vol.astype(np.float64), axes=(1, 2))
    s = Stage(dev, vol)
    errs, alone = [], []
    for coeff, t in cases:
        got = s.time(make_op(d, sr.STAGE_C0, t, coeff, sr.STAGE_Y))
        want = np.fft.irfftn(X * fr.H((ex, ey), d, sr.STAGE_C0, t, coeff, sr.STAGE_Y), s=vol.shape[1:], axes=(1, 2))
        assert np.linalg.norm(want) > 1e-3 * np.linalg.norm(vol)   # the result has not vanished
        errs.append(sr.rel_l2(got, want))
        if frame is not None:
            alone.append(sr.rel_l2(got[frame], want[frame]))
    s.close()
    return errs, alone


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length(dev, L):
    """(Ex, Ey, F) = (16, L, 3): k_yfused_second_order<L> on one column tile, 3 x 16 ... 3 x 1024 rows for the x passes (a
    masked last x tile wherever 3 L is no multiple of 32); (L, 16, 2): the x passes and the column addressing at every
    length — where L is a multiple of 32 the side array's one block runs with 2 of its positions valid.  Spacings
    STAGE_D[:2].  Lossless and absorbing (y = 1.5), c0 t = 0.37 of the smallest spacing and the time at which the largest |k|
    has made 10^4 turns.  Measured, (16, L, 3): lossless 1.0e-7 to 1.7e-7 near and 9.7e-8 to 2.5e-7 far (worst at L = 288),
    absorbing 1.0e-7 to 1.8e-7 near and 3.1e-8 to 1.3e-7 far; (L, 16, 2): lossless 1.0e-7 to 2.1e-7 near and 9.3e-8 to 3.0e-7 far
    (worst at L = 672), absorbing 1.0e-7 to 1.8e-7 near and 2.5e-8 to 1.3e-7 far."""
    for ex, ey, nf in ((16, L, 3), (L, 16, 2)):
        errs, _ = stage_errors(dev, ex, ey, nf)
        print(f"second-order frames stage {ex}x{ey}x{nf}: rel L2 lossless near {errs[0]:.3e} far {errs[1]:.3e}; "
              f"absorbing near {errs[2]:.3e} far {errs[3]:.3e}")
        assert max(errs) < PARITY, (ex, ey, nf)


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length_with_side_blocks(dev, L):
    """(96, L, 17): k_yfused_second_order<L> on three main column tiles and on the blocks of the x-Nyquist side array
    [17][L], which form H at kx = Ex/2: one full block of 16 frames and one with a single live frame (at 240 and 400, 32
    frames per block: one block with 17 live); the blocks past the last frame return.  Frame 16 alone is held to the bound
    as well, and the guard bands show that nothing is stored past it.  Measured: lossless 1.2e-7 to 1.8e-7 near and 1.1e-7 to
    1.9e-7 far, absorbing 1.3e-7 to 1.9e-7 near and 4.6e-8 to 9.3e-8 far; frame 16 alone 1.1e-7 to 3.5e-7 (worst at L = 504)."""
    errs, last = stage_errors(dev, 96, L, 17, frame=16)
    print(f"second-order frames stage 96x{L}x17: rel L2 lossless near {errs[0]:.3e} far {errs[1]:.3e}; absorbing near "
          f"{errs[2]:.3e} far {errs[3]:.3e}; frame 16 alone worst {max(last):.3e}")
    assert max(errs) < PARITY and max(last) < PARITY, L


# ---- 2. fused against twin ------------------------------------------------------------------------------------------------
TWIN = dict(d=(1.0e-4, 0.8e-4), t=37.3 * 0.8e-4 / C0)
# y = 1.5 (|k|^(y-1) by a square root), lossless, Stokes (y = 2: |k| itself), y = 1.1 (the float64 power function)
VARIANTS = ((0.75, 1.5), (0.0, 1.5), (0.2, 2.0), (0.75, 1.1))


def twin_stage(d2, vol, variants):
    """kw_fft_r2c_frames, kw_second_order_frames_mix, kw_fft_c2r_frames, one C2R transform per variant"""
    nf, ey, ex = vol.shape
    p = TWIN
    d2.call("second_order_frames_mix", None, None, None, C.c_float(1.0))   # no constants, no bins: no pointer is looked at
    set_constants(d2, ex, ey, nf)
    d2.call("fft_create_plans_frames")
    nr = (ex // 2 + 1) * ey * nf
    src, spec = Guarded(d2, vol), Guarded(d2, np.zeros(2 * nr, F32))
    d2.call("fft_r2c_frames", src.ptr, spec.ptr)
    d2.sync()
    spec_bytes = spec.read().view(np.uint8)
    mixed, out = Guarded(d2, np.full(2 * nr, np.nan, F32)), Guarded(d2, np.full(vol.shape, np.nan, F32))
    got = []
    for coeff, y in variants:
        op = make_op(p["d"], C0, p["t"], coeff, y)
        d2.call("second_order_frames_mix", mixed.ptr, spec.ptr, C.byref(op), C.c_float(1.0 / (ex * ey)))
        d2.call("fft_c2r_frames", mixed.ptr, out.ptr)
        d2.sync()
        got.append(out.read())
    assert np.array_equal(spec.read().view(np.uint8), spec_bytes)   # out of place: the spectra are read only
    for g in (src, spec, mixed, out):
        g.free()
    return got


def assert_underdamped(ex, ey):
    for coeff, y in VARIANTS:
        assert coeff == 0.0 or fr.b_margins((ex, ey), TWIN["d"], C0, coeff, y)[0] >= 0.25


@pytest.mark.parametrize("nf,ey,ex", [(5, 48, 32), (3, 64, 96)])
def test_fused_stage_and_rocfft_twin(dev, nf, ey, ex):
    """dy = 0.8 dx; (3, 64, 96) has the side array.  Measured: fused 1.1e-7 to 1.4e-7, twin 1.0e-7 to 1.8e-7, one against the
    other 1.3e-7 to 2.0e-7."""
    from kwave_amd import capi
    p = TWIN
    assert_underdamped(ex, ey)
    vol = source_frames(np.random.default_rng(nf + ey + ex), nf, ey, ex)
    s = Stage(dev, vol)
    fused = [s.time(make_op(p["d"], C0, p["t"], coeff, y)) for coeff, y in VARIANTS]
    s.close()
    d2 = capi.Device()
    try:
        twins = twin_stage(d2, vol, VARIANTS)
    finally:
        d2.close()
    for (coeff, y), f, t in zip(VARIANTS, fused, twins):
        want = fr.solve_expanded(vol, p["d"], C0, p["t"], coeff, y)
        ef, et, eb = sr.rel_l2(f, want), sr.rel_l2(t, want), sr.rel_l2(f, t)
        print(f"second-order frames [{nf}][{ey}][{ex}] alpha_coeff {coeff} y {y}: fused stage {ef:.3e}, rocFFT twin {et:.3e} "
              f"(rel L2 against float64), fused against twin {eb:.3e}")
        assert ef < PARITY and et < PARITY and eb < 2 * PARITY


def test_rocfft_twin_on_an_odd_grid(dev):
    nf, ey, ex = 4, 27, 33
    assert_underdamped(ex, ey)
    vol = source_frames(np.random.default_rng(2733), nf, ey, ex)
    for (coeff, y), t in zip(VARIANTS, twin_stage(dev, vol, VARIANTS)):
        err = sr.rel_l2(t, fr.solve_expanded(vol, TWIN["d"], C0, TWIN["t"], coeff, y))
        print(f"second-order frames twin [{nf}][{ey}][{ex}] alpha_coeff {coeff} y {y}: rel L2 {err:.3e}")
        assert err < PARITY


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def test_frames_entries_refuse_every_other_context(dev):
    from kwave_amd import capi
    a = Guarded(dev, np.zeros(2 * 32 * 32 * 16, F32))
    b = Guarded(dev, np.zeros(2 * 32 * 32 * 16, F32))
    op = make_op((1e-4, 1e-4), C0, 1e-7, 0.0, 1.5)
    n = C.c_size_t(12345)
    entries = (("fused_second_order_frames_time", (a.ptr, C.byref(op), b.ptr)),
               ("fused_second_order_frames_forward", (a.ptr, b.ptr)), ("fused_second_order_frames_elems", (C.byref(n),)))

    def refused(what):
        for entry, args in entries:
            with pytest.raises(capi.KWaveError, match="kw_" + entry + ": " + what):
                dev.call(entry, *args)

    # before kw_fused_create, on a context with constants and on one that has asked for frames
    set_constants(dev, 32, 32, 16)
    refused("kw_fused_create has not been called")
    dev.call("fused_set_frames", 1)
    refused("kw_fused_create has not been called")
    dev.call("fused_set_frames", 0)
    needs = r"needs a context in frames mode \(kw_fused_set_frames before kw_fused_create\)"
    for nz in (16, 1):   # a 3-D and a 2-D context
        set_constants(dev, 32, 32, nz)
        dev.call("fused_create")
        refused(needs)
        dev.call("fused_destroy")
    # one rank with an exchange callback = the slab path against itself; the callback is never reached
    exchange = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)(lambda *args: 1)
    set_constants(dev, 32, 32, 16)
    dev.call("fused_set_slab", 1, 0, 16, C.cast(exchange, C.c_void_p), None)
    dev.call("fused_create")
    refused(needs)
    dev.call("fused_destroy")
    # on a frames context: a dx of 0 is refused, a dz of 0 is not looked at (the stage test runs with it)
    set_constants(dev, 32, 32, 16)
    dev.call("fused_set_frames", 1)
    dev.call("fused_create")
    bad = make_op((0.0, 1e-4), C0, 1e-7, 0.0, 1.5)
    with pytest.raises(capi.KWaveError, match="kw_fused_second_order_frames_time"):
        dev.call("fused_second_order_frames_time", a.ptr, C.byref(bad), b.ptr)
    dev.call("fused_destroy")
    dev.sync()
    assert not a.read().any() and not b.read().any() and n.value == 12345   # nothing is written by a refused call
    a.free()
    b.free()


# ---- 4. SecondOrderFrames end to end ------------------------------------------------------------------------------------------
E2E_D = (1.0e-4, 1.2e-4)
E2E_TMAX = 1.03e-6
E2E_TIMES = E2E_TMAX * np.array([0.31, 0.05, 1.0, 0.0, 0.77, 0.12, 0.5, 0.93, 0.2, 0.68, 0.41, 0.86])   # unsorted, 0 among them
E2E_COEFF = 0.75
E2E_F = 5
RECORDS = ("p_raw", "p_max", "p_min", "p_rms", "p_final")


def e2e_p0(n, nf, seed):
    """every frame its own two Gaussian balls and 2 % noise"""
    rng = np.random.default_rng(seed)
    nx, ny = n
    y, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    out = np.empty((nf, ny, nx), F32)
    for f in range(nf):
        cx, cy, ax, ay = rng.uniform(0.25, 0.75, 4)
        out[f] = (np.exp(-((x - cx * nx) ** 2 + (y - cy * ny) ** 2) / 9.0) +
                  0.3 * np.exp(-((x - ax * nx) ** 2 + (y - ay * ny) ** 2) / 4.0) + 0.02 * rng.standard_normal((ny, nx)))
    return out


def e2e_sensors(n):
    """7 points of the plane, its corners among them"""
    nx, ny = n
    return np.array([0, nx - 1, nx * (ny - 1), nx * ny - 1, (ny // 2) * nx + nx // 2, 123, 3 * nx + 7], dtype=np.int64)


@pytest.mark.parametrize("n,fused,sides", [((24, 20), True, (48, 48)), ((23, 19), False, (39, 32))], ids=["fused", "rocfft"])
@pytest.mark.parametrize("coeff", [0.0, E2E_COEFF], ids=["lossless", "absorbing"])
def test_second_order_frames_against_the_restatement(second_order, coeff, n, fused, sides):
    """Measured: worst field(t) 1.8e-7 to 2.0e-7, field(0) 1.1e-7 to 1.2e-7, p_raw 1.2e-7 to 1.5e-7, p_final 1.5e-7 to 1.6e-7,
    p_rms 5.8e-8 to 8.6e-8."""
    sensors = e2e_sensors(n)
    kw = dict(alpha_coeff=coeff, alpha_power=1.5, t_max=E2E_TMAX, sensor_index=sensors, record=RECORDS, fused_kernels=fused)
    p = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    try:
        expanded = p.expanded
        assert expanded == sides == fr.default_sides(n, E2E_D, C0, E2E_TMAX, fused, LENGTHS)
        assert p.fused == fused and p.runs == 0 and p.shape == (E2E_F, n[1], n[0])
        assert coeff == 0.0 or fr.b_margins(expanded, E2E_D, C0, coeff, 1.5)[0] >= 0.25
        assert p.t_free == pytest.approx(min((e - m) * d for e, m, d in zip(expanded, n, E2E_D)) / C0, rel=1e-12)
        assert p.t_free >= E2E_TMAX
        p0 = e2e_p0(n, E2E_F, 1)
        p.set_p0(p0)
        want = fr.solve(p0, expanded, E2E_D, C0, E2E_TIMES, coeff, 1.5)
        # field(t), time by time; field(0) is p0 through the forward and inverse pipeline alone
        fields = np.array([p.field(t) for t in E2E_TIMES])
        assert fields.dtype == F32 and fields.shape == (12,) + p0.shape
        e_field = max(sr.rel_l2(fields[i], want[i]) for i in range(12))
        e_zero = sr.rel_l2(p.field(0.0), p0)
        # run(times): the record (n_times, F, n_sensor) and the aggregates
        rec = p.run(E2E_TIMES)
        assert rec.dtype == F32 and rec.shape == (12, E2E_F, 7) and p.runs == 1
        e_raw = sr.rel_l2(rec, want.reshape(12, E2E_F, -1)[:, :, sensors])
        assert np.array_equal(rec, fields.reshape(12, E2E_F, -1)[:, :, sensors])
        e_final = sr.rel_l2(p.p_final(), want[-1])
        e_rms = sr.rel_l2(p.p_rms(), np.sqrt(np.mean(want ** 2, axis=0)))
        print(f"SecondOrderFrames {n} x {E2E_F} alpha_coeff {coeff} fused {fused} E {expanded}: rel L2 worst field {e_field:.3e}, "
              f"field(0) {e_zero:.3e}, p_raw {e_raw:.3e}, p_final {e_final:.3e}, p_rms {e_rms:.3e}")
        assert max(e_field, e_raw, e_final, e_rms) < PARITY
        assert e_zero < 1e-6
        assert np.array_equal(p.p_max(), fields.max(axis=0)) and np.array_equal(p.p_min(), fields.min(axis=0))
        assert np.array_equal(p.p_final(), fields[-1])
        # the same p0 again gives identical bits
        p.set_p0(p0)
        assert np.array_equal(p.field(E2E_TIMES[2]), fields[2])
    finally:
        p.close()
    # a frame alone (frames = 1, a 2-D p0) gives the bits it has in the batch
    q = second_order.SecondOrderFrames(n, E2E_D, C0, 1, **kw)
    try:
        assert q.expanded == sides and q.fused == fused
        for f in (0, E2E_F - 1):
            q.set_p0(p0[f])
            assert np.array_equal(q.field(E2E_TIMES[2])[0], fields[2][f]), f
        assert np.array_equal(q.run(E2E_TIMES[:3])[:, 0], rec[:3, E2E_F - 1])
    finally:
        q.close()


@pytest.mark.parametrize("n,fused", [((24, 20), True), ((23, 19), False)], ids=["fused", "rocfft"])
def test_run_again_regrows_reuses_and_resets(second_order, n, fused):
    """run three times on one object: three times, five others (the record grows), the three again (the larger record is
    kept).  Every run's record and aggregates are those of its own times alone: the bits of field(t), p_rms within the
    parity bound of the float64 root mean square of those float32 fields."""
    sensors = e2e_sensors(n)
    t1, t2 = E2E_TIMES[[5, 3, 10]], E2E_TIMES[[2, 7, 0, 4, 9]]
    p = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, alpha_coeff=E2E_COEFF, alpha_power=1.5, t_max=E2E_TMAX,
                                       sensor_index=sensors, record=RECORDS, fused_kernels=fused)
    try:
        assert p.fused == fused
        p.set_p0(e2e_p0(n, E2E_F, 5))
        fields = np.array([p.field(t) for t in t2])
        first = p.run(t1)
        assert first.shape == (3, E2E_F, 7)
        rec = p.run(t2)
        assert rec.shape == (5, E2E_F, 7) and np.array_equal(rec, fields.reshape(5, E2E_F, -1)[:, :, sensors])
        assert np.array_equal(p.p_max(), fields.max(axis=0)) and np.array_equal(p.p_min(), fields.min(axis=0))
        assert np.array_equal(p.p_final(), fields[-1])
        e_rms = sr.rel_l2(p.p_rms(), np.sqrt(np.mean(fields.astype(np.float64) ** 2, axis=0)))
        print(f"SecondOrderFrames {n} x {E2E_F} fused {fused}: p_rms of a second run against its own fields {e_rms:.3e}")
        assert e_rms < PARITY
        again = p.run(t1)
        assert again.shape == (3, E2E_F, 7) and np.array_equal(again, first)
        p_max = p.p_max()
        assert np.array_equal(p_max, np.array([p.field(t) for t in t1]).max(axis=0))
        assert p.runs == 3
    finally:
        p.close()


def test_two_interleaved_propagators_do_not_disturb_each_other(second_order):
    n = (24, 20)
    pa, pb = e2e_p0(n, E2E_F, 2), e2e_p0(n, E2E_F, 3)
    t = E2E_TIMES[:4]
    kw = dict(alpha_coeff=E2E_COEFF, t_max=E2E_TMAX)
    alone = []
    for p0 in (pa, pb):
        q = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
        try:
            q.set_p0(p0)
            alone.append([q.field(x) for x in t])
        finally:
            q.close()
    a = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    b = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    try:
        a.set_p0(pa)
        b.set_p0(pb)
        for i, x in enumerate(t):
            fa = a.field(x)
            fb = b.field(x)
            assert np.array_equal(fa, alone[0][i]) and np.array_equal(fb, alone[1][i])
    finally:
        a.close()
        b.close()


def test_times_and_shapes_are_checked(second_order):
    from kwave_amd import capi
    p = second_order.SecondOrderFrames((24, 20), E2E_D, C0, 2, t_max=E2E_TMAX)
    try:
        with pytest.raises(capi.KWaveError, match="field: no p0 yet"):
            p.field(1e-7)
        with pytest.raises(ValueError, match=r"p0 must be \(F, Ny, Nx\) = \(2, 20, 24\)"):
            p.set_p0(np.zeros((20, 24), F32))   # a plane alone is a batch only when frames == 1
        p.set_p0(e2e_p0((24, 20), 2, 4))
        with pytest.raises(capi.KWaveError, match=r"t: -0.000001 is not a time >= 0"):
            p.field(-1e-6)
        with pytest.raises(capi.KWaveError, match=r"n_times: 0 is not a number of output times"):
            p.run([])
        with pytest.raises(capi.KWaveError, match=r"p_max: no run yet"):
            p.p_max()
        assert p.run([1e-7]).shape == (1, 2, 0)
        with pytest.raises(capi.KWaveError, match=r"p_max: not recorded"):
            p.p_max()
    finally:
        p.close()


# ---- 5. next to the 3-D class ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coeff", [0.0, E2E_COEFF], ids=["lossless", "absorbing"])
def test_a_plane_next_to_the_three_d_class_on_a_field_constant_along_z(second_order, coeff):
    """SecondOrder(n = (24, 20, 16), expanded = (48, 48, 16)): z is periodic with nothing along it, so a p0 held constant
    along z stays the 2-D solution on every plane (tests/test_second_order_frames_host.py shows the two float64
    restatements agree to 1e-12); both GPU results are within 1e-5 of that field, hence within 2e-5 of each other.
    Measured: SecondOrder 1.4e-7 to 2.0e-7, SecondOrderFrames 1.5e-7 to 1.9e-7, one against the other 1.0e-7 to 1.3e-7."""
    n, e, d3 = (24, 20), (48, 48), E2E_D + (0.9e-4,)
    plane = e2e_p0(n, 1, 5)[0]
    t = E2E_TIMES[[2, 4]]
    a = second_order.SecondOrder(n + (16,), d3, C0, alpha_coeff=coeff, expanded=e + (16,))
    try:
        assert a.fused
        a.set_p0(np.broadcast_to(plane, (16,) + plane.shape))
        three = [a.field(x) for x in t]
    finally:
        a.close()
    b = second_order.SecondOrderFrames(n, E2E_D, C0, 1, alpha_coeff=coeff, expanded=e)
    try:
        assert b.fused
        b.set_p0(plane)
        two = [b.field(x)[0] for x in t]
    finally:
        b.close()
    for x, v3, v2 in zip(t, three, two):
        want = fr.solve(plane[None], e, E2E_D, C0, [x], coeff, 1.5)[0, 0]
        e3, e2 = max(sr.rel_l2(v3[z], want) for z in range(16)), sr.rel_l2(v2, want)
        eb = max(sr.rel_l2(v3[z], v2) for z in range(16))
        print(f"a plane at t = {x:.3e}, alpha_coeff {coeff}: SecondOrder {e3:.3e}, SecondOrderFrames {e2:.3e} (rel L2 against "
              f"float64), one against the other {eb:.3e}")
        assert e3 < PARITY and e2 < PARITY and eb < 2 * PARITY


# ---- 6. the wrap-around rule ------------------------------------------------------------------------------------------------
def test_field_inside_the_domain_is_free_of_wrap_around_up_to_t_free(second_order):
    """three Gaussian discs in (16, 16) domains, c0 t_max = 5.5 points: the default sides (32, 32), t_free = 16 points,
    against sides twice as large, at t_free of the smaller plane.  The discs' band limit makes the two float64 fields differ
    a little: that difference is computed and added.  Measured: 1.159e-3 on the GPU, 1.159e-3 in float64 (in 2-D a disc's
    wave has a tail, and at t_free of the smaller plane its images have just reached the domain's edge)."""
    n, d = (16, 16), (1.0e-4, 1.0e-4)
    t_max = 5.5 * d[0] / C0
    y, x = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    p0 = np.array([np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / 6.0) for cx, cy in ((7.5, 8.0), (5.0, 9.5), (10.0, 6.0))]).astype(F32)
    got = []
    a = second_order.SecondOrderFrames(n, d, C0, 3, t_max=t_max)
    try:
        t = a.t_free
        assert a.expanded == (32, 32) and a.fused and t == pytest.approx(16 * d[0] / C0) and t >= t_max
        a.set_p0(p0)
        got.append(a.field(t))
    finally:
        a.close()
    b = second_order.SecondOrderFrames(n, d, C0, 3, expanded=(64, 64))
    try:
        assert b.fused and b.t_free == pytest.approx(48 * d[0] / C0)
        b.set_p0(p0)
        got.append(b.field(t))
    finally:
        b.close()
    ref = [fr.solve(p0, (e, e), d, C0, [t])[0] for e in (32, 64)]
    own = sr.rel_l2(ref[0], ref[1])
    err = sr.rel_l2(got[0], got[1])
    print(f"frames wrap-around at t_free: E = 32 against E = 64 on the GPU {err:.3e}; the restatement's own difference {own:.3e}")
    assert err <= 2e-5 + own
