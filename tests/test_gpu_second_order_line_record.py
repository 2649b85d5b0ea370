"""Line-sensor record of the batched 2-D exact k-space propagator on the GPU: kw_second_order_line_prepare and
kw_second_order_line_record through the C ABI with the x-inverse done in float64 on the host, then
kwave_amd.second_order.SecondOrderFrames.line_record: the time 0, the bits of a value under everything they must not depend
on, end to end against the float64 restatement of tests/second_order_line_record_reference.py and against the device's own
run(times), through recon.LineRecon, and the refusals.

Bounds.
  stages, line_record      1e-5 relative L2, the project's parity bound, against float64 of the same float32 inputs.  The
                           absorbing variants assert first that B >= 1/4 on every bin of their grid, and every stage case that
                           the expected result has not vanished — conditions on the inputs.
  line_record against run(times), LineRecon of the two records   2e-5: two results within 1e-5 of the same float64 values.
  t = 0                    1e-6: H = 1, the transforms and the sum alone (the bound of field(0)).
  a frame alone or in a batch, a time alone or in a list, the chunks of times, the order of the times, a second set_p0,
  interleaved propagators, interleaved field and run   exact.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import second_order_frames_reference as fr  # noqa: E402
import second_order_line_record_reference as lr  # noqa: E402
import second_order_reference as sr  # noqa: E402
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
PARITY = 1e-5
C0 = 1500.0
ENTRIES = ("kw_second_order_line_elems", "kw_second_order_line_prepare", "kw_second_order_line_record")
FRAME_TILE, TIME_TILE = 64, 256   # k_line_record's largest frame tile and its time tile


@pytest.fixture(scope="module")
def second_order():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, second_order
    for name in ENTRIES:
        assert name in capi._SIG
    assert hasattr(second_order.SecondOrderFrames, "line_record")
    return second_order


@pytest.fixture()
def dev(second_order):
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def make_op(d, c0, coeff, y):
    """kw_second_order_op of a plane; t is NaN and dz is 0: the record looks at neither"""
    from kwave_amd import capi
    op = capi.SecondOrderOp()
    op.dx, op.dy, op.dz, op.c0, op.t = d[0], d[1], 0.0, c0, float("nan")
    op.a, op.alpha_power = sr.neper(coeff, y), y
    op.absorbing = int(coeff > 0.0)
    return op


# ---- 1. the stages through the C ABI ------------------------------------------------------------------------------------------
class Stage:
    """a context of (ex, ey, F) with the natural spectra of a batch; record(row, op, times) -> G [F][n_times][Ex/2 + 1]"""

    def __init__(self, dev, vol):
        nf, ey, ex = vol.shape
        self.dev, self.shape = dev, vol.shape
        self.nxc, self.mf = ex // 2 + 1, ey // 2 + 1
        set_constants(dev, ex, ey, nf)
        dev.call("fft_create_plans_frames")
        src = Guarded(dev, vol)
        self.spec = Guarded(dev, np.zeros(2 * self.nxc * ey * nf, F32))
        dev.call("fft_r2c_frames", src.ptr, self.spec.ptr)
        dev.sync()
        src.free()
        self.spec_bytes = self.spec.read().view(np.uint8)
        n = C.c_size_t()
        dev.call("second_order_line_elems", C.byref(n))
        assert n.value == self.nxc * self.mf * nf
        self.q = Guarded(dev, np.full(2 * n.value, np.nan, F32))

    def record(self, row, op, times):
        nf = self.shape[0]
        times = np.ascontiguousarray(times, dtype=np.float64)
        self.dev.call("second_order_line_prepare", self.q.ptr, self.spec.ptr, row)
        t = Guarded(self.dev, times, dtype=np.float64)
        g = Guarded(self.dev, np.full((nf, times.size, self.nxc, 2), np.nan, F32))
        self.dev.call("second_order_line_record", g.ptr, self.q.ptr, C.byref(op), t.ptr, times.size)
        self.dev.sync()
        out = g.read()   # (the guard bands: nothing is stored outside G)
        assert np.array_equal(t.read(), times)
        self.q.read()    # (nor outside Q)
        t.free()
        g.free()
        assert np.isfinite(out).all()
        return out[..., 0].astype(np.float64) + 1j * out[..., 1].astype(np.float64)

    def close(self):
        assert np.array_equal(self.spec.read().view(np.uint8), self.spec_bytes)   # the spectra are read only
        self.spec.free()
        self.q.free()


def stage_errors(dev, ex, ey, nf, rows, groups, d, seed=0):
    """groups: (alpha_coeff, y, times); returns the relative L2 of the rows [F][n_times][Ex] per row and group"""
    vol = lr.source_frames(np.random.default_rng(ex * 1009 + ey * 31 + nf + seed), nf, ey, ex)
    s = Stage(dev, vol)
    errs = []
    for row in rows:
        for coeff, y, times in groups:
            got = lr.rows_of(s.record(row, make_op(d, sr.STAGE_C0, coeff, y), times), ex)
            want = lr.record_expanded(vol, d, sr.STAGE_C0, times, row, coeff, y)
            for i in range(len(times)):
                assert np.linalg.norm(want[:, i]) > 1e-3 * np.linalg.norm(vol[:, row])   # the result has not vanished
            errs.append(max(sr.rel_l2(got[:, i], want[:, i]) for i in range(len(times))))
    s.close()
    return errs


def stage_groups(ex, ey):
    """the four stage_case variants as two calls: lossless near and far, absorbing near and far"""
    cases = fr.stage_case((ex, ey))
    assert fr.b_margins((ex, ey), sr.STAGE_D[:2], sr.STAGE_C0, cases[3][0], sr.STAGE_Y)[0] >= 0.25
    return [(0.0, sr.STAGE_Y, [cases[0][1], cases[1][1]]), (cases[2][0], sr.STAGE_Y, [cases[2][1], cases[3][1]])]


@pytest.mark.parametrize("ex,ey,nf", [(16, 1024, 3), (16, 17, 2), (33, 27, 4), (1024, 16, 2)])
def test_prepare_and_record_against_float64(dev, ex, ey, nf):
    """(16, 1024, 3): 513 folded bins in nine chunks, the last of one bin; (16, 17, 2) and (33, 27, 4): odd sides, no
    Nyquist bin along y (every bin above 0 has a partner) or along x; (1024, 16, 2): 513 kx columns, whose last tile of the
    transposition holds one.  Rows 0, Ey - 1 and Ey/2, lossless and absorbing (y = 1.5), near (c0 t = 0.37 of the smallest
    spacing) and at 10^4 turns of the largest |k|; spacings STAGE_D[:2].  The worst of each call's two times is held.
    Measured: (16, 1024, 3) 4.3e-7 to 8.2e-7, (16, 17, 2) 5.0e-8 to 1.2e-7, (33, 27, 4) 1.3e-7 to 1.9e-7, (1024, 16, 2) 9.9e-8 to
    2.0e-7."""
    # sr.stage_case is written for the even grids of the fused stage; its numbers are as good on odd ones
    errs = stage_errors(dev, ex, ey, nf, (0, ey - 1, ey // 2), stage_groups(ex, ey), sr.STAGE_D[:2])
    print(f"line record stage {ex}x{ey}x{nf}: rel L2 per row (0, Ey - 1, Ey/2) and (lossless, absorbing): " +
          " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) < PARITY, (ex, ey, nf)


def test_record_with_a_partly_filled_frame_tile_and_time_tile(dev):
    """(Ex, Ey, F) = (16, 32, 65) and 257 times: F and n_times one more than the frame tile of 64 and the time tile of 256 —
    a second frame tile with one live frame, a second time tile with one live thread.  Measured: lossless 1.7e-7, absorbing
    6.2e-8."""
    ex, ey, nf = 16, 32, FRAME_TILE + 1
    near, far = fr.stage_case((ex, ey))[0][1], fr.stage_case((ex, ey))[1][1]
    times = np.random.default_rng(7).uniform(near, far, TIME_TILE + 1)
    times[[0, -1]] = near, far
    coeff = fr.stage_case((ex, ey))[3][0]
    errs = stage_errors(dev, ex, ey, nf, (5,), [(0.0, sr.STAGE_Y, times), (coeff, sr.STAGE_Y, times[-3:])], sr.STAGE_D[:2])
    print(f"line record stage {ex}x{ey}x{nf}, {times.size} times: lossless {errs[0]:.3e}, absorbing {errs[1]:.3e}")
    assert max(errs) < PARITY


def test_record_with_the_stokes_and_the_general_power(dev):
    """y = 2 (|k| itself) and y = 1.1 (the float64 power function) on (33, 27, 4); dy = 0.8 dx, c0 t = 37.3 dy.  Measured: 8.1e-8 to
    2.0e-7."""
    d, t = (1.0e-4, 0.8e-4), 37.3 * 0.8e-4 / C0
    groups = [(0.2, 2.0, [t]), (0.75, 1.1, [t, 0.0])]
    for coeff, y, _ in groups:
        assert fr.b_margins((33, 27), d, C0, coeff, y)[0] >= 0.25
    errs = stage_errors(dev, 33, 27, 4, (0, 26, 13), groups, d, seed=1)
    print("line record stage 33x27x4, y = 2 and y = 1.1 per row: " + " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) < PARITY


def test_entries_refuse_bad_arguments(dev):
    from kwave_amd import capi
    a = Guarded(dev, np.zeros(4096, F32))
    b = Guarded(dev, np.zeros(4096, F32))
    t = Guarded(dev, np.zeros(4), dtype=np.float64)
    op = make_op((1e-4, 1e-4), C0, 0.0, 1.5)
    with pytest.raises(capi.KWaveError, match="kw_set_constants has not been called"):
        dev.call("second_order_line_prepare", a.ptr, b.ptr, 0)
    set_constants(dev, 16, 16, 2)
    with pytest.raises(capi.KWaveError, match="kw_second_order_line_prepare"):
        dev.call("second_order_line_prepare", a.ptr, b.ptr, 16)   # a row outside the plane
    with pytest.raises(capi.KWaveError, match="kw_second_order_line_record"):
        dev.call("second_order_line_record", a.ptr, b.ptr, C.byref(op), t.ptr, 0)
    with pytest.raises(capi.KWaveError, match="kw_second_order_line_record"):
        dev.call("second_order_line_record", a.ptr, b.ptr, C.byref(make_op((0.0, 1e-4), C0, 0.0, 1.5)), t.ptr, 4)
    dev.sync()
    assert not a.read().any() and not b.read().any()   # nothing is written by a refused call
    for g in (a, b, t):
        g.free()


# ---- 2. SecondOrderFrames.line_record ---------------------------------------------------------------------------------------
E2E_D = (1.0e-4, 1.2e-4)
E2E_TMAX = 1.03e-6
E2E_TIMES = E2E_TMAX * np.array([0.31, 0.05, 1.0, 0.0, 0.77, 0.12, 0.5, 0.93, 0.2, 0.68, 0.41, 0.86])   # unsorted, 0 among them
E2E_COEFF = 0.75
E2E_F = 5
N = (24, 20)


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


@pytest.mark.parametrize("n,fused,sides", [((24, 20), True, (48, 48)), ((23, 19), False, (39, 32))], ids=["fused", "rocfft"])
@pytest.mark.parametrize("coeff", [0.0, E2E_COEFF], ids=["lossless", "absorbing"])
@pytest.mark.parametrize("row", [0, 7])
def test_line_record_against_the_restatement_and_against_run(second_order, row, coeff, n, fused, sides):
    """F = 5, 12 unsorted times.  On the fused context the record takes its (kx, ky) spectra from a batched 2-D transform of
    its own; on the rocFFT context from the kept ones.  Measured: against float64 1.4e-7 to 1.7e-7, against run(times) 1.3e-7 to
    2.1e-7, t = 0 against the row of p0 1.1e-7 to 3.1e-7."""
    sensors = row * n[0] + np.arange(n[0])
    p = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, alpha_coeff=coeff, t_max=E2E_TMAX, sensor_index=sensors,
                                       fused_kernels=fused, line_row=row)
    try:
        assert p.expanded == sides and p.fused == fused and p.line_row == row
        assert coeff == 0.0 or fr.b_margins(sides, E2E_D, C0, coeff, 1.5)[0] >= 0.25
        p0 = e2e_p0(n, E2E_F, 1)
        p.set_p0(p0)
        rec = p.line_record(E2E_TIMES)
        assert rec.dtype == F32 and rec.shape == (E2E_F, 12, n[0])
        want = lr.record(p0, sides, E2E_D, C0, E2E_TIMES, row, coeff, 1.5)
        e_rec = sr.rel_l2(rec, want)
        raw = p.run(E2E_TIMES)   # (n_times, F, Nx)
        e_run = sr.rel_l2(rec, raw.transpose(1, 0, 2))
        e_zero = sr.rel_l2(rec[:, 3], p0[:, row, :])
        print(f"line_record {n} x {E2E_F} row {row} alpha_coeff {coeff} fused {fused}: rel L2 against float64 {e_rec:.3e}, "
              f"against run(times) {e_run:.3e}, t = 0 against p0 {e_zero:.3e}")
        assert e_rec < PARITY and e_run < 2 * PARITY and e_zero < 1e-6
        assert np.array_equal(p.line_record(E2E_TIMES), rec)   # run(times) in between has changed nothing
    finally:
        p.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
def test_time_zero_returns_the_row_of_p0(second_order, fused):
    for row in (0, N[1] - 1):
        p = second_order.SecondOrderFrames(N, E2E_D, C0, E2E_F, alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, fused_kernels=fused,
                                           line_row=row)
        try:
            p0 = e2e_p0(N, E2E_F, 6)
            p.set_p0(p0)
            err = sr.rel_l2(p.line_record([0.0])[:, 0], p0[:, row, :])
            print(f"line_record at t = 0, row {row}, fused {fused}: {err:.3e}")
            assert err < 1e-6
        finally:
            p.close()


@pytest.fixture(scope="module")
def batch_record(second_order):
    """the record of F = 5 frames, row 7, absorbing, on the fused context: what the bit-for-bit tests compare with"""
    p0 = e2e_p0(N, E2E_F, 1)
    p = second_order.SecondOrderFrames(N, E2E_D, C0, E2E_F, alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, line_row=7)
    try:
        p.set_p0(p0)
        return p0, p.line_record(E2E_TIMES)
    finally:
        p.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
def test_a_frame_alone_has_the_bits_it_has_in_the_batch(second_order, fused):
    kw = dict(alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, line_row=7, fused_kernels=fused, expanded=(48, 48))
    p0 = e2e_p0(N, E2E_F, 1)
    p = second_order.SecondOrderFrames(N, E2E_D, C0, E2E_F, **kw)
    q = second_order.SecondOrderFrames(N, E2E_D, C0, 1, **kw)
    try:
        p.set_p0(p0)
        rec = p.line_record(E2E_TIMES)
        for f in (0, E2E_F - 1):
            q.set_p0(p0[f])
            assert np.array_equal(q.line_record(E2E_TIMES)[0], rec[f]), f
    finally:
        p.close()
        q.close()


def test_a_time_has_its_bits_alone_in_a_list_and_under_every_chunking(second_order, batch_record):
    p0, rec = batch_record
    p = second_order.SecondOrderFrames(N, E2E_D, C0, E2E_F, alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, line_row=7)
    try:
        p.set_p0(p0)
        default = p.line_chunk_times
        assert default == (256 << 20) // (25 * E2E_F * 8)
        for i in (0, 3, 11):
            assert np.array_equal(p.line_record([E2E_TIMES[i]])[:, 0], rec[:, i]), i
        for chunk in (5, 1):   # passes of 5, 5, 2 times and of one time each
            p.line_chunk_times = chunk
            assert p.line_chunk_times == chunk
            assert np.array_equal(p.line_record(E2E_TIMES), rec), chunk
        p.line_chunk_times = None
        assert p.line_chunk_times == default
        # sorted and shuffled, row for row
        order = np.argsort(E2E_TIMES)
        assert np.array_equal(p.line_record(E2E_TIMES[order]), rec[:, order])
        shuffled = np.random.default_rng(3).permutation(12)
        assert np.array_equal(p.line_record(E2E_TIMES[shuffled]), rec[:, shuffled])
    finally:
        p.close()


def test_a_second_set_p0_and_interleaved_propagators(second_order, batch_record):
    pa, rec_a = batch_record
    pb = e2e_p0(N, E2E_F, 3)
    kw = dict(alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, line_row=7)
    a = second_order.SecondOrderFrames(N, E2E_D, C0, E2E_F, **kw)
    b = second_order.SecondOrderFrames(N, E2E_D, C0, E2E_F, **kw)
    try:
        b.set_p0(pb)
        rec_b = b.line_record(E2E_TIMES)
        assert not np.array_equal(rec_b, rec_a)
        a.set_p0(pb)
        a.set_p0(pa)   # a second set_p0 replaces the first
        for lo in (0, 4, 8):
            ra = a.line_record(E2E_TIMES[lo:lo + 4])
            rb = b.line_record(E2E_TIMES[lo:lo + 4])
            assert np.array_equal(ra, rec_a[:, lo:lo + 4]) and np.array_equal(rb, rec_b[:, lo:lo + 4])
        b.set_p0(pa)
        assert np.array_equal(b.line_record(E2E_TIMES), rec_a)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
def test_field_run_and_line_record_may_be_interleaved(second_order, fused):
    """the record neither reads nor writes the field state, the aggregates or the record of run"""
    sensors = np.array([0, 23, 7 * 24 + 5])
    kw = dict(alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, sensor_index=sensors, record=("p_raw", "p_max", "p_final"),
              fused_kernels=fused, expanded=(48, 48))
    p0 = e2e_p0(N, E2E_F, 8)
    plain = second_order.SecondOrderFrames(N, E2E_D, C0, E2E_F, **kw)   # no line row: the class as it was
    try:
        plain.set_p0(p0)
        field = plain.field(E2E_TIMES[2])
        raw = plain.run(E2E_TIMES[:5])
        p_max, p_final = plain.p_max(), plain.p_final()
    finally:
        plain.close()
    p = second_order.SecondOrderFrames(N, E2E_D, C0, E2E_F, line_row=7, **kw)
    try:
        p.set_p0(p0)
        rec = p.line_record(E2E_TIMES)
        assert np.array_equal(p.field(E2E_TIMES[2]), field)
        assert np.array_equal(p.line_record(E2E_TIMES), rec)
        assert np.array_equal(p.run(E2E_TIMES[:5]), raw)
        assert np.array_equal(p.line_record(E2E_TIMES), rec)
        assert np.array_equal(p.p_max(), p_max) and np.array_equal(p.p_final(), p_final) and p.runs == 1
        assert np.array_equal(p._get("p", p.shape), p_final)   # the last field computed is run's, not the record's
    finally:
        p.close()


# ---- 3. with LineRecon ------------------------------------------------------------------------------------------------------
def test_the_record_is_line_recon_s_input(second_order):
    """row 0 at t_n = n dt into LineRecon(ny = Nx, dy = dx, the same c0 and dt), order "ty": the image of the device's
    record against the image of the float64 record rounded to float32 — the layout (F, Nt, Nx) and the time convention of
    the two classes, not how well the image recovers p0.  Measured: 2.6e-7."""
    from kwave_amd import recon
    nt, dt = 48, E2E_D[0] / C0
    times = dt * np.arange(nt)
    p0 = e2e_p0(N, E2E_F, 9)
    p = second_order.SecondOrderFrames(N, E2E_D, C0, E2E_F, t_max=nt * dt, line_row=0)
    try:
        sides = p.expanded
        p.set_p0(p0)
        rec = p.line_record(times)
    finally:
        p.close()
    want = lr.record(p0, sides, E2E_D, C0, times, 0).astype(F32)
    assert sr.rel_l2(rec, want) < PARITY
    r = recon.LineRecon(N[0], E2E_D[0], dt, nt, C0, frames=E2E_F)
    try:
        got, ref = r.run(rec), r.run(want)
    finally:
        r.close()
    err = sr.rel_l2(got, ref)
    print(f"LineRecon of line_record against LineRecon of the float64 record: {err:.3e}")
    assert np.linalg.norm(ref) > 0 and err < 2 * PARITY


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_line_record_refusals(second_order):
    from kwave_amd import capi
    with pytest.raises(capi.KWaveError, match=r"line_row: 20 is outside the plane's rows 0 ... 19"):
        second_order.SecondOrderFrames(N, E2E_D, C0, 2, t_max=E2E_TMAX, line_row=20)
    p = second_order.SecondOrderFrames(N, E2E_D, C0, 2, t_max=E2E_TMAX)
    try:
        assert p.line_row is None
        p.set_p0(e2e_p0(N, 2, 4))
        with pytest.raises(capi.KWaveError, match="line_record: no line row set"):
            p.line_record([1e-7])
        with pytest.raises(capi.KWaveError, match=r"line_row: -2 is outside"):
            p.line_row = -2
        p.line_row = 3
        assert p.line_row == 3
        with pytest.raises(capi.KWaveError, match="line_record: no p0 since the line row was set"):
            p.line_record([1e-7])
        p.set_p0(e2e_p0(N, 2, 4))
        with pytest.raises(capi.KWaveError, match=r"n_times: 0 is not a number of output times"):
            p.line_record([])
        with pytest.raises(capi.KWaveError, match=r"t: -0.000001 is not a time >= 0"):
            p.line_record([1e-7, -1e-6])
        with pytest.raises(capi.KWaveError, match=r"t: nan is not a time >= 0"):
            p.line_record([float("nan")])
        with pytest.raises(capi.KWaveError, match=r"line_chunk_times: "):
            p.line_chunk_times = 1 << 40
        first = p.line_record([1e-7, 3e-7])
        assert first.shape == (2, 2, 24)
        p.line_row = 5                      # another row: the old Q is not used
        with pytest.raises(capi.KWaveError, match="line_record: no p0 since the line row was set"):
            p.line_record([1e-7])
        p.line_row = None                   # off: the arrays are freed
        with pytest.raises(capi.KWaveError, match="line_record: no line row set"):
            p.line_record([1e-7])
        p.line_row = 3
        p.set_p0(e2e_p0(N, 2, 4))
        assert np.array_equal(p.line_record([1e-7, 3e-7]), first)
    finally:
        p.close()
