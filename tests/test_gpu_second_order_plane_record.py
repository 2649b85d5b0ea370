"""Plane-sensor record of the 3-D exact k-space propagator on the GPU: kw_second_order_plane_prepare and
kw_second_order_plane_record through the C ABI with the 2-D inverse done in float64 on the host, then
kwave_amd.second_order.SecondOrder.plane_record: the time 0, the bits of a value under everything they must not depend on,
end to end against the float64 restatement of tests/second_order_plane_record_reference.py and against the device's own
run(times), through recon.PlaneRecon, and the refusals.

Bounds.
  stages, plane_record     1e-5 relative L2, the project's parity bound, against float64 of the same float32 inputs.  The
                           absorbing variants assert first that B >= 1/4 on every bin of their grid, and every stage case that
                           the expected result has not vanished — conditions on the inputs.
  plane_record against run(times), PlaneRecon of the two records   2e-5: two results within 1e-5 of the same float64 values.
  t = 0                    1e-6: H = 1, the transforms and the sum alone (the bound of field(0)).
  a time alone or in a list, the passes, the order of the times, a second set_p0, interleaved propagators, interleaved
  field and run   exact.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import second_order_plane_record_reference as pr  # noqa: E402
import second_order_reference as sr  # noqa: E402
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
PARITY = 1e-5
C0 = 1500.0
ENTRIES = ("kw_second_order_plane_elems", "kw_second_order_plane_prepare", "kw_second_order_plane_record")
TIME_TILE = 256   # k_plane_record's time tile


@pytest.fixture(scope="module")
def second_order():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, second_order
    for name in ENTRIES:
        assert name in capi._SIG
    assert hasattr(second_order.SecondOrder, "plane_record")
    return second_order


@pytest.fixture()
def dev(second_order):
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def make_op(d, c0, coeff, y):
    """kw_second_order_op of a volume; t is NaN: the record does not look at it"""
    from kwave_amd import capi
    op = capi.SecondOrderOp()
    op.dx, op.dy, op.dz, op.c0, op.t = d[0], d[1], d[2], c0, float("nan")
    op.a, op.alpha_power = sr.neper(coeff, y), y
    op.absorbing = int(coeff > 0.0)
    return op


# ---- 1. the stages through the C ABI ------------------------------------------------------------------------------------------
class Stage:
    """a context of (ex, ey, ez) with the natural spectrum of a volume; record(plane, op, times) -> G [n_times][Ey][Ex/2 + 1]"""

    def __init__(self, dev, vol):
        ez, ey, ex = vol.shape
        self.dev, self.shape = dev, vol.shape
        self.nxc, self.mf = ex // 2 + 1, ez // 2 + 1
        set_constants(dev, ex, ey, ez)
        dev.call("fft_create_plans_3d")
        src = Guarded(dev, vol)
        self.spec = Guarded(dev, np.zeros(2 * self.nxc * ey * ez, F32))
        dev.call("fft_r2c_3d", src.ptr, self.spec.ptr)
        dev.sync()
        src.free()
        self.spec_bytes = self.spec.read().view(np.uint8)
        n = C.c_size_t()
        dev.call("second_order_plane_elems", C.byref(n))
        assert n.value == ey * self.nxc * self.mf
        self.q = Guarded(dev, np.full(2 * n.value, np.nan, F32))

    def record(self, plane, op, times):
        ez, ey, ex = self.shape
        times = np.ascontiguousarray(times, dtype=np.float64)
        self.dev.call("second_order_plane_prepare", self.q.ptr, self.spec.ptr, plane)
        t = Guarded(self.dev, times, dtype=np.float64)
        g = Guarded(self.dev, np.full((times.size, ey, self.nxc, 2), np.nan, F32))
        self.dev.call("second_order_plane_record", g.ptr, self.q.ptr, C.byref(op), t.ptr, times.size)
        self.dev.sync()
        out = g.read()   # (the guard bands: nothing is stored outside G)
        assert np.array_equal(t.read(), times)
        self.q.read()    # (nor outside Q)
        t.free()
        g.free()
        assert np.isfinite(out).all()   # every value of G has been written
        return out[..., 0].astype(np.float64) + 1j * out[..., 1].astype(np.float64)

    def close(self):
        assert np.array_equal(self.spec.read().view(np.uint8), self.spec_bytes)   # the spectrum is read only
        self.spec.free()
        self.q.free()


def stage_errors(dev, ex, ey, ez, planes, groups, d, seed=0):
    """groups: (alpha_coeff, y, times); returns the worst relative L2 over the times of the planes [Ey][Ex] per plane and group"""
    vol = pr.source_volume(np.random.default_rng(ex * 1009 + ey * 31 + ez + seed), ex, ey, ez)
    s = Stage(dev, vol)
    errs = []
    for plane in planes:
        Q = pr.folded_q(vol, plane)
        for coeff, y, times in groups:
            got = pr.planes_of(s.record(plane, make_op(d, sr.STAGE_C0, coeff, y), times), ex)
            want = pr.planes_of(pr.spectrum(Q, (ex, ey, ez), d, sr.STAGE_C0, times, coeff, y), ex)
            for i in range(len(times)):
                assert np.linalg.norm(want[i]) > 1e-3 * np.linalg.norm(vol[plane])   # the result has not vanished
            errs.append(max(sr.rel_l2(got[i], want[i]) for i in range(len(times))))
    s.close()
    return errs


def stage_groups(expanded):
    """the four stage_case variants as two calls: lossless near and far, absorbing near and far"""
    cases = sr.stage_case(expanded)
    assert sr.b_margins(expanded, sr.STAGE_D, sr.STAGE_C0, cases[3][0], sr.STAGE_Y)[0] >= 0.25
    return [(0.0, sr.STAGE_Y, [cases[0][1], cases[1][1]]), (cases[2][0], sr.STAGE_Y, [cases[2][1], cases[3][1]])]


@pytest.mark.parametrize("ex,ey,ez", [(16, 16, 1024), (16, 17, 18), (33, 27, 21), (1024, 16, 16), (16, 1024, 16)])
def test_prepare_and_record_against_float64(dev, ex, ey, ez):
    """(16, 16, 1024): 513 folded bins in nine chunks, the last of one bin, kx tiles of 4, 4 and 1 columns; (16, 17, 18): odd
    Ey, no self-paired Nyquist row (every row above 0 has a partner); (33, 27, 21): all odd; (1024, 16, 16): 513 kx columns;
    (16, 1024, 16): 513 ky pairs.  Planes 0, Ez - 1 and Ez/2, lossless and absorbing (y = 1.5), near (c0 t = 0.37 of the
    smallest spacing) and at 10^4 turns of the largest |k|; spacings STAGE_D.  The worst of each call's two times is held.
    Measured: (16, 16, 1024) 4.1e-7 to 1.1e-6, (16, 17, 18) 1.7e-7 to 3.2e-7, (33, 27, 21) 1.1e-7 to 1.7e-7, (1024, 16, 16) 6.8e-8
    to 2.0e-7, (16, 1024, 16) 5.9e-8 to 1.3e-7."""
    # sr.stage_case is written for the even grids of the fused stage; its numbers are as good on odd ones
    errs = stage_errors(dev, ex, ey, ez, (0, ez - 1, ez // 2), stage_groups((ex, ey, ez)), sr.STAGE_D)
    print(f"plane record stage {ex}x{ey}x{ez}: rel L2 per plane (0, Ez - 1, Ez/2) and (lossless, absorbing): " +
          " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) < PARITY, (ex, ey, ez)


def test_record_with_a_partly_filled_time_tile(dev):
    """(Ex, Ey, Ez) = (16, 16, 32) and 257 times: one more than the time tile of 256 — a second time tile with one live
    thread.  Measured: lossless 2.7e-7, absorbing 4.9e-8."""
    e = (16, 16, 32)
    cases = sr.stage_case(e)
    near, far = cases[0][1], cases[1][1]
    times = np.random.default_rng(7).uniform(near, far, TIME_TILE + 1)
    times[[0, -1]] = near, far
    errs = stage_errors(dev, *e, (5,), [(0.0, sr.STAGE_Y, times), (cases[3][0], sr.STAGE_Y, times[-3:])], sr.STAGE_D)
    print(f"plane record stage {e}, {times.size} times: lossless {errs[0]:.3e}, absorbing {errs[1]:.3e}")
    assert max(errs) < PARITY


def test_record_with_the_stokes_and_the_general_power(dev):
    """y = 2 (|k| itself) and y = 1.1 (the float64 power function) on the odd box (33, 27, 21); c0 t = 37.3 dy.  Measured: 1.2e-7
    to 2.8e-7."""
    d, t = sr.STAGE_D, 37.3 * 0.8e-4 / C0
    groups = [(0.2, 2.0, [t]), (0.75, 1.1, [t, 0.0])]
    for coeff, y, _ in groups:
        assert sr.b_margins((33, 27, 21), d, C0, coeff, y)[0] >= 0.25
    errs = stage_errors(dev, 33, 27, 21, (0, 20, 10), groups, d, seed=1)
    print("plane record stage 33x27x21, y = 2 and y = 1.1 per plane: " + " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) < PARITY


def test_entries_refuse_bad_arguments(dev):
    from kwave_amd import capi
    a = Guarded(dev, np.zeros(8192, F32))
    b = Guarded(dev, np.zeros(8192, F32))
    t = Guarded(dev, np.zeros(4), dtype=np.float64)
    op = make_op((1e-4, 1e-4, 1e-4), C0, 0.0, 1.5)
    n = C.c_size_t()
    with pytest.raises(capi.KWaveError, match="kw_set_constants has not been called"):
        dev.call("second_order_plane_prepare", a.ptr, b.ptr, 0)
    set_constants(dev, 16, 16, 16)
    prepare, record = "kw_second_order_plane_prepare", "kw_second_order_plane_record"
    with pytest.raises(capi.KWaveError, match="kw_second_order_plane_elems"):
        dev.call("second_order_plane_elems", None)
    dev.call("second_order_plane_elems", C.byref(n))
    assert n.value == 16 * 9 * 9
    bad = [(prepare, ("second_order_plane_prepare", None, b.ptr, 0)),
           (prepare, ("second_order_plane_prepare", a.ptr, None, 0)),
           (prepare, ("second_order_plane_prepare", a.ptr, a.ptr, 0)),            # aliased
           (prepare, ("second_order_plane_prepare", a.ptr, b.ptr, 16)),           # a plane outside the volume
           (record, ("second_order_plane_record", None, b.ptr, C.byref(op), t.ptr, 4)),
           (record, ("second_order_plane_record", a.ptr, None, C.byref(op), t.ptr, 4)),
           (record, ("second_order_plane_record", a.ptr, b.ptr, None, t.ptr, 4)),
           (record, ("second_order_plane_record", a.ptr, b.ptr, C.byref(op), None, 4)),
           (record, ("second_order_plane_record", a.ptr, a.ptr, C.byref(op), t.ptr, 4)),   # aliased
           (record, ("second_order_plane_record", a.ptr, b.ptr, C.byref(op), t.ptr, 0)),
           (record, ("second_order_plane_record", a.ptr, b.ptr, C.byref(make_op((1e-4, 1e-4, 0.0), C0, 0.0, 1.5)), t.ptr, 4))]
    for who, call in bad:
        with pytest.raises(capi.KWaveError, match=who):
            dev.call(*call)
    dev.sync()
    assert not a.read().any() and not b.read().any()   # nothing is written by a refused call
    for g in (a, b, t):
        g.free()


# ---- 2. SecondOrder.plane_record ------------------------------------------------------------------------------------------------
E2E_D = (1.0e-4, 1.2e-4, 0.9e-4)
E2E_TMAX = 1.03e-6
E2E_TIMES = E2E_TMAX * np.array([0.31, 0.05, 1.0, 0.0, 0.77, 0.12, 0.5, 0.93, 0.2, 0.68, 0.41, 0.86])   # unsorted, 0 among them
E2E_COEFF = 0.75
N = (24, 20, 18)


def e2e_p0(n, seed):
    """two Gaussian balls and 2 % noise"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = n
    cx, cy, cz, ax, ay, az = rng.uniform(0.25, 0.75, 6)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (np.exp(-((x - cx * nx) ** 2 + (y - cy * ny) ** 2 + (z - cz * nz) ** 2) / 9.0) +
            0.3 * np.exp(-((x - ax * nx) ** 2 + (y - ay * ny) ** 2 + (z - az * nz) ** 2) / 4.0) +
            0.02 * rng.standard_normal((nz, ny, nx))).astype(F32)


@pytest.mark.parametrize("n,fused,sides", [((24, 20, 18), True, (48, 48, 48)), ((23, 19, 17), False, (39, 32, 35))],
                         ids=["fused", "rocfft"])
@pytest.mark.parametrize("coeff", [0.0, E2E_COEFF], ids=["lossless", "absorbing"])
@pytest.mark.parametrize("plane", [0, 7])
def test_plane_record_against_the_restatement_and_against_run(second_order, plane, coeff, n, fused, sides):
    """12 unsorted times.  On the fused context the record takes its (kx, ky, kz) spectrum from a 3-D transform of its own;
    on the rocFFT context from the kept one.  Measured: against float64 1.5e-7 to 2.0e-7, against run(times) 1.2e-7 to
    1.6e-7, t = 0 against the plane of p0 1.4e-7 to 6.4e-7."""
    points = n[0] * n[1]
    sensors = plane * points + np.arange(points)
    p = second_order.SecondOrder(n, E2E_D, C0, alpha_coeff=coeff, t_max=E2E_TMAX, sensor_index=sensors, fused_kernels=fused,
                                 plane=plane)
    try:
        assert p.expanded == sides and p.fused == fused and p.plane == plane
        assert coeff == 0.0 or sr.b_margins(sides, E2E_D, C0, coeff, 1.5)[0] >= 0.25
        p0 = e2e_p0(n, 1)
        p.set_p0(p0)
        rec = p.plane_record(E2E_TIMES)
        assert rec.dtype == F32 and rec.shape == (12, n[1], n[0])
        want = pr.record(p0, sides, E2E_D, C0, E2E_TIMES, plane, coeff, 1.5)
        e_rec = sr.rel_l2(rec, want)
        raw = p.run(E2E_TIMES)   # (n_times, Nx Ny)
        e_run = sr.rel_l2(rec, raw.reshape(rec.shape))
        e_zero = sr.rel_l2(rec[3], p0[plane])
        print(f"plane_record {n} plane {plane} alpha_coeff {coeff} fused {fused}: rel L2 against float64 {e_rec:.3e}, "
              f"against run(times) {e_run:.3e}, t = 0 against p0 {e_zero:.3e}")
        assert e_rec < PARITY and e_run < 2 * PARITY and e_zero < 1e-6
        assert np.array_equal(p.plane_record(E2E_TIMES), rec)   # run(times) in between has changed nothing
    finally:
        p.close()


@pytest.fixture(scope="module")
def reference_record(second_order):
    """the record of plane 7, absorbing, on the fused context: what the bit-for-bit tests compare with"""
    p0 = e2e_p0(N, 1)
    p = second_order.SecondOrder(N, E2E_D, C0, alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, plane=7)
    try:
        p.set_p0(p0)
        return p0, p.plane_record(E2E_TIMES)
    finally:
        p.close()


def test_a_time_has_its_bits_alone_in_a_list_and_under_every_chunking(second_order, reference_record):
    p0, rec = reference_record
    p = second_order.SecondOrder(N, E2E_D, C0, alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, plane=7)
    try:
        p.set_p0(p0)
        default = p.plane_chunk_times
        assert default == (256 << 20) // (25 * 48 * 8)
        for i in (0, 3, 11):
            assert np.array_equal(p.plane_record([E2E_TIMES[i]])[0], rec[i]), i
        for chunk in (5, 1):   # passes of 5, 5, 2 times and of one time each
            p.plane_chunk_times = chunk
            assert p.plane_chunk_times == chunk
            assert np.array_equal(p.plane_record(E2E_TIMES), rec), chunk
        p.plane_chunk_times = None
        assert p.plane_chunk_times == default
        # sorted and shuffled, plane for plane
        order = np.argsort(E2E_TIMES)
        assert np.array_equal(p.plane_record(E2E_TIMES[order]), rec[order])
        shuffled = np.random.default_rng(3).permutation(12)
        assert np.array_equal(p.plane_record(E2E_TIMES[shuffled]), rec[shuffled])
    finally:
        p.close()


def test_a_second_set_p0_and_interleaved_propagators(second_order, reference_record):
    pa, rec_a = reference_record
    pb = e2e_p0(N, 3)
    kw = dict(alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, plane=7)
    a = second_order.SecondOrder(N, E2E_D, C0, **kw)
    b = second_order.SecondOrder(N, E2E_D, C0, **kw)
    try:
        b.set_p0(pb)
        rec_b = b.plane_record(E2E_TIMES)
        assert not np.array_equal(rec_b, rec_a)
        a.set_p0(pb)
        a.set_p0(pa)   # a second set_p0 replaces the first
        for lo in (0, 4, 8):
            ra = a.plane_record(E2E_TIMES[lo:lo + 4])
            rb = b.plane_record(E2E_TIMES[lo:lo + 4])
            assert np.array_equal(ra, rec_a[lo:lo + 4]) and np.array_equal(rb, rec_b[lo:lo + 4])
        b.set_p0(pa)
        assert np.array_equal(b.plane_record(E2E_TIMES), rec_a)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
def test_field_run_and_plane_record_may_be_interleaved(second_order, fused):
    """the record neither reads nor writes the field state, the aggregates or the record of run, whose results keep the
    bits they have with no plane set"""
    sensors = np.array([0, 23, (7 * 20 + 5) * 24 + 3])
    kw = dict(alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, sensor_index=sensors, record=("p_raw", "p_max", "p_final"),
              fused_kernels=fused, expanded=(48, 48, 48))
    p0 = e2e_p0(N, 8)
    plain = second_order.SecondOrder(N, E2E_D, C0, **kw)   # no plane: the class as it was
    try:
        assert plain.plane is None
        plain.set_p0(p0)
        field = plain.field(E2E_TIMES[2])
        raw = plain.run(E2E_TIMES[:5])
        p_max, p_final = plain.p_max(), plain.p_final()
    finally:
        plain.close()
    p = second_order.SecondOrder(N, E2E_D, C0, plane=7, **kw)
    try:
        p.set_p0(p0)
        rec = p.plane_record(E2E_TIMES)
        assert np.array_equal(p.field(E2E_TIMES[2]), field)
        assert np.array_equal(p.plane_record(E2E_TIMES), rec)
        assert np.array_equal(p.run(E2E_TIMES[:5]), raw)
        assert np.array_equal(p.plane_record(E2E_TIMES), rec)
        assert np.array_equal(p.p_max(), p_max) and np.array_equal(p.p_final(), p_final) and p.runs == 1
        assert np.array_equal(p._get("p", p.shape), p_final)   # the last field computed is run's, not the record's
    finally:
        p.close()


# ---- 3. with PlaneRecon -----------------------------------------------------------------------------------------------------
def test_the_record_is_plane_recon_s_input(second_order):
    """plane 0 at t_n = n dt into PlaneRecon(dims = (Nx, Ny), spacing = (dx, dy), the same c0 and dt): the image of the
    device's record against the image of the float64 record rounded to float32 — the layout (Nt, Ny, Nx) and the time
    convention of the two classes, not how well the image recovers p0.  Measured: 2.6e-7."""
    from kwave_amd import recon
    nt, dt = 32, E2E_D[2] / C0
    times = dt * np.arange(nt)
    p0 = e2e_p0(N, 9)
    p = second_order.SecondOrder(N, E2E_D, C0, t_max=nt * dt, plane=0)
    try:
        sides = p.expanded
        p.set_p0(p0)
        rec = p.plane_record(times)
    finally:
        p.close()
    want = pr.record(p0, sides, E2E_D, C0, times, 0).astype(F32)
    assert sr.rel_l2(rec, want) < PARITY
    r = recon.PlaneRecon(N[:2], E2E_D[:2], dt, nt, C0)
    try:
        got, ref = r.run(rec), r.run(want)
    finally:
        r.close()
    err = sr.rel_l2(got, ref)
    print(f"PlaneRecon of plane_record against PlaneRecon of the float64 record: {err:.3e}")
    assert np.linalg.norm(ref) > 0 and err < 2 * PARITY


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_plane_record_refusals(second_order):
    from kwave_amd import capi
    with pytest.raises(capi.KWaveError, match=r"plane: 18 is outside the domain's planes 0 ... 17"):
        second_order.SecondOrder(N, E2E_D, C0, t_max=E2E_TMAX, plane=18)
    p = second_order.SecondOrder(N, E2E_D, C0, t_max=E2E_TMAX)
    try:
        assert p.plane is None
        p.set_p0(e2e_p0(N, 4))
        with pytest.raises(capi.KWaveError, match="plane_record: no plane set"):
            p.plane_record([1e-7])
        with pytest.raises(capi.KWaveError, match=r"plane: -2 is outside"):
            p.plane = -2
        p.plane = 3
        assert p.plane == 3
        with pytest.raises(capi.KWaveError, match="plane_record: no p0 since the plane was set"):
            p.plane_record([1e-7])
        p.set_p0(e2e_p0(N, 4))
        with pytest.raises(capi.KWaveError, match=r"n_times: 0 is not a number of output times"):
            p.plane_record([])
        with pytest.raises(capi.KWaveError, match=r"t: -0.000001 is not a time >= 0"):
            p.plane_record([1e-7, -1e-6])
        with pytest.raises(capi.KWaveError, match=r"t: nan is not a time >= 0"):
            p.plane_record([float("nan")])
        with pytest.raises(capi.KWaveError, match=r"t: inf is not a time >= 0"):
            p.plane_record([float("inf")])
        with pytest.raises(capi.KWaveError, match=r"plane_chunk_times: "):
            p.plane_chunk_times = 1 << 40
        first = p.plane_record([1e-7, 3e-7])
        assert first.shape == (2, 20, 24)
        p.set_dp0dt(np.zeros(p.shape, F32))
        with pytest.raises(capi.KWaveError, match=r"plane_record: a dp0dt is set .*not built: dp0dt in plane_record"):
            p.plane_record([1e-7])
        p.set_dp0dt(None)
        assert np.array_equal(p.plane_record([1e-7, 3e-7]), first)
        p.plane = 5                         # another plane: the old Q is not used
        with pytest.raises(capi.KWaveError, match="plane_record: no p0 since the plane was set"):
            p.plane_record([1e-7])
        p.plane = None                      # off: the arrays are freed
        with pytest.raises(capi.KWaveError, match="plane_record: no plane set"):
            p.plane_record([1e-7])
        p.plane = 3
        p.set_p0(e2e_p0(N, 4))
        assert np.array_equal(p.plane_record([1e-7, 3e-7]), first)
    finally:
        p.close()
