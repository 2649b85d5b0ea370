"""Exact k-space propagator on the GPU: the fused stage (forward, k_zfused_second_order, y- and x-inverse) at every
fast-path line length, the stage against its rocFFT twin, the refusals, kwave_amd.second_order.SecondOrder end to end
against the float64 NumPy restatement of tests/second_order_reference.py, the wrap-around rule, and the propagator next to
the time loop on the K1 configuration.

Bounds.
  stage, twin, SecondOrder   1e-5 relative L2, the project's parity bound (PARITY of the sibling tests), against float64 of
                             the same float32 inputs.  The absorbing variants assert first that B >= 1/4 on every bin of
                             their grid (second_order_reference.b_margins) — a condition on the inputs.
  field(0)                   1e-6: H = 1, the forward and inverse pipeline alone.
  p_max, p_min               exact: the max and min of the device's own field(t) results.
  wrap-around                2e-5 (two results, each within 1e-5 of its float64 field) plus the restatement's own difference
                             between the two expansions.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import cw_reference as cr  # noqa: E402
import second_order_reference as sr  # noqa: E402
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
PARITY = 1e-5
LENGTHS = cr.fast_lengths()
C0 = 1500.0


@pytest.fixture(scope="module")
def second_order():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, second_order
    assert "kw_fused_second_order_time" in capi._SIG
    return second_order


@pytest.fixture()
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def make_op(d, c0, t, coeff, y):
    from kwave_amd import capi
    op = capi.SecondOrderOp()
    op.dx, op.dy, op.dz, op.c0, op.t = d[0], d[1], d[2], c0, t
    op.a, op.alpha_power = sr.neper(coeff, y), y
    op.absorbing = int(coeff > 0.0)
    return op


def source_volume(rng, ex, ey, ez):
    """a smooth random field on the whole expanded volume plus 5 % white noise, so that every bin (the x-Nyquist column
    among them) carries something"""
    z, y, x = np.meshgrid(np.arange(ez) / ez, np.arange(ey) / ey, np.arange(ex) / ex, indexing="ij")
    c = rng.uniform(-1.0, 1.0, 8)
    s = (c[0] + c[1] * np.cos(2 * np.pi * x + c[2]) * np.sin(2 * np.pi * z + c[6]) +
         c[3] * np.sin(4 * np.pi * y + c[4]) * np.cos(2 * np.pi * x) * np.cos(4 * np.pi * z) +
         c[5] * np.exp(-((x - 0.4) ** 2 + (y - 0.6) ** 2 + (z - 0.5) ** 2) / 0.02) * np.cos(6 * np.pi * z + c[7]))
    return (s + 0.05 * rng.standard_normal((ez, ey, ex))).astype(F32)


class Stage:
    """a fused context of (ex, ey, ez) with a volume transformed once and kept; time(op) gives the field at one time"""

    def __init__(self, dev, ex, ey, ez, vol):
        self.dev = dev
        set_constants(dev, ex, ey, ez)
        ok = C.c_int()
        dev.call("fused_supported", C.byref(ok))
        assert ok.value == 1, (ex, ey, ez)
        dev.call("fused_create")
        n = C.c_size_t()
        dev.call("fused_second_order_elems", C.byref(n))
        assert n.value == (ex // 2 + 1 + 15) // 16 * 16 * ey * ez
        self.vol = Guarded(dev, vol)
        self.kept = Guarded(dev, np.full(2 * n.value, np.nan, F32))
        dev.call("fused_second_order_forward", self.vol.ptr, self.kept.ptr)
        dev.sync()
        self.kept_bytes = self.kept.read().view(np.uint8)
        self.out = Guarded(dev, np.full((ez, ey, ex), np.nan, F32))

    def time(self, op):
        self.dev.call("fused_second_order_time", self.kept.ptr, C.byref(op), self.out.ptr)
        self.dev.sync()
        return self.out.read()

    def close(self):
        assert np.array_equal(self.kept.read().view(np.uint8), self.kept_bytes)  # the kept spectrum survives every time
        self.dev.call("fused_destroy")
        for g in (self.vol, self.kept, self.out):
            g.free()


# ---- 1. the fused stage at every line length ------------------------------------------------------------------------------
def stage_errors(dev, ex, ey, ez):
    """lossless near and far, absorbing near and far (second_order_reference.stage_case); the whole expanded output"""
    cases = sr.stage_case((ex, ey, ez))
    assert sr.b_margins((ex, ey, ez), sr.STAGE_D, sr.STAGE_C0, cases[3][0], sr.STAGE_Y)[0] >= 0.25
    rng = np.random.default_rng(ex * 1009 + ey * 31 + ez)
    vol = source_volume(rng, ex, ey, ez)
    X = np.fft.rfftn(vol.astype(np.float64))
    s = Stage(dev, ex, ey, ez, vol)
    errs = []
    for coeff, t in cases:
        got = s.time(make_op(sr.STAGE_D, sr.STAGE_C0, t, coeff, sr.STAGE_Y))
        H = sr.H((ex, ey, ez), sr.STAGE_D, sr.STAGE_C0, t, coeff, sr.STAGE_Y)
        want = np.fft.irfftn(X * H, s=vol.shape, axes=(0, 1, 2))
        assert np.linalg.norm(want) > 1e-3 * np.linalg.norm(vol)   # the result has not vanished
        errs.append(sr.rel_l2(got, want))
    s.close()
    return errs


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length(dev, L):
    """(L, 16, 16): the x-passes at every length; (16, 16, L): k_zfused_second_order<L> on one column tile, no side array.
    Three unequal spacings.  Lossless and absorbing (y = 1.5), c0 t = 0.37 of the smallest spacing and the time at which
    the largest |k| has made 10^4 turns, where the slowest mode of the absorbing medium keeps exp(-2).  Measured: lossless
    1.1e-7 to 2.3e-7 near and 9.6e-8 to 5.1e-7 far (worst at (16, 16, 192)); absorbing 1.1e-7 to 2.7e-7 near and 2.4e-8 to
    1.7e-7 far."""
    for ex, ey, ez in ((L, 16, 16), (16, 16, L)):
        errs = stage_errors(dev, ex, ey, ez)
        print(f"second-order stage {ex}x{ey}x{ez}: rel L2 lossless near {errs[0]:.3e} far {errs[1]:.3e}; "
              f"absorbing near {errs[2]:.3e} far {errs[3]:.3e}")
        assert max(errs) < PARITY, (ex, ey, ez)


@pytest.mark.parametrize("L", LENGTHS)
def test_stage_at_every_line_length_with_side_array(dev, L):
    """(96, 16, L): k_zfused_second_order<L> on three main column tiles and on the side block of the x-Nyquist column,
    which forms H at kx = Ex/2 for 16 rows ky.  The variants of the test above; the whole expanded output.  Measured:
    lossless 1.2e-7 to 2.5e-7 near and 1.1e-7 to 3.8e-7 far (worst at 576); absorbing 1.1e-7 to 2.7e-7 near and 2.9e-8 to
    1.8e-7 far."""
    errs = stage_errors(dev, 96, 16, L)
    print(f"second-order stage 96x16x{L}: rel L2 lossless near {errs[0]:.3e} far {errs[1]:.3e}; "
          f"absorbing near {errs[2]:.3e} far {errs[3]:.3e}")
    assert max(errs) < PARITY, L


# ---- 2. fused against twin ------------------------------------------------------------------------------------------------
TWIN = dict(d=(1.0e-4, 0.8e-4, 1.3e-4), coeff=0.75, y=1.5, t=37.3 * 0.8e-4 / C0)


def twin_errors(d2, vol, variants):
    """kw_second_order_mix on the natural half-spectrum of a context with 3-D plans, one C2R transform per variant"""
    ez, ey, ex = vol.shape
    p = TWIN
    set_constants(d2, ex, ey, ez)
    d2.call("fft_create_plans_3d")
    nr = (ex // 2 + 1) * ey * ez
    src, spec = Guarded(d2, vol), Guarded(d2, np.zeros(2 * nr, F32))
    d2.call("fft_r2c_3d", src.ptr, spec.ptr)
    d2.sync()
    spec_bytes = spec.read().view(np.uint8)
    mixed, out = Guarded(d2, np.full(2 * nr, np.nan, F32)), Guarded(d2, np.full(vol.shape, np.nan, F32))
    errs = []
    for coeff, y in variants:
        op = make_op(p["d"], C0, p["t"], coeff, y)
        d2.call("second_order_mix", mixed.ptr, spec.ptr, C.byref(op), C.c_float(1.0 / (ex * ey * ez)))
        d2.call("fft_c2r_3d", mixed.ptr, out.ptr)
        d2.sync()
        errs.append(sr.rel_l2(out.read(), sr.solve_expanded(vol, p["d"], C0, p["t"], coeff, y)))
    assert np.array_equal(spec.read().view(np.uint8), spec_bytes)   # out of place: the spectrum is read only
    for g in (src, spec, mixed, out):
        g.free()
    return errs


# y = 1.5 (|k|^(y-1) by a square root), lossless, Stokes (y = 2: |k| itself), y = 1.1 (the float64 power function)
VARIANTS = ((0.75, 1.5), (0.0, 1.5), (0.2, 2.0), (0.75, 1.1))


@pytest.mark.parametrize("ex,ey,ez", [(32, 48, 48), (48, 16, 64)])
def test_fused_stage_and_rocfft_twin(dev, ex, ey, ez):
    from kwave_amd import capi
    p = TWIN
    for coeff, y in VARIANTS:
        assert coeff == 0.0 or sr.b_margins((ex, ey, ez), p["d"], C0, coeff, y)[0] >= 0.25
    vol = source_volume(np.random.default_rng(ex + ey + ez), ex, ey, ez)
    s = Stage(dev, ex, ey, ez, vol)
    fused = [sr.rel_l2(s.time(make_op(p["d"], C0, p["t"], coeff, y)), sr.solve_expanded(vol, p["d"], C0, p["t"], coeff, y))
             for coeff, y in VARIANTS]
    s.close()
    d2 = capi.Device()
    try:
        d2.call("second_order_mix", None, None, None, C.c_float(1.0))   # no constants, no bins: no pointer is looked at
        twins = twin_errors(d2, vol, VARIANTS)
    finally:
        d2.close()
    print(f"second-order {ex}x{ey}x{ez} (y = 1.5, lossless, Stokes, y = 1.1): fused stage " + " ".join(f"{e:.3e}" for e in fused) +
          "; rocFFT twin " + " ".join(f"{e:.3e}" for e in twins) + " (rel L2 against float64)")
    assert max(fused) < PARITY and max(twins) < PARITY


def test_rocfft_twin_on_an_odd_grid(dev):
    ex, ey, ez = 27, 20, 33
    for coeff, y in VARIANTS:
        assert coeff == 0.0 or sr.b_margins((ex, ey, ez), TWIN["d"], C0, coeff, y)[0] >= 0.25
    vol = source_volume(np.random.default_rng(2733), ex, ey, ez)
    twins = twin_errors(dev, vol, VARIANTS)
    print("second-order twin 27x20x33 (y = 1.5, lossless, Stokes, y = 1.1): " + " ".join(f"{e:.3e}" for e in twins))
    assert max(twins) < PARITY


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def test_stage_refuses_two_d_slab_and_frames_contexts(dev):
    from kwave_amd import capi
    a = Guarded(dev, np.zeros(2 * 32 * 32 * 16, F32))
    b = Guarded(dev, np.zeros(2 * 32 * 32 * 16, F32))
    op = make_op((1e-4, 1e-4, 1e-4), C0, 1e-7, 0.0, 1.5)
    entries = (("fused_second_order_time", (a.ptr, C.byref(op), b.ptr)), ("fused_second_order_forward", (a.ptr, b.ptr)))
    set_constants(dev, 32, 32, 1)
    dev.call("fused_create")
    for entry, args in entries:
        with pytest.raises(capi.KWaveError, match="kw_" + entry + r": single GPU and 3-D only \(no Z-slabs, no Nz == 1\)"):
            dev.call(entry, *args)
    dev.call("fused_destroy")
    # a frames context: kw_fused_line_recon is its one stage
    set_constants(dev, 32, 32, 16)
    dev.call("fused_set_frames", 1)
    dev.call("fused_create")
    for entry, args in entries:
        with pytest.raises(capi.KWaveError, match="kw_" + entry + r": .*frames mode"):
            dev.call(entry, *args)
    n = C.c_size_t()
    with pytest.raises(capi.KWaveError, match=r"kw_fused_second_order_elems: .*frames mode"):
        dev.call("fused_second_order_elems", C.byref(n))
    dev.call("fused_destroy")
    # one rank with an exchange callback = the slab path against itself; the callback is never reached
    exchange = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)(lambda *args: 1)
    set_constants(dev, 32, 32, 16)
    dev.call("fused_set_slab", 1, 0, 16, C.cast(exchange, C.c_void_p), None)
    dev.call("fused_create")
    for entry, args in entries:
        with pytest.raises(capi.KWaveError, match="kw_" + entry + r": single GPU and 3-D only \(no Z-slabs, no Nz == 1\)"):
            dev.call(entry, *args)
    dev.call("fused_destroy")
    for g in (a, b):
        g.free()


# ---- 4. SecondOrder end to end ------------------------------------------------------------------------------------------------
E2E_D = (1.0e-4, 1.2e-4, 0.9e-4)
E2E_TMAX = 1.03e-6
E2E_TIMES = E2E_TMAX * np.array([0.31, 0.05, 1.0, 0.0, 0.77, 0.12, 0.5, 0.93, 0.2, 0.68, 0.41, 0.86])   # unsorted, 0 among them
E2E_COEFF = 0.75


def e2e_p0(n, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = n
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ball = np.exp(-((x - 0.45 * nx) ** 2 + (y - 0.55 * ny) ** 2 + (z - 0.5 * nz) ** 2) / 9.0)
    return (ball + 0.3 * np.exp(-((x - 0.7 * nx) ** 2 + (y - 0.3 * ny) ** 2 + (z - 0.3 * nz) ** 2) / 4.0) +
            0.02 * rng.standard_normal((nz, ny, nx))).astype(F32)


def e2e_sensors(n):
    """7 points, the domain's corners among them"""
    nx, ny, nz = n
    last = nx * ny * nz - 1
    return np.array([0, nx - 1, nx * (ny - 1), last, last - (nx - 1), (nz // 2 * ny + ny // 2) * nx + nx // 2, 1234], dtype=np.int64)


@pytest.mark.parametrize("n,fused", [((24, 20, 18), True), ((23, 19, 17), False)], ids=["fused", "rocfft"])
@pytest.mark.parametrize("coeff", [0.0, E2E_COEFF], ids=["lossless", "absorbing"])
def test_second_order_against_the_restatement(second_order, coeff, n, fused):
    sensors = e2e_sensors(n)
    p = second_order.SecondOrder(n, E2E_D, C0, alpha_coeff=coeff, alpha_power=1.5, t_max=E2E_TMAX, sensor_index=sensors,
                                 record=("p_raw", "p_max", "p_min", "p_rms", "p_final"), fused_kernels=fused)
    try:
        expanded = p.expanded
        assert p.fused == fused and expanded == sr.default_sides(n, E2E_D, C0, E2E_TMAX, fused, LENGTHS) and p.runs == 0
        assert coeff == 0.0 or sr.b_margins(expanded, E2E_D, C0, coeff, 1.5)[0] >= 0.25
        assert p.t_free == pytest.approx(min((e - m) * d for e, m, d in zip(expanded, n, E2E_D)) / C0, rel=1e-12)
        assert p.t_free >= E2E_TMAX
        p0 = e2e_p0(n, 1)
        p.set_p0(p0)
        want = sr.solve(p0, expanded, E2E_D, C0, E2E_TIMES, coeff, 1.5)
        # field(t), time by time; field(0) is p0 through the forward and inverse pipeline alone
        fields = np.array([p.field(t) for t in E2E_TIMES])
        assert fields.dtype == F32 and fields.shape == (12,) + p0.shape
        e_field = max(sr.rel_l2(fields[i], want[i]) for i in range(12))
        e_zero = sr.rel_l2(p.field(0.0), p0)
        # run(times): the record and the aggregates
        rec = p.run(E2E_TIMES)
        assert rec.dtype == F32 and rec.shape == (12, 7) and p.runs == 1
        e_raw = sr.rel_l2(rec, want.reshape(12, -1)[:, sensors])
        assert np.array_equal(rec, fields.reshape(12, -1)[:, sensors])
        e_final = sr.rel_l2(p.p_final(), want[-1])
        e_rms = sr.rel_l2(p.p_rms(), np.sqrt(np.mean(want ** 2, axis=0)))
        print(f"SecondOrder {n} alpha_coeff {coeff} fused {fused} E {expanded}: rel L2 worst field {e_field:.3e}, field(0) {e_zero:.3e}, "
              f"p_raw {e_raw:.3e}, p_final {e_final:.3e}, p_rms {e_rms:.3e}")
        assert max(e_field, e_raw, e_final, e_rms) < PARITY
        assert e_zero < 1e-6
        assert np.array_equal(p.p_max(), fields.max(axis=0)) and np.array_equal(p.p_min(), fields.min(axis=0))
        assert np.array_equal(p.p_final(), fields[-1])
        # the same p0 again gives identical bits
        p.set_p0(p0)
        assert np.array_equal(p.field(E2E_TIMES[2]), fields[2])
    finally:
        p.close()


@pytest.mark.parametrize("n,fused", [((24, 20, 18), True), ((23, 19, 17), False)], ids=["fused", "rocfft"])
def test_run_again_regrows_reuses_and_resets(second_order, n, fused):
    """run three times on one object: three times, five others (the record grows), the three again (the larger record is
    kept).  Every run's record and aggregates are those of its own times alone: the bits of field(t), p_rms within the
    parity bound of the float64 root mean square of those float32 fields."""
    sensors = e2e_sensors(n)
    t1, t2 = E2E_TIMES[[5, 3, 10]], E2E_TIMES[[2, 7, 0, 4, 9]]
    p = second_order.SecondOrder(n, E2E_D, C0, alpha_coeff=E2E_COEFF, alpha_power=1.5, t_max=E2E_TMAX, sensor_index=sensors,
                                 record=("p_raw", "p_max", "p_min", "p_rms", "p_final"), fused_kernels=fused)
    try:
        assert p.fused == fused
        p.set_p0(e2e_p0(n, 5))
        fields = np.array([p.field(t) for t in t2])
        first = p.run(t1)
        assert first.shape == (3, 7)
        rec = p.run(t2)
        assert rec.shape == (5, 7) and np.array_equal(rec, fields.reshape(5, -1)[:, sensors])
        assert np.array_equal(p.p_max(), fields.max(axis=0)) and np.array_equal(p.p_min(), fields.min(axis=0))
        assert np.array_equal(p.p_final(), fields[-1])
        e_rms = sr.rel_l2(p.p_rms(), np.sqrt(np.mean(fields.astype(np.float64) ** 2, axis=0)))
        print(f"SecondOrder {n} fused {fused}: p_rms of a second run against its own fields {e_rms:.3e}")
        assert e_rms < PARITY
        again = p.run(t1)
        assert again.shape == (3, 7) and np.array_equal(again, first)
        p_max = p.p_max()
        assert np.array_equal(p_max, np.array([p.field(t) for t in t1]).max(axis=0))
        assert p.runs == 3
    finally:
        p.close()


def test_two_interleaved_propagators_do_not_disturb_each_other(second_order):
    n = (24, 20, 18)
    pa, pb = e2e_p0(n, 2), e2e_p0(n, 3)
    t = E2E_TIMES[:4]
    alone = []
    for p0 in (pa, pb):
        q = second_order.SecondOrder(n, E2E_D, C0, alpha_coeff=E2E_COEFF, t_max=E2E_TMAX)
        try:
            q.set_p0(p0)
            alone.append([q.field(x) for x in t])
        finally:
            q.close()
    a = second_order.SecondOrder(n, E2E_D, C0, alpha_coeff=E2E_COEFF, t_max=E2E_TMAX)
    b = second_order.SecondOrder(n, E2E_D, C0, alpha_coeff=E2E_COEFF, t_max=E2E_TMAX)
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


def test_times_are_checked(second_order):
    from kwave_amd import capi
    p = second_order.SecondOrder((24, 20, 18), E2E_D, C0, t_max=E2E_TMAX)
    try:
        with pytest.raises(capi.KWaveError, match="field: no p0 yet"):
            p.field(1e-7)
        p.set_p0(e2e_p0((24, 20, 18), 4))
        with pytest.raises(capi.KWaveError, match=r"t: -0.000001 is not a time >= 0"):
            p.field(-1e-6)
        with pytest.raises(capi.KWaveError, match=r"t: nan is not a time >= 0"):
            p.run([1e-7, float("nan")])
        with pytest.raises(capi.KWaveError, match=r"n_times: 0 is not a number of output times"):
            p.run([])
        with pytest.raises(capi.KWaveError, match=r"p_max: no run yet"):
            p.p_max()
        assert p.run([1e-7]).shape == (1, 0)
        with pytest.raises(capi.KWaveError, match=r"p_max: not recorded"):
            p.p_max()
    finally:
        p.close()


# ---- 5. the wrap-around rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused,side", [(True, 32), (False, 22)], ids=["fused", "rocfft"])
def test_field_inside_the_domain_is_free_of_wrap_around_up_to_t_free(second_order, fused, side):
    """a Gaussian ball in a (16, 16, 16) domain, c0 t_max = 5.5 points: the minimal default sides (22, the number itself, on
    the rocFFT path, t_free = 6 points with the wave still inside the domain; the fast-path length 32 on the fused path,
    t_free = 16 points with most of it gone) against sides twice as large, at t_free of the smaller box.  The ball's band
    limit makes the two float64 fields differ a little (3e-6 and 1e-4): that difference is computed and added."""
    n, d = (16, 16, 16), (1.0e-4, 1.0e-4, 1.0e-4)
    t_max = 5.5 * d[0] / C0
    z, y, x = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    p0 = np.exp(-((x - 7.5) ** 2 + (y - 8.0) ** 2 + (z - 7.0) ** 2) / 6.0).astype(F32)
    got = []
    a = second_order.SecondOrder(n, d, C0, t_max=t_max, fused_kernels=fused)
    try:
        t = a.t_free
        assert a.expanded == (side,) * 3 and a.fused == fused and t == pytest.approx((side - 16) * d[0] / C0) and t >= t_max
        a.set_p0(p0)
        got.append(a.field(t))
    finally:
        a.close()
    b = second_order.SecondOrder(n, d, C0, expanded=(2 * side,) * 3, fused_kernels=fused)
    try:
        assert b.fused == fused and b.t_free == pytest.approx((2 * side - 16) * d[0] / C0)
        b.set_p0(p0)
        got.append(b.field(t))
    finally:
        b.close()
    ref = [sr.solve(p0, (e,) * 3, d, C0, [t])[0] for e in (side, 2 * side)]
    own = sr.rel_l2(ref[0], ref[1])
    err = sr.rel_l2(got[0], got[1])
    print(f"wrap-around at t_free: E = {side} against E = {2 * side} on the GPU {err:.3e}; the restatement's own difference {own:.3e}")
    assert err <= 2e-5 + own


# ---- 6. next to the time loop ------------------------------------------------------------------------------------------------
def test_k1_configuration_next_to_the_time_loop(second_order):
    """K1 at 32^3 (homogeneous, lossless, PML off, p0 only): SecondOrder(expanded = N).field(20 dt) against the float64 closed
    form; the time loop's own distance after 20 steps is printed (test_k1_closed_form_on_gpu owns its bound)"""
    import kwave_amd  # noqa: F401
    from kwave_amd import synthetic
    from kwave_amd.solver import HostSolver
    from oracle.kwave_np import closed_form_pressure
    pr = synthetic.make_problem(32, heterogeneous=False, nonlinear=False, absorbing=False, pml_off=True, source="p0")
    sc = lambda k: float(np.asarray(pr[k]).reshape(-1)[0])   # noqa: E731
    want = closed_form_pressure(pr, 20)
    g = HostSolver(pr)
    try:
        g.run(21)   # sample 0 is p0 itself: the field after step 20 is the 21st sample
        loop = sr.rel_l2(g.field("p"), want)
    finally:
        g.close()
    p = second_order.SecondOrder((32, 32, 32), (sc("dx"), sc("dy"), sc("dz")), sc("c0"), expanded=(32, 32, 32))
    try:
        assert p.fused and p.t_free == 0.0
        p.set_p0(np.asarray(pr["p0_source_input"], dtype=F32).reshape(32, 32, 32))
        err = sr.rel_l2(p.field(20 * sc("dt")), want)
    finally:
        p.close()
    print(f"K1 32^3 after 20 steps against the closed form: SecondOrder {err:.3e}, time loop {loop:.3e}")
    assert err < PARITY
