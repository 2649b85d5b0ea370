"""dp0/dt as a second initial condition of the batched 2-D exact k-space propagator on the GPU: the fused pair stage of a
frames context (both kept spectra, k_yfused_second_order_pair, x-inverse) at every fast-path line length, with and without
the side array's blocks, the stage and its rocFFT twin kw_second_order_frames_mix_pair, the refusals,
kwave_amd.second_order.SecondOrderFrames with set_dp0dt end to end against the float64 restatement of
tests/second_order_dp0dt_reference.py, the single path after set_dp0dt(None), the travelling wave and the line record's
refusal.

Bounds: those of tests/test_gpu_second_order_dp0dt.py (PARITY = 1e-5 relative L2 against float64 of the same float32
inputs over the whole expanded output; the second batch scaled per case to the float64 norm of the first term, with
|want| >= 0.5 |either term| and B >= 1/4 asserted as conditions on the inputs; field(0) 1e-6; bits where bits are claimed;
the travelling wave PARITY plus the restatement's own difference).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import cw_reference as cr  # noqa: E402
import second_order_dp0dt_reference as dr  # noqa: E402
import second_order_frames_reference as fr  # noqa: E402
import second_order_reference as sr  # noqa: E402
import test_gpu_second_order_frames as sib  # noqa: E402  (source_frames, make_op, the end-to-end inputs)
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
    assert "kw_fused_second_order_frames_time_pair" in capi._SIG and "kw_second_order_frames_mix_pair" in capi._SIG
    assert hasattr(second_order.SecondOrderFrames, "set_dp0dt")
    return second_order


@pytest.fixture()
def dev(second_order):
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def equal_norm_scale(term_p, term_v):
    """the factor for the second batch: the two terms' float64 norms equal, their inner product non-negative"""
    s = np.linalg.norm(term_p) / np.linalg.norm(term_v)
    return -s if np.vdot(term_p, term_v) < 0 else s


class PairStage:
    """a frames context of (ex, ey, F) with p0's batch transformed once and kept; keep_v forwards a second batch into a kept
    array of its own; time(op) gives every frame of both at one time"""

    def __init__(self, dev, vol_p):
        nf, ey, ex = vol_p.shape
        self.dev = dev
        set_constants(dev, ex, ey, nf)
        dev.call("fused_set_frames", 1)
        ok = C.c_int()
        dev.call("fused_supported", C.byref(ok))
        assert ok.value == 1, (ex, ey, nf)
        dev.call("fused_create")
        n = C.c_size_t()
        dev.call("fused_second_order_frames_elems", C.byref(n))
        self.vol = Guarded(dev, vol_p)
        self.kept_p = Guarded(dev, np.full(2 * n.value, np.nan, F32))
        self.kept_v = Guarded(dev, np.full(2 * n.value, np.nan, F32))
        dev.call("fused_second_order_frames_forward", self.vol.ptr, self.kept_p.ptr)
        dev.sync()
        self.p_bytes = self.kept_p.read().view(np.uint8)
        self.v_bytes = None
        self.out = Guarded(dev, np.full(vol_p.shape, np.nan, F32))

    def keep_v(self, vol_v):
        self.check_kept()
        self.vol.write(vol_v)
        self.dev.call("fused_second_order_frames_forward", self.vol.ptr, self.kept_v.ptr)
        self.dev.sync()
        self.v_bytes = self.kept_v.read().view(np.uint8)

    def time(self, op):
        self.dev.call("fused_second_order_frames_time_pair", self.kept_p.ptr, self.kept_v.ptr, C.byref(op), self.out.ptr)
        self.dev.sync()
        return self.out.read()   # (the guard bands: nothing is stored outside the batch)

    def check_kept(self):
        """both kept arrays are byte-identical after every pair pass"""
        assert np.array_equal(self.kept_p.read().view(np.uint8), self.p_bytes)
        assert self.v_bytes is None or np.array_equal(self.kept_v.read().view(np.uint8), self.v_bytes)

    def close(self):
        self.check_kept()
        self.dev.call("fused_destroy")
        for g in (self.vol, self.kept_p, self.kept_v, self.out):
            g.free()


def pair_case(s, vol_p, raw_v, d, c0, t, coeff, y, zero_p=False):
    """one variant on a PairStage: scale and forward the second batch, run the pair stage; (got, want, |Hs V| / |Hc P| unscaled)"""
    term_p, term_v = dr.frames_terms_expanded(vol_p, raw_v, d, c0, t, coeff, y)
    scale = 1.0 if zero_p else equal_norm_scale(term_p, term_v)
    vol_v = (raw_v.astype(np.float64) * scale).astype(F32)
    term_v = dr.frames_terms_expanded(vol_p, vol_v, d, c0, t, coeff, y)[1]   # of the float32 batch that the device gets
    want = term_p + term_v
    assert np.linalg.norm(want) >= 0.5 * max(np.linalg.norm(term_p), np.linalg.norm(term_v))
    s.keep_v(vol_v)
    return s.time(sib.make_op(d, c0, t, coeff, y)), want, abs(1.0 / scale)


# ---- 1. the fused pair stage at every line length -----------------------------------------------------------------------------
def stage_errors(dev, ex, ey, nf, frame=None):
    d = sr.STAGE_D[:2]
    cases = fr.stage_case((ex, ey))
    assert fr.b_margins((ex, ey), d, sr.STAGE_C0, cases[3][0], sr.STAGE_Y)[0] >= 0.25
    vol_p = sib.source_frames(np.random.default_rng(ex * 1009 + ey * 31 + nf), nf, ey, ex)
    raw_v = sib.source_frames(np.random.default_rng(ex * 1013 + ey * 37 + nf + 5), nf, ey, ex)
    s = PairStage(dev, vol_p)
    errs, alone, ratios = [], [], []
    for coeff, t in cases:
        got, want, ratio = pair_case(s, vol_p, raw_v, d, sr.STAGE_C0, t, coeff, sr.STAGE_Y)
        errs.append(sr.rel_l2(got, want))
        ratios.append(ratio)
        if frame is not None:
            alone.append(sr.rel_l2(got[frame], want[frame]))
    s.close()
    return errs, alone, ratios


@pytest.mark.parametrize("L", LENGTHS)
def test_pair_stage_at_every_line_length(dev, L):
    """(Ex, Ey, F) = (16, L, 3): k_yfused_second_order_pair<L> on one column tile, no side array.  Spacings STAGE_D[:2];
    lossless and absorbing (y = 1.5), near and far (second_order_reference.stage_case on the plane).  Measured: lossless
    1.02e-7 to 1.84e-7 near and 8.3e-8 to 1.93e-7 far; absorbing 9.4e-8 to 1.93e-7 near and 3.4e-8 to 1.27e-7 far."""
    errs, _, ratios = stage_errors(dev, 16, L, 3)
    print(f"second-order frames pair stage 16x{L}x3: rel L2 lossless near {errs[0]:.3e} far {errs[1]:.3e}; absorbing near "
          f"{errs[2]:.3e} far {errs[3]:.3e}  (|Hs V| / |Hc P| unscaled " + " ".join(f"{r:.1e}" for r in ratios) + ")")
    assert max(errs) < PARITY, L


@pytest.mark.parametrize("L", LENGTHS)
def test_pair_stage_at_every_line_length_with_side_blocks(dev, L):
    """(96, L, 17): three main column tiles and the blocks of the x-Nyquist side array [17][L], the last live one partly past
    the last frame; frame 16 alone is held to the bound as well, and the guard bands show that nothing is stored past it.
    Measured: lossless 1.31e-7 to 1.86e-7 near and 1.03e-7 to 1.57e-7 far; absorbing 1.33e-7 to 1.85e-7 near and 4.8e-8 to
    1.15e-7 far; frame 16 alone 1.08e-7 to 3.24e-6 (worst at L = 432: the norms are equalised over the batch, so within one
    frame the two terms may largely cancel).  Unscaled |Hs V| / |Hc P| over both tests: 1.0e-8 to 2.0e-3."""
    errs, last, ratios = stage_errors(dev, 96, L, 17, frame=16)
    print(f"second-order frames pair stage 96x{L}x17: rel L2 lossless near {errs[0]:.3e} far {errs[1]:.3e}; absorbing near "
          f"{errs[2]:.3e} far {errs[3]:.3e}; frame 16 alone worst {max(last):.3e}  (|Hs V| / |Hc P| unscaled " +
          " ".join(f"{r:.1e}" for r in ratios) + ")")
    assert max(errs) < PARITY and max(last) < PARITY, L


# ---- 2. fused pair stage and rocFFT twin ----------------------------------------------------------------------------------------
TWIN = sib.TWIN
# y = 1.5, lossless, Stokes, y = 1.1, and with p0 = 0 lossless and y = 1.5: Hs on its own
VARIANTS = tuple(v + (False,) for v in sib.VARIANTS) + ((0.0, 1.5, True), (0.75, 1.5, True))


def twin_errors(d2, vol_p, raw_v):
    """kw_fft_r2c_frames twice, kw_second_order_frames_mix_pair, kw_fft_c2r_frames, per variant"""
    nf, ey, ex = vol_p.shape
    p = TWIN
    d2.call("second_order_frames_mix_pair", None, None, None, None, C.c_float(1.0))   # no constants, no bins: no pointer is looked at
    set_constants(d2, ex, ey, nf)
    d2.call("fft_create_plans_frames")
    nr = (ex // 2 + 1) * ey * nf
    src = Guarded(d2, vol_p)
    spec_p, spec_v = Guarded(d2, np.zeros(2 * nr, F32)), Guarded(d2, np.zeros(2 * nr, F32))
    mixed, out = Guarded(d2, np.full(2 * nr, np.nan, F32)), Guarded(d2, np.full(vol_p.shape, np.nan, F32))
    errs = []
    for coeff, y, zero_p in VARIANTS:
        vp = np.zeros_like(vol_p) if zero_p else vol_p
        term_p, term_v = dr.frames_terms_expanded(vp, raw_v, p["d"], C0, p["t"], coeff, y)
        scale = 1.0 if zero_p else equal_norm_scale(term_p, term_v)
        vol_v = (raw_v.astype(np.float64) * scale).astype(F32)
        want = dr.frames_solve_expanded(vp, vol_v, p["d"], C0, p["t"], coeff, y)
        src.write(vp)
        d2.call("fft_r2c_frames", src.ptr, spec_p.ptr)
        src.write(vol_v)
        d2.call("fft_r2c_frames", src.ptr, spec_v.ptr)
        d2.sync()
        bytes_p, bytes_v = spec_p.read().view(np.uint8), spec_v.read().view(np.uint8)
        op = sib.make_op(p["d"], C0, p["t"], coeff, y)
        d2.call("second_order_frames_mix_pair", mixed.ptr, spec_p.ptr, spec_v.ptr, C.byref(op), C.c_float(1.0 / (ex * ey)))
        d2.call("fft_c2r_frames", mixed.ptr, out.ptr)
        d2.sync()
        errs.append(sr.rel_l2(out.read(), want))
        # out of place: the spectra are read only
        assert np.array_equal(spec_p.read().view(np.uint8), bytes_p) and np.array_equal(spec_v.read().view(np.uint8), bytes_v)
    for g in (src, spec_p, spec_v, mixed, out):
        g.free()
    return errs


def assert_underdamped(ex, ey):
    for coeff, y, _ in VARIANTS:
        assert coeff == 0.0 or fr.b_margins((ex, ey), TWIN["d"], C0, coeff, y)[0] >= 0.25


def fused_errors(dev, vol_p, raw_v):
    p = TWIN
    errs = []
    for zero in (False, True):   # one context at a time on the device
        vp = np.zeros_like(vol_p) if zero else vol_p
        s = PairStage(dev, vp)
        for coeff, y, zero_p in VARIANTS:
            if zero_p == zero:
                got, want, _ = pair_case(s, vp, raw_v, p["d"], C0, p["t"], coeff, y, zero_p)
                errs.append(sr.rel_l2(got, want))
        s.close()
    return errs


@pytest.mark.parametrize("nf,ey,ex", [(5, 48, 32), (3, 64, 96)])
def test_fused_pair_stage_and_rocfft_twin(dev, nf, ey, ex):
    """dy = 0.8 dx; (3, 64, 96) has the side array.  Measured: fused 9.8e-8 to 1.44e-7, twin 1.20e-7 to 1.59e-7; the twin on
    the odd grid below 1.08e-7 to 1.46e-7."""
    from kwave_amd import capi
    assert_underdamped(ex, ey)
    vol_p = sib.source_frames(np.random.default_rng(nf + ey + ex), nf, ey, ex)
    raw_v = sib.source_frames(np.random.default_rng(nf + ey + ex + 77), nf, ey, ex)
    fused = fused_errors(dev, vol_p, raw_v)
    d2 = capi.Device()
    try:
        twins = twin_errors(d2, vol_p, raw_v)
    finally:
        d2.close()
    print(f"second-order frames pair [{nf}][{ey}][{ex}] (y = 1.5, lossless, Stokes, y = 1.1, p0 = 0 lossless, p0 = 0 y = 1.5): "
          "fused stage " + " ".join(f"{e:.3e}" for e in fused) + "; rocFFT twin " + " ".join(f"{e:.3e}" for e in twins) +
          " (rel L2 against float64)")
    assert max(fused) < PARITY and max(twins) < PARITY


def test_rocfft_twin_on_an_odd_grid(dev):
    nf, ey, ex = 4, 27, 33
    assert_underdamped(ex, ey)
    vol_p = sib.source_frames(np.random.default_rng(2733), nf, ey, ex)
    raw_v = sib.source_frames(np.random.default_rng(3327), nf, ey, ex)
    twins = twin_errors(dev, vol_p, raw_v)
    print(f"second-order frames pair twin [{nf}][{ey}][{ex}]: " + " ".join(f"{e:.3e}" for e in twins))
    assert max(twins) < PARITY


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def test_frames_pair_entry_refuses_every_other_context(dev):
    from kwave_amd import capi
    a = Guarded(dev, np.zeros(2 * 32 * 32 * 16, F32))
    b = Guarded(dev, np.zeros(2 * 32 * 32 * 16, F32))
    out = Guarded(dev, np.zeros(2 * 32 * 32 * 16, F32))
    op = sib.make_op((1e-4, 1e-4), C0, 1e-7, 0.0, 1.5)
    entry = "fused_second_order_frames_time_pair"

    def refused(what):
        with pytest.raises(capi.KWaveError, match="kw_" + entry + ": " + what):
            dev.call(entry, a.ptr, b.ptr, C.byref(op), out.ptr)

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
    # on a frames context: a NULL second spectrum and a dx of 0 are refused
    set_constants(dev, 32, 32, 16)
    dev.call("fused_set_frames", 1)
    dev.call("fused_create")
    with pytest.raises(capi.KWaveError, match="kw_" + entry):
        dev.call(entry, a.ptr, None, C.byref(op), out.ptr)
    bad = sib.make_op((0.0, 1e-4), C0, 1e-7, 0.0, 1.5)
    with pytest.raises(capi.KWaveError, match="kw_" + entry):
        dev.call(entry, a.ptr, b.ptr, C.byref(bad), out.ptr)
    dev.call("fused_destroy")
    dev.sync()
    assert not out.read().any()   # nothing is written by a refused call
    for g in (a, b, out):
        g.free()


# ---- 4. SecondOrderFrames end to end ------------------------------------------------------------------------------------------
E2E_D, E2E_TMAX, E2E_TIMES, E2E_COEFF, E2E_F = sib.E2E_D, sib.E2E_TMAX, sib.E2E_TIMES, sib.E2E_COEFF, sib.E2E_F
RECORDS = sib.RECORDS


def e2e_dp0dt(n, nf, seed):
    """a second batch of the sibling test's kind, in Pa/s: of the size c0 / dx times a pressure, so that both terms count"""
    return (sib.e2e_p0(n, nf, seed) * F32(0.5 * C0 / E2E_D[0])).astype(F32)


@pytest.mark.parametrize("n,fused", [((24, 20), True), ((23, 19), False)], ids=["fused", "rocfft"])
@pytest.mark.parametrize("coeff", [0.0, E2E_COEFF], ids=["lossless", "absorbing"])
def test_second_order_frames_with_dp0dt_against_the_restatement(second_order, coeff, n, fused):
    """Measured: worst field(t) 1.2e-7 to 1.4e-7, field(0) 1.1e-7 to 1.3e-7, p_raw 1.0e-7 to 1.2e-7, p_final 1.0e-7 to 1.1e-7,
    p_rms 5.8e-8 to 7.1e-8."""
    sensors = sib.e2e_sensors(n)
    p = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, alpha_coeff=coeff, alpha_power=1.5, t_max=E2E_TMAX,
                                       sensor_index=sensors, record=RECORDS, fused_kernels=fused)
    try:
        expanded = p.expanded
        assert p.fused == fused and not p.has_dp0dt
        assert coeff == 0.0 or fr.b_margins(expanded, E2E_D, C0, coeff, 1.5)[0] >= 0.25
        p0, v = sib.e2e_p0(n, E2E_F, 1), e2e_dp0dt(n, E2E_F, 11)
        p.set_dp0dt(v)   # (before set_p0: the two are independent)
        assert p.has_dp0dt
        p.set_p0(p0)
        want = dr.frames_solve(p0, v, expanded, E2E_D, C0, E2E_TIMES, coeff, 1.5)
        alone = fr.solve(p0, expanded, E2E_D, C0, E2E_TIMES, coeff, 1.5)
        assert sr.rel_l2(alone[2], want[2]) > 0.1   # the second condition counts in what is compared
        fields = np.array([p.field(t) for t in E2E_TIMES])
        assert fields.dtype == F32 and fields.shape == (12,) + p0.shape
        e_field = max(sr.rel_l2(fields[i], want[i]) for i in range(12))
        e_zero = sr.rel_l2(p.field(0.0), p0)
        rec = p.run(E2E_TIMES)
        assert rec.dtype == F32 and rec.shape == (12, E2E_F, 7) and p.runs == 1
        e_raw = sr.rel_l2(rec, want.reshape(12, E2E_F, -1)[:, :, sensors])
        assert np.array_equal(rec, fields.reshape(12, E2E_F, -1)[:, :, sensors])
        e_final = sr.rel_l2(p.p_final(), want[-1])
        e_rms = sr.rel_l2(p.p_rms(), np.sqrt(np.mean(want ** 2, axis=0)))
        print(f"SecondOrderFrames with dp0dt {n} x {E2E_F} alpha_coeff {coeff} fused {fused} E {expanded}: rel L2 worst field "
              f"{e_field:.3e}, field(0) {e_zero:.3e}, p_raw {e_raw:.3e}, p_final {e_final:.3e}, p_rms {e_rms:.3e}")
        assert max(e_field, e_raw, e_final, e_rms) < PARITY
        assert e_zero < 1e-6
        assert np.array_equal(p.p_max(), fields.max(axis=0)) and np.array_equal(p.p_min(), fields.min(axis=0))
        assert np.array_equal(p.p_final(), fields[-1])
    finally:
        p.close()


# ---- 5. the single path is untouched ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fused", [((24, 20), True), ((23, 19), False)], ids=["fused", "rocfft"])
def test_clearing_dp0dt_gives_the_bits_of_a_propagator_that_never_had_one(second_order, n, fused):
    sensors = sib.e2e_sensors(n)
    kw = dict(alpha_coeff=E2E_COEFF, alpha_power=1.5, t_max=E2E_TMAX, sensor_index=sensors, record=RECORDS, fused_kernels=fused)
    p0, p0b, v = sib.e2e_p0(n, E2E_F, 1), sib.e2e_p0(n, E2E_F, 2), e2e_dp0dt(n, E2E_F, 11)
    t = E2E_TIMES[[2, 5, 7]]
    never = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    try:
        never.set_p0(p0)
        f_never = [never.field(x) for x in t]
        r_never = never.run(E2E_TIMES)
        agg_never = [never.p_max(), never.p_min(), never.p_rms(), never.p_final()]
    finally:
        never.close()
    fresh = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    try:
        fresh.set_p0(p0b)
        fresh.set_dp0dt(v)
        f_fresh = [fresh.field(x) for x in t]
    finally:
        fresh.close()
    p = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    try:
        p.set_p0(p0)
        p.set_dp0dt(v)
        with_v = p.field(t[0])
        assert p.has_dp0dt and not np.array_equal(with_v, f_never[0])
        p.set_dp0dt(None)
        assert not p.has_dp0dt
        for x, want in zip(t, f_never):
            assert np.array_equal(p.field(x), want)
        assert np.array_equal(p.run(E2E_TIMES), r_never)
        for got, want in zip([p.p_max(), p.p_min(), p.p_rms(), p.p_final()], agg_never):
            assert np.array_equal(got, want)
        # set again (the second array is there already), then another p0: the dp0dt is kept
        p.set_dp0dt(v)
        assert np.array_equal(p.field(t[0]), with_v)
        p.set_p0(p0b)
        assert p.has_dp0dt
        for x, want in zip(t, f_fresh):
            assert np.array_equal(p.field(x), want)
        with pytest.raises(ValueError, match=r"dp0dt must be \(F, Ny, Nx\)"):
            p.set_dp0dt(np.zeros((n[1], n[0]), F32))
    finally:
        p.close()


def test_interleaved_propagators_with_and_without_dp0dt(second_order):
    n = (24, 20)
    pa, pb, v = sib.e2e_p0(n, E2E_F, 2), sib.e2e_p0(n, E2E_F, 3), e2e_dp0dt(n, E2E_F, 12)
    t = E2E_TIMES[:4]
    kw = dict(alpha_coeff=E2E_COEFF, t_max=E2E_TMAX)
    alone = []
    for p0, dv in ((pa, v), (pb, None)):
        q = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
        try:
            q.set_p0(p0)
            q.set_dp0dt(dv)
            alone.append([q.field(x) for x in t])
        finally:
            q.close()
    a = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    b = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    try:
        a.set_p0(pa)
        b.set_p0(pb)
        a.set_dp0dt(v)
        for i, x in enumerate(t):
            fa = a.field(x)
            fb = b.field(x)
            assert np.array_equal(fa, alone[0][i]) and np.array_equal(fb, alone[1][i])
    finally:
        a.close()
        b.close()


# ---- 6. the travelling wave ----------------------------------------------------------------------------------------------------
def test_travelling_wave_on_frames(second_order):
    """(32, 16) periodic planes, F = 3 different profiles, lossless: p0_f = f_f(x), dp0dt_f = -c0 df_f/dx; at t = n dx / c0
    every frame is roll(p0_f, n, axis=x) within PARITY plus the restatement's own difference; without dp0dt more than 0.1 off.
    Measured, worst frame, n = 1, 5, 37: 1.8e-7, 2.0e-7, 7.7e-7 (the restatement's own 3.5e-8, 8.6e-8, 1.4e-7); without
    0.67 to 0.71."""
    n, d = (32, 16), (1.0e-4, 1.0e-4)
    pairs = [dr.wave_inputs((16, 32), d[0], C0, seed) for seed in (0, 1, 2)]
    p0, v = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    assert not np.array_equal(p0[0], p0[1]) and not np.array_equal(p0[1], p0[2])
    p = second_order.SecondOrderFrames(n, d, C0, 3, expanded=n)
    try:
        assert p.fused and p.expanded == n
        p.set_p0(p0)
        for with_v in (True, False):
            p.set_dp0dt(v if with_v else None)
            for steps in (1, 5, 37):
                t = steps * d[0] / C0
                want = np.roll(p0.astype(np.float64), steps, axis=2)
                got = p.field(t)
                err = max(sr.rel_l2(got[f], want[f]) for f in range(3))
                own = max(sr.rel_l2(dr.frames_solve(p0, v, n, d, C0, [t])[0][f], want[f]) for f in range(3))
                print(f"frames travelling wave n = {steps}, dp0dt {with_v}: GPU against roll(p0, n), worst frame {err:.3e}; the "
                      f"restatement's own {own:.3e}")
                if with_v:
                    assert err <= PARITY + own
                else:
                    assert min(sr.rel_l2(got[f], want[f]) for f in range(3)) > 0.1
    finally:
        p.close()


# ---- 7. the line record ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rocfft"])
def test_line_record_is_refused_while_a_dp0dt_is_set(second_order, fused):
    from kwave_amd import capi
    n = (24, 20) if fused else (23, 19)
    kw = dict(alpha_coeff=E2E_COEFF, t_max=E2E_TMAX, line_row=7, fused_kernels=fused)
    p0, v = sib.e2e_p0(n, E2E_F, 1), e2e_dp0dt(n, E2E_F, 11)
    never = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    try:
        never.set_p0(p0)
        want = never.line_record(E2E_TIMES)
    finally:
        never.close()
    p = second_order.SecondOrderFrames(n, E2E_D, C0, E2E_F, **kw)
    try:
        assert p.fused == fused
        p.set_p0(p0)
        p.set_dp0dt(v)
        with pytest.raises(capi.KWaveError, match=r"line_record: a dp0dt is set.*run\(times\)"):
            p.line_record(E2E_TIMES)
        p.field(E2E_TIMES[2])   # (the pair path runs in between)
        p.set_dp0dt(None)
        assert np.array_equal(p.line_record(E2E_TIMES), want)
    finally:
        p.close()
