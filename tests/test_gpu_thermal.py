"""Bioheat solver on the GPU: kw_thermal_update and kw_thermal_dose on their own against float64 of the same float32 inputs,
and the solver (kwave_amd.thermal.ThermalSolver) against the float64 NumPy restatement of tests/thermal_reference.py on

  * 16 x 32 x 48 with fused_kernels on  — the hand-written FFT pipeline (three different sides catch axis mix-ups),
  * 16 x 32 x 48 with fused_kernels off — rocFFT and the granular kernels on the same grid,
  * 24 x 20 x 18                        — rocFFT: none of the sides is a fast-path length.

Bounds.  Solver level: 1e-5 relative L2, the project's parity bound (tests/test_thermal_host.py shows the float32
restatement alone at 6e-8 on the heterogeneous case).  kw_thermal_update, per element:
    |T - T64| <= 8 * 2^-24 * M,   M = |T_in| + dt * (|diff_scale * a| * (|d0| + |d1| + |d2|) + |P * (T_in - T_a)| + |a * Q|)
from the kernel's association order  s = (d0 + d1) + d2;  r = (diff_scale * a) * s;  r = fma(-P, T - T_a, r);
r = fma(a, Q, r);  T = fma(dt, r, T):  each rounding is at most 2^-24 of a partial result, and a partial result is at
most the part of M it has gathered so far.  The diffusion part passes through 7 roundings (2 in s, 1 in diff_scale * a,
1 in the product, 3 fma), the perfusion part through 4, the source part through 2 and T_in through 1: at most 7 * 2^-24 * M
to first order, inside the bound of 8.  kw_thermal_dose, per element: (4 + |s * (T - 43)|) * 2^-23 relative — dt / 60, exp2f
and the product are within 4 * 2^-23 together, and the fp32 rounding of the argument s * (T - 43) moves the power by
ln 2 * 2^-24 * |s * (T - 43)| relative."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import thermal_reference as tr  # noqa: E402
from gpu_buffers import run  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
PARITY = 1e-5
D0 = tr.K0 / (tr.RHO0 * tr.C0)
CONFIGS = [pytest.param(tr.FUSED_GRID, True, id="16x32x48-fused"), pytest.param(tr.FUSED_GRID, False, id="16x32x48-rocfft"),
           pytest.param(tr.ROCFFT_GRID, True, id="24x20x18-rocfft")]
SIZES = [1, 3, 4, 5, 255, 256, 257, 1027, "n_big"]


@pytest.fixture(scope="module")
def thermal():
    import kwave_amd  # noqa: F401
    from kwave_amd import thermal
    return thermal


@pytest.fixture(scope="module")
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    d.close()


def make_solver(thermal, pr, dims, fused, **opts):
    s = thermal.ThermalSolver(pr, fused_kernels=fused, **opts)
    assert s.fused == (fused and dims == tr.FUSED_GRID)   # the path the case is meant to take
    return s


# ---- references, computed once -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mode_case(dims, flux, past_euler):
    pr = tr.mode_problem(dims, flux, (10.0 if past_euler else 0.5) * tr.euler_limit(dims, D0))
    return pr, tr.mode_decay(pr, 10)


@functools.lru_cache(maxsize=None)
def het_case(dims):
    pr = tr.heterogeneous_problem(dims)
    return pr, tr.Reference(pr).run(tr.HET_STEPS).T


@functools.lru_cache(maxsize=None)
def heat_case(dims):
    pr = tr.heating_problem(dims)
    r64 = tr.Reference(pr).run(tr.HEAT_STEPS).run(tr.HEAT_STEPS, heat_on=False)
    r32 = tr.Reference(pr, np.float32).run(tr.HEAT_STEPS).run(tr.HEAT_STEPS, heat_on=False)
    floor = max(float(np.max(np.abs(r32.T - r64.T))), float(np.max(np.abs(r32.T_max - r64.T_max))))
    return pr, r64, floor


HET_GPU = {}  # (dims, fused) -> T of the heterogeneous case on the GPU, shared by the parity and the cross-path test


def het_gpu(thermal, dims, fused):
    if (dims, fused) not in HET_GPU:
        s = make_solver(thermal, het_case(dims)[0], dims, fused)
        s.run(tr.HET_STEPS)
        HET_GPU[(dims, fused)] = s.T
        s.close()
    return HET_GPU[(dims, fused)]


# ---- 1. mode decay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,fused", CONFIGS)
@pytest.mark.parametrize("past_euler", [False, True], ids=["stable_dt", "ten_times_euler_limit"])
@pytest.mark.parametrize("flux", [False, True], ids=["laplacian", "flux"])
def test_mode_decay(thermal, dims, fused, past_euler, flux):
    """ambient 0, amplitude 1, one mode, 10 steps: within 1e-5 relative L2 of T0 exp(-D |k|^2 dt n)"""
    pr, want = mode_case(dims, flux, past_euler)
    s = make_solver(thermal, pr, dims, fused)
    s.run(10)
    got = s.T
    s.close()
    err = tr.rel_l2(got, want)
    print(f"mode decay {dims} fused={fused} flux={flux} past_euler={past_euler}: rel L2 {err:.3e}")
    assert err < PARITY


# ---- 2. heterogeneous parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,fused", CONFIGS)
def test_heterogeneous_parity(thermal, dims, fused):
    """K, rho, C with contrast 3, array perfusion, a Gaussian Q, 10 steps: within 1e-5 relative L2 of float64"""
    got = het_gpu(thermal, dims, fused)
    err = tr.rel_l2(got, het_case(dims)[1])
    print(f"heterogeneous {dims} fused={fused}: rel L2 {err:.3e}")
    assert err < PARITY


def test_fused_and_rocfft_paths_agree(thermal):
    """the two paths on the same grid: each is within 1e-5 of one reference, so within 2e-5 of each other"""
    a, b = het_gpu(thermal, tr.FUSED_GRID, True), het_gpu(thermal, tr.FUSED_GRID, False)
    err = tr.rel_l2(a, b)
    print(f"fused against rocFFT path: rel L2 {err:.3e}")
    assert err < 2 * PARITY
    assert not np.array_equal(a, b)   # two different FFT implementations were compared


# ---- 3. heating, then cooling ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,fused", CONFIGS)
def test_heating_then_cooling(thermal, dims, fused):
    """T0 = T_a = 37, Q on for 10 steps and off for 10.  T and T_max may differ from float64 by 4 x the absolute distance of
    the float32 restatement from float64 on this case (the factor: another summation order in the GPU's FFT); the measured
    floor is 1.3e-5 K at 16 x 32 x 48 and at 24 x 20 x 18, a few float32 spacings at 45 degC (3.8e-6); the GPU: 1.2e-5 K.  cem43
    within 1e-4 relative where it exceeds 1e-3 of its maximum: looser than T on purpose, a T error e changes an increment by
    ln 2 * s * e."""
    pr, ref, floor = heat_case(dims)
    assert ref.T_max.max() > 43.5 and ref.T.max() < ref.T_max.max()    # past 43 degC at the focus, cooler at the end
    s = make_solver(thermal, pr, dims, fused, t_max=True)
    s.run(tr.HEAT_STEPS, heat_on=True)
    s.run(tr.HEAT_STEPS, heat_on=False)
    assert s.t == 2 * tr.HEAT_STEPS
    T, T_max, cem = s.T, s.T_max, s.cem43
    e_T, e_max = float(np.max(np.abs(T - ref.T))), float(np.max(np.abs(T_max - ref.T_max)))
    big = ref.cem43 > 1e-3 * ref.cem43.max()
    e_cem = float(np.max(np.abs(cem - ref.cem43)[big] / ref.cem43[big]))
    print(f"heating {dims} fused={fused}: |T| {e_T:.3e} |T_max| {e_max:.3e} (float32 floor {floor:.3e}), cem43 rel {e_cem:.3e}")
    assert e_T <= 4 * floor and e_max <= 4 * floor
    assert big.sum() > 20 and e_cem < 1e-4
    # the lesion volume is the count of the GPU's own cem43 times the cell volume
    threshold = float(0.25 * cem.max())
    count = int(np.count_nonzero(cem >= F32(threshold)))
    cell = float(np.prod([np.float64(F32(d)) for d in tr.SPACING]))
    assert count > 0 and s.lesion_volume(threshold) == pytest.approx(count * cell, rel=1e-12)
    assert s.lesion_volume(240.0) == 0.0 and s.lesion_volume(0.0) == pytest.approx(cem.size * cell, rel=1e-12)
    s.close()


@pytest.mark.parametrize("dims,fused", CONFIGS)
@pytest.mark.parametrize("flux", [False, True], ids=["laplacian", "flux"])
def test_uniform_temperature_without_source_or_perfusion_does_not_move(thermal, dims, fused, flux):
    """heat_on = False from the start, P = 0, uniform T0: T stays bit-identical to T0"""
    pr = tr.mode_problem(dims, flux, 0.5 * tr.euler_limit(dims, D0))
    pr["T0"] = np.array([[[37.3]]], F32)
    pr["Q"] = tr.heating_problem(dims)["Q"]
    s = make_solver(thermal, pr, dims, fused)
    s.run(5, heat_on=False)
    T = s.T
    s.close()
    assert np.array_equal(T.view(np.uint32), np.full(T.shape, 37.3, F32).view(np.uint32))


# ---- 4. kw_thermal_update alone ----------------------------------------------------------------------------------------
def big_size(dev):
    """past one pass of the update kernel's capped grid: CU count x 8 blocks (kBlocksPerCu of csrc/kw_thermal.hip) of 256
    threads with 4 elements each, ragged"""
    cap = dev.info().compute_units * 8 * 256 * 4
    return cap + 4 * 257 + 3


def update_inputs(n, seed):
    rng = np.random.default_rng(seed)
    f = lambda lo, hi: rng.uniform(lo, hi, n).astype(F32)  # noqa: E731
    return {"T": f(30, 50), "cem43": f(0, 5), "T_max": f(30, 50), "d0": (rng.standard_normal(n) * 2e7).astype(F32),
            "d1": (rng.standard_normal(n) * 2e7).astype(F32), "d2": (rng.standard_normal(n) * 2e7).astype(F32),
            "a": f(1.4e-7, 4.2e-7), "P": f(0.0, 0.05), "T_a": f(36, 38), "Q": f(0, 2e7)}


SCALARS = {"a": F32(2.9e-7), "P": F32(0.013), "T_a": F32(36.6)}
DIFF_SCALE, DT = F32(0.55), F32(0.2)


def update_once(dev, h, flux, arrays, with_q, with_tmax, heat_on=1, offset=0):
    """one kw_thermal_update call through guarded buffers; returns (outputs, T64, M)"""
    n = h["T"].size
    arr = lambda name, on: (name, h[name], True) if on else (name, None, True)  # noqa: E731
    items = [("T", h["T"], False, offset), ("cem43", h["cem43"], False),
             ("T_max", h["T_max"] if with_tmax else None, False), ("d0", h["d0"], True), arr("d1", flux), arr("d2", flux),
             float(DIFF_SCALE), arr("a", "a" in arrays), float(SCALARS["a"]), arr("P", "P" in arrays), float(SCALARS["P"]),
             arr("T_a", "T_a" in arrays), float(SCALARS["T_a"]), arr("Q", with_q), float(DT), heat_on, n]
    out = run(dev, "thermal_update", items)
    g = lambda name: (h[name] if name in arrays else np.full(n, SCALARS[name], F32)).astype(np.float64)  # noqa: E731
    T, a, P, Ta = h["T"].astype(np.float64), g("a"), g("P"), g("T_a")
    d = [h["d0"].astype(np.float64)] + ([h["d1"].astype(np.float64), h["d2"].astype(np.float64)] if flux else [])
    q = h["Q"].astype(np.float64) if (with_q and heat_on) else np.zeros(n)
    ds, dt = float(DIFF_SCALE), float(DT)
    T64 = T + dt * (ds * a * sum(d) - P * (T - Ta) + a * q)
    M = np.abs(T) + dt * (np.abs(ds * a) * sum(np.abs(x) for x in d) + np.abs(P * (T - Ta)) + np.abs(a * q))
    return out, T64, M


def check_update(label, h, out, T64, M, with_tmax):
    T = out["T"].astype(np.float64)
    ratio = np.abs(T - T64) / (U * M)
    assert ratio.max() <= 8.0, f"{label}: |T - T64| = {ratio.max():.2f} x 2^-24 M at {int(ratio.argmax())}"
    # the dose and the maximum are taken from the updated T: checked against the T the kernel wrote
    s = np.where(T >= 43, 1.0, 2.0)
    inc = tr.dose_increment(T, float(DT))
    cem_in = h["cem43"].astype(np.float64)
    tol = (4 + np.abs(s * (T - 43))) * 2.0 ** -23 * inc + U * (cem_in + inc) * 1.01
    assert np.all(np.abs(out["cem43"].astype(np.float64) - (cem_in + inc)) <= tol), f"{label}: cem43"
    assert np.all(out["cem43"][T < 37] == h["cem43"][T < 37]), f"{label}: dose below 37"
    if with_tmax:
        assert np.array_equal(out["T_max"], np.maximum(h["T_max"], out["T"])), f"{label}: T_max"
    else:
        assert "T_max" not in out
    return float(ratio.max())


@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_against_float64(dev, n):
    """every array / scalar combination of a, P, T_a, with and without Q and T_max, one and three divergence arrays, at
    sizes around the 16-byte groups and the block, and past one pass of the capped grid; a misaligned T takes the
    element-by-element kernel.  Guard bands either side of every buffer stay untouched (gpu_buffers.Guarded)."""
    big = n == "n_big"
    n = big_size(dev) if big else n
    h = update_inputs(n, 11 + n % 1000)
    subsets = [(), ("a",), ("P",), ("T_a",), ("a", "P"), ("a", "T_a"), ("P", "T_a"), ("a", "P", "T_a")]
    combos = [(flux, arrays, q, tm) for flux in (False, True) for arrays in subsets for q in (False, True) for tm in (False, True)]
    if big:  # the grid-stride loop does not depend on the mask: both ends of it, in both kernels
        combos = [(True, ("a", "P", "T_a"), True, True), (False, (), False, False)]
    worst = 0.0
    for flux, arrays, q, tm in combos:
        out, T64, M = update_once(dev, h, flux, arrays, q, tm)
        worst = max(worst, check_update(f"n={n} flux={flux} arrays={arrays} Q={q} T_max={tm}", h, out, T64, M, tm))
    # a pointer that is not 16-byte aligned: the element-by-element kernel (its grid cap is a quarter of the elements)
    out, T64, M = update_once(dev, h, True, ("a", "P", "T_a"), True, True, offset=4)
    worst = max(worst, check_update(f"n={n} misaligned", h, out, T64, M, True))
    # heat_on = 0 with Q given is Q = NULL, bit for bit
    off, _, _ = update_once(dev, h, True, ("a",), True, True, heat_on=0)
    none, T64, M = update_once(dev, h, True, ("a",), False, True)
    assert all(np.array_equal(off[k].view(np.uint32), none[k].view(np.uint32)) for k in ("T", "cem43", "T_max"))
    check_update(f"n={n} heat off", h, off, T64, M, True)
    print(f"kw_thermal_update n={n}: worst |T - T64| = {worst:.2f} x 2^-24 M (bound 8)")


def test_zero_size_looks_at_no_pointer(dev):
    from kwave_amd import capi
    assert dev.L.kw_thermal_update(dev.ctx, None, None, None, None, None, None, 1.0, None, 1.0, None, 0.0, None, 0.0, None,
                                   0.1, 1, 0) == 0
    assert dev.L.kw_thermal_dose(dev.ctx, None, None, 0.1, 0) == 0
    # and a NULL state with work to do is refused, not dereferenced
    assert dev.L.kw_thermal_update(dev.ctx, None, None, None, None, None, None, 1.0, None, 1.0, None, 0.0, None, 0.0, None,
                                   0.1, 1, 8) == 1
    assert b"kw_thermal_update" in capi.load().kw_last_error()


# ---- 5. kw_thermal_dose alone ------------------------------------------------------------------------------------------
DOSE_T = np.array([36.999, 37.0, 42.999, 43.0, 43.001, 60.0, 100.0], dtype=F32)


@pytest.mark.parametrize("n", SIZES)
def test_dose_kernel_against_float64(dev, n):
    n = big_size(dev) if n == "n_big" else n
    T = np.resize(np.roll(DOSE_T, n % 7), n).astype(F32)
    dt = F32(0.37)
    for offset in (0, 4):
        out = run(dev, "thermal_dose", [("cem43", np.zeros(n, F32), False, offset), ("T", T, True), float(dt), n])["cem43"]
        T64 = T.astype(np.float64)
        want = tr.dose_increment(T64, float(dt))
        s = np.where(T64 >= 43, 1.0, 2.0)
        assert np.all(out[T < 37] == 0.0) and np.all(np.signbit(out) == 0)
        live = T >= 37
        rel = np.abs(out.astype(np.float64) - want)[live] / want[live]
        assert np.all(rel <= ((4 + np.abs(s * (T64 - 43))) * 2.0 ** -23)[live]), f"n={n} offset={offset}: {rel.max():.3e}"
    # a second call adds to what is there
    twice = run(dev, "thermal_dose", [("cem43", out, False), ("T", T, True), float(dt), n])["cem43"]
    assert np.array_equal(twice, out + out)


# ---- 6. the sensor stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,fused", CONFIGS)
def test_sensor_series_is_the_temperature_read_back(thermal, dims, fused):
    """T_raw at a handful of points equals T read back after each step, bit for bit"""
    pr = dict(het_case(dims)[0])
    n = int(np.prod(dims))
    index = np.array([1, 2, dims[0] + 1, n // 2, n - dims[0], n], dtype=np.uint64)   # 1-based, corners and interior
    pr["sensor_mask_index"] = index.reshape(1, 1, -1)
    s = make_solver(thermal, pr, dims, fused)
    rows = []
    for step in range(4):
        s.run(1, heat_on=step % 2 == 0)
        rows.append(s.T.reshape(-1)[index.astype(np.int64) - 1])
    series = s.series("T_raw")
    s.close()
    assert series.shape == (4, index.size)
    assert np.array_equal(series.view(np.uint32), np.array(rows).view(np.uint32))
    assert not np.array_equal(series[0], series[3])
