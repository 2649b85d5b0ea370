"""Exact k-space propagator, CPU side: the NumPy restatement (tests/second_order_reference.py) against the K1 closed form
of the oracle, its absorbing H against the matrix exponential of the mode's own equation and against the plane-wave
amplitude decay; the inputs of the GPU stage test against the damping rule; the size rules and every refusal through
kwh_second_order_plan without a device; the host code in a stand-alone program built with AddressSanitizer and UBSan;
and the declarations.  No GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import cw_reference as cr  # noqa: E402
import second_order_reference as sr  # noqa: E402

C0 = 1500.0
ENTRY_POINTS = {"kw_fused_second_order_elems", "kw_fused_second_order_forward", "kw_fused_second_order_time",
                "kw_second_order_mix"}


@pytest.fixture(scope="module", autouse=True)
def second_order():
    """without the propagator's entry points nothing in this file passes"""
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, second_order
    assert ENTRY_POINTS <= set(capi._SIG)
    return second_order


# ---- 1. the restatement -------------------------------------------------------------------------------------------------
def test_lossless_restatement_is_the_k1_closed_form():
    """12 x 10 x 8 periodic box, three unequal spacings: solve(expanded = N) at n dt against oracle closed_form_pressure"""
    from oracle import kwave_np
    nx, ny, nz = 12, 10, 8
    d = (1.0e-4, 0.8e-4, 1.3e-4)
    dt = 0.3 * min(d) / C0
    p0 = np.random.default_rng(20261020).standard_normal((nz, ny, nx))
    pr = dict(Nx=nx, Ny=ny, Nz=nz, dx=d[0], dy=d[1], dz=d[2], c0=C0, dt=dt, p0_source_input=p0)
    for n in (0, 1, 7, 250):
        want = kwave_np.closed_form_pressure(pr, n)
        got = sr.solve(p0, (nx, ny, nz), d, C0, [n * dt])[0]
        err = sr.rel_l2(got, want)
        print(f"restatement against K1 at n = {n}: {err:.3e}")
        assert err <= 1e-12


@pytest.mark.parametrize("y", [1.1, 1.5, 2.0, 0.5])
def test_absorbing_h_is_the_matrix_exponential_of_the_mode(y):
    """every non-zero bin of a 16 x 12 x 10 grid: H against the first component of exp(A t) (1, 0)^T, A = [[0, 1], [-Omega^2,
    -2 gamma]], through numpy.linalg.eig.  A is taken in the mode's own time unit 1 / (c0 |k|) — A = [[0, 1], [-(1 - 2 g T),
    -2 g]], t' = c0 |k| t — so that its entries are O(1) and the eigenvectors well scaled.  The coefficient puts the
    largest g of the grid at 0.3: B >= 0.31 for y = 0.5 (T = 1), above 1 for the others."""
    expanded, d = (16, 12, 10), (1.0e-4, 0.8e-4, 1.3e-4)
    k = sr.wavenumbers(expanded, d)
    nzb = k > 0
    g1 = sr.damping(k[nzb], C0, 1.0, y)[0]
    coeff = 0.3 / g1.max()
    assert sr.b_margins(expanded, d, C0, coeff, y)[0] >= 0.25
    g = coeff * g1
    T = sr.tangent(y)
    A = np.zeros((g.size, 2, 2))
    A[:, 0, 1] = 1.0
    A[:, 1, 0] = -(1.0 - 2.0 * g * T)
    A[:, 1, 1] = -2.0 * g
    lam, V = np.linalg.eig(A)
    coef = np.linalg.solve(V, np.tile(np.array([1.0, 0.0]), (g.size, 1))[..., None])[..., 0]
    for t in (0.0, 3.1e-8, 2.7e-7):
        tp = C0 * k[nzb] * t
        first = np.sum(V[:, 0, :] * np.exp(lam * tp[:, None]) * coef, axis=1)
        got = sr.H_of_k(k, C0, t, coeff, y)
        assert np.all(got[~nzb] == 1.0)
        err = float(np.abs(got[nzb] - first.real).max())
        print(f"absorbing H against exp(A t), y = {y}, t = {t}: max |dH| {err:.3e}, max |imag| {np.abs(first.imag).max():.3e}")
        assert err <= 1e-9 and np.abs(first.imag).max() <= 1e-9


def test_plane_wave_amplitude_decays_as_alpha_c0_t():
    """p0 = cos(k x) in the periodic box: after n = 3 lossless periods t_n = 2 pi n / (c0 k) the mode's amplitude is
    exp(-alpha c0 t_n), alpha = a (c0 k)^y [Np/m], to first order in g.  H(t_n) = exp(-gamma t_n) (cos(2 pi n r) + (g / r)
    sin(2 pi n r)) with gamma t = alpha c0 t exactly and r - 1 = -g T + O(g^2): the bracket is off 1 by at most
    ((2 pi n T)^2 / 2 + 2 pi n |T| + 1) g^2 plus higher orders — the bound below, doubled for those."""
    n, d, y, coeff, periods = (32, 8, 8), (1.0e-4, 1.0e-4, 1.0e-4), 1.5, 0.75, 3
    m = 4
    k = 2.0 * math.pi * m / (n[0] * d[0])
    x = np.arange(n[0]) * d[0]
    p0 = np.broadcast_to(np.cos(k * x), (n[2], n[1], n[0])).copy()
    t = 2.0 * math.pi * periods / (C0 * k)
    p = sr.solve(p0, n, d, C0, [t], coeff, y)[0]
    amplitude = 2.0 * np.fft.rfft(p[0, 0])[m].real / n[0]
    alpha = sr.neper(coeff, y) * (C0 * k) ** y
    g = float(sr.damping(np.array([k]), C0, coeff, y)[0][0])
    T = abs(sr.tangent(y))
    bound = 2.0 * ((2.0 * math.pi * periods * T) ** 2 / 2.0 + 2.0 * math.pi * periods * T + 1.0) * g * g
    ratio = amplitude / math.exp(-alpha * C0 * t)
    print(f"plane wave: amplitude {amplitude:.9f}, exp(-alpha c0 t) {math.exp(-alpha * C0 * t):.9f}, g {g:.3e}, bound {bound:.3e}")
    assert 0.0 < g < 0.01 and abs(ratio - 1.0) <= bound


def test_gpu_stage_inputs_keep_every_mode_underdamped():
    """the numbers of tests/test_gpu_second_order.py's stage test at every fast-path length: B >= 1/4 on every non-zero bin,
    the far time at 10^4 turns of the largest |k|, and a slowest mode that keeps exp(-2)"""
    for L in cr.fast_lengths():
        for expanded in ((L, 16, 16), (16, 16, L), (96, 16, L)):
            cases = sr.stage_case(expanded)
            coeff, t_far = cases[3]
            assert cases[0][0] == 0.0 and cases[1] == (0.0, t_far) and cases[2][0] == coeff
            lowest, at_smallest, at_largest = sr.b_margins(expanded, sr.STAGE_D, sr.STAGE_C0, coeff, sr.STAGE_Y)
            assert lowest >= 0.25 and lowest == pytest.approx(min(at_smallest, at_largest), rel=1e-12), expanded
            k = sr.wavenumbers(expanded, sr.STAGE_D)
            assert sr.STAGE_C0 * k.max() * t_far / (2.0 * math.pi) == pytest.approx(1.0e4, rel=1e-12)
            g = sr.damping(k[k > 0].min(), sr.STAGE_C0, coeff, sr.STAGE_Y)[0]
            assert sr.STAGE_C0 * k[k > 0].min() * g * t_far == pytest.approx(2.0, rel=1e-12)
            assert sr.STAGE_C0 * cases[0][1] == pytest.approx(0.37 * min(sr.STAGE_D))


def test_a_float32_phase_would_fail_the_far_time_of_the_stage_test():
    """the lossless far-time variant on (96, 16, 64): the phase c0 |k| t formed in float32 puts the field 1.6e-3 off float64
    — the stage test's bound of 1e-5 tells the phase word from it.  (The absorbing far time does not: the modes with many
    turns have decayed.)"""
    e = (96, 16, 64)
    t = sr.stage_case(e)[1][1]
    vol = np.random.default_rng(9664).standard_normal((e[2], e[1], e[0]))
    X = np.fft.rfftn(vol, axes=(0, 1, 2))
    k = sr.wavenumbers(e, sr.STAGE_D)
    ph32 = (np.float32(sr.STAGE_C0) * k.astype(np.float32) * np.float32(t)).astype(np.float64)
    want = np.fft.irfftn(X * sr.H_of_k(k, sr.STAGE_C0, t), s=vol.shape, axes=(0, 1, 2))
    got = np.fft.irfftn(X * np.cos(ph32), s=vol.shape, axes=(0, 1, 2))
    err = sr.rel_l2(got, want)
    print(f"float32 phase at 10^4 turns: {err:.3e}")
    assert err > 1e-4


# ---- 2. the rules and the refusals, through kwh_second_order_plan without a device ----------------------------------------
D3 = (1.0e-4, 1.2e-4, 0.9e-4)
RULE_TABLE = [  # n, t_max, fused -> expanded, fast.  c0 t_max = 1.545 mm: 15.45, 12.875 and 17.17 points, so 16, 13 and 18 more
    ((24, 20, 18), 1.03e-6, True, (48, 48, 48), True),       # 40, 33, 36 -> 48 each
    ((24, 20, 18), 1.03e-6, False, (40, 33, 36), False),
    ((23, 19, 17), 1.03e-6, False, (39, 32, 35), False),     # odd sizes: the twin path
    ((100, 16, 16), 1.03e-6, True, (120, 32, 48), True),     # 116 -> 120, 29 -> 32, 34 -> 48
    ((1020, 16, 16), 1.03e-6, True, (1036, 32, 48), False),  # no fast length above 1024: the number itself on that axis
]


@pytest.mark.parametrize("n,t_max,fused,expanded,fast", RULE_TABLE)
def test_default_sides_follow_the_rule(second_order, n, t_max, fused, expanded, fast):
    got = second_order.SecondOrder.plan(n, D3, C0, t_max=t_max, fused_kernels=fused)
    assert got == (expanded, fast)
    assert got[0] == sr.default_sides(n, D3, C0, t_max, fused, cr.fast_lengths())


def test_given_sides_are_kept(second_order):
    plan = second_order.SecondOrder.plan
    assert plan((24, 20, 18), D3, C0, expanded=(24, 20, 18)) == ((24, 20, 18), False)        # the periodic box of K1
    assert plan((32, 32, 32), D3, C0, expanded=(32, 32, 32)) == ((32, 32, 32), True)
    assert plan((24, 20, 18), D3, C0, expanded=(32, 48, 64), t_max=1.0) == ((32, 48, 64), True)   # t_max is not read
    assert plan((24, 20, 18), D3, C0, expanded=(27, 20, 33)) == ((27, 20, 33), False)        # odd sides: the twin path
    assert plan((24, 20, 18), D3, C0, expanded=(32, 48, 64), fused_kernels=False) == ((32, 48, 64), False)


REFUSALS = [
    (dict(n=(0, 20, 18)), "Nx: 0 is not a grid size"),
    (dict(n=(24, 0, 18)), "Ny: 0 is not a grid size"),
    (dict(n=(24, 20, 0)), "Nz: 0 is not a grid size"),
    (dict(d=(0.0, 1e-4, 1e-4)), "dx: 0.000000 is not a positive spacing"),
    (dict(d=(1e-4, float("nan"), 1e-4)), "dy: nan is not a positive spacing"),
    (dict(d=(1e-4, 1e-4, -1.0)), "dz: -1.000000 is not a positive spacing"),
    (dict(c0=0.0), "c0: 0.000000 is not a positive sound speed"),
    (dict(t_max=None), "t_max: 0.000000 is not a positive time (the default expanded sides are sized by it)"),
    (dict(t_max=-1.0), "t_max: -1.000000 is not a positive time (the default expanded sides are sized by it)"),
    (dict(t_max=float("inf")), "t_max: inf is not a positive time (the default expanded sides are sized by it)"),
    (dict(alpha_coeff=-1.0), "alpha_coeff: -1.000000 is not an absorption >= 0 in dB/(MHz^y cm)"),
    (dict(alpha_coeff=0.75, alpha_power=1.0), "alpha_power: 1.000000 is outside the power law's range 0 <= y < 3, y != 1"),
    (dict(alpha_power=3.0), "alpha_power: 3.000000 is outside the power law's range 0 <= y < 3, y != 1"),
    (dict(alpha_power=-0.5), "alpha_power: -0.500000 is outside the power law's range 0 <= y < 3, y != 1"),
    (dict(expanded=(48, 0, 48)), "Ey: missing while the other side of the expanded grid is given"),
    (dict(expanded=(48, 48, 0)), "Ez: missing while the other sides of the expanded grid are given"),
    (dict(expanded=(23, 48, 48)), "Ex: 23 is below N = 24"),
    (dict(expanded=(48, 48, 17)), "Ez: 17 is below N = 18"),
    (dict(expanded=(2048, 2048, 1024)), "E: 2048 x 2048 x 1024 points is not below 2^32"),
    (dict(sensor_index=[0, 8640]), "sensor_index: sensor_index[1] = 8640 is outside the domain of 8640 points"),
    (dict(alpha_coeff=500.0), "alpha_coeff: 500.000000: a mode of this grid is damped beyond B = 1/4 (B = %.6f at the largest |k|)"
     % sr.b_margins((48, 48, 48), D3, C0, 500.0, 1.5)[2]),
    (dict(alpha_coeff=100.0, alpha_power=0.5),
     "alpha_coeff: 100.000000: a mode of this grid is damped beyond B = 1/4 (B = %.6f at the smallest non-zero |k|)"
     % sr.b_margins((48, 48, 48), D3, C0, 100.0, 0.5)[1]),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(":")[0] + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_every_refusal_names_its_parameter(second_order, change, message):
    from kwave_amd import capi
    args = dict(n=(24, 20, 18), d=D3, c0=C0, t_max=1.03e-6)
    args.update(change)
    with pytest.raises(capi.KWaveError) as e:
        second_order.SecondOrder.plan(**args)
    assert str(e.value) == message
    with pytest.raises(capi.KWaveError) as e:   # the same from create, before any device is looked for
        second_order.SecondOrder(**args)
    assert str(e.value) == message


def test_damping_rule(second_order):
    """0.75 dB/(MHz^1.5 cm) on a 0.1 mm grid passes; a coefficient that puts B at 0.2 at the grid's largest |k| is refused,
    one that puts it at 0.3 passes"""
    from kwave_amd import capi
    plan = second_order.SecondOrder.plan
    n, d, e = (24, 24, 24), (1.0e-4, 1.0e-4, 1.0e-4), (48, 48, 48)
    assert plan(n, d, C0, alpha_coeff=0.75, alpha_power=1.5, expanded=e) == (e, True)
    assert sr.b_margins(e, d, C0, 0.75, 1.5)[0] >= 0.25
    bad = sr.coeff_for_b(e, d, C0, 1.5, 0.2)
    assert sr.b_margins(e, d, C0, bad, 1.5)[2] == pytest.approx(0.2, abs=1e-12)
    with pytest.raises(capi.KWaveError) as err:
        plan(n, d, C0, alpha_coeff=bad, alpha_power=1.5, expanded=e)
    assert str(err.value).startswith("alpha_coeff: ")
    assert str(err.value).endswith(": a mode of this grid is damped beyond B = 1/4 (B = 0.200000 at the largest |k|)")
    assert plan(n, d, C0, alpha_coeff=sr.coeff_for_b(e, d, C0, 1.5, 0.3), alpha_power=1.5, expanded=e) == (e, True)
    # Stokes: T = 0, B = 1 - g^2
    stokes = sr.coeff_for_b(e, d, C0, 2.0, 0.2)
    with pytest.raises(capi.KWaveError, match="damped beyond B = 1/4"):
        plan(n, d, C0, alpha_coeff=stokes, alpha_power=2.0, expanded=e)
    assert plan(n, d, C0, alpha_coeff=0.5 * stokes, alpha_power=2.0, expanded=e) == (e, True)


def test_python_front_end_checks_its_arguments(second_order):
    plan = second_order.SecondOrder.plan
    with pytest.raises(ValueError):
        plan((24, 20), D3, C0, t_max=1e-6)
    with pytest.raises(ValueError):
        plan((24, 20, 18), D3, C0, t_max=1e-6, record=("p_raw", "u_max"))
    with pytest.raises(ValueError):
        plan((24, 20, 18), D3, C0, t_max=1e-6, expanded=(48, 48))
    with pytest.raises(ValueError):
        plan((24, 20, 18), D3, C0, t_max=1e-6, sensor_index=[-1])


# ---- 3. the host code, stand-alone under the sanitizers --------------------------------------------------------------------
EXPECTED = {
    "default": "ok E=48x48x48 fast=1 t_free=1.600000e-06 B=1.000000/1.000000 last=40103",   # (17 48 + 19) 48 + 23
    "rocfft": "ok E=40x33x36 fast=0 t_free=1.040000e-06 B=1.000000/1.000000 last=23223",    # (17 33 + 19) 40 + 23
    "beyond_1024": "ok E=1036x48x48 fast=0 t_free=1.066667e-06",
    "box": "ok E=24x20x18 fast=0 t_free=0.000000e+00 B=1.000000/1.000000 last=8639",
    "given_odd": "ok E=27x20x33 fast=0 t_free=0.000000e+00 B=1.000000/1.000000 last=9716",   # (17 20 + 19) 27 + 23
    "absorbing": "ok E=48x48x48 fast=1 t_free=1.600000e-06 B=%.6f/%.6f" % sr.b_margins((48, 48, 48), D3, C0, 0.75, 1.5)[1:],
    "stokes": "ok E=48x48x48 fast=1 t_free=1.600000e-06 B=%.6f/%.6f" % sr.b_margins((48, 48, 48), D3, C0, 0.01, 2.0)[1:],
    "no_sensors": "ok E=48x48x48 fast=1 t_free=1.600000e-06 B=1.000000/1.000000 last=0",
    "overdamped": REFUSALS[-2][1],
    "overdamped_low_k": REFUSALS[-1][1],
    "nz_zero": "Nz: 0 is not a grid size",
    "dz_zero": "dz: 0.000000 is not a positive spacing",
    "c0_negative": "c0: -1.000000 is not a positive sound speed",
    "t_max_missing": "t_max: 0.000000 is not a positive time",
    "alpha_negative": "alpha_coeff: -1.000000 is not an absorption >= 0",
    "power_one": "alpha_power: 1.000000 is outside the power law's range",
    "power_three": "alpha_power: 3.000000 is outside the power law's range",
    "e_missing": "Ez: missing while the other sides of the expanded grid are given",
    "e_small": "Ez: 17 is below N = 18",
    "too_large": "E: 2048 x 2048 x 1024 points is not below 2^32",
    "sensor_outside": "sensor_index: sensor_index[3] = 8640 is outside the domain of 8640 points",
    "t_zero": "ok",
    "t_negative": "t: -0.000001 is not a time >= 0",
    "t_nan": "t: nan is not a time >= 0",
}


def test_host_parameters_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/second_order_host_check.cpp: SecondOrderParameters::init through valid inputs and refusals, by its
    message"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "second_order_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "second_order_host_check.cpp"),
           os.path.join(host, "SecondOrderParameters.cpp"), os.path.join(host, "GridRules.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
    lines = dict(line.split(": ", 1) for line in r.stdout.strip().splitlines())
    assert sorted(lines) == sorted(EXPECTED)
    for name, what in EXPECTED.items():
        assert lines[name].startswith(what), (name, lines[name])


# ---- 4. declarations ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(second_order):
    from kwave_amd import capi
    assert ENTRY_POINTS <= set(capi.declared_symbols())
    counts = {"kw_fused_second_order_elems": 2, "kw_fused_second_order_forward": 3, "kw_fused_second_order_time": 4,
              "kw_second_order_mix": 5}
    header = open(os.path.join(ROOT, "include", "kwave_hip.h")).read()
    for name, n in counts.items():
        assert len(capi._SIG[name]) == n, name
        decl = header.split("KW_API kw_status " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n, name
    host = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in ("plan", "create", "destroy", "set_p0", "field", "run", "get", "get_scalar", "context"):
        assert "kwh_second_order_" + name + "(" in host, name
    assert C.sizeof(second_order.Config) == 16 * 8
    assert C.sizeof(capi.SecondOrderOp) == 8 * 8
    for name in ("plan", "set_p0", "field", "run", "p_max", "p_min", "p_rms", "p_final", "close"):
        assert callable(getattr(second_order.SecondOrder, name))
    for name in ("expanded", "t_free", "fused", "runs", "ctx"):
        assert isinstance(getattr(second_order.SecondOrder, name), property)


def test_library_exports_the_entry_points():
    from kwave_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
