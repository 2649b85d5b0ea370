"""Batched 2-D exact k-space propagator, CPU side: the wrapped restatement (tests/second_order_frames_reference.py) against
irfft2(rfft2 H) written out independently and against the 3-D restatement of a field held constant along a periodic z; the
inputs of the GPU stage test against the damping rule; the size rules and every refusal through
kwh_second_order_frames_plan without a device; the parameter class in a stand-alone program built with AddressSanitizer and
UBSan; and the declarations.  No GPU."""
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
import second_order_frames_reference as fr  # noqa: E402
import second_order_reference as sr  # noqa: E402

C0 = 1500.0
ENTRY_POINTS = {"kw_fused_second_order_frames_elems", "kw_fused_second_order_frames_forward",
                "kw_fused_second_order_frames_time", "kw_second_order_frames_mix"}


@pytest.fixture(scope="module", autouse=True)
def second_order():
    """without the batched propagator's entry points nothing in this file passes"""
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, second_order
    assert ENTRY_POINTS <= set(capi._SIG)
    assert hasattr(second_order, "SecondOrderFrames")
    return second_order


# ---- 1. the restatement -------------------------------------------------------------------------------------------------
VARIANTS = ((0.0, 1.5), (0.75, 1.5), (0.2, 2.0), (0.75, 1.1))


def independent_frame(p0, expanded, d, t, coeff, y):
    """one frame written out with no call into either restatement: bins, H and the 2-D transforms"""
    ex, ey = expanded
    ny, nx = p0.shape
    v = np.zeros((ey, ex))
    v[:ny, :nx] = p0
    ix, iy = np.arange(ex // 2 + 1), np.arange(ey)
    kx = 2.0 * math.pi / (ex * d[0]) * np.minimum(ix, ex - ix)
    ky = 2.0 * math.pi / (ey * d[1]) * np.minimum(iy, ey - iy)
    k = np.sqrt(kx[None, :] ** 2 + ky[:, None] ** 2)
    if coeff == 0.0:
        H = np.cos(C0 * k * t)
    else:
        a = coeff * 100.0 * (1.0e-6 / (2.0 * math.pi)) ** y / (20.0 * math.log10(math.e))
        ks = np.where(k > 0, k, 1.0)
        g = a * C0 ** y * ks ** (y - 1.0)
        T = 0.0 if y == 2.0 else math.tan(math.pi * y / 2.0)
        r = np.sqrt(1.0 - 2.0 * g * T - g * g)
        H = np.where(k > 0, np.exp(-C0 * ks * g * t) * (np.cos(C0 * ks * r * t) + g / r * np.sin(C0 * ks * r * t)), 1.0)
    return np.fft.irfft2(np.fft.rfft2(v) * H, s=(ey, ex))[:ny, :nx]


@pytest.mark.parametrize("expanded", [(32, 48), (27, 33)])
def test_wrapped_restatement_is_irfft2_of_rfft2_times_h(expanded):
    n, d = (20, 17), (1.0e-4, 0.8e-4)
    p0 = np.random.default_rng(sum(expanded)).standard_normal((3, n[1], n[0]))
    times = [0.0, 3.1e-8, 2.7e-6]
    for coeff, y in VARIANTS:
        assert coeff == 0.0 or fr.b_margins(expanded, d, C0, coeff, y)[0] >= 0.25
        got = fr.solve(p0, expanded, d, C0, times, coeff, y)
        assert got.shape == (3, 3, n[1], n[0])
        for i, t in enumerate(times):
            for f in range(3):
                err = sr.rel_l2(got[i, f], independent_frame(p0[f], expanded, d, t, coeff, y))
                assert err <= 1e-12, (coeff, y, t, f, err)
        whole = fr.solve_expanded(sr.embed(p0, (expanded[0], expanded[1], 3)), d, C0, times[2], coeff, y)
        assert sr.rel_l2(whole[:, :n[1], :n[0]], got[2]) <= 1e-12


def test_a_frame_is_the_three_d_restatement_of_a_field_constant_along_a_periodic_z():
    """expanded_z = Nz: nothing along z, every bin with kz != 0 is empty, so every plane stays the 2-D solution"""
    n, e, d3 = (24, 20), (48, 48), (1.0e-4, 1.2e-4, 0.9e-4)
    plane = np.random.default_rng(2420).standard_normal((n[1], n[0]))
    times = [0.0, 4.1e-7, 1.03e-6]
    for coeff, y in VARIANTS:
        assert coeff == 0.0 or sr.b_margins(e + (16,), d3, C0, coeff, y)[0] >= 0.25
        three = sr.solve(np.broadcast_to(plane, (16,) + plane.shape), e + (16,), d3, C0, times, coeff, y)
        two = fr.solve(plane[None], e, d3[:2], C0, times, coeff, y)[:, 0]
        err = max(sr.rel_l2(three[i, z], two[i]) for i in range(3) for z in range(16))
        print(f"2-D frame against 3-D constant along z, alpha_coeff {coeff} y {y}: {err:.3e}")
        assert err <= 1e-12


def test_gpu_stage_inputs_keep_every_mode_underdamped_and_every_result_alive():
    """the numbers of tests/test_gpu_second_order_frames.py's stage tests at every fast-path length: B >= 1/4 on every
    non-zero bin of the planes (L, 16), (16, L), (96, L) — worst 1.0008 — the far time at 10^4 turns of the largest |k|, and a
    slowest mode that keeps exp(-2)"""
    d = sr.STAGE_D[:2]
    worst = math.inf
    for L in cr.fast_lengths():
        for expanded in ((L, 16), (16, L), (96, L)):
            cases = fr.stage_case(expanded)
            coeff, t_far = cases[3]
            assert cases[0][0] == 0.0 and cases[1] == (0.0, t_far) and cases[2][0] == coeff
            lowest, at_smallest, at_largest = fr.b_margins(expanded, d, sr.STAGE_C0, coeff, sr.STAGE_Y)
            assert lowest >= 0.25 and lowest == pytest.approx(min(at_smallest, at_largest), rel=1e-12), expanded
            worst = min(worst, lowest)
            k = sr.wavenumbers(fr.plane(expanded), fr.spacings(d))
            assert sr.STAGE_C0 * k.max() * t_far / (2.0 * math.pi) == pytest.approx(1.0e4, rel=1e-12)
            g = sr.damping(k[k > 0].min(), sr.STAGE_C0, coeff, sr.STAGE_Y)[0]
            assert sr.STAGE_C0 * k[k > 0].min() * g * t_far == pytest.approx(2.0, rel=1e-12)
    print(f"worst B over the stage grids: {worst:.4f}")


# ---- 2. the rules and the refusals, through kwh_second_order_frames_plan without a device ---------------------------------
D2 = (1.0e-4, 1.2e-4)
RULE_TABLE = [  # n, t_max, fused -> expanded, fast.  c0 t_max = 1.545 mm: 15.45 and 12.875 points, so 16 and 13 more
    ((24, 20), 1.03e-6, True, (48, 48), True),        # 40, 33 -> 48 each
    ((24, 20), 1.03e-6, False, (40, 33), False),
    ((23, 19), 1.03e-6, False, (39, 32), False),      # odd sizes: the twin path
    ((100, 16), 1.03e-6, True, (120, 32), True),      # 116 -> 120, 29 -> 32
    ((1020, 16), 1.03e-6, True, (1036, 32), False),   # no fast length above 1024: the number itself on that axis
]


@pytest.mark.parametrize("n,t_max,fused,expanded,fast", RULE_TABLE)
def test_default_sides_follow_the_rule(second_order, n, t_max, fused, expanded, fast):
    got = second_order.SecondOrderFrames.plan(n, D2, C0, 5, t_max=t_max, fused_kernels=fused)
    assert got == (expanded, fast)
    assert got[0] == fr.default_sides(n, D2, C0, t_max, fused, cr.fast_lengths())


def test_given_sides_are_kept(second_order):
    plan = second_order.SecondOrderFrames.plan
    assert plan((24, 20), D2, C0, 5, expanded=(24, 20)) == ((24, 20), False)              # the periodic plane
    assert plan((32, 32), D2, C0, 5, expanded=(32, 32)) == ((32, 32), True)
    assert plan((24, 20), D2, C0, 5, expanded=(32, 48), t_max=1.0) == ((32, 48), True)    # t_max is not read
    assert plan((24, 20), D2, C0, 5, expanded=(27, 33)) == ((27, 33), False)              # odd sides: the twin path
    assert plan((24, 20), D2, C0, 5, expanded=(32, 48), fused_kernels=False) == ((32, 48), False)
    assert plan((24, 20), D2, C0, 1, expanded=(32, 48)) == ((32, 48), True)
    assert plan((24, 20), D2, C0, 65535, expanded=(32, 48)) == ((32, 48), True)           # the most one batch takes


REFUSALS = [
    (dict(n=(0, 20)), "Nx: 0 is not a grid size"),
    (dict(n=(24, 0)), "Ny: 0 is not a grid size"),
    (dict(frames=0), "frames: 0 is not a number of frames"),
    (dict(frames=65536), "frames: 65536 is above 65535, the most one batch takes"),
    (dict(d=(0.0, 1e-4)), "dx: 0.000000 is not a positive spacing"),
    (dict(d=(1e-4, float("nan"))), "dy: nan is not a positive spacing"),
    (dict(c0=0.0), "c0: 0.000000 is not a positive sound speed"),
    (dict(t_max=None), "t_max: 0.000000 is not a positive time (the default expanded sides are sized by it)"),
    (dict(t_max=float("inf")), "t_max: inf is not a positive time (the default expanded sides are sized by it)"),
    (dict(alpha_coeff=-1.0), "alpha_coeff: -1.000000 is not an absorption >= 0 in dB/(MHz^y cm)"),
    (dict(alpha_coeff=0.75, alpha_power=1.0), "alpha_power: 1.000000 is outside the power law's range 0 <= y < 3, y != 1"),
    (dict(alpha_power=3.0), "alpha_power: 3.000000 is outside the power law's range 0 <= y < 3, y != 1"),
    (dict(expanded=(48, 0)), "Ey: missing while the other side of the expanded grid is given"),
    (dict(expanded=(0, 48)), "Ex: missing while the other side of the expanded grid is given"),
    (dict(expanded=(23, 48)), "Ex: 23 is below N = 24"),
    (dict(expanded=(48, 19)), "Ey: 19 is below N = 20"),
    (dict(expanded=(2048, 2048), frames=1024), "E: 2048 x 2048 x 1024 points is not below 2^32"),
    (dict(sensor_index=[0, 480]), "sensor_index: sensor_index[1] = 480 is outside the plane of 480 points"),
    (dict(alpha_coeff=500.0), "alpha_coeff: 500.000000: a mode of this grid is damped beyond B = 1/4 (B = %.6f at the largest |k|)"
     % fr.b_margins((48, 48), D2, C0, 500.0, 1.5)[2]),
    (dict(alpha_coeff=100.0, alpha_power=0.5),
     "alpha_coeff: 100.000000: a mode of this grid is damped beyond B = 1/4 (B = %.6f at the smallest non-zero |k|)"
     % fr.b_margins((48, 48), D2, C0, 100.0, 0.5)[1]),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(":")[0] + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_every_refusal_names_its_parameter(second_order, change, message):
    from kwave_amd import capi
    args = dict(n=(24, 20), d=D2, c0=C0, frames=5, t_max=1.03e-6)
    args.update(change)
    with pytest.raises(capi.KWaveError) as e:
        second_order.SecondOrderFrames.plan(**args)
    assert str(e.value) == message
    with pytest.raises(capi.KWaveError) as e:   # the same from create, before any device is looked for
        second_order.SecondOrderFrames(**args)
    assert str(e.value) == message


def test_damping_rule_is_taken_on_the_two_d_grid(second_order):
    """a coefficient that puts B at 0.2 at the largest |k| of the plane (48, 48) is refused, one that puts it at 0.3 passes;
    the coefficient that the 3-D grid (48, 48, 48) of the same spacings would refuse (B = 0.2 at ITS largest |k|, which lies
    further out) passes on the plane: the third axis is not there"""
    from kwave_amd import capi
    plan = second_order.SecondOrderFrames.plan
    n, d, e = (24, 24), (1.0e-4, 1.0e-4), (48, 48)
    assert plan(n, d, C0, 3, alpha_coeff=0.75, alpha_power=1.5, expanded=e) == (e, True)
    coeff_for_b = lambda b, y: sr.coeff_for_b(fr.plane(e), fr.spacings(d), C0, y, b)   # noqa: E731
    bad = coeff_for_b(0.2, 1.5)
    assert fr.b_margins(e, d, C0, bad, 1.5)[2] == pytest.approx(0.2, abs=1e-12)
    with pytest.raises(capi.KWaveError) as err:
        plan(n, d, C0, 3, alpha_coeff=bad, alpha_power=1.5, expanded=e)
    assert str(err.value).startswith("alpha_coeff: ")
    assert str(err.value).endswith(": a mode of this grid is damped beyond B = 1/4 (B = 0.200000 at the largest |k|)")
    assert plan(n, d, C0, 3, alpha_coeff=coeff_for_b(0.3, 1.5), alpha_power=1.5, expanded=e) == (e, True)
    three_d = sr.coeff_for_b((48, 48, 48), (1.0e-4,) * 3, C0, 1.5, 0.2)
    assert three_d < bad and fr.b_margins(e, d, C0, three_d, 1.5)[0] >= 0.25
    with pytest.raises(capi.KWaveError, match="damped beyond B = 1/4"):
        second_order.SecondOrder.plan((24, 24, 24), (1.0e-4,) * 3, C0, alpha_coeff=three_d, expanded=(48, 48, 48))
    assert plan(n, d, C0, 3, alpha_coeff=three_d, alpha_power=1.5, expanded=e) == (e, True)
    # Stokes: T = 0, B = 1 - g^2
    stokes = coeff_for_b(0.2, 2.0)
    with pytest.raises(capi.KWaveError, match="damped beyond B = 1/4"):
        plan(n, d, C0, 3, alpha_coeff=stokes, alpha_power=2.0, expanded=e)
    assert plan(n, d, C0, 3, alpha_coeff=0.5 * stokes, alpha_power=2.0, expanded=e) == (e, True)


def test_python_front_end_checks_its_arguments(second_order):
    plan = second_order.SecondOrderFrames.plan
    with pytest.raises(ValueError):
        plan((24, 20, 18), D2, C0, 5, t_max=1e-6)
    with pytest.raises(ValueError):
        plan((24, 20), D2, C0, 5, t_max=1e-6, record=("p_raw", "u_max"))
    with pytest.raises(ValueError):
        plan((24, 20), D2, C0, 5, t_max=1e-6, expanded=(48, 48, 48))
    with pytest.raises(ValueError):
        plan((24, 20), D2, C0, 5, t_max=1e-6, sensor_index=[-1])
    with pytest.raises(ValueError):
        plan((24, 20), D2, C0, -1, t_max=1e-6)


# ---- 3. the parameter class, stand-alone under the sanitizers ------------------------------------------------------------
def ok(e, frames, fast, t_free, b=(1.0, 1.0), sensors=(0, 23, 479)):
    """the program's line for completed parameters: the last sensor point in frame 0 and in the last frame"""
    at = lambda f: (f * e[1] + sensors[-1] // 24) * e[0] + sensors[-1] % 24   # noqa: E731
    tail = f" n={len(sensors) * frames} first={at(0)} last={at(frames - 1)}" if sensors else " n=0 first=0 last=0"
    return f"ok E={e[0]}x{e[1]} F={frames} fast={fast} t_free={t_free:.6e} B={b[0]:.6f}/{b[1]:.6f}" + tail


EXPECTED = {
    "default": ok((48, 48), 5, 1, 1.6e-6),
    "rocfft": ok((40, 33), 5, 0, 1.04e-6),
    "beyond_1024": "ok E=1036x48 F=5 fast=0 t_free=1.066667e-06",
    "plane": ok((24, 20), 5, 0, 0.0),
    "given_odd": ok((27, 33), 5, 0, 2.0e-7),
    "one_frame": ok((48, 48), 1, 1, 1.6e-6),
    "most_frames": ok((48, 48), 65535, 1, 1.6e-6, sensors=(479,)),
    "absorbing": ok((48, 48), 5, 1, 1.6e-6, fr.b_margins((48, 48), D2, C0, 0.75, 1.5)[1:]),
    "stokes": ok((48, 48), 5, 1, 1.6e-6, fr.b_margins((48, 48), D2, C0, 0.01, 2.0)[1:]),
    "no_sensors": ok((48, 48), 5, 1, 1.6e-6, sensors=()),
    "overdamped": REFUSALS[-2][1],
    "overdamped_low_k": REFUSALS[-1][1],
    "nx_zero": "Nx: 0 is not a grid size",
    "frames_zero": "frames: 0 is not a number of frames",
    "frames_65536": "frames: 65536 is above 65535, the most one batch takes",
    "dy_zero": "dy: 0.000000 is not a positive spacing",
    "c0_negative": "c0: -1.000000 is not a positive sound speed",
    "t_max_missing": "t_max: 0.000000 is not a positive time",
    "alpha_negative": "alpha_coeff: -1.000000 is not an absorption >= 0",
    "power_one": "alpha_power: 1.000000 is outside the power law's range",
    "e_missing": "Ey: missing while the other side of the expanded grid is given",
    "e_small": "Ey: 19 is below N = 20",
    "too_large": "E: 2048 x 2048 x 1024 points is not below 2^32",
    "sensor_outside": "sensor_index: sensor_index[3] = 480 is outside the plane of 480 points",
}


def test_host_parameters_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/second_order_frames_host_check.cpp: SecondOrderFramesParameters::init through valid inputs and
    refusals, by its message"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "second_order_frames_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "second_order_frames_host_check.cpp"),
           os.path.join(host, "SecondOrderFramesParameters.cpp"), os.path.join(host, "GridRules.cpp"), "-o", exe]
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
    counts = {"kw_fused_second_order_frames_elems": 2, "kw_fused_second_order_frames_forward": 3,
              "kw_fused_second_order_frames_time": 4, "kw_second_order_frames_mix": 5}
    header = open(os.path.join(ROOT, "include", "kwave_hip.h")).read()
    for name, n in counts.items():
        assert len(capi._SIG[name]) == n, name
        decl = header.split("KW_API kw_status " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n, name
    host = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in ("plan", "create", "destroy", "set_p0", "field", "run", "get", "get_scalar", "context"):
        assert "kwh_second_order_frames_" + name + "(" in host, name
    assert C.sizeof(second_order.FramesConfig) == 14 * 8
    assert C.sizeof(second_order.Config) == 16 * 8   # the 3-D config keeps its layout
    for name in ("plan", "set_p0", "field", "run", "p_max", "p_min", "p_rms", "p_final", "close"):
        assert callable(getattr(second_order.SecondOrderFrames, name))
    for name in ("expanded", "t_free", "fused", "runs", "ctx", "shape"):
        assert isinstance(getattr(second_order.SecondOrderFrames, name), property)


def test_libraries_export_the_entry_points():
    from kwave_amd import capi
    from kwave_amd.solver import load_host
    L, H = capi.load(), load_host()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    for name in ("plan", "create", "destroy", "set_p0", "field", "run", "get", "get_scalar", "context"):
        assert hasattr(H, "kwh_second_order_frames_" + name)
