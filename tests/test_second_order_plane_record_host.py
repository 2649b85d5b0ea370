"""Plane-sensor record of the 3-D exact k-space propagator, CPU side: the float64 restatement
(tests/second_order_plane_record_reference.py: no 3-D inverse anywhere) against the plane of the 3-D restatement; a float32
emulation of the record kernel's sum over the folded bins at Ez = 1024 against float64; the plane, chunk and n_times rules
through kwh_second_order_plane_plan without a device; the parameter, chunk and indexing code in a stand-alone program built
with AddressSanitizer and UBSan; and the declarations.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import second_order_plane_record_reference as pr  # noqa: E402
import second_order_reference as sr  # noqa: E402

C0 = 1500.0
PARITY = 1e-5
ENTRY_POINTS = {"kw_second_order_plane_elems": 2, "kw_second_order_plane_prepare": 4, "kw_second_order_plane_record": 6}
HOST_ENTRIES = ("plane_plan", "set_plane", "set_plane_chunk_times", "plane_record")


@pytest.fixture(scope="module")
def second_order():
    import kwave_amd  # noqa: F401
    from kwave_amd import second_order
    return second_order


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------
VARIANTS = ((0.0, 1.5), (0.75, 1.5), (0.2, 2.0), (0.75, 1.1))
N3, D3 = (20, 17, 15), (1.0e-4, 0.8e-4, 1.3e-4)


@pytest.mark.parametrize("expanded", [(32, 24, 40), (27, 33, 21)], ids=["even", "odd"])
def test_restatement_is_the_plane_of_the_three_d_restatement(expanded):
    """an even box (the Nyquist bins, the self-paired bin Ez/2) and an odd one (none); planes 0, Nz - 1 and an interior one;
    lossless, y = 1.5, y = 2 and y = 1.1; the time 0 among the times"""
    p0 = np.random.default_rng(sum(expanded)).standard_normal((N3[2], N3[1], N3[0]))
    times = [0.0, 3.1e-8, 2.7e-6, 4.4e-7]
    worst = 0.0
    for coeff, y in VARIANTS:
        assert coeff == 0.0 or sr.b_margins(expanded, D3, C0, coeff, y)[0] >= 0.25
        whole = sr.solve(p0, expanded, D3, C0, times, coeff, y)   # [n_times][Nz][Ny][Nx]
        for plane in (0, N3[2] - 1, 6):
            got = pr.record(p0, expanded, D3, C0, times, plane, coeff, y)
            assert got.shape == (len(times), N3[1], N3[0])
            err = sr.rel_l2(got, whole[:, plane])
            worst = max(worst, err)
            assert err <= 1e-12, (coeff, y, plane, err)
            assert sr.rel_l2(got[0], p0[plane]) <= 1e-12, (coeff, y, plane)   # t = 0: the plane of p0
    print(f"plane record restatement against the 3-D restatement, E {expanded}: worst {worst:.3e}")


# ---- 2. the kernel's float32 sum at Ez = 1024 -------------------------------------------------------------------------------
def test_float32_sum_over_the_folded_bins_stays_within_the_bound_at_1024():
    """(Ex, Ey, Ez) = (16, 16, 1024), the stage test's input and its four cases: 513 folded bins, one float32 accumulator per
    value from zero in ascending m, as k_plane_record sums (its chunks of 64 bins stage Q; they do not split the sum).
    Relative L2 of G and of the planes against float64, float32 Q and H; the bound is the project's 1e-5.
    Measured: G 4.6e-9 to 1.2e-6, planes 4.6e-9 to 1.1e-6."""
    ex, ey, ez = 16, 16, 1024
    vol = pr.source_volume(np.random.default_rng(ex * 1009 + ey * 31 + ez), ex, ey, ez)
    k = pr.folded_k((ex, ey, ez), sr.STAGE_D)
    for plane in (0, ez // 2):
        Q = pr.folded_q(vol, plane)
        for coeff, t in sr.stage_case((ex, ey, ez)):
            H = sr.H_of_k(k, sr.STAGE_C0, t, coeff, sr.STAGE_Y)
            want = (Q * H).sum(axis=2)
            got = pr.accumulate_f32(Q, H)
            e_g = sr.rel_l2(np.stack([got.real, got.imag]), np.stack([want.real, want.imag]))
            e_p = sr.rel_l2(pr.planes_of(got[None], ex), pr.planes_of(want[None], ex))
            print(f"float32 sum over 513 folded bins, plane {plane}, alpha_coeff {coeff:.3g}, t {t:.3e}: G {e_g:.3e}, planes {e_p:.3e}")
            assert e_g < PARITY and e_p < PARITY


# ---- 3. the rules, through kwh_second_order_plane_plan without a device -----------------------------------------------------
BASE = dict(n=(24, 20, 18), d=(1.0e-4, 1.2e-4, 0.9e-4), c0=C0, t_max=1.03e-6)   # E = (48, 48, 48)
Q48 = 48 * 25 * 25
DEFAULT48 = (256 << 20) // (25 * 48 * 8)


def test_default_chunk_follows_the_byte_budget(second_order):
    plan = second_order.SecondOrder.plane_plan
    assert plan(plane=0, n_times=12, **BASE) == (DEFAULT48, 1, Q48)
    assert plan(plane=17, n_times=12, plane_chunk_times=5, **BASE) == (5, 3, Q48)
    assert plan(plane=17, n_times=12, plane_chunk_times=12, **BASE) == (12, 1, Q48)
    assert plan(plane=None, n_times=1, plane_chunk_times=1, **BASE) == (1, 1, Q48)
    # the measured shape: 128^3 in 256^3 takes 1016 times per pass
    big = dict(BASE, n=(128, 128, 128), expanded=(256, 256, 256))
    assert plan(plane=0, n_times=256, **big) == (1016, 1, 256 * 129 * 129)
    assert plan(plane=0, n_times=2048, **big)[1] == 3
    # odd sides
    assert plan(plane=3, n_times=9, plane_chunk_times=4, **dict(BASE, expanded=(27, 33, 21))) == (4, 3, 33 * 14 * 11)


REFUSALS = [
    (dict(plane=18), "plane: 18 is outside the domain's planes 0 ... 17 (-1: no record)"),
    (dict(plane=-2), "plane: -2 is outside the domain's planes 0 ... 17 (-1: no record)"),
    (dict(plane=47), "plane: 47 is outside the domain's planes 0 ... 17 (-1: no record)"),   # a plane of the expansion
    (dict(n_times=0), "n_times: 0 is not a number of output times"),
    (dict(plane_chunk_times=(1 << 32) // (48 * 48) + 1),
     "plane_chunk_times: 1864136 times of planes of 48 x 48 points are too many for one pass (2^32 points, 16776960 times)"),
    (dict(n=(0, 20, 18)), "Nx: 0 is not a grid size"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(":")[0] + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_every_refusal_names_its_parameter(second_order, change, message):
    from kwave_amd import capi
    args = dict(BASE, plane=0, n_times=12)
    args.update(change)
    with pytest.raises(capi.KWaveError) as e:
        second_order.SecondOrder.plane_plan(**args)
    assert str(e.value) == message


def test_the_largest_chunk_of_a_pass_is_taken(second_order):
    """Ex Ey times < 2^32: one below the refused number passes"""
    assert second_order.SecondOrder.plane_plan(plane=0, n_times=1, plane_chunk_times=(1 << 32) // (48 * 48) - 1, **BASE)[0] == 1864134


def test_python_front_end_checks_its_arguments(second_order):
    with pytest.raises(TypeError):
        second_order.SecondOrder.plane_plan(plane=0, n_times=1, no_such=1, **BASE)


# ---- 4. the parameter, chunk and indexing code, stand-alone under the sanitizers ---------------------------------------------
def ok(plane, chunk, passes, largest, q, g):
    return f"ok plane={plane} chunk={chunk} passes={passes} largest={largest} q={q} g={g}"


G48 = 25 * 48
EXPECTED = {
    "default": ok(0, DEFAULT48, 1, 12, Q48, G48 * 12),
    "last_plane": ok(17, DEFAULT48, 1, 1, Q48, G48),
    "off": ok(-1, DEFAULT48, 1, 3, Q48, G48 * 3),
    "one_pass_exact": ok(7, 12, 1, 12, Q48, G48 * 12),
    "two_passes": ok(7, 7, 2, 7, Q48, G48 * 7),
    "single_times": ok(7, 1, 5, 1, Q48, G48),
    "odd_box": ok(3, 4, 3, 4, 33 * 14 * 11, 14 * 33 * 4),
    "budget": ok(0, 1016, 1, 3, 256 * 129 * 129, 129 * 256 * 3),
    "budget_one_time": ok(0, 1, 2, 1, 16384 * 8193, 8193 * 16384),   # one time is over the budget: one at the least
    "plane_below": REFUSALS[1][1],
    "plane_at_nz": REFUSALS[0][1],
    "plane_in_expansion": REFUSALS[2][1],
    "no_times": REFUSALS[3][1],
    "chunk_too_many_points": REFUSALS[4][1],
    "chunk_too_many_times": "plane_chunk_times: 16776961 times of planes of 1 x 1 points are too many for one pass",
    "chunk_overflow": "plane_chunk_times: 18446744073709551615 times of planes of 48 x 48 points are too many for one pass",
    "bad_grid": "Nx: 0 is not a grid size",
}


def test_host_plane_record_code_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/second_order_plane_record_host_check.cpp: the plane rule, the times of a pass, the passes and the copy of
    every pass into the record, by its message"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "second_order_plane_record_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "second_order_plane_record_host_check.cpp"),
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


# ---- 5. declarations -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(second_order):
    from kwave_amd import capi
    assert set(ENTRY_POINTS) <= set(capi._SIG)
    assert set(ENTRY_POINTS) <= set(capi.declared_symbols())
    header = open(os.path.join(ROOT, "include", "kwave_hip.h")).read()
    for name, n in ENTRY_POINTS.items():
        assert len(capi._SIG[name]) == n, name
        decl = header.split("KW_API kw_status " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n, name
    host = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in HOST_ENTRIES:
        assert "kwh_second_order_" + name + "(" in host, name
    assert C.sizeof(second_order.Config) == 16 * 8   # the config keeps its layout
    for name in ("plane_record", "plane_plan"):
        assert callable(getattr(second_order.SecondOrder, name))
    for name in ("plane", "plane_chunk_times"):
        assert isinstance(getattr(second_order.SecondOrder, name), property)
    # the frames class keeps its interface: the plane record is the 3-D class's alone
    for name in ("plane", "plane_chunk_times", "plane_record", "plane_plan"):
        assert not hasattr(second_order.SecondOrderFrames, name)
    for name in ("line_record", "line_plan", "field", "run", "set_p0", "set_dp0dt", "p_max", "close"):
        assert callable(getattr(second_order.SecondOrderFrames, name))


def test_libraries_export_the_entry_points():
    from kwave_amd import capi
    from kwave_amd.solver import load_host
    L, H = capi.load(), load_host()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    for name in HOST_ENTRIES:
        assert hasattr(H, "kwh_second_order_" + name)
