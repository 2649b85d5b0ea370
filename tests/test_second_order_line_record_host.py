"""Line-sensor record of the batched 2-D exact k-space propagator, CPU side: the float64 restatement
(tests/second_order_line_record_reference.py: no 2-D inverse anywhere) against the row of the 2-D restatement; a float32
emulation of the record kernel's sum over the folded bins at Ey = 1024 against float64; the row, chunk and n_times rules
through kwh_second_order_frames_line_plan without a device; the parameter, chunk and indexing code in a stand-alone program
built with AddressSanitizer and UBSan; and the declarations.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import second_order_frames_reference as fr  # noqa: E402
import second_order_line_record_reference as lr  # noqa: E402
import second_order_reference as sr  # noqa: E402

C0 = 1500.0
PARITY = 1e-5
ENTRY_POINTS = {"kw_second_order_line_elems": 2, "kw_second_order_line_prepare": 4, "kw_second_order_line_record": 6}
HOST_ENTRIES = ("line_plan", "set_line_row", "set_line_chunk_times", "line_record")


@pytest.fixture(scope="module", autouse=True)
def second_order():
    """without the record's entry points nothing in this file passes"""
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, second_order
    assert set(ENTRY_POINTS) <= set(capi._SIG)
    assert hasattr(second_order.SecondOrderFrames, "line_record")
    return second_order


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------
VARIANTS = ((0.0, 1.5), (0.75, 1.5), (0.2, 2.0), (0.75, 1.1))


@pytest.mark.parametrize("expanded", [(32, 48), (27, 33)], ids=["even", "odd"])
def test_restatement_is_the_row_of_the_two_d_restatement(expanded):
    """an even plane (both Nyquist bins, the self-paired bin Ey/2) and an odd one (neither); rows 0, Ny - 1 and an interior
    one; lossless, y = 1.5, y = 2 and y = 1.1; the time 0 among the times"""
    n, d = (20, 17), (1.0e-4, 0.8e-4)
    p0 = np.random.default_rng(sum(expanded)).standard_normal((3, n[1], n[0]))
    times = [0.0, 3.1e-8, 2.7e-6, 4.4e-7]
    worst = 0.0
    for coeff, y in VARIANTS:
        assert coeff == 0.0 or fr.b_margins(expanded, d, C0, coeff, y)[0] >= 0.25
        whole = fr.solve(p0, expanded, d, C0, times, coeff, y)   # [n_times][F][Ny][Nx]
        for row in (0, n[1] - 1, 6):
            got = lr.record(p0, expanded, d, C0, times, row, coeff, y)
            assert got.shape == (3, len(times), n[0])
            err = sr.rel_l2(got, whole[:, :, row, :].transpose(1, 0, 2))
            worst = max(worst, err)
            assert err <= 1e-12, (coeff, y, row, err)
    print(f"line record restatement against the 2-D restatement, E {expanded}: worst {worst:.3e}")


def test_time_zero_is_the_row_of_p0():
    p0 = np.random.default_rng(5).standard_normal((2, 17, 20))
    for row in (0, 16, 9):
        assert sr.rel_l2(lr.record(p0, (27, 33), (1e-4, 0.8e-4), C0, [0.0], row, 0.75, 1.5)[:, 0], p0[:, row, :]) <= 1e-12


# ---- 2. the kernel's float32 sum at Ey = 1024 -------------------------------------------------------------------------------
def test_float32_sum_over_the_folded_bins_stays_within_the_bound_at_1024():
    """(Ex, Ey, F) = (16, 1024, 3), the stage test's inputs and its four cases: 513 folded bins, one float32 accumulator per
    value from zero in ascending m, as k_line_record sums (its chunks of 64 bins stage Q; they do not split the sum).
    Relative L2 of G and of the rows against float64, float32 Q and H; the bound is the project's 1e-5."""
    ex, ey, nf = 16, 1024, 3
    d = sr.STAGE_D[:2]
    vol = lr.source_frames(np.random.default_rng(ex * 1009 + ey * 31 + nf), nf, ey, ex)
    k = lr.folded_k((ex, ey), d)
    for row in (0, ey // 2):
        Q = lr.folded_q(vol, row)
        for coeff, t in fr.stage_case((ex, ey)):
            H = sr.H_of_k(k, sr.STAGE_C0, t, coeff, sr.STAGE_Y)
            want = (Q * H[None]).sum(axis=1)
            got = lr.accumulate_f32(Q, H)
            e_g = sr.rel_l2(np.stack([got.real, got.imag]), np.stack([want.real, want.imag]))
            e_r = sr.rel_l2(lr.rows_of(got[:, None], ex), lr.rows_of(want[:, None], ex))
            print(f"float32 sum over 513 folded bins, row {row}, alpha_coeff {coeff:.3g}, t {t:.3e}: G {e_g:.3e}, rows {e_r:.3e}")
            assert e_g < PARITY and e_r < PARITY


# ---- 3. the rules, through kwh_second_order_frames_line_plan without a device ---------------------------------------------
D2 = (1.0e-4, 1.2e-4)
BASE = dict(n=(24, 20), d=D2, c0=C0, frames=5, t_max=1.03e-6)   # E = (48, 48)


def test_default_chunk_follows_the_byte_budget(second_order):
    plan = second_order.SecondOrderFrames.line_plan
    q = 25 * 25 * 5
    assert plan(line_row=0, n_times=12, **BASE) == ((256 << 20) // (25 * 5 * 8), 1, q)
    assert plan(line_row=19, n_times=12, line_chunk_times=5, **BASE) == (5, 3, q)
    assert plan(line_row=19, n_times=12, line_chunk_times=12, **BASE) == (12, 1, q)
    assert plan(line_row=None, n_times=1, line_chunk_times=1, **BASE) == (1, 1, q)
    # the measured shape: 64 frames of 256 x 256 in 512 x 512 take 2040 times per pass
    big = dict(BASE, n=(256, 256), frames=64, expanded=(512, 512))
    assert plan(line_row=0, n_times=1024, **big) == (2040, 1, 257 * 257 * 64)
    assert plan(line_row=0, n_times=4096, **big)[1] == 3
    # odd sides
    assert plan(line_row=3, n_times=9, line_chunk_times=4, **dict(BASE, expanded=(27, 33))) == (4, 3, 14 * 17 * 5)


REFUSALS = [
    (dict(line_row=20), "line_row: 20 is outside the plane's rows 0 ... 19 (-1: no record)"),
    (dict(line_row=-2), "line_row: -2 is outside the plane's rows 0 ... 19 (-1: no record)"),
    (dict(line_row=47), "line_row: 47 is outside the plane's rows 0 ... 19 (-1: no record)"),   # a row of the expansion
    (dict(n_times=0), "n_times: 0 is not a number of output times"),
    (dict(line_chunk_times=(1 << 32) // 240 + 1),
     "line_chunk_times: 17895698 times of 5 rows of 48 points are too many for one pass (2^32 points, 16776960 times)"),
    (dict(n=(0, 20)), "Nx: 0 is not a grid size"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(":")[0] + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_every_refusal_names_its_parameter(second_order, change, message):
    from kwave_amd import capi
    args = dict(BASE, line_row=0, n_times=12)
    args.update(change)
    with pytest.raises(capi.KWaveError) as e:
        second_order.SecondOrderFrames.line_plan(**args)
    assert str(e.value) == message


def test_python_front_end_checks_its_arguments(second_order):
    with pytest.raises(TypeError):
        second_order.SecondOrderFrames.line_plan(line_row=0, n_times=1, no_such=1, **BASE)


# ---- 4. the parameter, chunk and indexing code, stand-alone under the sanitizers ---------------------------------------------
def ok(row, chunk, passes, largest, q, g):
    return f"ok row={row} chunk={chunk} passes={passes} largest={largest} q={q} g={g}"


Q48 = 25 * 25 * 5
DEFAULT48 = (256 << 20) // (25 * 5 * 8)
EXPECTED = {
    "default": ok(0, DEFAULT48, 1, 12, Q48, 25 * 5 * 12),
    "last_row": ok(19, DEFAULT48, 1, 1, Q48, 25 * 5),
    "off": ok(-1, DEFAULT48, 1, 3, Q48, 25 * 5 * 3),
    "one_pass_exact": ok(7, 12, 1, 12, Q48, 25 * 5 * 12),
    "two_passes": ok(7, 7, 2, 7, Q48, 25 * 5 * 7),
    "single_times": ok(7, 1, 5, 1, Q48, 25 * 5),
    "odd_plane": ok(3, 4, 3, 4, 14 * 17 * 5, 14 * 5 * 4),
    "one_frame": ok(3, 5, 3, 5, 25 * 25, 25 * 5),
    "budget": ok(0, 2040, 1, 3, 257 * 257 * 64, 257 * 64 * 3),
    "budget_one_time": ok(0, 1, 2, 1, 513 * 9 * 65535, 513 * 65535),   # one time is over the budget: one at the least
    "row_below": REFUSALS[1][1],
    "row_at_ny": REFUSALS[0][1],
    "row_in_expansion": REFUSALS[2][1],
    "no_times": REFUSALS[3][1],
    "chunk_too_many_points": REFUSALS[4][1],
    "chunk_too_many_times": "line_chunk_times: 16776961 times of 1 rows of 1 points are too many for one pass",
    "chunk_overflow": "line_chunk_times: 18446744073709551615 times of 5 rows of 48 points are too many for one pass",
    "bad_grid": "Nx: 0 is not a grid size",
}


def test_host_line_record_code_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/second_order_line_record_host_check.cpp: the row rule, the times of a pass, the passes and the copy of
    every pass into the record, by its message"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "second_order_line_record_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "second_order_line_record_host_check.cpp"),
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


# ---- 5. declarations -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(second_order):
    from kwave_amd import capi
    assert set(ENTRY_POINTS) <= set(capi.declared_symbols())
    header = open(os.path.join(ROOT, "include", "kwave_hip.h")).read()
    for name, n in ENTRY_POINTS.items():
        assert len(capi._SIG[name]) == n, name
        decl = header.split("KW_API kw_status " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n, name
    host = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in HOST_ENTRIES:
        assert "kwh_second_order_frames_" + name + "(" in host, name
    assert C.sizeof(second_order.FramesConfig) == 14 * 8   # the config keeps its layout
    for name in ("line_record", "line_plan"):
        assert callable(getattr(second_order.SecondOrderFrames, name))
    for name in ("line_row", "line_chunk_times"):
        assert isinstance(getattr(second_order.SecondOrderFrames, name), property)


def test_libraries_export_the_entry_points():
    from kwave_amd import capi
    from kwave_amd.solver import load_host
    L, H = capi.load(), load_host()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    for name in HOST_ENTRIES:
        assert hasattr(H, "kwh_second_order_frames_" + name)
