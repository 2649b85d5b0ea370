"""Batched k-space line reconstruction, CPU side: the NumPy restatement (tests/line_recon_reference.py) against the plane
restatement with one lateral axis, on a record that depends on t only, against a full complex transform and against a 2-D
phantom whose record is propagated exactly, with the Lt^-2 convergence of the interpolation error; the device's float32
steps emulated against float64; the size rules and every refusal through kwh_line_recon_plan without a device; the host
code in a stand-alone program built with AddressSanitizer and UBSan; and the declarations.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import line_recon_reference as lr  # noqa: E402
import plane_recon_reference as pr  # noqa: E402

C0 = 1500.0
DX = 1.0e-4
DT = DX / (C0 * np.pi)
ENTRY_POINTS = {"kw_fused_set_frames", "kw_fused_line_recon", "kw_fft_create_plans_frames", "kw_fft_r2c_frames",
                "kw_fft_c2r_frames", "kw_line_recon_mix", "kw_line_recon_embed", "kw_line_recon_crop"}


@pytest.fixture(scope="module", autouse=True)
def recon():
    """without the reconstruction's class and entry points nothing in this file passes"""
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, recon
    assert ENTRY_POINTS <= set(capi._SIG)
    assert hasattr(recon, "LineRecon") and hasattr(recon, "plan_line_recon")
    return recon


# ---- 1. the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", lr.INTERPS)
@pytest.mark.parametrize("ey,lt,dy", [(20, 64, DX), (32, 59, DX), (48, 96, 0.8 * DX)], ids=["20x64", "32x59", "48x96"])
def test_line_restatement_is_the_plane_restatement_with_one_lateral_axis(ey, lt, dy, interp):
    """plane_recon_reference.stage on [Lt][1][Ey] (its second lateral axis of one point: ky = 0), and on a volume that is
    constant along that axis (six points, another spacing): every row is the line result.  Measured 0 and 3.4e-16 to
    4.0e-16."""
    first, second = lr.margins(ey, lt, dy, DT, C0)
    assert first >= 1e-9 and second >= 1e-9
    assert (first, second) == pytest.approx(pr.margins((ey, 1), lt, (dy, dy), DT, C0), rel=1e-12)
    v = lr.even_frames((1, lt, ey), 20261020)[0].astype(np.float64)
    a = lr.stage(v, dy, DT, C0, interp)
    b = pr.stage(v[:, None, :], (dy, dy), DT, C0, interp)[:, 0, :]
    err = lr.rel_l2(a, b)
    rows = pr.stage(np.repeat(v[:, None, :], 6, axis=1), (dy, 1.3 * dy), DT, C0, interp)
    worst = max(lr.rel_l2(a, rows[:, r, :]) for r in range(6))
    print(f"line against plane at Ey = 1 on {ey} x {lt} {interp}: {err:.3e}; rows of a constant volume {worst:.3e}")
    assert err <= 1e-12 and worst <= 1e-12


@pytest.mark.parametrize("lt", [79, 80, 96])
def test_record_of_t_alone_gives_back_its_profile(lt):
    """p = g(c0 t) / 2 on every sensor: rho2 = 0 on the only bins that carry anything, f = m' and w = 1, so the image is
    g(x) to rounding.  Measured 1.6e-16 to 2.2e-16."""
    rec, g = lr.identity_record(40, 6)
    assert g[-1] < 1e-30  # the Gaussian is inside the record
    for interp in lr.INTERPS:
        out = lr.reconstruct(rec, 6, lt, DX, 1.0e-7, C0, interp=interp)
        err = float(np.max(np.abs(out - g[:, None])))
        print(f"identity Lt = {lt} {interp}: max error {err:.3e}")
        assert err <= 1e-12


@pytest.mark.parametrize("interp", lr.INTERPS)
@pytest.mark.parametrize("lt", [59, 64], ids=["odd", "even"])
def test_real_transform_form_equals_the_complex_form(lt, interp):
    """2 irfft2(G) on the half-spectrum against 2 ifft2(G) on all bins.  Measured 2.8e-16 to 3.1e-16."""
    dy = 1.2e-4
    first, second = lr.margins(12, lt, dy, DT, C0)
    assert first >= 1e-9 and second >= 1e-9
    v = lr.even_frames((1, lt, 12), 20261019)[0].astype(np.float64)
    a, b = lr.stage(v, dy, DT, C0, interp), lr.stage_complex(v, dy, DT, C0, interp)
    err = lr.rel_l2(a, b.real)
    print(f"real against complex form, Lt = {lt} {interp}: {err:.3e}, imaginary part {np.max(np.abs(b.imag)):.3e}")
    assert err <= 1e-12
    assert np.max(np.abs(b.imag)) <= 1e-12 * np.max(np.abs(a))


@pytest.fixture(scope="module")
def phantom():
    return lr.phantom_case()


# relative L2 over the first 64 rows, measured with this restatement: (Lt: figure)
PHANTOM_FIGURES = {"linear": {199: 3.05e-2, 256: 1.94e-2, 512: 4.65e-3, 1024: 1.20e-3},
                   "nearest": {199: 8.45e-2, 256: 7.01e-2, 512: 2.73e-2, 1024: 1.01e-2}}


@pytest.mark.parametrize("interp", lr.INTERPS)
def test_phantom_is_recovered_and_the_error_falls_with_the_record_length(phantom, interp):
    """The record of the 2-D phantom on the line x = 0 (exact propagation, Nt = 100, dt = dx / c0, tail 3.7e-5 of the peak)
    reconstructs the phantom; what is left is the interpolation error along w, which falls as Lt^-2 for the linear
    interpolant (Lt = 199 is k-Wave's own grid).  Each figure within 10 % above the one measured; linear at 1024 at least
    10 times better than at 256 (measured 16 times)."""
    rec, p0 = phantom
    assert np.max(np.abs(rec[-1])) <= 1e-4 * np.max(np.abs(rec))
    got = {}
    for lt, figure in PHANTOM_FIGURES[interp].items():
        out = lr.reconstruct(rec, 16, lt, 1.0, 1.0, 1.0, depth=64, interp=interp)
        got[lt] = lr.rel_l2(out, p0[:64])
        print(f"phantom {interp} Lt = {lt}: {got[lt]:.4e} (figure {figure:.3e})")
        assert got[lt] <= 1.10 * figure, (lt, got[lt])
    if interp == "linear":
        assert got[1024] * 10.0 <= got[256]


@pytest.mark.parametrize("interp", lr.INTERPS)
@pytest.mark.parametrize("ey,lt", [(32, 64), (48, 96), (20, 79)], ids=["32x64", "48x96", "20x79"])
def test_device_steps_in_float32_against_float64(ey, lt, interp):
    """The weight, the interpolation weight and the lerp in float32 (float64 to the square roots and i0) against the
    float64 restatement, on the spectrum rounded to float32.  Measured 4.4e-8 to 6.3e-8 against the project's 1e-5."""
    first, second = lr.margins(ey, lt, DX, DT, C0)
    assert first >= 1e-9 and second >= 1e-9
    v = lr.even_frames((1, lt, ey), 3)[0]
    err = lr.rel_l2(lr.stage_device(v, DX, DT, C0, interp), lr.stage(v, DX, DT, C0, interp))
    print(f"float32 device steps against float64 on {ey} x {lt} {interp}: {err:.3e}")
    assert err <= 1e-5


def test_frames_are_independent_and_the_embedding_is_even_in_time():
    p = np.arange(2 * 3 * 2, dtype=np.float64).reshape(2, 3, 2) + 1.0
    v = lr.embed(p, 3, 6)
    assert v.shape == (2, 6, 3)
    for f in range(2):
        assert np.array_equal(v[f, :3, :2], p[f]) and np.array_equal(v[f, 5, :2], p[f, 1]) and np.array_equal(v[f, 4, :2], p[f, 2])
        assert not v[f, 3].any() and not v[f, :, 2].any()
        for n in range(1, 6):
            assert np.array_equal(v[f, 6 - n], v[f, n])
    assert np.array_equal(lr.embed(p[0], 2, 5)[3], p[0, 2])
    both = lr.reconstruct(p, 4, 8, DX, DT, C0)
    for f in range(2):
        assert np.array_equal(both[f], lr.reconstruct(p[f], 4, 8, DX, DT, C0))


# ---- 2. the rules and the refusals, through kwh_line_recon_plan without a device -------------------------------------------
RULE_TABLE = [  # ny, nt, frames, fused, extra -> Ey, Lt, depth, chunk_frames, fast
    (24, 40, 6, True, {}, (24, 80, 40, 6, False)),                      # Ey = Ny, no fast-path length: the twin on a fast Lt
    (32, 40, 6, True, {}, (32, 80, 40, 6, True)),
    (32, 40, 6, False, {}, (32, 79, 40, 6, False)),                     # off the fused pipeline: k-Wave's own grid, odd
    (24, 30, 1, True, dict(expanded=32), (32, 64, 30, 1, True)),
    (16, 512, 3, True, {}, (16, 1024, 512, 3, True)),
    (16, 513, 3, True, {}, (16, 1025, 513, 3, False)),                  # no fast length above 1024
    (21, 1, 2, True, {}, (21, 16, 1, 2, False)),
    (24, 30, 7, True, dict(expanded=32, chunk_frames=3, depth=17), (32, 64, 17, 3, True)),
    (24, 30, 4, True, dict(expanded=32, time_length=59), (32, 59, 30, 4, False)),
    (600, 50, 4, True, dict(expanded=672, time_length=100, chunk_frames=1), (672, 100, 50, 1, False)),  # 100 rows: no whole x tiles
    (600, 50, 4, True, dict(expanded=672, time_length=100, chunk_frames=4), (672, 100, 50, 4, True)),   # 400 rows: 25 tiles
    (600, 50, 4, True, dict(expanded=640, time_length=100, chunk_frames=1), (640, 100, 50, 1, True)),   # masked x kernels exist
    (1024, 512, 5000, True, {}, (1024, 1024, 512, 992, True)),          # capped: 993 frames x 528 x 1024 bins pass 2^29
    (128, 512, 10000, True, {}, (128, 1024, 512, 6553, True)),          # 6553 x 80 x 1024 bins x 8 B end below 4 GiB, 6554 do not
    (128, 512, 10000, True, dict(chunk_frames=6553), (128, 1024, 512, 6553, True)),
    (128, 512, 10000, False, {}, (128, 1023, 512, 6560, False)),        # one rule on both paths: 80 x 1023 bins per frame
    (16, 8, 100000, True, {}, (16, 16, 8, 65535, True)),                # the frame is a block index: at most 65535 per chunk
]


@pytest.mark.parametrize("ny,nt,frames,fused,extra,want", RULE_TABLE)
def test_default_sizes_follow_the_rule(recon, ny, nt, frames, fused, extra, want):
    got = recon.plan_line_recon(ny, 1e-3, 2e-7, nt, C0, frames=frames, fused_kernels=fused, **extra)
    assert got == want
    assert got == lr.plan(ny, nt, frames, fused, **extra)
    assert got[1] >= 2 * nt - 1 and got[3] <= frames


def test_lengths_without_masked_x_kernels_match_the_source():
    """LineReconParameters.cpp and the restatement repeat has_partial_x_tiles of csrc/kw_fused.hip; their x tiles take
    2 nl_x = 16 rows"""
    csrc = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "csrc", "kw_fused.hip")
    src = open(csrc).read()
    body = src.split("constexpr bool has_partial_x_tiles(int L)", 1)[1].split("default:", 1)[0]
    listed = tuple(int(x) for x in re.findall(r"case (\d+):", body))
    assert listed == lr.NO_PARTIAL_X_TILES
    host = open(os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host", "LineReconParameters.cpp")).read()
    table = host.split("kNoPartialTiles[] = {", 1)[1].split("}", 1)[0]
    assert tuple(int(x) for x in table.split(",")) == listed
    nlx = src.split("constexpr int nl_x(int L)", 1)[1].split("#endif", 1)[0]
    special = [int(x) for x in re.findall(r"case (\d+):", nlx)]
    assert not set(listed) & set(special) and "return L >= 400 ? 8 : 16;" in nlx and min(listed) >= 400
    assert lr.ROWS_PER_TILE == 16


REFUSALS = [
    (dict(ny=0), "Ny: 0 is not a grid size"),
    (dict(nt=0), "Nt: 0 is not a grid size"),
    (dict(frames=0), "frames: 0 is not a grid size"),
    (dict(dy=0.0), "dy: 0.000000 is not a positive spacing"),
    (dict(dy=float("nan")), "dy: nan is not a positive spacing"),
    (dict(dt=0.0), "dt: 0.000000 is not a positive time step"),
    (dict(dt=-1.0), "dt: -1.000000 is not a positive time step"),
    (dict(c0=0.0), "c0: 0.000000 is not a positive sound speed"),
    (dict(c0=float("inf")), "c0: inf is not a positive sound speed"),
    (dict(depth=41), "depth: 41 is above Nt = 40"),
    (dict(expanded=23), "Ey: 23 is below Ny = 24"),
    (dict(time_length=78), "Lt: 78 is below 2 Nt - 1 = 79"),
    (dict(chunk_frames=7), "chunk_frames: 7 is above frames = 6"),
    (dict(expanded=1024, time_length=1024, frames=5000, chunk_frames=993),
     "chunk_frames: 993 frames of 1024 x 1024 points is not below 2^29 bins of 528 per row (at most 992)"),
    (dict(ny=128, nt=512, frames=10000, chunk_frames=6554),
     "chunk_frames: 6554 frames of 128 x 1024 points is not below 2^29 bins of 80 per row (at most 6553)"),
    (dict(ny=16, nt=8, frames=100000, chunk_frames=65536), "chunk_frames: 65536 is above 65535, the most one chunk takes"),
    (dict(expanded=1 << 22, time_length=1024), "E: 4194304 x 1024 points of one frame is not below 2^29 bins of 2097168 per row"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(":")[0] + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_every_refusal_names_its_parameter(recon, change, message):
    from kwave_amd import capi
    args = dict(ny=24, dy=1e-3, dt=2e-7, nt=40, c0=C0, frames=6)
    args.update(change)
    with pytest.raises(capi.KWaveError) as e:
        recon.plan_line_recon(**args)
    assert str(e.value) == message
    with pytest.raises(capi.KWaveError) as e:   # the same from create, before any device is looked for
        recon.LineRecon(**args)
    assert str(e.value) == message


def test_interpolant_and_order_are_refused_by_name(recon):
    from kwave_amd import capi
    with pytest.raises(ValueError, match="interp must be one of"):
        recon.plan_line_recon(24, 1e-3, 2e-7, 40, C0, interp="cubic")
    with pytest.raises(ValueError, match="order must be"):
        recon.LineRecon(24, 1e-3, 2e-7, 40, C0, order="xy")
    L = recon._lib()
    c = recon._line_config(24, 1e-3, 2e-7, 40, C0, 1, None, "linear", False, None, None, None)
    c.interp = 2
    o = recon.Options()
    with pytest.raises(capi.KWaveError) as e:
        recon._check(L.kwh_line_recon_plan(C.byref(c), C.byref(o), None, None))
    assert str(e.value) == "interp: 2 is neither linear (0) nor nearest (1)"


# ---- 3. the host code, stand-alone under the sanitizers --------------------------------------------------------------------
EXPECTED = {
    "default": "ok Ey=24 Lt=80 depth=40 chunk=6 chunks=1 fast=0 dx=3.000000e-04",
    "rocfft": "ok Ey=24 Lt=79 depth=40 chunk=6 chunks=1 fast=0",
    "fast_axis": "ok Ey=32 Lt=80 depth=40 chunk=6 chunks=1 fast=1",
    "beyond_1024": "ok Ey=24 Lt=1025 depth=513 chunk=6 chunks=1 fast=0",
    "given": "ok Ey=32 Lt=96 depth=17 chunk=4 chunks=2 fast=1",
    "given_odd": "ok Ey=25 Lt=81 depth=40 chunk=6 chunks=1 fast=0",
    "nearest": "ok Ey=24 Lt=80 depth=40 chunk=6 chunks=1 fast=0",
    "no_masked_tiles_one": "ok Ey=672 Lt=100 depth=40 chunk=1 chunks=6 fast=0",
    "no_masked_tiles_four": "ok Ey=672 Lt=100 depth=40 chunk=4 chunks=2 fast=1",
    "chunk_capped": "ok Ey=1024 Lt=1024 depth=40 chunk=992 chunks=6 fast=1",
    "chunk_at_byte_limit": "ok Ey=128 Lt=1024 depth=512 chunk=6553 chunks=2 fast=1",
    "chunk_past_byte_limit": "chunk_frames: 6554 frames of 128 x 1024 points is not below 2^29 bins of 80 per row (at most 6553)",
    "chunk_block_index": "ok Ey=16 Lt=16 depth=8 chunk=65535 chunks=2 fast=1",
    "chunk_past_block_index": "chunk_frames: 65536 is above 65535, the most one chunk takes",
    "depth_above": "depth: 41 is above Nt = 40",
    "interp_other": "interp: 2 is neither linear (0) nor nearest (1)",
    "ny_zero": "Ny: 0 is not a grid size",
    "nt_zero": "Nt: 0 is not a grid size",
    "frames_zero": "frames: 0 is not a grid size",
    "dy_zero": "dy: 0.000000 is not a positive spacing",
    "dt_zero": "dt: 0.000000 is not a positive time step",
    "c0_negative": "c0: -1.000000 is not a positive sound speed",
    "lt_small": "Lt: 78 is below 2 Nt - 1 = 79",
    "ey_small": "Ey: 23 is below Ny = 24",
    "chunk_above": "chunk_frames: 7 is above frames = 6",
    "chunk_too_large": "chunk_frames: 993 frames of 1024 x 1024 points is not below 2^29 bins of 528 per row (at most 992)",
    "too_large": "E: 4194304 x 1024 points of one frame is not below 2^29 bins of 2097168 per row",
}


def test_host_parameters_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/line_recon_host_check.cpp: LineReconParameters::init through valid inputs and refusals, by its
    message"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "line_recon_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "line_recon_host_check.cpp"),
           os.path.join(host, "LineReconParameters.cpp"), os.path.join(host, "GridRules.cpp"), "-o", exe]
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
def test_entry_points_are_declared_and_bound(recon):
    from kwave_amd import capi
    assert ENTRY_POINTS <= set(capi.declared_symbols())
    counts = {"kw_fused_set_frames": 2, "kw_fused_line_recon": 4, "kw_fft_create_plans_frames": 1, "kw_fft_r2c_frames": 3,
              "kw_fft_c2r_frames": 3, "kw_line_recon_mix": 5, "kw_line_recon_embed": 8, "kw_line_recon_crop": 9}
    header = open(os.path.join(ROOT, "include", "kwave_hip.h")).read()
    for name, n in counts.items():
        assert len(capi._SIG[name]) == n, name
        decl = header.split("KW_API kw_status " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n, name
    host = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in ("plan", "create", "destroy", "run", "get", "get_scalar", "context"):
        assert "kwh_line_recon_" + name + "(" in host, name
    assert C.sizeof(recon.LineConfig) == 11 * 8
    struct = host.split("typedef struct kwh_line_recon_config", 1)[1].split("} kwh_line_recon_config;", 1)[0]
    fields = [f.strip() for line in re.findall(r"^\s*(?:uint64_t|double|int32_t)\s+([^;]+);", struct, re.M) for f in line.split(",")]
    assert fields == [name for name, _ in recon.LineConfig._fields_]
    for name in ("run", "close"):
        assert callable(getattr(recon.LineRecon, name))
    for name in ("dx", "time_length", "expanded", "chunk_frames", "fused", "runs", "ctx"):
        assert isinstance(getattr(recon.LineRecon, name), property)


def test_library_exports_the_entry_points():
    from kwave_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
    from kwave_amd import solver
    H = solver.load_host()
    for name in ("plan", "create", "destroy", "run", "get", "get_scalar", "context"):
        assert hasattr(H, "kwh_line_recon_" + name)
