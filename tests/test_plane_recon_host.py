"""k-space plane reconstruction, CPU side: the NumPy restatement (tests/plane_recon_reference.py) on a record that depends on
t only, against a full complex transform and against a phantom whose record is propagated exactly, with the Lt^-2
convergence of the interpolation error; the device's float32 steps emulated against float64; the margins; the size rules
and every refusal through kwh_plane_recon_plan without a device; the host code in a stand-alone program built with
AddressSanitizer and UBSan; and the declarations.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_recon_reference as pr  # noqa: E402

C0 = 1500.0
ENTRY_POINTS = {"kw_fused_plane_recon", "kw_plane_recon_mix", "kw_plane_recon_embed", "kw_plane_recon_crop"}


@pytest.fixture(scope="module", autouse=True)
def recon():
    """without the reconstruction's module and entry points nothing in this file passes"""
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, recon
    assert ENTRY_POINTS <= set(capi._SIG)
    return recon


# ---- 1. the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lt", [79, 80, 96])
def test_record_of_t_alone_gives_back_its_profile(lt):
    """p = g(c0 t) / 2 on every sensor point: rho2 = 0 on the only bins that carry anything, f = m' and w = 1, so the
    reconstruction is g(z) to rounding.  Measured 1.2e-16 to 4.4e-16."""
    dx, dt = 1.0e-4, 1.0e-7
    rec, g = pr.identity_record(40, 4, 4, C0, dt)
    assert g[-1] < 1e-30  # the Gaussian is inside the record
    for interp in pr.INTERPS:
        out = pr.reconstruct(rec, (4, 4), lt, (dx, dx), dt, C0, interp=interp)
        err = float(np.max(np.abs(out - g[:, None, None])))
        print(f"identity Lt = {lt} {interp}: max error {err:.3e}")
        assert err <= 1e-12


@pytest.mark.parametrize("interp", pr.INTERPS)
@pytest.mark.parametrize("lt", [59, 64], ids=["odd", "even"])
def test_real_transform_form_equals_the_complex_form(lt, interp):
    """2 irfftn(G) on the half-spectrum against 2 ifftn(G) on all bins.  Measured 3.8e-16 to 4.0e-16."""
    spacing = (1.0e-4, 1.2e-4)
    dt = spacing[0] / (C0 * np.pi)
    first, second = pr.margins((10, 12), lt, spacing, dt, C0)
    assert first >= 1e-9 and second >= 1e-9
    v = pr.even_volume((lt, 12, 10), 20261019).astype(np.float64)
    a, b = pr.stage(v, spacing, dt, C0, interp), pr.stage_complex(v, spacing, dt, C0, interp)
    err = pr.rel_l2(a, b.real)
    print(f"real against complex form, Lt = {lt} {interp}: {err:.3e}, imaginary part {np.max(np.abs(b.imag)):.3e}")
    assert err <= 1e-12
    assert np.max(np.abs(b.imag)) <= 1e-12 * np.max(np.abs(a))


@pytest.fixture(scope="module")
def phantom():
    return pr.phantom_case()


# relative L2 over the first 64 planes, measured with this restatement: (Lt: figure)
PHANTOM_FIGURES = {"linear": {199: 3.36e-2, 256: 2.14e-2, 512: 5.13e-3, 1024: 1.33e-3},
                   "nearest": {199: 9.33e-2, 256: 7.74e-2, 512: 3.02e-2, 1024: 1.12e-2}}


@pytest.mark.parametrize("interp", pr.INTERPS)
def test_phantom_is_recovered_and_the_error_falls_with_the_record_length(phantom, interp):
    """The record of the phantom at z = 0 (exact propagation, Nt = 100, dt = dx / c0, tail 5e-5 of the peak) reconstructs
    the phantom; what is left is the interpolation error along w, which falls as Lt^-2 for the linear interpolant
    (Lt = 199 is k-Wave's own grid).  Each figure within 10 % above the one measured; linear at 1024 at least 10 times
    better than at 256 (measured 16 times)."""
    rec, p0 = phantom
    assert np.max(np.abs(rec[-1])) <= 1e-4 * np.max(np.abs(rec))
    got = {}
    for lt, figure in PHANTOM_FIGURES[interp].items():
        out = pr.reconstruct(rec, (16, 16), lt, (1.0, 1.0), 1.0, 1.0, planes=64, interp=interp)
        got[lt] = pr.rel_l2(out, p0[:64])
        print(f"phantom {interp} Lt = {lt}: {got[lt]:.4e} (figure {figure:.3e})")
        assert got[lt] <= 1.10 * figure, (lt, got[lt])
    if interp == "linear":
        assert got[1024] * 10.0 <= got[256]


EMULATION_GRIDS = [((32, 48), 64), ((48, 16), 96), ((20, 24), 79)]


@pytest.mark.parametrize("interp", pr.INTERPS)
@pytest.mark.parametrize("expanded,lt", EMULATION_GRIDS, ids=["32x48x64", "48x16x96", "20x24x79"])
def test_device_steps_in_float32_against_float64(expanded, lt, interp):
    """The weight, the interpolation weight and the lerp in float32 (float64 to the square roots and i0) against the
    float64 restatement, on the spectrum rounded to float32.  Measured 4.7e-8 to 6.9e-8 against the project's 1e-5."""
    dx = 1.0e-4
    dt = dx / (C0 * np.pi)
    first, second = pr.margins(expanded, lt, (dx, dx), dt, C0)
    assert first >= 1e-9 and second >= 1e-9
    v = pr.even_volume((lt, expanded[1], expanded[0]), 3)
    err = pr.rel_l2(pr.stage_device(v, (dx, dx), dt, C0, interp), pr.stage(v, (dx, dx), dt, C0, interp))
    print(f"float32 device steps against float64 on {expanded} x {lt} {interp}: {err:.3e}")
    assert err <= 1e-5


def test_margins_measure_both_discontinuities():
    """a grid built to put a bin on each: rho2 = 9 at (ix, iy) = (3, 0) with dkx = dk gives f = 5 = M at m' = 4 (Lt = 10);
    rho2 = 2.25 at ix = 3 with dkx = dk / 2 gives f = 2.5 at m' = 2"""
    lt, dt = 10, 1.0e-7
    dx = lt * dt * C0 / 16.0                      # dkx = 2 pi / (16 dx) = dk
    assert pr.margins((16, 16), lt, (dx, dx), dt, C0)[0] <= 1e-12
    first, second = pr.margins((16, 16), lt, (2.0 * dx, 2.0 * dx), dt, C0)
    assert second <= 1e-12
    first, second = pr.margins((16, 16), 64, (1e-4, 1e-4), 1e-4 / (C0 * np.pi), C0)
    assert first >= 1e-9 and second >= 1e-9


def test_embedding_is_even_in_time():
    p = np.arange(3 * 2 * 2, dtype=np.float64).reshape(3, 2, 2) + 1.0
    v = pr.embed(p, (3, 2), 6)
    assert v.shape == (6, 2, 3)
    assert np.array_equal(v[:3, :, :2], p) and np.array_equal(v[5, :, :2], p[1]) and np.array_equal(v[4, :, :2], p[2])
    assert not v[3].any() and not v[:, :, 2].any()
    for n in range(1, 6):
        assert np.array_equal(v[6 - n], v[n])
    assert np.array_equal(pr.embed(p, (2, 2), 5)[3], p[2])


# ---- 2. the rules and the refusals, through kwh_plane_recon_plan without a device ------------------------------------------
RULE_TABLE = [  # dims, nt, fused -> expanded, Lt, fast
    ((24, 20), 40, True, (24, 20), 80, False),           # E = (Nx, Ny), not fast-path sides: the twin on a fast Lt
    ((32, 48), 40, True, (32, 48), 80, True),
    ((32, 48), 40, False, (32, 48), 79, False),          # off the fused pipeline: k-Wave's own grid, odd
    ((32, 48), 30, True, (32, 48), 64, True),
    ((16, 16), 100, True, (16, 16), 200, True),
    ((16, 16), 512, True, (16, 16), 1024, True),
    ((16, 16), 513, True, (16, 16), 1025, False),        # no fast length above 1024
    ((21, 17), 1, True, (21, 17), 16, False),
]


@pytest.mark.parametrize("dims,nt,fused,expanded,lt,fast", RULE_TABLE)
def test_default_sides_and_time_length_follow_the_rule(recon, dims, nt, fused, expanded, lt, fast):
    got = recon.plan_recon(dims, (1e-3, 1e-3), 2e-7, nt, C0, fused_kernels=fused)
    assert got == (expanded, lt, fast)
    assert got == pr.plan_recon(dims, nt, fused)
    assert lt >= 2 * nt - 1


def test_given_sides_and_time_length_are_kept(recon):
    args = ((24, 20), (1e-3, 1e-3), 2e-7, 30, C0)
    assert recon.plan_recon(*args, expanded=(32, 32)) == ((32, 32), 64, True)
    assert recon.plan_recon(*args, expanded=(32, 32), time_length=59) == ((32, 32), 59, False)
    assert recon.plan_recon(*args, expanded=(32, 32), time_length=96, fused_kernels=False) == ((32, 32), 96, False)
    assert recon.plan_recon(*args, expanded=(25, 21), time_length=61) == ((25, 21), 61, False)
    assert recon.plan_recon(*args, planes=30, interp="nearest", positivity=True) == ((24, 20), 64, False)


REFUSALS = [
    (dict(dims=(0, 20)), "Nx: 0 is not a grid size"),
    (dict(dims=(24, 0)), "Ny: 0 is not a grid size"),
    (dict(nt=0), "Nt: 0 is not a grid size"),
    (dict(spacing=(0.0, 1e-3)), "dx: 0.000000 is not a positive spacing"),
    (dict(spacing=(1e-3, float("nan"))), "dy: nan is not a positive spacing"),
    (dict(dt=0.0), "dt: 0.000000 is not a positive time step"),
    (dict(dt=-1.0), "dt: -1.000000 is not a positive time step"),
    (dict(c0=0.0), "c0: 0.000000 is not a positive sound speed"),
    (dict(c0=float("inf")), "c0: inf is not a positive sound speed"),
    (dict(planes=41), "planes: 41 is above Nt = 40"),
    (dict(expanded=(24, 0)), "Ey: missing while the other side of the expanded grid is given"),
    (dict(expanded=(0, 20)), "Ex: missing while the other side of the expanded grid is given"),
    (dict(expanded=(24, 18)), "Ey: 18 is below N = 20"),
    (dict(expanded=(23, 20)), "Ex: 23 is below N = 24"),
    (dict(time_length=78), "Lt: 78 is below 2 Nt - 1 = 79"),
    (dict(expanded=(2048, 2048), time_length=1024), "E: 2048 x 2048 x 1024 points is not below 2^32"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(":")[0] + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_every_refusal_names_its_parameter(recon, change, message):
    from kwave_amd import capi
    args = dict(dims=(24, 20), spacing=(1e-3, 1e-3), dt=2e-7, nt=40, c0=C0)
    args.update(change)
    with pytest.raises(capi.KWaveError) as e:
        recon.plan_recon(**args)
    assert str(e.value) == message
    with pytest.raises(capi.KWaveError) as e:   # the same from create, before any device is looked for
        recon.PlaneRecon(**args)
    assert str(e.value) == message


def test_interpolant_is_refused_by_name(recon):
    from kwave_amd import capi
    with pytest.raises(ValueError, match="interp must be one of"):
        recon.plan_recon((24, 20), (1e-3, 1e-3), 2e-7, 40, C0, interp="cubic")
    L = recon._lib()
    c = recon._config((24, 20), (1e-3, 1e-3), 2e-7, 40, C0, None, "linear", False, None, None)
    c.interp = 2
    o = recon.Options()
    with pytest.raises(capi.KWaveError) as e:
        recon._check(L.kwh_plane_recon_plan(C.byref(c), C.byref(o), None, None))
    assert str(e.value) == "interp: 2 is neither linear (0) nor nearest (1)"


# ---- 3. the host code, stand-alone under the sanitizers --------------------------------------------------------------------
EXPECTED = {
    "default": "ok E=24x20 Lt=80 planes=40 fast=0 dz=3.000000e-04",
    "rocfft": "ok E=24x20 Lt=79 planes=40 fast=0",
    "fast_sides": "ok E=32x48 Lt=80 planes=40 fast=1",
    "beyond_1024": "ok E=24x20 Lt=1025 planes=513 fast=0",
    "given": "ok E=32x32 Lt=96 planes=17 fast=1",
    "given_odd": "ok E=25x21 Lt=81 planes=40 fast=0",
    "nearest": "ok E=24x20 Lt=80 planes=40 fast=0",
    "planes_nt": "ok E=24x20 Lt=80 planes=40 fast=0",
    "planes_above": "planes: 41 is above Nt = 40",
    "interp_other": "interp: 2 is neither linear (0) nor nearest (1)",
    "nx_zero": "Nx: 0 is not a grid size",
    "nt_zero": "Nt: 0 is not a grid size",
    "dt_zero": "dt: 0.000000 is not a positive time step",
    "c0_negative": "c0: -1.000000 is not a positive sound speed",
    "lt_small": "Lt: 78 is below 2 Nt - 1 = 79",
    "e_missing": "Ey: missing while the other side of the expanded grid is given",
    "e_small": "Ey: 18 is below N = 20",
    "too_large": "E: 2048 x 2048 x 1024 points is not below 2^32",
}


def test_host_parameters_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/plane_recon_host_check.cpp: PlaneReconParameters::init through valid inputs and refusals, by its
    message"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "plane_recon_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "plane_recon_host_check.cpp"),
           os.path.join(host, "PlaneReconParameters.cpp"), os.path.join(host, "GridRules.cpp"), "-o", exe]
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
    counts = {"kw_fused_plane_recon": 4, "kw_plane_recon_mix": 5, "kw_plane_recon_embed": 9, "kw_plane_recon_crop": 10}
    header = open(os.path.join(ROOT, "include", "kwave_hip.h")).read()
    for name, n in counts.items():
        assert len(capi._SIG[name]) == n, name
        decl = header.split("KW_API kw_status " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n, name
    host = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in ("plan", "create", "destroy", "run", "get", "get_scalar", "context"):
        assert "kwh_plane_recon_" + name + "(" in host, name
    assert C.sizeof(recon.Config) == 12 * 8
    assert C.sizeof(capi.PlaneReconOp) == 5 * 8
    for name in ("run", "close"):
        assert callable(getattr(recon.PlaneRecon, name))
    for name in ("dz", "time_length", "expanded", "fused", "runs", "ctx"):
        assert isinstance(getattr(recon.PlaneRecon, name), property)


def test_library_exports_the_entry_points():
    from kwave_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)
