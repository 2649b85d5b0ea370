"""Time-domain angular-spectrum projector, CPU side: the NumPy restatement (tests/angular_time_reference.py) against the CW
restatement for a one-bin sinusoid, against a full complex transform and against the exact field of a pulsed aperture; the
device's float32 steps emulated against float64 H; the size rules and every refusal through kwh_angular_time_plan without a
device; the host code in a stand-alone program built with AddressSanitizer and UBSan; and the declarations.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import angular_reference as ar  # noqa: E402
import angular_time_reference as tr  # noqa: E402

C0 = 1500.0
ENTRY_POINTS = {"kw_fused_angular_time_forward", "kw_fused_angular_time_plane", "kw_angular_time_mix",
                "kw_angular_time_embed", "kw_angular_time_reduce"}


@pytest.fixture(scope="module", autouse=True)
def angular():
    """without the projector's entry points nothing in this file passes"""
    import kwave_amd  # noqa: F401
    from kwave_amd import angular, capi
    assert ENTRY_POINTS <= set(capi._SIG)
    return angular


# ---- 1. the restatement -------------------------------------------------------------------------------------------------
def coeff_for(alpha_np, f, y):
    """alpha_coeff [dB / (MHz^y cm)] that gives alpha_np [Np/m] at f [Hz]"""
    return alpha_np / ((f * 1e-6) ** y * 100.0 * tr.NEPER_PER_DB)


@pytest.mark.parametrize("alpha_np", [0.0, 30.0], ids=["lossless", "absorbing"])
@pytest.mark.parametrize("restrict", [True, False], ids=["restricted", "unrestricted"])
def test_one_bin_sinusoid_is_the_cw_projection(alpha_np, restrict):
    """Re(P0 exp(i w t)) with Nt = Lt on bin 5 against Re(P(z) exp(i w t)) of angular_reference.project.  Measured 2.4e-15 to
    3.2e-15."""
    dx, dy, nt, m = 1.0e-3, 0.8e-3, 48, 5
    dt = dx / (C0 * np.pi)
    w = 2.0 * np.pi * m / (nt * dt)
    k = w / C0
    rng = np.random.default_rng(20261019)
    P0 = rng.standard_normal((20, 24)) + 1j * rng.standard_normal((20, 24))
    carrier = np.exp(1j * w * np.arange(nt) * dt)[:, None, None]
    p0 = np.real(P0[None] * carrier)
    zs = (0.5e-3, 4.4e-3)
    first, second = tr.margins((48, 48), nt, (dx, dy), dt, C0, zs)
    assert first >= 1e-9 and second >= 1e-9
    coeff = coeff_for(alpha_np, w / (2.0 * np.pi), 1.5)
    out = tr.project(p0, (48, 48), nt, (dx, dy), dt, C0, zs, alpha_coeff=coeff, alpha_power=1.5, restrict=restrict)
    for j, z in enumerate(zs):
        P = ar.project(P0, (dx, dy), k, alpha_np, z, 1e-3, 1, (48, 48), restrict)[0]
        err = tr.rel_l2(out[j], np.real(P[None] * carrier))
        print(f"one-bin sinusoid against the CW restatement, alpha {alpha_np}, restriction {restrict}, z {z}: {err:.3e}")
        assert err <= 1e-12


def test_real_transform_form_equals_the_complex_form():
    rng = np.random.default_rng(20261020)
    p0 = rng.standard_normal((30, 20, 24))
    dx, dy = 1.0e-3, 0.8e-3
    dt = dx / (C0 * np.pi)
    for coeff, restrict, retarded in ((0.0, True, False), (0.0, False, True), (0.6, True, True), (0.6, False, False)):
        kw = dict(alpha_coeff=coeff, alpha_power=1.5, restrict=restrict, retarded=retarded)
        a = tr.solve_expanded(p0, (48, 40), 32, (dx, dy), dt, C0, 2.3e-3, **kw)
        b = tr.solve_complex(p0, (48, 40), 32, (dx, dy), dt, C0, 2.3e-3, **kw)
        err = tr.rel_l2(a, b)
        print(f"irfftn form against fftn form, alpha_coeff {coeff}, restriction {restrict}, retarded {retarded}: {err:.3e}")
        assert err <= 1e-14
        assert np.abs(b.imag).max() <= 1e-14 * np.abs(b.real).max()


@pytest.fixture(scope="module")
def aperture():
    return tr.aperture_case()


@pytest.mark.parametrize("retarded", [False, True], ids=["absolute", "retarded"])
def test_restatement_gives_the_pulsed_aperture_field(aperture, retarded):
    """the signs, the retarded shift and the crop against sum w g(t - r / c0) / (4 pi r): a 3-cycle Gaussian tone burst
    (envelope three periods wide at half maximum) at 5 points per wavelength, 24 x 24 plane in E = 48, Nt = 200 in Lt = 256,
    projected over 3, 6, 9 and 12 dx.  Measured: 2.7e-3 to 5.5e-3 relative L2, peak map within 9.6e-4 of its maximum; the
    remainder is the lateral truncation of a broadband plane."""
    c = aperture
    out = tr.project(c["p0"], c["expanded"], c["lt"], (c["dx"], c["dx"]), c["dt"], c["c0"], c["zs"], restrict=True,
                     retarded=retarded)
    for j, z in enumerate(c["zs"]):
        exact = tr.aperture_exact(c, z, retarded)
        err = tr.rel_l2(out[j], exact)
        peak = float(np.abs(out[j].max(axis=0) - exact.max(axis=0)).max() / exact.max())
        print(f"restatement against the pulsed aperture, retarded {retarded}, z = {z / c['dx']:.0f} dx: {err:.3e}, peak map {peak:.3e}")
        assert err < 1e-2


EMULATION_GRIDS = [((256, 16), 16), ((16, 16), 1024), ((48, 48), 128)]


@pytest.mark.parametrize("expanded,lt", EMULATION_GRIDS, ids=["256x16x16", "16x16x1024", "48x48x128"])
def test_device_steps_in_float32_against_float64(expanded, lt):
    """H with every device step emulated (float64 to the phase word, float32 from there) against float64 H, 0.37 and 3785.47
    wavelengths out, both time references, lossless and absorbing.  Measured <= 3.2e-7.  A float32 product q z would be 1e-3
    off at the far plane."""
    lam = 1.0e-3
    spacing = (lam / 3, 0.8 * lam / 3)
    dt = spacing[0] / (C0 * np.pi)
    worst = 0.0
    for z in (0.37 * lam, 3785.47 * lam):
        for retarded in (False, True):
            for coeff in (0.0, 0.5):
                if coeff > 0.0:
                    assert tr.margins(expanded, lt, spacing, dt, C0, [z])[1] >= 1e-9
                kw = dict(alpha_coeff=coeff, alpha_power=1.5, restrict=False, retarded=retarded)
                err = float(np.abs(tr.H_device(expanded, lt, spacing, dt, C0, z, **kw) -
                                   tr.H_time(expanded, lt, spacing, dt, C0, z, half=True, **kw)).max())
                worst = max(worst, err)
                assert err <= 2e-6, (z, retarded, coeff, err)
    print(f"float32 device steps against float64 H on {expanded} x {lt}: max |dH| {worst:.3e}")


def test_ak_table_is_alpha_k_log2e(angular):
    lt, dt = 48, 2e-7
    ak = tr.ak_table(lt, dt, C0, 0.75, 1.5)
    f = 7 / (lt * dt)
    assert ak[0] == 0.0 and ak.shape == (lt // 2 + 1,)
    assert ak[7] == pytest.approx(angular.alpha_np(0.75, 1.5, f) * (2 * np.pi * f / C0) / np.log(2.0), rel=1e-13)


# ---- 2. the rules and the refusals, through kwh_angular_time_plan without a device ----------------------------------------
RULE_TABLE = [  # dims, nt, fused -> expanded, Lt, fast
    ((24, 20), 40, True, (48, 48), 48, True),
    ((24, 20), 40, False, (48, 40), 40, False),
    ((24, 20), 41, False, (48, 40), 42, False),
    ((24, 24), 200, True, (48, 48), 200, True),
    ((24, 24), 201, True, (48, 48), 216, True),
    ((32, 32), 1024, True, (64, 64), 1024, True),
    ((32, 32), 1025, True, (64, 64), 1026, False),       # no fast length above 1024: Nt rounded up to even
    ((600, 16), 100, True, (1200, 32), 100, False),      # the sides leave the fast path, Lt keeps its rule
    ((128, 128), 1, True, (256, 256), 16, True),
]


@pytest.mark.parametrize("dims,nt,fused,expanded,lt,fast", RULE_TABLE)
def test_default_sides_and_record_length_follow_the_rule(angular, dims, nt, fused, expanded, lt, fast):
    got = angular.plan_time(dims, (1e-3, 1e-3), 2e-7, nt, C0, (1e-3, 2e-3), fused_kernels=fused)
    assert got == (expanded, lt, fast)
    assert got == tr.plan_time(dims, nt, fused)
    assert lt % 2 == 0 and lt >= nt


def test_given_sides_and_record_length_are_kept(angular):
    args = ((24, 20), (1e-3, 1e-3), 2e-7, 40, C0, 1e-3)
    assert angular.plan_time(*args, expanded=(26, 20)) == ((26, 20), 48, False)
    assert angular.plan_time(*args, expanded=(32, 48), time_length=64) == ((32, 48), 64, True)
    assert angular.plan_time(*args, time_length=42) == ((48, 48), 42, False)
    assert angular.plan_time(*args, time_length=40, fused_kernels=False) == ((48, 40), 40, False)


REFUSALS = [
    (dict(dims=(0, 20)), "Nx: 0 is not a grid size"),
    (dict(dims=(24, 0)), "Ny: 0 is not a grid size"),
    (dict(nt=0), "Nt: 0 is not a grid size"),
    (dict(spacing=(0.0, 1e-3)), "dx: 0.000000 is not a positive spacing"),
    (dict(spacing=(1e-3, float("nan"))), "dy: nan is not a positive spacing"),
    (dict(dt=0.0), "dt: 0.000000 is not a positive time step"),
    (dict(dt=-1.0), "dt: -1.000000 is not a positive time step"),
    (dict(c0=0.0), "c0: 0.000000 is not a positive sound speed"),
    (dict(alpha_coeff=-1.0), "alpha_coeff: -1.000000 is not an absorption >= 0 in dB/(MHz^y cm)"),
    (dict(alpha_power=-0.5), "alpha_power: -0.500000 is not a power >= 0"),
    (dict(z=()), "n_planes: 0 is not a number of planes"),
    (dict(z=np.full(4097, 1e-3)), "n_planes: 4097 is above 4096"),
    (dict(z=(1e-3, -2e-3)), "z: z[1] = -0.002000 is not a distance >= 0 (reverse projection is not built)"),
    (dict(z=(float("inf"),)), "z: z[0] = inf is not a distance >= 0 (reverse projection is not built)"),
    (dict(expanded=(48, 0)), "Ey: missing while the other side of the expanded grid is given"),
    (dict(expanded=(49, 48)), "Ex: 49 is odd (the real transforms need even sides)"),
    (dict(expanded=(48, 18)), "Ey: 18 is below N = 20"),
    (dict(time_length=41), "Lt: 41 is odd (the Nyquist bin of the record is dropped: Lt is even)"),
    (dict(time_length=38), "Lt: 38 is below Nt = 40"),
    (dict(expanded=(2048, 2048), time_length=1024), "E: 2048 x 2048 x 1024 points is not below 2^32"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(":")[0] + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_every_refusal_names_its_parameter(angular, change, message):
    from kwave_amd import capi
    args = dict(dims=(24, 20), spacing=(1e-3, 1e-3), dt=2e-7, nt=40, c0=C0, z=(0.5e-3, 1.6e-3))
    args.update(change)
    with pytest.raises(capi.KWaveError) as e:
        angular.plan_time(**args)
    assert str(e.value) == message
    with pytest.raises(capi.KWaveError) as e:   # the same from create, before any device is looked for
        angular.AngularSpectrumTime(**args)
    assert str(e.value) == message


def test_4096_planes_are_accepted(angular):
    assert angular.plan_time((24, 20), (1e-3, 1e-3), 2e-7, 40, C0, np.full(4096, 1e-3)) == ((48, 48), 48, True)


# ---- 3. the host code, stand-alone under the sanitizers --------------------------------------------------------------------
EXPECTED = {
    "default": "ok E=48x48 Lt=48 fast=1 ak=25 last=0.000000e+00",
    "rocfft": "ok E=48x40 Lt=40 fast=0 ak=21",
    "odd_nt_rocfft": "ok E=48x40 Lt=42 fast=0 ak=22",
    "beyond_1024": "ok E=48x48 Lt=1026 fast=0 ak=514",
    "given": "ok E=32x48 Lt=64 fast=1 ak=33",
    "given_slow": "ok E=48x48 Lt=42 fast=0 ak=22",
    "absorbing": "ok E=48x48 Lt=48 fast=1 ak=25 last=%.6e" % tr.ak_table(48, 2e-7, 1500.0, 0.75, 1.5)[-1],
    "planes_4096": "ok E=48x48 Lt=48 fast=1",
    "planes_4097": "n_planes: 4097 is above 4096",
    "planes_0": "n_planes: 0 is not a number of planes",
    "z_negative": "z: z[1] = -0.001000 is not a distance >= 0",
    "nt_zero": "Nt: 0 is not a grid size",
    "dt_zero": "dt: 0.000000 is not a positive time step",
    "lt_odd": "Lt: 41 is odd",
    "lt_small": "Lt: 38 is below Nt = 40",
    "e_odd": "Ex: 49 is odd (the real transforms need even sides)",
    "e_small": "Ey: 18 is below N = 20",
    "alpha_negative": "alpha_coeff: -1.000000 is not an absorption >= 0",
    "power_negative": "alpha_power: -1.000000 is not a power >= 0",
    "too_large": "E: 2048 x 2048 x 1024 points is not below 2^32",
}


def test_host_parameters_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/angular_time_host_check.cpp: AngularTimeParameters::init through valid inputs and refusals, by its
    message"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "angular_time_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "angular_time_host_check.cpp"),
           os.path.join(host, "AngularTimeParameters.cpp"), os.path.join(host, "GridRules.cpp"), "-o", exe]
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
def test_entry_points_are_declared_and_bound(angular):
    from kwave_amd import capi
    names = ENTRY_POINTS | {"kw_fused_angular_time_elems"}
    assert names <= set(capi.declared_symbols())
    counts = {"kw_fused_angular_time_elems": 2, "kw_fused_angular_time_forward": 3, "kw_fused_angular_time_plane": 4,
              "kw_angular_time_mix": 5, "kw_angular_time_embed": 9, "kw_angular_time_reduce": 11}
    header = open(os.path.join(ROOT, "include", "kwave_hip.h")).read()
    for name, n in counts.items():
        assert len(capi._SIG[name]) == n, name
        decl = header.split("KW_API kw_status " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n, name
    host = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in ("plan", "create", "destroy", "set_input", "run", "get", "series", "project", "get_scalar", "context"):
        assert "kwh_angular_time_" + name + "(" in host, name
    assert C.sizeof(angular.TimeConfig) == 15 * 8
    for name in ("run", "set_input", "p_max", "p_min", "series", "project", "close"):
        assert callable(getattr(angular.AngularSpectrumTime, name))
    for name in ("expanded", "time_length", "fused", "runs", "ctx"):
        assert isinstance(getattr(angular.AngularSpectrumTime, name), property)


def test_library_exports_the_entry_points():
    from kwave_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS | {"kw_fused_angular_time_elems"}:
        assert hasattr(L, name)
