"""Angular-spectrum projector, CPU side: the NumPy restatement (tests/angular_reference.py) against the exact field of a
Gaussian-apodised aperture, the integer phase accumulator in emulated float32, the size rules and every refusal through
kwh_angular_* without a device, the host code in a stand-alone program built with AddressSanitizer and UBSan, and the
declarations.  No GPU."""
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
import cw_reference as cr  # noqa: E402

C0 = 1500.0
ENTRY_POINTS = {"kw_angular_operator", "kw_fused_angular_elems", "kw_fused_angular_forward", "kw_fused_angular_planes",
                "kw_angular_mix"}


@pytest.fixture(scope="module", autouse=True)
def angular():
    """without the projector's entry points nothing in this file passes"""
    import kwave_amd  # noqa: F401
    from kwave_amd import angular, capi
    assert ENTRY_POINTS <= set(capi._SIG)
    return angular


# ---- 1. the restatement -------------------------------------------------------------------------------------------------
def aperture_case():
    """32 x 32 plane at 3 points per wavelength, 4 dx above a Gaussian-apodised (sigma = 3 dx) aperture of point sources,
    projected over 12 dx on E = 64"""
    n, dx = 32, 1.0e-3
    k = 2.0 * np.pi / (3.0 * dx)
    P0 = ar.aperture_field(n, dx, k, 4 * dx)
    exact = np.stack([ar.aperture_field(n, dx, k, (4 + j) * dx) for j in range(13)])
    return n, dx, k, P0, exact


@pytest.fixture(scope="module")
def aperture():
    return aperture_case()


def test_pair_form_equals_the_complex_form():
    rng = np.random.default_rng(20261019)
    P0 = rng.standard_normal((20, 24)) + 1j * rng.standard_normal((20, 24))
    dx, dy = 1.0e-3, 0.8e-3
    k = 2.0 * np.pi / (3.0 * dx)
    for alpha, restrict in ((0.0, True), (0.0, False), (40.0, True), (40.0, False)):
        args = ((48, 64), (dx, dy), k, alpha, 0.4e-3, 1.3e-3, 9, restrict)
        Pr, Pi = ar.solve_pair(P0.real, P0.imag, *args)
        Pc = ar.solve_complex(P0, *args)
        err = ar.rel_l2(Pr + 1j * Pi, Pc)
        print(f"pair form against complex form, alpha {alpha}, restriction {restrict}: {err:.3e}")
        assert err <= 1e-14


@pytest.mark.parametrize("restrict", [True, False], ids=["restricted", "unrestricted"])
def test_restatement_gives_the_exact_aperture_field(aperture, restrict):
    """the signs, the restriction and the crop against sum w exp(-i k r) / (4 pi r).  Measured 1.75e-7 / 1.79e-7."""
    n, dx, k, P0, exact = aperture
    P = ar.project(P0, (dx, dx), k, 0.0, 0.0, dx, 13, (64, 64), restrict)
    err = ar.rel_l2(P, exact)
    print(f"restatement against the exact aperture field, restriction {restrict}: {err:.3e}")
    assert err <= 1e-6


def test_integer_phase_accumulator_in_float32_at_plane_1023():
    """H from the tables with every device step emulated in float32 against float64 at j = 1023; a float32 product q z would
    be ~3e-4 off here.  Measured 9.1e-7."""
    lam = 1.0e-3
    k = 2.0 * np.pi / lam
    expanded, spacing = (256, 16), (lam / 3, lam / 3)
    tab = ar.tables(expanded, spacing, k, 0.0, 0.0, 3.7 * lam, 1024, restrict=False)
    H32 = ar.H_tables(tab, 1023, np.float32)
    H64 = ar.H_exact(expanded, spacing, k, 0.0, 1023 * 3.7 * lam, restrict=False, half=True)
    err = float(np.abs(H32 - H64).max())
    print(f"integer-accumulator H in float32 against float64 at j = 1023: max |dH| {err:.3e}")
    assert err <= 2e-6
    # and the naive float32 product is what the accumulator is there to avoid
    q = np.sqrt(np.abs(k * k - ar.radial(expanded, spacing, half=True)))
    naive = np.exp(-1j * (q.astype(np.float32) * np.float32(1023 * 3.7 * lam)).astype(np.float64))
    prop = ar.radial(expanded, spacing, half=True) < k * k
    assert float(np.abs(naive - H64)[prop].max()) > 5e-5


def test_tables_give_h_on_every_plane():
    lam = 1.0e-3
    k = 2.0 * np.pi / lam
    expanded, spacing = (48, 16), (lam / 3, 0.8 * lam / 3)
    for alpha, restrict in ((0.0, True), (25.0, True), (25.0, False)):
        tab = ar.tables(expanded, spacing, k, alpha, 0.37 * lam, 3.7 * lam, 40, restrict)
        for j in (0, 1, 17, 39):
            H = ar.H_exact(expanded, spacing, k, alpha, 0.37 * lam + j * 3.7 * lam, restrict, half=True)
            assert np.abs(ar.H_tables(tab, j) - H).max() <= 1e-7


# ---- 2. the rules and the refusals, through kwh_angular_* without a device -------------------------------------------------
RULE_TABLE = [  # dims, planes, fused -> expanded, chunk, fast
    ((24, 20), 20, True, (48, 48), 32, True),
    ((24, 20), 20, False, (48, 40), 32, False),
    ((32, 32), 13, True, (64, 64), 16, True),
    ((32, 32), 16, True, (64, 64), 16, True),
    ((32, 32), 17, True, (64, 64), 32, True),
    ((33, 100), 48, True, (72, 200), 48, True),
    ((128, 128), 49, True, (256, 256), 64, True),
    ((200, 256), 4096, True, (400, 512), 64, True),
    ((512, 512), 256, True, (1024, 1024), 64, True),     # exactly 1 GiB
    ((600, 16), 100, True, (1200, 32), 64, False),       # no fast length above 1024: 2 N on both axes
    ((768, 768), 100, True, (1536, 1536), 16, False),    # 32 planes would take 1.2 GiB
    ((1024, 1024), 100, True, (2048, 2048), 16, False),  # the floor
]


@pytest.mark.parametrize("dims,planes,fused,expanded,chunk,fast", RULE_TABLE)
def test_default_sides_and_chunk_follow_the_rule(angular, dims, planes, fused, expanded, chunk, fast):
    got = angular.plan(dims, (1e-3, 1e-3), C0, 500e3, 0.0, 1e-3, planes, fused_kernels=fused)
    assert got == (expanded, chunk, fast)
    assert expanded == ar.plan(dims, fused) and chunk == ar.chunk_planes(expanded, planes)
    assert all(e >= 2 * n and e % 2 == 0 for e, n in zip(expanded, dims))
    assert 16 * expanded[0] * expanded[1] * chunk <= (1 << 30) or chunk == 16


def test_given_sides_and_chunk_are_kept(angular):
    assert angular.plan((24, 20), (1e-3, 1e-3), C0, 500e3, 0.0, 1e-3, 20, expanded=(26, 20)) == ((26, 20), 32, False)
    assert angular.plan((24, 20), (1e-3, 1e-3), C0, 500e3, 0.0, 1e-3, 20, expanded=(32, 48), chunk_planes=16) == ((32, 48), 16, True)
    assert angular.plan((24, 20), (1e-3, 1e-3), C0, 500e3, 0.0, 1e-3, 20, chunk_planes=7, fused_kernels=False) == ((48, 40), 7, False)


REFUSALS = [
    (dict(dims=(0, 20)), "Nx: 0 is not a grid size"),
    (dict(dims=(24, 0)), "Ny: 0 is not a grid size"),
    (dict(spacing=(0.0, 1e-3)), "dx: 0.000000 is not a positive spacing"),
    (dict(spacing=(1e-3, float("nan"))), "dy: nan is not a positive spacing"),
    (dict(c0=0.0), "c0: 0.000000 is not a positive sound speed"),
    (dict(f0=0.0), "f0: 0.000000 is not a positive frequency"),
    (dict(f0=-1.0), "f0: -1.000000 is not a positive frequency"),
    (dict(z0=-1e-3), "z0: -0.001000 is not a distance >= 0 (reverse projection is not built)"),
    (dict(dz=0.0), "dz: 0.000000 is not a positive plane spacing"),
    (dict(dz=-1e-3), "dz: -0.001000 is not a positive plane spacing"),
    (dict(planes=0), "planes: 0 is not a number of planes"),
    (dict(planes=4097), "planes: 4097 is above 4096 (the phase accumulator is specified up to plane index 4095)"),
    (dict(alpha_np=-1.0), "alpha_np: -1.000000 is not an absorption >= 0 in Np/m"),
    (dict(expanded=(48, 0)), "Ey: missing while the other side of the expanded grid is given"),
    (dict(expanded=(49, 48)), "Ex: 49 is odd (the real transforms need even sides)"),
    (dict(expanded=(48, 18)), "Ey: 18 is below N = 20"),
    (dict(chunk_planes=20), "chunk_planes: 20 is no fast-path length (16, 32, 48, 64 ...) on a fast-path grid"),
    (dict(dims=(600, 600), expanded=(32768, 32768), chunk_planes=5), "E: 32768 x 32768 x 5 points per chunk is not below 2^32"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(":")[0] + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_every_refusal_names_its_parameter(angular, change, message):
    from kwave_amd import capi
    args = dict(dims=(24, 20), spacing=(1e-3, 1e-3), c0=C0, f0=500e3, z0=0.0, dz=1e-3, planes=20)
    args.update(change)
    with pytest.raises(capi.KWaveError) as e:
        angular.plan(**args)
    assert str(e.value) == message
    with pytest.raises(capi.KWaveError) as e:   # the same from create, before any device is looked for
        angular.AngularSpectrum(**args)
    assert str(e.value) == message


def test_4096_planes_are_accepted(angular):
    assert angular.plan((24, 20), (1e-3, 1e-3), C0, 500e3, 0.0, 1e-3, 4096)[0] == (48, 48)


def test_alpha_np_helper(angular):
    # 0.75 dB / (MHz^1.5 cm) at 2 MHz: 0.75 * 2^1.5 dB/cm = 212.13 dB/m = 24.42 Np/m
    assert angular.alpha_np(0.75, 1.5, 2e6) == pytest.approx(0.75 * 2 ** 1.5 * 100 * np.log(10) / 20, rel=1e-14)
    assert angular.alpha_np(0.0, 1.5, 2e6) == 0.0


# ---- 3. the host code, stand-alone under the sanitizers --------------------------------------------------------------------
EXPECTED = {
    "default": "ok E=48x48 chunk=32 fast=1",
    "rocfft": "ok E=48x40 chunk=32 fast=0",
    "chunk16": "ok E=2048x2048 chunk=16 fast=0",
    "chunk48": "ok E=300x256 chunk=48 fast=1",
    "beyond_1024": "ok E=1200x32 chunk=64 fast=0",
    "given": "ok E=32x48 chunk=16 fast=1",
    "planes_4096": "ok E=48x48 chunk=64 fast=1",
    "z0_negative": "z0: -0.001000 is not a distance >= 0 (reverse projection is not built)",
    "dz_zero": "dz: 0.000000 is not a positive plane spacing",
    "planes_4097": "planes: 4097 is above 4096",
    "e_odd": "Ex: 49 is odd (the real transforms need even sides)",
    "e_small": "Ey: 18 is below N = 20",
    "alpha_negative": "alpha_np: -1.000000 is not an absorption >= 0 in Np/m",
    "f0_zero": "f0: 0.000000 is not a positive frequency",
    "chunk_20": "chunk_planes: 20 is no fast-path length",
}


def test_host_parameters_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/angular_host_check.cpp: AngularParameters::init through valid inputs and refusals, by its message"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "angular_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "angular_host_check.cpp"), os.path.join(host, "AngularParameters.cpp"),
           os.path.join(host, "GridRules.cpp"), "-o", exe]
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
def test_angular_entry_points_are_declared_and_bound(angular):
    from kwave_amd import capi
    assert ENTRY_POINTS <= set(capi.declared_symbols())
    counts = {"kw_angular_operator": 11, "kw_fused_angular_elems": 2, "kw_fused_angular_forward": 5,
              "kw_fused_angular_planes": 7, "kw_angular_mix": 10}
    header = open(os.path.join(ROOT, "include", "kwave_hip.h")).read()
    for name, n in counts.items():
        assert len(capi._SIG[name]) == n, name
        decl = header.split("KW_API kw_status " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n, name
    host = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in ("plan", "create", "destroy", "run", "get", "heat", "project", "get_scalar", "context"):
        assert "kwh_angular_" + name + "(" in host, name
    assert C.sizeof(angular.Config) == 14 * 8
    for name in ("run", "run_parts", "amplitude", "phase", "heat", "project", "close"):
        assert callable(getattr(angular.AngularSpectrum, name))
    for name in ("expanded", "fused", "chunk_planes", "runs"):
        assert isinstance(getattr(angular.AngularSpectrum, name), property)


def test_library_exports_the_entry_points():
    from kwave_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)


def test_fast_lengths_up_to_64_are_the_chunk_sizes():
    assert [v for v in cr.fast_lengths() if v <= 64] == [16, 32, 48, 64]
