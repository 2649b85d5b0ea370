"""CW field propagator, CPU side: the NumPy restatement (tests/cw_reference.py) against closed forms, the no-wrap-around
rule and every refusal through kwh_cw_* without a device, the host code in a stand-alone program built with
AddressSanitizer and UBSan, and the declarations.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import cw_reference as cr  # noqa: E402

C0, DX, PPW, N, E = 1500.0, 1e-3, 6, 32, 96
F0 = C0 / (PPW * DX)
W = 2.0 * np.pi * F0


@pytest.fixture(scope="module", autouse=True)
def cw():
    """without the propagator's entry points nothing in this file passes"""
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, cw
    assert {"kw_cw_operator", "kw_fused_cw_pair", "kw_cw_mix", "kw_cw_embed", "kw_cw_extract"} <= set(capi._SIG)
    return cw


@pytest.fixture(scope="module")
def case():
    """the 32^3 domain at 6 points per wavelength on its default expanded grid"""
    dims, spacing = (N, N, N), (DX, DX, DX)
    T, expanded = cr.plan(dims, spacing, C0)
    assert expanded == (E, E, E)
    return dims, spacing, T, expanded


# ---- 1. the operator ---------------------------------------------------------------------------------------------------
def test_regular_form_equals_the_textbook_form_away_from_the_resonance(case):
    _, spacing, T, expanded = case
    a = C0 * cr.wavenumber_magnitude(expanded, spacing)
    G = cr.operator(a, W, T)
    keep = (np.abs(a - W) * T > 1e-3) & (a > 0)
    assert keep.sum() > 0.99 * a.size
    err = np.abs(G[keep] - cr.operator_textbook(a[keep], W, T)).max() / np.abs(G).max()
    print(f"regular against textbook form: {err:.3e} of max|G|")
    assert err < 1e-10


def test_regular_form_is_finite_and_right_at_the_resonance_and_at_zero(case):
    T = case[2]
    G = cr.operator(np.array([W, 0.0]), W, T)
    assert np.all(np.isfinite(G))
    for got, want in ((G[0], cr.limit_at_resonance(W, T)), (G[1], cr.limit_at_zero(W, T))):
        assert abs(got - want) <= 1e-14 * abs(want)
    # and continuous there: a bin one part in 1e9 off the resonance, one tiny wavenumber
    near = cr.operator(np.array([W * (1 + 1e-9), 1e-6]), W, T)
    assert abs(near[0] - G[0]) < 1e-6 * abs(G[0]) and abs(near[1] - G[1]) < 1e-6 * abs(G[1])


# ---- 2. the solution ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_pair(case):
    dims, spacing, T, expanded = case
    rng = np.random.default_rng(20261019)
    S = rng.standard_normal((N, N, N)) + 1j * rng.standard_normal((N, N, N))
    Ee = cr.embed(S, expanded)
    Gh = cr.stored_operator(expanded, spacing, C0, F0, T, half=True)
    return Ee, Gh, cr.solve_pair(Ee.real.copy(), Ee.imag.copy(), Gh)


def test_pair_form_equals_the_complex_form(case, random_pair):
    dims, spacing, T, expanded = case
    Ee, _, (Pr, Pi) = random_pair
    Pc = cr.solve_complex(Ee, cr.stored_operator(expanded, spacing, C0, F0, T))
    err = cr.rel_l2(Pr + 1j * Pi, Pc)
    print(f"pair form against complex form: {err:.3e}")
    assert err < 1e-12


def test_float32_twin_is_close_to_float64(random_pair):
    pytest.importorskip("scipy.fft")
    Ee, Gh, (Pr, Pi) = random_pair
    Pr32, Pi32 = cr.solve_pair_f32(Ee.real.copy(), Ee.imag.copy(), Gh)
    err = cr.rel_l2(Pr32 + 1j * Pi32, Pr + 1j * Pi)
    print(f"float32 twin against float64: {err:.3e}")
    assert err < 1e-5


def test_point_source_gives_the_free_space_greens_function(case):
    """a unit point source (1 / dV at one grid point): within 5e-3 relative L2 of exp(-i k r) / (4 pi c0^2 r) for r > 3 dx,
    i.e. no periodic image has reached the domain and the field there is steady.  Measured 2.8e-3."""
    dims, spacing, T, expanded = case
    src = (N // 2, N // 2, N // 2)
    S = np.zeros((N, N, N), dtype=np.complex128)
    S[src] = 1.0 / DX ** 3
    P = cr.propagate(S, spacing, C0, F0, T, expanded)
    z, y, x = np.meshgrid(*(np.arange(N),) * 3, indexing="ij")
    r = DX * np.sqrt((z - src[0]) ** 2 + (y - src[1]) ** 2 + (x - src[2]) ** 2)
    far = r > 3 * DX
    err = cr.rel_l2(P[far], cr.green(r[far], C0, F0))
    print(f"point source against the free-space Green's function: {err:.3e}")
    assert err < 5e-3


# ---- 3. the rule and the refusals, through kwh_cw_* without a device --------------------------------------------------
RULE_TABLE = [  # dims, spacing, c0, fused -> expanded
    ((32, 32, 32), (1e-3, 1e-3, 1e-3), 1500.0, True, (96, 96, 96)),
    ((32, 32, 32), (1e-3, 1e-3, 1e-3), 1500.0, False, (88, 88, 88)),
    ((8, 12, 10), (1e-3, 0.7e-3, 0.9e-3), 1500.0, True, (32, 48, 32)),
    ((8, 12, 10), (1e-3, 0.7e-3, 0.9e-3), 1500.0, False, (24, 34, 28)),
    ((64, 48, 20), (0.5e-3, 0.5e-3, 1e-3), 1480.0, True, (160, 140, 72)),
    ((100, 100, 100), (2e-4, 2e-4, 2e-4), 1540.0, True, (280, 280, 280)),
    ((600, 16, 16), (1e-3, 1e-3, 1e-3), 1500.0, True, (1202, 618, 618)),   # no fast length above 1024: even sides everywhere
]


@pytest.mark.parametrize("dims,spacing,c0,fused,expanded", RULE_TABLE)
def test_default_time_and_expanded_grid_follow_the_rule(cw, dims, spacing, c0, fused, expanded):
    f0 = 0.25 * c0 / max(spacing)
    T, got, fast = cw.plan(dims, spacing, c0, f0, fused_kernels=fused)
    assert T == cr.default_time(dims, spacing, c0)
    assert got == expanded == cr.plan(dims, spacing, c0, fused=fused)[1]
    least = cr.least_sides(dims, spacing, c0, T)
    assert all(e >= v and e % 2 == 0 for e, v in zip(got, least))
    assert fast == (fused and all(e in cr.fast_lengths() for e in got))


def test_given_time_and_sides_are_kept(cw):
    T, got, fast = cw.plan((6, 8, 8), (1e-3,) * 3, 1500.0, 250e3, expanded=(22, 24, 26))
    assert got == (22, 24, 26) and not fast and T == cr.default_time((6, 8, 8), (1e-3,) * 3, 1500.0)
    T, got, fast = cw.plan((32, 32, 32), (1e-3,) * 3, 1500.0, 250e3, t=2e-5)
    assert T == 2e-5 and got == (64, 64, 64) and fast


def test_host_length_table_is_the_pipelines(cw):
    """GridRules.cpp carries the host's copy of KW_FUSED_LENGTHS: every length and its neighbours, through the rule"""
    lengths = cr.fast_lengths()
    for length in lengths:
        for want in (length, length - 2):
            # a 2-point domain with T chosen so that N + ceil(c0 T / d) = want
            if want < 4:
                continue
            _, got, fast = cw.plan((2, 2, 2), (1e-3,) * 3, 1000.0, 100e3, t=(want - 2 - 0.5) * 1e-6)
            assert got == (min(v for v in lengths if v >= want),) * 3 and fast


REFUSALS = [
    (dict(dims=(0, 32, 32)), "Nx: 0 is not a grid size"),
    (dict(dims=(32, 32, 0)), "Nz: 0 is not a grid size"),
    (dict(dims=(32, 32, 1)), "Nz: 1 selects a 2-D simulation, which is not built for the CW propagator"),
    (dict(spacing=(0.0, 1e-3, 1e-3)), "dx: 0.000000 is not a positive spacing"),
    (dict(spacing=(1e-3, -1e-3, 1e-3)), "dy: -0.001000 is not a positive spacing"),
    (dict(spacing=(1e-3, 1e-3, float("nan"))), "dz: nan is not a positive spacing"),
    (dict(c0=0.0), "c0: 0.000000 is not a positive sound speed"),
    (dict(f0=-1.0), "f0: -1.000000 is not a positive frequency"),
    (dict(f0=800e3, spacing=(1e-3, 1e-3, 1.25e-3)), "f0: 800000.000000 Hz is above the grid's Nyquist frequency c0 / (2 max d) = 600000.000000 Hz"),
    (dict(t=-1e-6), "T: -0.000001 is not a positive time"),
    (dict(t=1e9), "T: 1000000000.000000 s needs an expanded grid of more than 2^31 points along one axis"),
    (dict(expanded=(96, 0, 96)), "Ey: missing while another side of the expanded grid is given"),
    (dict(expanded=(96, 97, 96)), "Ey: 97 is odd (the real transforms need even sides)"),
    (dict(expanded=(96, 96, 86)), "Ez: 86 is below N + ceil(c0 T / d) = 88: the periodic images would reach the domain by T"),
    (dict(expanded=(2048, 2048, 2048)), "E: 2048 x 2048 x 2048 points is not below 2^32"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(":")[0] + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_every_refusal_names_its_parameter(cw, change, message):
    from kwave_amd import capi
    args = dict(dims=(32, 32, 32), spacing=(1e-3, 1e-3, 1e-3), c0=1500.0, f0=250e3)
    args.update(change)
    with pytest.raises(capi.KWaveError) as e:
        cw.plan(**args)
    assert str(e.value) == message
    with pytest.raises(capi.KWaveError) as e:   # the same from create, before any device is looked for
        cw.FieldPropagator(**args)
    assert str(e.value) == message


def test_valid_create_without_a_device_is_no_device(cw):
    """kwh_cw_create hands the device library's status through: 6 = KW_ERR_NO_DEVICE"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from kwave_amd.solver import Options
    L = cw._lib()
    c = cw._config((32, 32, 32), (1e-3,) * 3, 1500.0, 250e3, None, None, 1)
    o, h = Options(), C.c_void_p()
    o.device_idx, o.fused_kernels = -1, 1
    assert L.kwh_cw_create(C.byref(c), C.byref(o), C.byref(h)) == 6
    assert not h.value and L.kwh_last_error()


def test_source_scale_arguments(cw):
    with pytest.raises(ValueError):
        cw.plan((32, 32, 32), (1e-3,) * 3, 1500.0, 250e3, source_scale="k-wave")
    with pytest.raises(ValueError):
        cw.plan((32, 32, 32), (1e-3,) * 3, 1500.0, 250e3, source_scale=0)
    assert cw.plan((32, 32, 32), (1e-3,) * 3, 1500.0, 250e3, source_scale="kwave")[1] == (96, 96, 96)
    assert cr.kwave_scale((1e-3,) * 3, 1500.0, 250e3) == 2j * 2 * np.pi * 250e3 * 1500.0 / 1e-3


# ---- 4. the host code, stand-alone under the sanitizers ------------------------------------------------------------------
EXPECTED = {
    "cube32": "ok T=3.695041723e-05 E=96x96x96 fast=1 scale=1,0",
    "cube32_rocfft": "ok T=3.695041723e-05 E=88x88x88 fast=0 scale=1,0",
    "three_sides": "ok T=9.787974481e-06 E=32x48x32 fast=1 scale=1,0",
    "given_t": "ok T=2.000000000e-05 E=64x64x64 fast=1 scale=1,0",
    "given_e": "ok T=8.537498983e-06 E=22x24x26 fast=0 scale=1,0",
    "given_e_fast": "ok T=3.695041723e-05 E=128x128x128 fast=1 scale=1,0",
    "beyond_1024": "ok T=4.002843434e-04 E=1202x618x618 fast=0 scale=1,0",
    "kwave_scale": "ok T=3.695041723e-05 E=96x96x96 fast=1 scale=0,4.71239e+12",
    "lengths": "ok",
    "nx_zero": "Nx: 0 is not a grid size",
    "ny_zero": "Ny: 0 is not a grid size",
    "two_d": "Nz: 1 selects a 2-D simulation, which is not built for the CW propagator",
    "dx_zero": "dx: 0.000000 is not a positive spacing",
    "dy_negative": "dy: -0.001000 is not a positive spacing",
    "dz_nan": "dz: nan is not a positive spacing",
    "c0_zero": "c0: 0.000000 is not a positive sound speed",
    "f0_zero": "f0: 0.000000 is not a positive frequency",
    "f0_nyquist": "f0: 800000.000000 Hz is above the grid's Nyquist frequency c0 / (2 max d) = 600000.000000 Hz",
    "t_negative": "T: -0.000001 is not a positive time",
    "t_huge": "T: 1000000000.000000 s needs an expanded grid of more than 2^31 points along one axis",
    "e_partial": "Ey: missing while another side of the expanded grid is given",
    "e_odd": "Ey: 97 is odd (the real transforms need even sides)",
    "e_small": "Ez: 86 is below N + ceil(c0 T / d) = 88: the periodic images would reach the domain by T",
    "e_total": "E: 2048 x 2048 x 2048 points is not below 2^32",
    "scale_nan": "source_scale: is not finite",
}


def test_host_parameters_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/cw_host_check.cpp: CwParameters::init through its valid inputs and every refusal, by its message"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "cw_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "cw_host_check.cpp"), os.path.join(host, "CwParameters.cpp"),
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
    # the times are the restatement's
    assert float(lines["cube32"].split("T=")[1].split()[0]) == pytest.approx(cr.default_time((32,) * 3, (1e-3,) * 3, 1500.0), rel=1e-9)


# ---- 5. declarations -----------------------------------------------------------------------------------------------------
def test_cw_entry_points_are_declared_and_bound(cw):
    from kwave_amd import capi
    declared = set(capi.declared_symbols())
    assert {"kw_cw_operator", "kw_fused_cw_pair", "kw_cw_mix", "kw_cw_embed", "kw_cw_extract"} <= declared
    assert len(capi._SIG["kw_cw_operator"]) == 9 and len(capi._SIG["kw_cw_extract"]) == 16 and len(capi._SIG["kw_cw_embed"]) == 14
    header = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in ("plan", "create", "destroy", "run", "get", "heat", "propagate", "get_scalar", "context"):
        assert "kwh_cw_" + name + "(" in header, name
    assert C.sizeof(cw.Config) == 15 * 8
    for name in ("run", "run_parts", "run_elements", "amplitude", "phase", "heat", "close"):
        assert callable(getattr(cw.FieldPropagator, name))
