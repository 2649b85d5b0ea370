"""dp0/dt as a second initial condition of the exact k-space propagators, without a GPU: the float64 restatement
tests/second_order_dp0dt_reference.py (Hs against the matrix exponential of the mode, its limits, the travelling wave), and
the declarations through every layer (device entry points, host C API, Python classes)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import second_order_dp0dt_reference as dr  # noqa: E402
import second_order_reference as sr  # noqa: E402

C0 = 1500.0
PAIR_ENTRY_POINTS = {"kw_fused_second_order_time_pair": 5, "kw_second_order_mix_pair": 6,
                     "kw_fused_second_order_frames_time_pair": 5, "kw_second_order_frames_mix_pair": 6}


# ---- 1. the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y", [1.1, 1.5, 2.0, 0.5])
def test_hs_is_the_matrix_exponential_of_the_mode(y):
    """every non-zero bin of a 16 x 12 x 10 grid: Hs against the [0, 1] element of exp(A t), A = [[0, 1], [-Omega^2,
    -2 gamma]], through numpy.linalg.eig in the mode's own time unit 1 / (c0 |k|) — A' = [[0, 1], [-(1 - 2 g T), -2 g]],
    t' = c0 |k| t, and exp(A t)[0, 1] = exp(A' t')[0, 1] / (c0 |k|).  The comparison is made in that unit (Hs c0 |k|, O(1)),
    as the test of H compares an O(1) quantity; bound 1e-9, that test's.  The coefficient puts the largest g at 0.3."""
    expanded, d = (16, 12, 10), (1.0e-4, 0.8e-4, 1.3e-4)
    k = sr.wavenumbers(expanded, d)
    nzb = k > 0
    coeff = 0.3 / sr.damping(k[nzb], C0, 1.0, y)[0].max()
    assert sr.b_margins(expanded, d, C0, coeff, y)[0] >= 0.25
    g = coeff * sr.damping(k[nzb], C0, 1.0, y)[0]
    T = sr.tangent(y)
    A = np.zeros((g.size, 2, 2))
    A[:, 0, 1] = 1.0
    A[:, 1, 0] = -(1.0 - 2.0 * g * T)
    A[:, 1, 1] = -2.0 * g
    lam, V = np.linalg.eig(A)
    coef = np.linalg.solve(V, np.tile(np.array([0.0, 1.0]), (g.size, 1))[..., None])[..., 0]   # exp(A t) (0, 1)^T
    for t in (0.0, 3.1e-8, 2.7e-7):
        tp = C0 * k[nzb] * t
        first = np.sum(V[:, 0, :] * np.exp(lam * tp[:, None]) * coef, axis=1)
        got = dr.Hs_of_k(k, C0, t, coeff, y)
        assert np.all(got[~nzb] == t)
        err = float(np.abs(got[nzb] * (C0 * k[nzb]) - first.real).max())
        print(f"Hs against exp(A t)[0, 1], y = {y}, t = {t}: max |d(Hs c0 k)| {err:.3e}, max |imag| {np.abs(first.imag).max():.3e}")
        assert err <= 1e-9 and np.abs(first.imag).max() <= 1e-9


@pytest.mark.parametrize("coeff", [0.0, 0.75])
def test_hs_limits(coeff):
    """Hs(k = 0) = t, Hs(t = 0) = 0 on every bin; and d Hs / dt (0) = 1 on every bin (p'(0) = V0), by a central difference"""
    expanded, d = (16, 12, 10), (1.0e-4, 0.8e-4, 1.3e-4)
    k = sr.wavenumbers(expanded, d)
    for t in (0.0, 3.1e-8, 2.7e-7):
        assert dr.Hs(expanded, d, C0, t, coeff)[0, 0, 0] == t
    assert np.all(dr.Hs(expanded, d, C0, 0.0, coeff) == 0.0)
    h = 1e-4 / (C0 * k.max())
    slope = (dr.Hs_of_k(k, C0, h, coeff) - dr.Hs_of_k(k, C0, -h, coeff)) / (2 * h) if coeff == 0.0 else \
        dr.Hs_of_k(k, C0, h, coeff) / h
    # lossless: 1 - O(h^2 w^2); absorbing (one-sided): 1 - gamma h - ..., gamma h <= g w h <= 1e-4
    assert np.abs(slope - 1.0).max() <= (1e-7 if coeff == 0.0 else 2e-4)


def test_travelling_wave_needs_the_second_condition():
    """periodic 32 x 16 x 16 box, p0 = f(x) (harmonics 1, 3, 7, 12), dp0dt = -c0 df/dx (float64 spectral derivative cast to
    float32): at t = n dx / c0 the field is roll(p0, n, axis=x) to 1e-6; without the second term it is more than 0.1 off"""
    n, d = (32, 16, 16), (1.0e-4, 1.0e-4, 1.0e-4)
    p0, v = dr.wave_inputs((16, 16, 32), d[0], C0)
    for steps in (1, 5, 37):
        t = steps * d[0] / C0
        want = np.roll(p0.astype(np.float64), steps, axis=2)
        both = sr.rel_l2(dr.solve(p0, v, n, d, C0, [t])[0], want)
        alone = sr.rel_l2(sr.solve(p0, n, d, C0, [t])[0], want)
        print(f"travelling wave n = {steps}: with dp0dt {both:.3e}, without {alone:.3e}")
        assert both <= 1e-6 and alone > 0.1


def test_frames_restatement_is_the_three_d_one_on_a_single_plane():
    rng = np.random.default_rng(7)
    p, v = rng.standard_normal((3, 10, 12)), rng.standard_normal((3, 10, 12))
    d, t = (1.0e-4, 0.8e-4), 2.3e-7
    got = dr.frames_solve(p, v, (16, 12), d, C0, [t], 0.75, 1.5)[0]
    for f in range(3):
        want = dr.solve(p[f][None], v[f][None], (16, 12, 1), (d[0], d[1], 1.0), C0, [t], 0.75, 1.5)[0, 0]
        assert np.array_equal(got[f], want)
    assert dr.frames_Hs((16, 12), d, C0, t)[0, 0] == t


# ---- 2. declarations ---------------------------------------------------------------------------------------------------------
def test_pair_entry_points_are_declared_and_bound():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    assert set(PAIR_ENTRY_POINTS) <= set(capi._SIG)
    assert set(PAIR_ENTRY_POINTS) <= set(capi.declared_symbols())
    header = open(os.path.join(ROOT, "include", "kwave_hip.h")).read()
    for name, n in PAIR_ENTRY_POINTS.items():
        assert len(capi._SIG[name]) == n, name
        decl = header.split("KW_API kw_status " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n, name
    L = capi.load()
    for name in PAIR_ENTRY_POINTS:
        assert hasattr(L, name)


def test_host_library_exports_set_dp0dt_and_the_classes_have_it():
    import kwave_amd  # noqa: F401
    from kwave_amd import second_order
    L = second_order._lib()
    host = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    for name in ("kwh_second_order_set_dp0dt", "kwh_second_order_frames_set_dp0dt"):
        assert hasattr(L, name) and name + "(" in host
    for cls in (second_order.SecondOrder, second_order.SecondOrderFrames):
        assert callable(cls.set_dp0dt) and isinstance(cls.has_dp0dt, property)
    assert second_order.SecondOrderFrames.set_dp0dt is not second_order.SecondOrder.set_dp0dt


def test_not_built_lists_no_longer_name_the_second_condition():
    """dp0/dt left the "Not built" lists; dp0/dt in the line record stays there"""
    for path in (os.path.join(ROOT, "include", "kwave_hip.h"), os.path.join(ROOT, "include", "kwave_host.h")):
        text = open(path).read()
        assert "dp0/dt as a second initial condition and time-varying" not in text
        assert "dp0/dt in the line" in text


def test_valid_create_without_a_device_is_no_device():
    """creation still hands the device library's status through: 6 = KW_ERR_NO_DEVICE"""
    import kwave_amd  # noqa: F401
    from kwave_amd import capi, second_order
    from kwave_amd.solver import Options
    try:   # the device library's own answer: it is what kwh_*_create asks
        capi.Device().close()
    except capi.KWaveError:
        pass
    else:
        pytest.skip("GPU present")
    L = second_order._lib()
    o = Options()
    o.device_idx, o.fused_kernels = -1, 1
    c, _idx = second_order._config((24, 20, 18), (1e-4,) * 3, C0, 0.0, 1.5, 1e-6, None, None, ("p_raw",))
    h = C.c_void_p()
    assert L.kwh_second_order_create(C.byref(c), C.byref(o), C.byref(h)) == 6 and not h.value
    c, _idx = second_order._config((24, 20), (1e-4,) * 2, C0, 0.0, 1.5, 1e-6, None, None, ("p_raw",), frames=3)
    assert L.kwh_second_order_frames_create(C.byref(c), C.byref(o), C.byref(h)) == 6 and not h.value
    # a NULL propagator is refused by name, not dereferenced
    assert L.kwh_second_order_set_dp0dt(None, None) != 0 and L.kwh_second_order_frames_set_dp0dt(None, None) != 0
