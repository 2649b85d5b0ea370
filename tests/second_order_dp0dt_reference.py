"""Float64 NumPy restatement of the exact k-space propagator with dp0/dt as a second initial condition (include/kwave_hip.h
"Exact k-space propagator", "dp0/dt"; a plain module, imported by name from tests/), on top of tests/second_order_reference.py,
whose H is the Hc here.  Arrays are [z][y][x] (frames: [F][y][x]); n, d and expanded are given as (x, y, z) (frames: (x, y)).

    per mode p'' + 2 gamma p' + Omega^2 p = 0, p(0) = P0, p'(0) = V0:   p^(t) = Hc(|k|; t) P0 + Hs(|k|; t) V0
    lossless   Hs = sin(c0 |k| t) / (c0 |k|)
    absorbing  Hs = exp(-gamma t) sin(w_d t) / w_d,  gamma = c0 |k| g,  w_d = c0 |k| r  (g, B, r: second_order_reference)
    |k| = 0    Hs = t
"""
import numpy as np

import second_order_frames_reference as sfr
import second_order_reference as sr


def Hs_of_k(k, c0, t, alpha_coeff=0.0, y=1.5):
    k = np.asarray(k, dtype=np.float64)
    safe = np.where(k > 0, k, 1.0)
    if alpha_coeff == 0.0:
        w = c0 * safe
        return np.where(k > 0, np.sin(w * t) / w, t)
    g, B = sr.damping(safe, c0, alpha_coeff, y)
    with np.errstate(invalid="ignore"):   # (the stand-in |k| = 1 of the zero bins may be overdamped: not used)
        w = c0 * safe * np.sqrt(B)
        return np.where(k > 0, np.exp(-c0 * safe * g * t) * np.sin(w * t) / w, t)


def Hs(expanded, d, c0, t, alpha_coeff=0.0, y=1.5, half=True):
    return Hs_of_k(sr.wavenumbers(expanded, d, half), c0, t, alpha_coeff, y)


def terms_expanded(vol_p, vol_v, d, c0, t, alpha_coeff=0.0, y=1.5):
    """(irfftn(Hc P), irfftn(Hs V)) on the whole expanded volume [Ez][Ey][Ex]: the two terms of the field at time t"""
    vol_p, vol_v = np.asarray(vol_p, dtype=np.float64), np.asarray(vol_v, dtype=np.float64)
    ez, ey, ex = vol_p.shape
    k = sr.wavenumbers((ex, ey, ez), d)
    inv = lambda X: np.fft.irfftn(X, s=vol_p.shape, axes=(0, 1, 2))   # noqa: E731
    return (inv(np.fft.rfftn(vol_p, axes=(0, 1, 2)) * sr.H_of_k(k, c0, t, alpha_coeff, y)),
            inv(np.fft.rfftn(vol_v, axes=(0, 1, 2)) * Hs_of_k(k, c0, t, alpha_coeff, y)))


def solve_expanded(vol_p, vol_v, d, c0, t, alpha_coeff=0.0, y=1.5):
    """the whole expanded volume [Ez][Ey][Ex] at time t"""
    a, b = terms_expanded(vol_p, vol_v, d, c0, t, alpha_coeff, y)
    return a + b


def solve(p0, dp0dt, expanded, d, c0, times, alpha_coeff=0.0, y=1.5):
    """[n_times][Nz][Ny][Nx]: the domain crop at every time"""
    nz, ny, nx = p0.shape
    vp, vv = sr.embed(p0, expanded), sr.embed(dp0dt, expanded)
    return np.array([solve_expanded(vp, vv, d, c0, t, alpha_coeff, y)[:nz, :ny, :nx] for t in np.atleast_1d(times)])


# ---- frames: the plane (Ex, Ey, 1) of second_order_frames_reference, frame by frame ---------------------------------------
def frames_Hs(expanded, d, c0, t, alpha_coeff=0.0, y=1.5):
    """[Ey][Ex/2 + 1]"""
    return Hs(sfr.plane(expanded), sfr.spacings(d), c0, t, alpha_coeff, y)[0]


def frames_terms_expanded(vol_p, vol_v, d, c0, t, alpha_coeff=0.0, y=1.5):
    pairs = [terms_expanded(p[None], v[None], sfr.spacings(d), c0, t, alpha_coeff, y) for p, v in zip(vol_p, vol_v)]
    return np.array([a[0] for a, _ in pairs]), np.array([b[0] for _, b in pairs])


def frames_solve_expanded(vol_p, vol_v, d, c0, t, alpha_coeff=0.0, y=1.5):
    """every expanded plane [F][Ey][Ex] at time t"""
    a, b = frames_terms_expanded(vol_p, vol_v, d, c0, t, alpha_coeff, y)
    return a + b


def frames_solve(p0, dp0dt, expanded, d, c0, times, alpha_coeff=0.0, y=1.5):
    """[n_times][F][Ny][Nx]"""
    out = [solve(p[None], v[None], sfr.plane(expanded), sfr.spacings(d), c0, times, alpha_coeff, y)[:, 0]
           for p, v in zip(np.asarray(p0, dtype=np.float64), np.asarray(dp0dt, dtype=np.float64))]
    return np.stack(out, axis=1)


# ---- the travelling wave -----------------------------------------------------------------------------------------------------
WAVE_HARMONICS = (1, 3, 7, 12)


def wave_profile(nx, seed=0):
    """(f, df/dx per point spacing) in float64 on nx periodic points: harmonics 1, 3, 7, 12 with seeded amplitudes and
    phases; the derivative is the spectral one"""
    rng = np.random.default_rng(seed)
    x = np.arange(nx)
    f, df = np.zeros(nx), np.zeros(nx)
    for h in WAVE_HARMONICS:
        a, ph = rng.uniform(0.5, 1.0), rng.uniform(0.0, 2.0 * np.pi)
        w = 2.0 * np.pi * h / nx
        f += a * np.cos(w * x + ph)
        df += -a * w * np.sin(w * x + ph)
    return f, df


def wave_inputs(shape, dx, c0, seed=0):
    """(p0, dp0dt) float32 of shape (..., Nx): p0 = f(x), dp0dt = -c0 df/dx, the same profile on every row; the wave that
    runs towards +x, so that p(n dx / c0) = roll(p0, n, axis=x)"""
    f, df = wave_profile(shape[-1], seed)
    p0 = np.broadcast_to(f, shape).astype(np.float32)
    v = np.broadcast_to(-c0 * df / dx, shape).astype(np.float32)
    return np.ascontiguousarray(p0), np.ascontiguousarray(v)
