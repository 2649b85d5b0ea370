"""Float64 NumPy restatement of the exact k-space propagator (include/kwave_hip.h "Exact k-space propagator"; a plain
module, imported by name from tests/).  Arrays are [z][y][x]; n, d and expanded are given as (x, y, z).

    p(t) = irfftn( rfftn(p0 embedded in Ez x Ey x Ex) H(|k|; t) ),  bins k? = 2 pi / (E? d?) min(i, E? - i)
    lossless   H = cos(c0 |k| t)
    absorbing  g = a c0^y |k|^(y-1), T = tan(pi y / 2), B = 1 - 2 g T - g^2, r = sqrt(B)
               H = exp(-c0 |k| g t) (cos(c0 |k| r t) + (g / r) sin(c0 |k| r t)),  H(0) = 1
"""
import math

import numpy as np


def neper(alpha_coeff, y):
    """a [Np (rad/s)^-y m^-1] of alpha_coeff [dB / (MHz^y cm)]: the time loop's conversion"""
    return alpha_coeff * 100.0 * (1.0e-6 / (2.0 * math.pi)) ** y / (20.0 * math.log10(math.e))


def wavenumbers(expanded, d, half=True):
    """|k| on [Ez][Ey][Ex/2 + 1] (half) or [Ez][Ey][Ex]"""
    ex, ey, ez = expanded

    def axis(n, dd, count):
        i = np.arange(count)
        return 2.0 * math.pi / (n * dd) * np.minimum(i, n - i)

    kx = axis(ex, d[0], ex // 2 + 1 if half else ex)
    ky, kz = axis(ey, d[1], ey), axis(ez, d[2], ez)
    return np.sqrt((kx ** 2).reshape(1, 1, -1) + (ky ** 2).reshape(1, -1, 1) + (kz ** 2).reshape(-1, 1, 1))


def tangent(y):
    return 0.0 if y == 2.0 else math.tan(math.pi * y / 2.0)


def damping(k, c0, alpha_coeff, y):
    """(g, B) of the bins k"""
    with np.errstate(divide="ignore"):
        s = np.where(k > 0, np.asarray(k, dtype=np.float64) ** (y - 1.0), 0.0)
    g = neper(alpha_coeff, y) * c0 ** y * s
    return g, 1.0 - 2.0 * g * tangent(y) - g * g


def H_of_k(k, c0, t, alpha_coeff=0.0, y=1.5):
    k = np.asarray(k, dtype=np.float64)
    if alpha_coeff == 0.0:
        return np.cos(c0 * k * t)
    g, B = damping(k, c0, alpha_coeff, y)
    r = np.sqrt(B)
    ph = c0 * k * r * t
    return np.where(k > 0, np.exp(-c0 * k * g * t) * (np.cos(ph) + g / r * np.sin(ph)), 1.0)


def H(expanded, d, c0, t, alpha_coeff=0.0, y=1.5, half=True):
    return H_of_k(wavenumbers(expanded, d, half), c0, t, alpha_coeff, y)


def b_margins(expanded, d, c0, alpha_coeff, y):
    """(min B over every non-zero bin of the grid, B at the smallest non-zero |k|, B at the largest |k|)"""
    k = wavenumbers(expanded, d)
    nz = k[k > 0]
    B = damping(nz, c0, alpha_coeff, y)[1]
    return float(B.min()), float(damping(nz.min(), c0, alpha_coeff, y)[1]), float(damping(nz.max(), c0, alpha_coeff, y)[1])


def coeff_for_b(expanded, d, c0, y, b):
    """alpha_coeff that puts B = b at the grid's largest |k| (the positive root of g^2 + 2 T g - (1 - b) = 0)"""
    T = tangent(y)
    g = -T + math.sqrt(T * T + (1.0 - b))
    kmax = float(wavenumbers(expanded, d).max())
    return g / (neper(1.0, y) * c0 ** y * kmax ** (y - 1.0))


def embed(p0, expanded):
    ex, ey, ez = expanded
    nz, ny, nx = p0.shape
    v = np.zeros((ez, ey, ex), dtype=np.float64)
    v[:nz, :ny, :nx] = p0
    return v


def solve_expanded(vol, d, c0, t, alpha_coeff=0.0, y=1.5):
    """the whole expanded volume [Ez][Ey][Ex] at time t"""
    vol = np.asarray(vol, dtype=np.float64)
    ez, ey, ex = vol.shape
    X = np.fft.rfftn(vol, axes=(0, 1, 2))
    return np.fft.irfftn(X * H((ex, ey, ez), d, c0, t, alpha_coeff, y), s=vol.shape, axes=(0, 1, 2))


def solve(p0, expanded, d, c0, times, alpha_coeff=0.0, y=1.5):
    """[n_times][Nz][Ny][Nx]: the domain crop at every time"""
    nz, ny, nx = p0.shape
    X = np.fft.rfftn(embed(p0, expanded), axes=(0, 1, 2))
    shape = (expanded[2], expanded[1], expanded[0])
    k = wavenumbers(expanded, d)
    out = [np.fft.irfftn(X * H_of_k(k, c0, t, alpha_coeff, y), s=shape, axes=(0, 1, 2))[:nz, :ny, :nx] for t in np.atleast_1d(times)]
    return np.array(out)


def default_sides(n, d, c0, t_max, fused=True, lengths=None):
    """the rule of SecondOrderParameters: per axis the fast-path length at or above N + ceil(c0 t_max / d), or that number"""
    out = []
    for na, da in zip(n, d):
        m = na + int(math.ceil(c0 * t_max / da))
        fast = [L for L in (lengths or []) if L >= m] if fused else []
        out.append(min(fast) if fast else m)
    return tuple(out)


STAGE_C0 = 1500.0
STAGE_D = (1.0e-4, 0.8e-4, 1.3e-4)   # three unequal spacings: an exchanged axis shows
STAGE_Y = 1.5


def stage_case(expanded):
    """the four variants of the GPU stage test on the grid `expanded` (even sides), as (alpha_coeff, t):
    near time: c0 t = 0.37 of the smallest spacing; far time: c0 |k|max t / 2 pi = 10^4 turns, where a float32 phase is off by
    several 1e-3 rad; the coefficient lets the slowest-decaying non-zero mode keep exp(-2) at the far time:
    gamma(kmin) t_far = a c0^(y+1) kmin^y t_far = 2"""
    k = wavenumbers(expanded, STAGE_D)
    kmax, kmin = float(k.max()), float(k[k > 0].min())
    t_near = 0.37 * min(STAGE_D) / STAGE_C0
    t_far = 1.0e4 * 2.0 * math.pi / (STAGE_C0 * kmax)
    a = 2.0 / (t_far * STAGE_C0 ** (STAGE_Y + 1.0) * kmin ** STAGE_Y)
    coeff = a / neper(1.0, STAGE_Y)
    return [(0.0, t_near), (0.0, t_far), (coeff, t_near), (coeff, t_far)]


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
