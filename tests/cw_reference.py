"""float64 NumPy restatement of the CW field propagator (DESIGN.md "CW field propagator"), the checker of
tests/test_cw_host.py and tests/test_gpu_cw.py.  A plain module, imported by name from tests/.

Problem: p_tt - c0^2 lap(p) = S(x) exp(i w t), p = p_t = 0 at t = 0, homogeneous lossless medium, periodic grid.  Per
wavenumber bin, a = c0 |k|, d = a - w:

    p^(k, T) = S^(k) G(a),    G(a) = i [ sin(a T)/a - T exp(i (a + w) T/2) sinc(d T/2) ] / (a + w)

and the reported field is the complex amplitude P(x) = p(x, T) exp(-i w T).  Arrays are [z][y][x]; `dims`, `spacing` and
`expanded` are (x, y, z) triples as in kwave_amd.cw.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the operator -------------------------------------------------------------------------------------------------------
def _sinc(x):
    """sin(x) / x with the value 1 at 0"""
    x = np.asarray(x, dtype=np.float64)
    safe = np.where(x == 0.0, 1.0, x)
    return np.where(x == 0.0, 1.0, np.sin(safe) / safe)


def operator(a, w, T):
    """G(a) in the regular form: finite at the resonance a = w and at a = 0, no bin treated apart"""
    a = np.asarray(a, dtype=np.float64)
    s1 = T * _sinc(a * T)                                   # sin(a T) / a, -> T at a = 0
    return 1j * (s1 - T * np.exp(1j * (a + w) * T / 2) * _sinc((a - w) * T / 2)) / (a + w)


def operator_textbook(a, w, T):
    """the same as (exp(i w T) - cos(a T) - i (w / a) sin(a T)) / (a^2 - w^2): singular at a = w and a = 0"""
    a = np.asarray(a, dtype=np.float64)
    return (np.exp(1j * w * T) - np.cos(a * T) - 1j * (w / a) * np.sin(a * T)) / (a * a - w * w)


def limit_at_resonance(w, T):
    return 1j * (np.sin(w * T) / w - T * np.exp(1j * w * T)) / (2 * w)


def limit_at_zero(w, T):
    return 1j * T * (1 - np.exp(1j * w * T / 2) * _sinc(w * T / 2)) / w


def wavenumber_magnitude(expanded, spacing, half=False):
    """|k| on the expanded grid [ez][ey][ex] (half: the reduced grid [ez][ey][ex // 2 + 1]); the bins are counted as the
    device counts them: k = 2 pi / (E d) * min(i, E - i)"""
    (ex, ey, ez), (dx, dy, dz) = expanded, spacing
    def axis(n, d, count):
        i = np.arange(count, dtype=np.float64)
        return (2.0 * np.pi / (n * d)) * np.where(i <= n // 2, i, n - i)
    kx = axis(ex, dx, ex // 2 + 1 if half else ex)
    ky, kz = axis(ey, dy, ey), axis(ez, dz, ez)
    return np.sqrt(kx[None, None, :] ** 2 + ky[None, :, None] ** 2 + kz[:, None, None] ** 2)


def stored_operator(expanded, spacing, c0, f0, T, half=False):
    """G exp(-i w T) / (Ex Ey Ez) as kw_cw_operator stores it, complex128"""
    w = 2.0 * np.pi * f0
    a = c0 * wavenumber_magnitude(expanded, spacing, half)
    return operator(a, w, T) * np.exp(-1j * w * T) / float(expanded[0] * expanded[1] * expanded[2])


# ---- the solution on the expanded grid ----------------------------------------------------------------------------------
def solve_complex(S, G_full):
    """complex FFT form: P = N ifftn(G' fftn(S)), G' = stored operator on the full grid (carries 1 / N)"""
    return np.fft.ifftn(G_full * np.fft.fftn(S)) * S.size


def solve_pair(Sr, Si, G_half):
    """real-transform form: two rfftn, the 2x2 mix, two irfftn -> (Re P, Im P)"""
    n = Sr.size
    Xr, Xi = np.fft.rfftn(Sr), np.fft.rfftn(Si)
    Gr, Gi = G_half.real, G_half.imag
    Pr = np.fft.irfftn(Gr * Xr - Gi * Xi, s=Sr.shape, axes=(0, 1, 2)) * n
    Pi = np.fft.irfftn(Gi * Xr + Gr * Xi, s=Sr.shape, axes=(0, 1, 2)) * n
    return Pr, Pi


def solve_pair_f32(Sr, Si, G_half):
    """float32 twin of solve_pair (scipy.fft keeps complex64), operators rounded once to float32"""
    import scipy.fft as sf
    n = np.float32(Sr.size)
    Sr, Si = Sr.astype(np.float32), Si.astype(np.float32)
    Gr, Gi = G_half.real.astype(np.float32), G_half.imag.astype(np.float32)
    Xr, Xi = sf.rfftn(Sr), sf.rfftn(Si)
    assert Xr.dtype == np.complex64
    Pr = sf.irfftn(Gr * Xr - Gi * Xi, s=Sr.shape, axes=(0, 1, 2)) * n
    Pi = sf.irfftn(Gi * Xr + Gr * Xi, s=Sr.shape, axes=(0, 1, 2)) * n
    assert Pr.dtype == np.float32
    return Pr, Pi


# ---- the no-wrap-around rule --------------------------------------------------------------------------------------------
def fast_lengths():
    """the fused pipeline's line lengths, read from csrc/kw_fused.hip"""
    src = open(os.path.join(ROOT, "k-wave-fluid-cuda_amd", "csrc", "kw_fused.hip")).read()
    short = re.search(r"#define KW_FUSED_LENGTHS_SHORT\(X\)(.*?)\n#define", src, re.S).group(1)
    long_ = re.search(r"#define KW_FUSED_LENGTHS_LONG\(X\)(.*?)\n#if", src, re.S).group(1)
    return sorted(int(x) for x in re.findall(r"X\((\d+)\)", short + long_))


def default_time(dims, spacing, c0):
    return float(np.sqrt(sum((n * d) ** 2 for n, d in zip(dims, spacing))) / c0)


def least_sides(dims, spacing, c0, T):
    return tuple(int(n + np.ceil(c0 * T / d)) for n, d in zip(dims, spacing))


def plan(dims, spacing, c0, T=None, fused=True):
    """(T, expanded) by the rule: the smallest fast-path lengths, or the smallest even sides"""
    T = default_time(dims, spacing, c0) if T is None else T
    least = least_sides(dims, spacing, c0, T)
    lengths = fast_lengths()
    if fused and all(v <= lengths[-1] for v in least):
        return T, tuple(min(length for length in lengths if length >= v) for v in least)
    return T, tuple(v + v % 2 for v in least)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def embed(S, expanded):
    """zero-filled [ez][ey][ex] array with S in its [0, N) corner"""
    out = np.zeros((expanded[2], expanded[1], expanded[0]), dtype=S.dtype)
    out[:S.shape[0], :S.shape[1], :S.shape[2]] = S
    return out


def propagate(S, spacing, c0, f0, T, expanded, scale=1.0):
    """P on the domain for the complex source S [nz][ny][nx] (float64 of whatever the caller rounded)"""
    G = stored_operator(expanded, spacing, c0, f0, T, half=True)
    E = embed(np.asarray(S, dtype=np.complex128) * scale, expanded)
    Pr, Pi = solve_pair(E.real.copy(), E.imag.copy(), G)
    nz, ny, nx = S.shape
    return (Pr + 1j * Pi)[:nz, :ny, :nx]


def kwave_scale(spacing, c0, f0):
    """2 i w c0 / dx: the factor that turns the time loop's additive pressure source amplitude into S"""
    return 2j * (2.0 * np.pi * f0) * c0 / spacing[0]


def green(r, c0, f0):
    """free-space solution for a unit point source: exp(-i k r) / (4 pi c0^2 r)"""
    k = 2.0 * np.pi * f0 / c0
    return np.exp(-1j * k * r) / (4.0 * np.pi * c0 * c0 * r)


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
