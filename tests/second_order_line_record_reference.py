"""Float64 restatement of the line-sensor record of the batched 2-D exact k-space propagator (include/kwave_hip.h
"Line-sensor record of the propagator on frames"; a plain module, imported by name from tests/).  Arrays are [F][y][x]; n, d
and expanded are given as (x, y).  For the row y = r dy:

    p_f(x, y_r; t) = irfft_x[ G_f(kx; t) ],   kx = 0 ... Ex/2
    G_f(kx; t)     = sum over m = 0 ... Ey/2 of H(kx, m; t) Q_f(kx, m)
    Q_f(kx, m)     = q_f(kx, m) + q_f(kx, Ey - m)   (bins 0 and, Ey even, Ey/2 pair with themselves: q_f(kx, m) alone)
    q_f(kx, ky)    = rfft2(p0_f embedded)(kx, ky) exp(+2 pi i ky r / Ey) / (Ex Ey)

written out directly: no 2-D inverse anywhere.  Also the inputs of the GPU stage tests and a float32 emulation of the record
kernel's accumulation over the folded bins.
"""
import math

import numpy as np

import second_order_reference as sr


def folded_q(vol, row):
    """Q [F][Ey/2 + 1][Ex/2 + 1] (complex128) of the expanded planes vol [F][Ey][Ex]"""
    vol = np.asarray(vol, dtype=np.float64)
    nf, ey, ex = vol.shape
    m = np.arange(ey)
    phase = np.exp(2j * math.pi * ((m * row) % ey) / ey)
    q = np.fft.rfft2(vol) * phase[None, :, None] / (ex * ey)
    mf = ey // 2 + 1
    Q = q[:, :mf].copy()
    for i in range(1, mf):
        if ey - i != i:
            Q[:, i] += q[:, ey - i]
    return Q


def folded_k(expanded, d):
    """|k| on [Ey/2 + 1][Ex/2 + 1]"""
    ex, ey = expanded
    ix, iy = np.arange(ex // 2 + 1), np.arange(ey // 2 + 1)
    kx = 2.0 * math.pi / (ex * d[0]) * np.minimum(ix, ex - ix)
    ky = 2.0 * math.pi / (ey * d[1]) * iy
    return np.sqrt(kx[None, :] ** 2 + ky[:, None] ** 2)


def spectrum(Q, expanded, d, c0, times, alpha_coeff=0.0, y=1.5):
    """G [F][n_times][Ex/2 + 1] (complex128)"""
    k = folded_k(expanded, d)
    return np.stack([(Q * sr.H_of_k(k, c0, t, alpha_coeff, y)[None]).sum(axis=1) for t in np.atleast_1d(times)], axis=1)


def rows_of(G, ex):
    """the x-inverse: [F][n_times][Ex] of G (the divider is in Q already)"""
    return np.fft.irfft(G, n=ex, axis=-1) * ex


def record_expanded(vol, d, c0, times, row, alpha_coeff=0.0, y=1.5):
    """[F][n_times][Ex]: the row of every expanded plane of vol [F][Ey][Ex] at every time"""
    nf, ey, ex = np.shape(vol)
    return rows_of(spectrum(folded_q(vol, row), (ex, ey), d, c0, times, alpha_coeff, y), ex)


def record(p0, expanded, d, c0, times, row, alpha_coeff=0.0, y=1.5):
    """[F][n_times][Nx]: the record of the domain's row"""
    p0 = np.asarray(p0, dtype=np.float64)
    nf, ny, nx = p0.shape
    vol = np.zeros((nf, expanded[1], expanded[0]))
    vol[:, :ny, :nx] = p0
    return record_expanded(vol, d, c0, times, row, alpha_coeff, y)[:, :, :nx]


def source_frames(rng, nf, ey, ex):
    """the inputs of the stage tests, drawn as tests/test_gpu_second_order_frames.py draws its own: every frame a smooth random
    field on the whole expanded plane plus 5 % white noise"""
    y, x = np.meshgrid(np.arange(ey) / ey, np.arange(ex) / ex, indexing="ij")
    out = np.empty((nf, ey, ex), np.float32)
    for f in range(nf):
        c = rng.uniform(-1.0, 1.0, 8)
        s = (c[0] + c[1] * np.cos(2 * np.pi * x + c[2]) * np.sin(2 * np.pi * y + c[6]) +
             c[3] * np.sin(4 * np.pi * y + c[4]) * np.cos(2 * np.pi * x) +
             c[5] * np.exp(-((x - 0.4) ** 2 + (y - 0.6) ** 2) / 0.02) * np.cos(6 * np.pi * y + c[7]))
        out[f] = s + 0.05 * rng.standard_normal((ey, ex))
    return out


def accumulate_f32(Q, H):
    """the record kernel's sum in its order: per (frame, kx) and part one float32 accumulator from zero that takes the folded
    bins in ascending m by acc = fma(H, Q, acc), H and Q rounded to float32 first.  (The kernel's chunks of 64 bins stage Q
    in LDS; they do not split the sum.)  Q [F][Mf][nxc] complex, H [Mf][nxc] real; returns [F][nxc] complex128 of float32
    values.  The fma is taken as the float64 sum of the exact product rounded to float32."""
    q32r, q32i = Q.real.astype(np.float32).astype(np.float64), Q.imag.astype(np.float32).astype(np.float64)
    h32 = H.astype(np.float32).astype(np.float64)
    ar = np.zeros((Q.shape[0], Q.shape[2]), np.float32)
    ai = np.zeros_like(ar)
    for m in range(Q.shape[1]):
        ar = (h32[m][None] * q32r[:, m] + ar.astype(np.float64)).astype(np.float32)
        ai = (h32[m][None] * q32i[:, m] + ai.astype(np.float64)).astype(np.float32)
    return ar.astype(np.float64) + 1j * ai.astype(np.float64)
