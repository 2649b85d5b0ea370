"""Float64 restatement of the plane-sensor record of the 3-D exact k-space propagator (include/kwave_hip.h "Plane-sensor
record of the 3-D propagator"; a plain module, imported by name from tests/).  Arrays are [z][y][x]; n, d and expanded are
given as (x, y, z).  For the plane z = r dz:

    p(x, y, z_r; t) = irfft2_xy[ G(kx, ky; t) ],   kx = 0 ... Ex/2, ky = 0 ... Ey - 1
    G(kx, ky; t)    = sum over m = 0 ... Ez/2 of H(kx, ky, m; t) Q(kx, ky, m)
    Q(kx, ky, m)    = q(kx, ky, m) + q(kx, ky, Ez - m)   (bins 0 and, Ez even, Ez/2 pair with themselves: q(kx, ky, m) alone)
    q(kx, ky, kz)   = rfftn(p0 embedded)(kx, ky, kz) exp(+2 pi i kz r / Ez) / (Ex Ey Ez)

written out directly: no 3-D inverse anywhere.  Also the inputs of the GPU stage tests and a float32 emulation of the record
kernel's accumulation over the folded bins.
"""
import math

import numpy as np

import second_order_reference as sr


def folded_q(vol, plane):
    """Q [Ey][Ex/2 + 1][Ez/2 + 1] (complex128, the device's layout) of the expanded volume vol [Ez][Ey][Ex]"""
    vol = np.asarray(vol, dtype=np.float64)
    ez, ey, ex = vol.shape
    m = np.arange(ez)
    phase = np.exp(2j * math.pi * ((m * plane) % ez) / ez)
    q = np.fft.rfftn(vol, axes=(0, 1, 2)) * phase[:, None, None] / (ex * ey * ez)
    mf = ez // 2 + 1
    Q = q[:mf].copy()
    for i in range(1, mf):
        if ez - i != i:
            Q[i] += q[ez - i]
    return np.ascontiguousarray(Q.transpose(1, 2, 0))


def folded_k(expanded, d):
    """|k| on [Ey][Ex/2 + 1][Ez/2 + 1]"""
    ex, ey, ez = expanded
    ix, iy, iz = np.arange(ex // 2 + 1), np.arange(ey), np.arange(ez // 2 + 1)
    kx = 2.0 * math.pi / (ex * d[0]) * np.minimum(ix, ex - ix)
    ky = 2.0 * math.pi / (ey * d[1]) * np.minimum(iy, ey - iy)
    kz = 2.0 * math.pi / (ez * d[2]) * iz
    return np.sqrt(kx[None, :, None] ** 2 + ky[:, None, None] ** 2 + kz[None, None, :] ** 2)


def spectrum(Q, expanded, d, c0, times, alpha_coeff=0.0, y=1.5):
    """G [n_times][Ey][Ex/2 + 1] (complex128)"""
    k = folded_k(expanded, d)
    return np.stack([(Q * sr.H_of_k(k, c0, t, alpha_coeff, y)).sum(axis=2) for t in np.atleast_1d(times)])


def planes_of(G, ex):
    """the inverse over the record: [n_times][Ey][Ex] of G [n_times][Ey][Ex/2 + 1] (the divider is in Q already)"""
    ey = G.shape[-2]
    return np.fft.irfft2(G, s=(ey, ex), axes=(-2, -1)) * (ex * ey)


def record_expanded(vol, d, c0, times, plane, alpha_coeff=0.0, y=1.5):
    """[n_times][Ey][Ex]: the plane of the expanded volume vol [Ez][Ey][Ex] at every time"""
    ez, ey, ex = np.shape(vol)
    return planes_of(spectrum(folded_q(vol, plane), (ex, ey, ez), d, c0, times, alpha_coeff, y), ex)


def record(p0, expanded, d, c0, times, plane, alpha_coeff=0.0, y=1.5):
    """[n_times][Ny][Nx]: the record of the domain's plane"""
    p0 = np.asarray(p0, dtype=np.float64)
    nz, ny, nx = p0.shape
    return record_expanded(sr.embed(p0, expanded), d, c0, times, plane, alpha_coeff, y)[:, :ny, :nx]


def source_volume(rng, ex, ey, ez):
    """the input of the stage tests, drawn as tests/test_gpu_second_order.py draws its own: a smooth random field on the
    whole expanded volume plus 5 % white noise, so that every bin carries something"""
    z, y, x = np.meshgrid(np.arange(ez) / ez, np.arange(ey) / ey, np.arange(ex) / ex, indexing="ij")
    c = rng.uniform(-1.0, 1.0, 8)
    s = (c[0] + c[1] * np.cos(2 * np.pi * x + c[2]) * np.sin(2 * np.pi * z + c[6]) +
         c[3] * np.sin(4 * np.pi * y + c[4]) * np.cos(2 * np.pi * x) * np.cos(4 * np.pi * z) +
         c[5] * np.exp(-((x - 0.4) ** 2 + (y - 0.6) ** 2 + (z - 0.5) ** 2) / 0.02) * np.cos(6 * np.pi * z + c[7]))
    return (s + 0.05 * rng.standard_normal((ez, ey, ex))).astype(np.float32)


def accumulate_f32(Q, H):
    """the record kernel's sum in its order: per (ky, kx) and part one float32 accumulator from zero that takes the folded
    bins in ascending m by acc = fma(H, Q, acc), H and Q rounded to float32 first.  (The kernel's chunks of 64 bins stage Q
    in LDS; they do not split the sum.)  Q [Ey][nxc][Mf] complex, H [Ey][nxc][Mf] real; returns [Ey][nxc] complex128 of
    float32 values.  The fma is taken as the float64 sum of the exact product rounded to float32."""
    q32r, q32i = Q.real.astype(np.float32).astype(np.float64), Q.imag.astype(np.float32).astype(np.float64)
    h32 = H.astype(np.float32).astype(np.float64)
    ar = np.zeros(Q.shape[:2], np.float32)
    ai = np.zeros_like(ar)
    for m in range(Q.shape[2]):
        ar = (h32[..., m] * q32r[..., m] + ar.astype(np.float64)).astype(np.float32)
        ai = (h32[..., m] * q32i[..., m] + ai.astype(np.float64)).astype(np.float32)
    return ar.astype(np.float64) + 1j * ai.astype(np.float64)
