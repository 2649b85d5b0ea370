"""float64 NumPy restatement of the k-space plane reconstruction (DESIGN.md "k-space plane reconstruction"), the checker of
tests/test_plane_recon_host.py and tests/test_gpu_plane_recon.py.  A plain module, imported by name from tests/.

The record p[t][y][x] (spacing dx, dy, time step dt) of a planar sensor in a homogeneous medium of sound speed c0 is
embedded, mirrored in time, in a zero volume v [Lt][Ey][Ex], Lt >= 2 Nt - 1:

    v[n] = p[n], 0 <= n < Nt;   v[Lt - n] = p[n], 1 <= n < Nt
    out = crop( positivity( 2 irfftn(G) ) )                  axes (t -> z, y, x);  z_j = j c0 dt,  j < planes <= Nt
    S = fftn(v);  M = floor(Lt / 2);  m' = min(m, Lt - m);  dk = 2 pi / (Lt dt c0);  rho2 = (kx^2 + ky^2) / dk^2
    T[m'] = S[m'] w(m'):  w = sqrt(m'^2 - rho2) / m' where m'^2 >= rho2 and m' > 0;  w(0) = 1 if rho2 = 0;  else w = 0
    f = sqrt(m'^2 + rho2),  i0 = floor(f),  a = f - i0
    linear :  G[m] = T[i0] + a (T[min(i0 + 1, M)] - T[i0])       nearest:  G[m] = T[i0] if a < 1/2 else T[min(i0 + 1, M)]
    G[m] = 0 where f > M

Bins are counted as angular_reference.wavenumbers counts them.  Arrays are [t][y][x]; `expanded`, `dims` and `spacing` are
(x, y) pairs as in kwave_amd.recon.
"""
import numpy as np

import angular_reference as ar

rel_l2 = ar.rel_l2
INTERPS = ("linear", "nearest")


def time_bins(lt):
    """m' = min(m, Lt - m) as int64, [lt]"""
    m = np.arange(lt, dtype=np.int64)
    return np.where(m <= lt // 2, m, lt - m)


def rho2(expanded, lt, spacing, dt, c0, half=True):
    """(kx^2 + ky^2) / dk^2 in the device's order, float64 [ey][ex // 2 + 1] (half) or [ey][ex]"""
    kx, ky = ar.wavenumbers(expanded, spacing, half)
    dk = 2.0 * np.pi / (lt * dt * c0)
    return ((kx * kx) + (ky * ky)) / (dk * dk)


def weight(r2, lt):
    """w(m') for m' = 0 ... M, float64 [M + 1][ey][nkx]"""
    mp = np.arange(lt // 2 + 1, dtype=np.float64)[:, None, None]
    d = (mp * mp) - r2[None]
    w = np.sqrt(np.maximum(d, 0.0)) / np.maximum(mp, 1.0)
    w = np.where(d >= 0.0, w, 0.0)
    w[0] = np.where(r2 == 0.0, 1.0, 0.0)
    return w


def positions(r2, lt):
    """(f, inside, i0, i1, a) for m' = 0 ... M; the indices are clamped into the line where f > M"""
    M = lt // 2
    mp = np.arange(M + 1, dtype=np.float64)[:, None, None]
    f = np.sqrt((mp * mp) + r2[None])
    inside = f <= M
    i0 = np.where(inside, np.floor(f), M).astype(np.int64)
    i1 = np.minimum(i0 + 1, M)
    return f, inside, i0, i1, f - i0


def regrid(S, r2, interp="linear"):
    """G [lt][ey][nkx] from the spectrum S [lt][ey][nkx] (nkx = Ex or Ex // 2 + 1, r2 to match), complex128"""
    assert interp in INTERPS
    lt = S.shape[0]
    M = lt // 2
    T = S[:M + 1] * weight(r2, lt)
    f, inside, i0, i1, a = positions(r2, lt)
    T0, T1 = np.take_along_axis(T, i0, axis=0), np.take_along_axis(T, i1, axis=0)
    Gh = T0 + a * (T1 - T0) if interp == "linear" else np.where(a < 0.5, T0, T1)
    Gh = np.where(inside, Gh, 0.0)
    return Gh[time_bins(lt)]


def embed(p, expanded, lt):
    """the record mirrored in time in the zero volume [lt][ey][ex]"""
    p = np.asarray(p)
    nt, ny, nx = p.shape
    assert lt >= 2 * nt - 1 and expanded[0] >= nx and expanded[1] >= ny
    out = np.zeros((lt, expanded[1], expanded[0]), dtype=p.dtype)
    out[:nt, :ny, :nx] = p
    if nt > 1:
        out[lt - nt + 1:, :ny, :nx] = p[:0:-1]
    return out


def stage(vol, spacing, dt, c0, interp="linear"):
    """the real-transform form on the expanded grid: 2 irfftn(G) of the (t-even) volume [lt][ey][ex], float64"""
    vol = np.asarray(vol, dtype=np.float64)
    lt, ey, ex = vol.shape
    G = regrid(np.fft.rfftn(vol), rho2((ex, ey), lt, spacing, dt, c0, half=True), interp)
    return 2.0 * np.fft.irfftn(G, s=vol.shape, axes=(0, 1, 2))


def stage_complex(vol, spacing, dt, c0, interp="linear"):
    """the same with full complex transforms: complex128 (its imaginary part is rounding for a t-even volume)"""
    vol = np.asarray(vol, dtype=np.float64)
    lt, ey, ex = vol.shape
    G = regrid(np.fft.fftn(vol), rho2((ex, ey), lt, spacing, dt, c0, half=False), interp)
    return 2.0 * np.fft.ifftn(G)


def crop(vol, dims, planes, positivity=False):
    out = vol[:planes, :dims[1], :dims[0]]
    return np.where(out > 0, out, 0).astype(out.dtype) if positivity else out.copy()


def reconstruct(p, expanded, lt, spacing, dt, c0, planes=None, interp="linear", positivity=False):
    """p0 on the domain: float64 [planes][ny][nx]"""
    p = np.asarray(p, dtype=np.float64)
    nt, ny, nx = p.shape
    planes = nt if planes is None else planes
    return crop(stage(embed(p, expanded, lt), spacing, dt, c0, interp), (nx, ny), planes, positivity)


def margins(expanded, lt, spacing, dt, c0):
    """(smallest |f - M| / M, smallest |a - 1/2| among the bins gathered) over the bins with rho2 > 0: how far the inputs
    keep every bin from the two discontinuities of G (the end of the line; the switch of the nearest neighbour)"""
    r2 = rho2(expanded, lt, spacing, dt, c0, half=True)
    M = lt // 2
    f, inside, _i0, _i1, a = positions(r2, lt)
    on = np.broadcast_to(r2[None] > 0.0, f.shape)
    first = float(np.min(np.abs(f[on] - M) / M))
    second = float(np.min(np.abs(a[on & inside] - 0.5)))
    return first, second


# ---- float32 emulation of the device's steps (kwave_hip.h "k-space plane reconstruction") ----------------------------------
def regrid_device(S, r2, interp="linear", scale=2.0):
    """G with the device's order: float64 up to the square roots and i0, float32 from there; S is rounded to complex64
    first; complex64 [lt][ey][nkx]"""
    f32 = np.float32
    lt = S.shape[0]
    M = lt // 2
    mp = np.arange(M + 1, dtype=np.float64)[:, None, None]
    d = (mp * mp) - r2[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (np.sqrt(np.maximum(d, 0.0)).astype(f32) / mp.astype(f32)) * f32(scale)
    w = np.where(d >= 0.0, w, f32(0.0)).astype(f32)
    w[0] = np.where(r2 == 0.0, f32(scale), f32(0.0))
    Sr, Si = S[:M + 1].real.astype(f32), S[:M + 1].imag.astype(f32)
    Tr, Ti = (w * Sr).astype(f32), (w * Si).astype(f32)
    f, inside, i0, i1, a = positions(r2, lt)
    a = a.astype(f32)
    out = []
    for T in (Tr, Ti):
        T0, T1 = np.take_along_axis(T, i0, axis=0), np.take_along_axis(T, i1, axis=0)
        g = ((a * (T1 - T0)).astype(f32) + T0).astype(f32) if interp == "linear" else np.where(a < f32(0.5), T0, T1)
        out.append(np.where(inside, g, f32(0.0)).astype(f32)[time_bins(lt)])
    return out[0].astype(np.complex64) + 1j * out[1].astype(np.complex64)


def stage_device(vol, spacing, dt, c0, interp="linear"):
    """2 irfftn(G) with G from regrid_device (the transforms themselves in float64)"""
    vol = np.asarray(vol, dtype=np.float64)
    lt, ey, ex = vol.shape
    G = regrid_device(np.fft.rfftn(vol), rho2((ex, ey), lt, spacing, dt, c0, half=True), interp, scale=2.0)
    return np.fft.irfftn(G.astype(np.complex128), s=vol.shape, axes=(0, 1, 2))


# ---- inputs ------------------------------------------------------------------------------------------------------------
def even_volume(shape, seed):
    """a random float32 volume [lt][ey][ex], even in t with period lt"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape).astype(np.float32)
    lt = shape[0]
    for n in range(1, lt):
        if lt - n > n:
            v[lt - n] = v[n]
    return v


def identity_record(nt, ny, nx, c0, dt, centre=12.0, width=3.0):
    """(record, g): p = g(c0 t) / 2 on every sensor point, g a Gaussian over the planes j, inside the record"""
    j = np.arange(nt, dtype=np.float64)
    g = np.exp(-((j - centre) / width) ** 2)
    return np.broadcast_to(0.5 * g[:, None, None], (nt, ny, nx)).copy(), g


def phantom_case(nt=100, nz=512, n=16):
    """the physics check: p0 = g(z) (1 + cos(2 pi x / 16) / 2 + sin(2 pi y / 16) / 4), g = exp(-((z - 30) / 6)^2)
    cos(2 pi (z - 30) / 6) (units of dx) in a periodic box nz x n x n; the record is the plane z = 0 of the exact
    propagation ifftn(P0 cos(c0 |k| t)) at t_n = n dx / c0.  Returns (record [nt][n][n], phantom [nz][n][n]), float64."""
    z = np.arange(nz, dtype=np.float64)[:, None, None]
    y = np.arange(n, dtype=np.float64)[None, :, None]
    x = np.arange(n, dtype=np.float64)[None, None, :]
    g = np.exp(-((z - 30.0) / 6.0) ** 2) * np.cos(2.0 * np.pi * (z - 30.0) / 6.0)
    p0 = g * (1.0 + 0.5 * np.cos(2.0 * np.pi * x / 16.0) + 0.25 * np.sin(2.0 * np.pi * y / 16.0))
    P0 = np.fft.fftn(p0)
    k1 = lambda m: 2.0 * np.pi * np.fft.fftfreq(m)
    k = np.sqrt(k1(nz)[:, None, None] ** 2 + k1(n)[None, :, None] ** 2 + k1(n)[None, None, :] ** 2)
    rec = np.empty((nt, n, n))
    for i in range(nt):
        rec[i] = np.fft.ifft2((P0 * np.cos(k * i)).mean(axis=0)).real  # the plane z = 0 of the inverse transform along z
    return rec, p0


# ---- the size rules --------------------------------------------------------------------------------------------------
def plan_recon(dims, nt, fused=True, expanded=None, time_length=None, lengths=None):
    """((Ex, Ey), Lt, fast): E = (Nx, Ny) unless given; Lt the smallest fast-path length >= 2 Nt - 1, or 2 Nt - 1 itself
    when there is none or off the fused pipeline"""
    from cw_reference import fast_lengths
    lengths = fast_lengths() if lengths is None else lengths
    expanded = tuple(dims) if expanded is None else tuple(expanded)
    least = 2 * nt - 1
    if time_length is not None:
        lt = time_length
    elif fused and least <= lengths[-1]:
        lt = min(length for length in lengths if length >= least)
    else:
        lt = least
    fast = fused and all(v in lengths for v in expanded + (lt,))
    return expanded, lt, fast
