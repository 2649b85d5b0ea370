"""float64 NumPy restatement of the batched k-space line reconstruction (DESIGN.md "k-space line reconstruction"), the
checker of tests/test_line_recon_host.py and tests/test_gpu_line_recon.py.  A plain module, imported by name from tests/.

One frame p[t][y] (sensor pitch dy, time step dt) of a linear array in a homogeneous medium of sound speed c0 is embedded,
mirrored in time, in a zero plane v [Lt][Ey], Lt >= 2 Nt - 1:

    v[n] = p[n], 0 <= n < Nt;   v[Lt - n] = p[n], 1 <= n < Nt
    out = crop( positivity( 2 irfft2(G) ) )                  axes (t -> x, y);  x_j = j c0 dt,  j < depth <= Nt
    S = fft2(v);  M = floor(Lt / 2);  m' = min(m, Lt - m);  dk = 2 pi / (Lt dt c0);  rho2 = ky^2 / dk^2
    T[m'] = S[m'] w(m'):  w = sqrt(m'^2 - rho2) / m' where m'^2 >= rho2 and m' > 0;  w(0) = 1 if rho2 = 0;  else w = 0
    f = sqrt(m'^2 + rho2),  i0 = floor(f),  a = f - i0
    linear :  G[m] = T[i0] + a (T[min(i0 + 1, M)] - T[i0])       nearest:  G[m] = T[i0] if a < 1/2 else T[min(i0 + 1, M)]
    G[m] = 0 where f > M

— plane_recon_reference's definition with one lateral axis, written out again here so that the two can be compared.  Frames
are independent: arrays are [t][y] for one frame and [F][t][y] for a batch.
"""
import numpy as np

INTERPS = ("linear", "nearest")


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def time_bins(lt):
    """m' = min(m, Lt - m) as int64, [lt]"""
    m = np.arange(lt, dtype=np.int64)
    return np.where(m <= lt // 2, m, lt - m)


def wavenumber(ey, dy, half=True):
    """ky = 2 pi / (Ey dy) * min(i, Ey - i), [Ey // 2 + 1] (half) or [Ey]"""
    i = np.arange(ey // 2 + 1 if half else ey, dtype=np.float64)
    return (2.0 * np.pi / (ey * dy)) * np.where(i <= ey // 2, i, ey - i)


def rho2(ey, lt, dy, dt, c0, half=True):
    """ky^2 / dk^2 in the device's order, float64 [nky]"""
    k = wavenumber(ey, dy, half)
    dk = 2.0 * np.pi / (lt * dt * c0)
    return (k * k) / (dk * dk)


def weight(r2, lt):
    """w(m') for m' = 0 ... M, float64 [M + 1][nky]"""
    mp = np.arange(lt // 2 + 1, dtype=np.float64)[:, None]
    d = (mp * mp) - r2[None]
    w = np.sqrt(np.maximum(d, 0.0)) / np.maximum(mp, 1.0)
    w = np.where(d >= 0.0, w, 0.0)
    w[0] = np.where(r2 == 0.0, 1.0, 0.0)
    return w


def positions(r2, lt):
    """(f, inside, i0, i1, a) for m' = 0 ... M, [M + 1][nky]; the indices are clamped into the line where f > M"""
    M = lt // 2
    mp = np.arange(M + 1, dtype=np.float64)[:, None]
    f = np.sqrt((mp * mp) + r2[None])
    inside = f <= M
    i0 = np.where(inside, np.floor(f), M).astype(np.int64)
    i1 = np.minimum(i0 + 1, M)
    return f, inside, i0, i1, f - i0


def regrid(S, r2, interp="linear"):
    """G [lt][nky] from the spectrum S [lt][nky] of one frame (nky = Ey or Ey // 2 + 1, r2 to match), complex128"""
    assert interp in INTERPS
    lt = S.shape[0]
    M = lt // 2
    T = S[:M + 1] * weight(r2, lt)
    f, inside, i0, i1, a = positions(r2, lt)
    T0, T1 = np.take_along_axis(T, i0, axis=0), np.take_along_axis(T, i1, axis=0)
    Gh = T0 + a * (T1 - T0) if interp == "linear" else np.where(a < 0.5, T0, T1)
    Gh = np.where(inside, Gh, 0.0)
    return Gh[time_bins(lt)]


def embed(p, ey, lt):
    """the frames [F][nt][ny] (or one [nt][ny]) mirrored in time in zero planes [F][lt][ey] ([lt][ey])"""
    p = np.asarray(p)
    if p.ndim == 2:
        return embed(p[None], ey, lt)[0]
    nf, nt, ny = p.shape
    assert lt >= 2 * nt - 1 and ey >= ny
    out = np.zeros((nf, lt, ey), dtype=p.dtype)
    out[:, :nt, :ny] = p
    if nt > 1:
        out[:, lt - nt + 1:, :ny] = p[:, :0:-1]
    return out


def stage(vol, dy, dt, c0, interp="linear"):
    """the real-transform form: 2 irfft2(G) of every (t-even) plane of vol [F][lt][ey] (or one [lt][ey]), float64"""
    vol = np.asarray(vol, dtype=np.float64)
    if vol.ndim == 3:
        return np.stack([stage(v, dy, dt, c0, interp) for v in vol])
    lt, ey = vol.shape
    G = regrid(np.fft.rfft2(vol), rho2(ey, lt, dy, dt, c0, half=True), interp)
    return 2.0 * np.fft.irfft2(G, s=vol.shape)


def stage_complex(vol, dy, dt, c0, interp="linear"):
    """the same for one plane with full complex transforms: complex128 (its imaginary part is rounding for a t-even plane)"""
    vol = np.asarray(vol, dtype=np.float64)
    lt, ey = vol.shape
    G = regrid(np.fft.fft2(vol), rho2(ey, lt, dy, dt, c0, half=False), interp)
    return 2.0 * np.fft.ifft2(G)


def crop(vol, ny, depth, positivity=False):
    out = vol[..., :depth, :ny]
    return np.where(out > 0, out, 0).astype(out.dtype) if positivity else out.copy()


def reconstruct(p, ey, lt, dy, dt, c0, depth=None, interp="linear", positivity=False):
    """p0: float64 [F][depth][ny] for frames [F][nt][ny], [depth][ny] for one frame [nt][ny]"""
    p = np.asarray(p, dtype=np.float64)
    nt, ny = p.shape[-2:]
    depth = nt if depth is None else depth
    return crop(stage(embed(p, ey, lt), dy, dt, c0, interp), ny, depth, positivity)


def margins(ey, lt, dy, dt, c0):
    """(smallest |f - M| / M, smallest |a - 1/2| among the bins gathered) over the bins with rho2 > 0: how far the inputs
    keep every bin from the two discontinuities of G (the end of the line; the switch of the nearest neighbour).
    (inf, inf) where no bin has rho2 > 0 (Ey = 1)."""
    r2 = rho2(ey, lt, dy, dt, c0, half=True)
    M = lt // 2
    f, inside, _i0, _i1, a = positions(r2, lt)
    on = np.broadcast_to(r2[None] > 0.0, f.shape)
    if not on.any():
        return float("inf"), float("inf")
    first = float(np.min(np.abs(f[on] - M) / M))
    gathered = on & inside
    second = float(np.min(np.abs(a[gathered] - 0.5))) if gathered.any() else float("inf")
    return first, second


# ---- float32 emulation of the device's steps (kwave_hip.h "k-space plane reconstruction") ------------------------------
def regrid_device(S, r2, interp="linear", scale=2.0):
    """G of one frame with the device's order: float64 up to the square roots and i0, float32 from there; S is rounded to
    complex64 first; complex64 [lt][nky]"""
    f32 = np.float32
    lt = S.shape[0]
    M = lt // 2
    mp = np.arange(M + 1, dtype=np.float64)[:, None]
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


def stage_device(vol, dy, dt, c0, interp="linear"):
    """2 irfft2(G) of one plane with G from regrid_device (the transforms themselves in float64)"""
    vol = np.asarray(vol, dtype=np.float64)
    lt, ey = vol.shape
    G = regrid_device(np.fft.rfft2(vol), rho2(ey, lt, dy, dt, c0, half=True), interp, scale=2.0)
    return np.fft.irfft2(G.astype(np.complex128), s=vol.shape)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def even_frames(shape, seed):
    """random float32 planes [F][lt][ey], each even in t with period lt"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape).astype(np.float32)
    lt = shape[1]
    for n in range(1, lt):
        if lt - n > n:
            v[:, lt - n] = v[:, n]
    return v


def identity_record(nt, ny, centre=12.0, width=3.0):
    """(record [nt][ny], g): p = g(c0 t) / 2 on every sensor, g a Gaussian over the rows j, inside the record"""
    j = np.arange(nt, dtype=np.float64)
    g = np.exp(-((j - centre) / width) ** 2)
    return np.broadcast_to(0.5 * g[:, None], (nt, ny)).copy(), g


def phantom_case(nt=100, nx=512, n=16):
    """the physics check in 2-D: p0 = g(x) (1 + cos(2 pi y / 16) / 2), g = exp(-((x - 30) / 6)^2) cos(2 pi (x - 30) / 6)
    (units of dx) in a periodic box nx x n; the record is the line x = 0 of the exact propagation
    ifft2(P0 cos(c0 |k| t)) at t_n = n dx / c0.  Returns (record [nt][n], phantom [nx][n]), float64."""
    x = np.arange(nx, dtype=np.float64)[:, None]
    y = np.arange(n, dtype=np.float64)[None, :]
    g = np.exp(-((x - 30.0) / 6.0) ** 2) * np.cos(2.0 * np.pi * (x - 30.0) / 6.0)
    p0 = g * (1.0 + 0.5 * np.cos(2.0 * np.pi * y / 16.0))
    P0 = np.fft.fft2(p0)
    k1 = lambda m: 2.0 * np.pi * np.fft.fftfreq(m)
    k = np.sqrt(k1(nx)[:, None] ** 2 + k1(n)[None, :] ** 2)
    rec = np.empty((nt, n))
    for i in range(nt):
        rec[i] = np.fft.ifft((P0 * np.cos(k * i)).mean(axis=0)).real  # the line x = 0 of the inverse transform along x
    return rec, p0


# ---- the size rules --------------------------------------------------------------------------------------------------
NO_PARTIAL_X_TILES = (672, 700, 720, 756, 784, 800, 840, 864, 900, 960)  # csrc/kw_fused.hip has_partial_x_tiles: false
CHUNK_BINS = 2 ** 29        # padded bins of one chunk: the pass along t addresses them by 32-bit byte offsets (8 B each)
CHUNK_FRAMES_MAX = 65535    # the frame is a block index of that pass
ROWS_PER_TILE = 16                                                       # 2 nl_x of those lengths


def plan(ny, nt, frames=1, fused=True, expanded=None, time_length=None, depth=None, chunk_frames=None, lengths=None):
    """(Ey, Lt, depth, chunk_frames, fast): Ey = Ny unless given; Lt the smallest fast-path length >= 2 Nt - 1, or 2 Nt - 1
    itself when there is none or off the fused pipeline; chunk_frames all frames, capped at CHUNK_FRAMES_MAX and so that the
    padded bins of a chunk stay below CHUNK_BINS; fast when
    Ey and Lt are fast-path lengths and, where Ey has no masked x kernels, the rows of a chunk make whole x tiles"""
    from cw_reference import fast_lengths
    lengths = fast_lengths() if lengths is None else lengths
    ey = ny if expanded is None else expanded
    least = 2 * nt - 1
    if time_length is not None:
        lt = time_length
    elif fused and least <= lengths[-1]:
        lt = min(length for length in lengths if length >= least)
    else:
        lt = least
    pitch = (ey // 2 + 1 + 15) // 16 * 16
    cap = min(CHUNK_FRAMES_MAX, (CHUNK_BINS - 1) // (pitch * lt))
    chunk = min(frames, cap) if chunk_frames is None else chunk_frames
    whole = ey not in NO_PARTIAL_X_TILES or (lt * chunk) % ROWS_PER_TILE == 0
    fast = bool(fused and ey in lengths and lt in lengths and whole)
    return ey, lt, nt if depth is None else depth, chunk, fast
