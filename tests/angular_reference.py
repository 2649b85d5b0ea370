"""float64 NumPy restatement of the angular-spectrum CW projector (DESIGN.md "Angular-spectrum projector"), the checker
of tests/test_angular_host.py and tests/test_gpu_angular.py.  A plain module, imported by name from tests/.

A complex pressure plane P0[y][x] (spacing dx, dy) is projected to the planes z_j = z0 + j dz, j < Nz, of a homogeneous
medium with wavenumber k = 2 pi f0 / c0 and absorption alpha [Np/m] (time factor exp(+i w t), outgoing exp(-i k r)):

    P(., ., z_j) = crop( ifft2( fft2(P0 embedded in Ex x Ey) H(kx, ky, z_j) ) )
    kr^2 < k^2:  H = exp(-i q z) exp(-alpha z k / q)     q = |k^2 - kr^2|^(1/2)
    kr^2 = k^2:  H = 1 (lossless), 0 (absorbing)
    kr^2 > k^2:  H = exp(-q z)
    angular restriction:  H = 0 where kr > kc(z) = k sqrt(D^2/2 / (D^2/2 + z^2)),  D = min((Ex - 1) dx, (Ey - 1) dy)

Bins are counted as cw_reference.wavenumber_magnitude counts them.  Arrays are [y][x] and [z][y][x]; `expanded`, `dims` and
`spacing` are (x, y) pairs as in kwave_amd.angular.
"""
import numpy as np

LOG2E = 1.0 / np.log(2.0)
MAX_PLANES = 4096


def wavenumbers(expanded, spacing, half=False):
    """(kx[None, :], ky[:, None]) with k = 2 pi / (E d) * min(i, E - i); half: kx on the Ex // 2 + 1 reduced bins"""
    (ex, ey), (dx, dy) = expanded, spacing

    def axis(n, d, count):
        i = np.arange(count, dtype=np.float64)
        return (2.0 * np.pi / (n * d)) * np.where(i <= n // 2, i, n - i)
    return axis(ex, dx, ex // 2 + 1 if half else ex)[None, :], axis(ey, dy, ey)[:, None]


def radial(expanded, spacing, half=False):
    kx, ky = wavenumbers(expanded, spacing, half)
    return kx * kx + ky * ky


def aperture(expanded, spacing):
    """D of the angular restriction"""
    return min((expanded[0] - 1) * spacing[0], (expanded[1] - 1) * spacing[1])


def cutoff(expanded, spacing, k, z):
    """kc(z)"""
    h = 0.5 * aperture(expanded, spacing) ** 2
    z = np.asarray(z, dtype=np.float64)
    return k * np.sqrt(h / (h + z * z))


def planes(z0, dz, nz):
    return z0 + np.arange(nz, dtype=np.float64) * dz


def tables(expanded, spacing, k, alpha, z0, dz, nz, restrict=True, half=True):
    """the five per-bin tables of kw_angular_operator: (a0, a1) uint32 phase words in turns / 2^32, (b0, b1) float64
    decay exponents in log2 units, alive uint32 = number of leading planes on which the bin is kept"""
    kr2 = radial(expanded, spacing, half)
    k2 = k * k
    prop, eva = kr2 < k2, kr2 > k2
    q = np.sqrt(np.abs(k2 - kr2))
    qs = np.where(q == 0.0, 1.0, q)

    def word(zz):
        t = q * zz / (2.0 * np.pi)
        w = np.rint((t - np.floor(t)) * 4294967296.0)
        return np.where(prop, np.mod(w, 4294967296.0), 0.0).astype(np.uint32)

    def decay(zz):
        return np.where(prop, alpha * zz * k / qs, np.where(eva, q * zz, 0.0)) * LOG2E
    if restrict:
        kc = cutoff(expanded, spacing, k, planes(z0, dz, nz))
        alive = (np.sqrt(kr2)[..., None] <= kc).sum(axis=-1).astype(np.uint32)
    else:
        alive = np.full(kr2.shape, nz, dtype=np.uint32)
    if alpha > 0.0:
        alive = np.where(kr2 == k2, 0, alive).astype(np.uint32)
    return word(z0), word(dz), decay(z0), decay(dz), alive


def H_exact(expanded, spacing, k, alpha, z, restrict=True, half=False):
    """H(kx, ky, z) straight from the definition, complex128"""
    kr2 = radial(expanded, spacing, half)
    k2 = k * k
    q = np.sqrt(np.abs(k2 - kr2))
    qs = np.where(q == 0.0, 1.0, q)
    H = np.where(kr2 < k2, np.exp(-1j * q * z) * np.exp(-alpha * z * k / qs), np.exp(-q * z) + 0j)
    H = np.where(kr2 == k2, 0.0 if alpha > 0.0 else 1.0, H)
    if restrict:
        H = np.where(np.sqrt(kr2) > cutoff(expanded, spacing, k, z), 0.0, H)
    return H


def H_tables(tab, j, dtype=np.float64):
    """H of plane j from the tables with the wrapping 32-bit phase accumulator; dtype float32 emulates the device's
    arithmetic (phase word -> signed float -> radians, one sincos, one exp2)"""
    a0, a1, b0, b1, alive = tab
    ph = (a0.astype(np.uint64) + np.uint64(j) * a1.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    signed = ph.astype(np.uint32).view(np.int32)
    if dtype == np.float32:
        ang = signed.astype(np.float32) * np.float32(2.0 * np.pi / 4294967296.0)
        mag = np.exp2(-(b0.astype(np.float32) + np.float32(j) * b1.astype(np.float32))).astype(np.float32)
        c, s = np.cos(ang.astype(np.float64)).astype(np.float32), np.sin(ang.astype(np.float64)).astype(np.float32)
        H = (mag * c).astype(np.complex64) - 1j * (mag * s).astype(np.complex64)
    else:
        ang = signed.astype(np.float64) * (2.0 * np.pi / 4294967296.0)
        H = np.exp2(-(b0 + j * b1)) * np.exp(-1j * ang)
    return np.where(alive > j, H, 0)


def embed(P0, expanded):
    out = np.zeros((expanded[1], expanded[0]), dtype=P0.dtype)
    out[:P0.shape[0], :P0.shape[1]] = P0
    return out


def solve_complex(P0, expanded, spacing, k, alpha, z0, dz, nz, restrict=True):
    """complex FFT form on the expanded grid: [nz][Ey][Ex] complex128"""
    X = np.fft.fft2(embed(np.asarray(P0, dtype=np.complex128), expanded))
    return np.stack([np.fft.ifft2(X * H_exact(expanded, spacing, k, alpha, z, restrict)) for z in planes(z0, dz, nz)])


def solve_pair(Pr, Pi, expanded, spacing, k, alpha, z0, dz, nz, restrict=True):
    """real-transform form: two rfft2, the 2x2 mix per plane, two irfft2 -> (Re P, Im P) on the expanded grid"""
    Er, Ei = embed(np.asarray(Pr, dtype=np.float64), expanded), embed(np.asarray(Pi, dtype=np.float64), expanded)
    Xr, Xi = np.fft.rfft2(Er), np.fft.rfft2(Ei)
    outr, outi = [], []
    for z in planes(z0, dz, nz):
        H = H_exact(expanded, spacing, k, alpha, z, restrict, half=True)
        outr.append(np.fft.irfft2(H.real * Xr - H.imag * Xi, s=Er.shape))
        outi.append(np.fft.irfft2(H.imag * Xr + H.real * Xi, s=Er.shape))
    return np.stack(outr), np.stack(outi)


def project(P0, spacing, k, alpha, z0, dz, nz, expanded, restrict=True):
    """P on the domain, [nz][ny][nx] complex128, for the complex plane P0 [ny][nx]"""
    P0 = np.asarray(P0, dtype=np.complex128)
    Pr, Pi = solve_pair(P0.real, P0.imag, expanded, spacing, k, alpha, z0, dz, nz, restrict)
    ny, nx = P0.shape
    return (Pr + 1j * Pi)[:, :ny, :nx]


def restriction_margin(expanded, spacing, k, z0, dz, nz, half=True):
    """smallest relative distance |kr - kc(z_j)| / k of any bin's kr from any plane's cut-off"""
    kr = np.sqrt(radial(expanded, spacing, half))
    kc = cutoff(expanded, spacing, k, planes(z0, dz, nz))
    return float(np.min(np.abs(kr[..., None] - kc)) / k)


# ---- the exact field of a Gaussian-apodised aperture of point sources ---------------------------------------------------
def gaussian_aperture(n, d, sigma_cells=3.0):
    """(x, y, w): the n x n grid points of a plane, centred, with weights exp(-r^2 / (2 sigma^2))"""
    c = (np.arange(n, dtype=np.float64) - (n - 1) / 2.0) * d
    x, y = np.meshgrid(c, c, indexing="xy")
    w = np.exp(-(x * x + y * y) / (2.0 * (sigma_cells * d) ** 2))
    return x, y, w


def aperture_field(n, d, k, z, sigma_cells=3.0):
    """sum_s w_s exp(-i k r) / (4 pi r) on the same n x n grid points at height z above the aperture, [y][x]"""
    x, y, w = gaussian_aperture(n, d, sigma_cells)
    xs, ys, ws = x.ravel(), y.ravel(), w.ravel()
    out = np.zeros((n, n), dtype=np.complex128)
    for iy in range(n):
        r = np.sqrt((x[iy][:, None] - xs[None, :]) ** 2 + (y[iy][:, None] - ys[None, :]) ** 2 + z * z)
        out[iy] = (ws[None, :] * np.exp(-1j * k * r) / (4.0 * np.pi * r)).sum(axis=1)
    return out


def plan(dims, fused=True, lengths=None):
    """default expanded sides: the smallest fast-path length >= 2 N per axis; off the fast path the smallest even number"""
    from cw_reference import fast_lengths
    lengths = fast_lengths() if lengths is None else lengths
    least = tuple(2 * int(n) for n in dims)
    if fused and all(v <= lengths[-1] for v in least):
        return tuple(min(length for length in lengths if length >= v) for v in least)
    return least


def chunk_planes(expanded, planes, budget=1 << 30):
    """default plane-chunk size: the smallest of 16, 32, 48, 64 that holds all the planes (64 beyond that), reduced while
    16 B per expanded point and plane exceed 1 GiB; floor 16"""
    for zc in (64, 48, 32):
        if planes > zc - 16 and 16 * expanded[0] * expanded[1] * zc <= budget:
            return zc
    return 16


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
