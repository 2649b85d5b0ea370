"""float64 NumPy restatement of the time-domain angular-spectrum projector (DESIGN.md "Time-domain angular-spectrum
projector"), the checker of tests/test_angular_time_host.py and tests/test_gpu_angular_time.py.  A plain module, imported
by name from tests/.

A real pressure record p0[t][y][x] (spacing dx, dy, time step dt) on a plane is projected to a parallel plane at distance z
of a homogeneous medium (time factor exp(+i w t), outgoing exp(-i k r)):

    p(., ., .; z) = crop( irfftn( rfftn(p0 embedded in Lt x Ey x Ex) H(kx, ky, m; z) ) )               axes (t, y, x)
    m' = min(m, Lt - m),  w = 2 pi m' / (Lt dt),  k = w / c0,  kr^2 = kx^2 + ky^2,  q = |k^2 - kr^2|^(1/2)
    m = 0 and m = Lt/2:  H = 0
    kr^2 < k^2:  H0 = exp(-i q z) exp(-alpha(m') z k / q)
    kr^2 = k^2:  H0 = 1 (alpha(m') = 0), 0 (absorbing)
    kr^2 > k^2:  H0 = exp(-q z)
    retarded time:        H0 <- H0 exp(+i k z)
    angular restriction:  H0 = 0 where kr^2 > k^2 (D^2/2) / (D^2/2 + z^2),  D = min((Ex - 1) dx, (Ey - 1) dy)
    H = H0 for 0 < m < Lt/2, conj(H0) for m > Lt/2
    alpha(m') = a0 f^y [Np/m] from alpha_coeff [dB / (MHz^y cm)] and alpha_power, no dispersion

Bins are counted as angular_reference.wavenumbers counts them.  Arrays are [t][y][x]; `expanded`, `dims` and `spacing` are
(x, y) pairs as in kwave_amd.angular.
"""
import numpy as np

import angular_reference as ar

LOG2E = 1.0 / np.log(2.0)
NEPER_PER_DB = np.log(10.0) / 20.0
rel_l2 = ar.rel_l2


def time_bins(lt):
    """m' = min(m, Lt - m) as float64, [lt]"""
    m = np.arange(lt, dtype=np.float64)
    return np.where(m <= lt // 2, m, lt - m)


def alpha_bins(lt, dt, alpha_coeff, alpha_power):
    """alpha(m') [Np/m] at f = m' / (Lt dt), [lt]"""
    f = time_bins(lt) / (lt * dt)
    return float(alpha_coeff) * (f * 1e-6) ** float(alpha_power) * 100.0 * NEPER_PER_DB


def ak_table(lt, dt, c0, alpha_coeff, alpha_power):
    """alpha(m') k(m') log2(e) for m' = 0 ... Lt/2: the device's `ak`"""
    f = np.arange(lt // 2 + 1, dtype=np.float64) / (lt * dt)
    alpha = float(alpha_coeff) * (f * 1e-6) ** float(alpha_power) * 100.0 * NEPER_PER_DB
    return alpha * (2.0 * np.pi * f / c0) * LOG2E


def cfac(expanded, spacing, z):
    h = 0.5 * ar.aperture(expanded, spacing) ** 2
    return h / (h + z * z)


def H_time(expanded, lt, spacing, dt, c0, z, alpha_coeff=0.0, alpha_power=1.5, restrict=True, retarded=False, half=True):
    """H(kx, ky, m; z) straight from the definition, complex128 [lt][ey][ex // 2 + 1] (half) or [lt][ey][ex]"""
    assert lt % 2 == 0
    kr2 = ar.radial(expanded, spacing, half)[None, :, :]
    mp = time_bins(lt)
    k = (2.0 * np.pi * mp / (lt * dt) / c0)[:, None, None]
    alpha = alpha_bins(lt, dt, alpha_coeff, alpha_power)[:, None, None]
    k2 = k * k
    q = np.sqrt(np.abs(k2 - kr2))
    qs = np.where(q == 0.0, 1.0, q)
    H = np.where(kr2 < k2, np.exp(-1j * q * z) * np.exp(-alpha * z * k / qs), np.exp(-q * z) + 0j)
    H = np.where(kr2 == k2, np.where(alpha > 0.0, 0.0, 1.0), H)
    if retarded:
        H = H * np.exp(1j * k * z)
    if restrict:
        H = np.where(kr2 > k2 * cfac(expanded, spacing, z), 0.0, H)
    m = np.arange(lt)
    H = np.where((m > lt // 2)[:, None, None], np.conj(H), H)
    H[0] = 0.0
    H[lt // 2] = 0.0
    return H


def embed(p0, expanded, lt):
    p0 = np.asarray(p0)
    out = np.zeros((lt, expanded[1], expanded[0]), dtype=p0.dtype)
    out[:p0.shape[0], :p0.shape[1], :p0.shape[2]] = p0
    return out


def solve_expanded(p0, expanded, lt, spacing, dt, c0, z, **kw):
    """the real-transform form on the expanded grid: float64 [lt][ey][ex] for the record p0 (any shape up to the grid)"""
    vol = embed(np.asarray(p0, dtype=np.float64), expanded, lt)
    X = np.fft.rfftn(vol)
    return np.fft.irfftn(X * H_time(expanded, lt, spacing, dt, c0, z, half=True, **kw), s=vol.shape, axes=(0, 1, 2))


def solve_complex(p0, expanded, lt, spacing, dt, c0, z, **kw):
    """the same with full complex transforms: complex128 [lt][ey][ex] (its imaginary part is rounding)"""
    vol = embed(np.asarray(p0, dtype=np.float64), expanded, lt)
    return np.fft.ifftn(np.fft.fftn(vol) * H_time(expanded, lt, spacing, dt, c0, z, half=False, **kw))


def project(p0, expanded, lt, spacing, dt, c0, zs, **kw):
    """the records on the domain: float64 [nz][nt][ny][nx]"""
    p0 = np.asarray(p0, dtype=np.float64)
    nt, ny, nx = p0.shape
    X = np.fft.rfftn(embed(p0, expanded, lt))
    shape = (lt, expanded[1], expanded[0])
    return np.stack([np.fft.irfftn(X * H_time(expanded, lt, spacing, dt, c0, float(z), half=True, **kw), s=shape, axes=(0, 1, 2))[:nt, :ny, :nx]
                     for z in np.atleast_1d(zs)])


def margins(expanded, lt, spacing, dt, c0, zs):
    """(smallest |kr - kc(z)| / k over bins and planes, smallest |kr^2 - k^2| / k^2 over bins): how far the inputs keep
    every bin from H's two discontinuities (the restriction's cut-off; the circle kr = k of an absorbing medium).  Bins
    with k = 0 carry H = 0 and are left out."""
    kr2 = ar.radial(expanded, spacing, half=True)[None, :, :]
    k = (2.0 * np.pi * np.arange(1, lt // 2 + 1, dtype=np.float64) / (lt * dt) / c0)[:, None, None]
    kr = np.sqrt(kr2)
    first = min(float(np.min(np.abs(kr - k * np.sqrt(cfac(expanded, spacing, float(z)))) / k)) for z in np.atleast_1d(zs))
    second = float(np.min(np.abs(kr2 - k * k) / (k * k)))
    return first, second


# ---- float32 emulation of the device's steps (kwave_hip.h "Time-domain angular-spectrum projector") --------------------------
def H_device(expanded, lt, spacing, dt, c0, z, alpha_coeff=0.0, alpha_power=1.5, restrict=True, retarded=False):
    """H on the reduced bins [lt][ey][ex // 2 + 1] with the device's order: float64 up to the phase word and the
    restriction test, float32 from there (divider = 1); complex64"""
    f32 = np.float32
    kx, ky = ar.wavenumbers(expanded, spacing, half=True)
    kr2 = ((kx * kx) + (ky * ky))[None, :, :]
    mp = time_bins(lt)
    dk = 2.0 * np.pi / (lt * dt * c0)
    k = (dk * mp)[:, None, None]
    k2 = k * k
    q = np.sqrt(np.abs(k2 - kr2))
    prop, evan = kr2 < k2, kr2 > k2
    qp = np.where(evan, 0.0, q)
    t = (qp - (k if retarded else 0.0)) * z / (2.0 * np.pi)
    word = np.mod(np.rint((t - np.floor(t)) * 4294967296.0), 4294967296.0).astype(np.uint32)
    ang = word.view(np.int32).astype(f32) * f32(1.4629180792671596e-9)
    cs, sn = np.cos(ang.astype(np.float64)).astype(f32), np.sin(ang.astype(np.float64)).astype(f32)
    q32 = q.astype(f32)
    absorbing = alpha_coeff > 0.0
    ak = np.zeros(lt // 2 + 1)
    if absorbing:
        ak = ak_table(lt, dt, c0, alpha_coeff, alpha_power)
    akm = ak[mp.astype(np.int64)][:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        b_prop = (akm * z).astype(f32) / q32 if absorbing else np.zeros_like(q32)
    b = np.where(prop, b_prop, np.where(evan, q32 * f32(z * LOG2E), f32(0.0))).astype(f32)
    mag = np.exp2(-b.astype(np.float64)).astype(f32)
    dead = (mp == 0)[:, None, None] | (2 * mp == lt)[:, None, None] | (~prop & ~evan & (akm > 0.0))
    if restrict:
        dead = dead | (kr2 > k2 * cfac(expanded, spacing, z))
    mag = np.where(dead, f32(0.0), mag).astype(f32)
    hr, hi = (mag * cs).astype(f32), (-(mag * sn)).astype(f32)
    hi = np.where((np.arange(lt) > lt // 2)[:, None, None], -hi, hi)
    return hr.astype(np.complex64) + 1j * hi.astype(np.complex64)


# ---- the exact field of a pulsed, Gaussian-apodised aperture of point sources ---------------------------------------------
def tone_burst(t, f0, cycles=3.0):
    """Gaussian tone burst whose envelope is `cycles` periods wide at half its maximum, centred 3 sigma after t = 0, in
    sine phase (zero mean)"""
    sigma = cycles / (f0 * 2.0 * np.sqrt(2.0 * np.log(2.0)))
    t0 = 3.0 * sigma
    return np.exp(-((t - t0) ** 2) / (2.0 * sigma * sigma)) * np.sin(2.0 * np.pi * f0 * (t - t0))


def pulsed_aperture_field(n, d, c0, f0, z, t, sigma_cells=3.0, cycles=3.0):
    """sum_s w_s g(t - r_s / c0) / (4 pi r_s) on the n x n grid points at height z above the aperture at the times t:
    float64 [nt][y][x]"""
    x, y, w = ar.gaussian_aperture(n, d, sigma_cells)
    xs, ys, ws = x.ravel(), y.ravel(), w.ravel()
    t = np.asarray(t, dtype=np.float64)
    out = np.zeros((t.size, n, n), dtype=np.float64)
    for iy in range(n):
        r = np.sqrt((x[iy][:, None] - xs[None, :]) ** 2 + (y[iy][:, None] - ys[None, :]) ** 2 + z * z)  # [x][s]
        g = tone_burst(t[:, None, None] - r[None, :, :] / c0, f0, cycles)
        out[:, iy, :] = (ws[None, None, :] * g / (4.0 * np.pi * r[None, :, :])).sum(axis=2)
    return out


def aperture_case():
    """the pulsed-aperture check: a 24 x 24 plane at 5 points per wavelength, 4 dx above the aperture, dt = 0.3 dx / c0,
    Nt = 200 in Lt = 256, E = 48; returns a dict with the record p0, the distances and the exact records"""
    n, dx, c0 = 24, 1.0e-3, 1500.0
    f0 = c0 / (5.0 * dx)
    dt = 0.3 * dx / c0
    nt = 200
    t = np.arange(nt) * dt
    zs = np.array([3.0, 6.0, 9.0, 12.0]) * dx
    return dict(n=n, dx=dx, c0=c0, f0=f0, dt=dt, nt=nt, lt=256, expanded=(48, 48), zs=zs, z_plane=4 * dx, t=t,
                p0=pulsed_aperture_field(n, dx, c0, f0, 4 * dx, t))


def aperture_exact(case, z, retarded):
    """the exact record at distance z from the measured plane, at t_n (+ z / c0 in retarded time)"""
    t = case["t"] + (z / case["c0"] if retarded else 0.0)
    return pulsed_aperture_field(case["n"], case["dx"], case["c0"], case["f0"], case["z_plane"] + z, t)


# ---- the size rules --------------------------------------------------------------------------------------------------
def plan_time(dims, nt, fused=True, lengths=None):
    """((Ex, Ey), Lt, fast): sides by angular_reference.plan; Lt the smallest fast-path length >= Nt, or Nt rounded up to
    even when there is none or off the fused pipeline"""
    from cw_reference import fast_lengths
    lengths = fast_lengths() if lengths is None else lengths
    expanded = ar.plan(dims, fused, lengths)
    if fused and nt <= lengths[-1]:
        lt = min(length for length in lengths if length >= nt)
    else:
        lt = nt + nt % 2
    fast = fused and all(v in lengths for v in expanded + (lt,))
    return expanded, lt, fast
