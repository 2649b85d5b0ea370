"""The bioheat scheme of DESIGN.md ("Bioheat") restated in NumPy (a plain module, imported by name from tests/): the fp64
reference of tests/test_gpu_thermal.py, the subject of the closed-form tests in tests/test_thermal_host.py, and — with
dtype=np.float32 — a float32 twin that shows how far fp32 arithmetic alone moves a case from the fp64 result.

    a = 1 / (rho C),  P = rho_b C_b W_b a,  D = K a,  D_ref = max D (or diffusion_coeff_ref)
    kappa_d(k) = (1 - exp(-D_ref |k|^2 dt)) / (D_ref |k|^2 dt),  kappa_d(0) = 1
    Laplacian form (scalar K):  term = K a F^-1{ -|k|^2 kappa_d F{T} }
    flux form (array K):        F_i = K_sg_i F^-1{ kappa_d i k_i e^{+i k_i d_i / 2} F{T} },
                                term = a sum_i F^-1{ i k_i e^{-i k_i d_i / 2} F{F_i} }
    T <- T + dt (term - P (T - T_a) + heat_on a Q);   cem43 += (dt / 60) R^(43 - T) on the new T,
    R = 0.5 for T >= 43, 0.25 for 37 <= T < 43, nothing below 37;   T_max = max(T_max, T)

The datasets are taken as the float32 numbers the solver gets; everything derived from them is computed in float64 and,
for the twin, rounded to float32 once, as the host layer does.  Arrays are (Nz, Ny, Nx).  The module also builds the
problems the CPU and the GPU tests share."""
import math

import numpy as np

F32, U64 = np.float32, np.uint64


def kvec(n, d):
    """k-Wave's wavenumber vector in FFT order (the Nyquist bin of an even axis is negative)"""
    j = np.arange(n)
    return 2.0 * math.pi / (n * d) * np.where(j < (n + 1) // 2, j, j - n)


def _f64(pr, name):
    return np.asarray(pr[name], dtype=F32).astype(np.float64)


def _scalar(pr, name):
    return float(np.asarray(pr[name], dtype=F32).ravel()[0])


def staggered(K, axis):
    """mean of each point and its +1 neighbour along `axis`; the last point keeps its own value"""
    nxt = np.roll(K, -1, axis=axis)
    last = [slice(None)] * 3
    last[axis] = -1
    nxt[tuple(last)] = K[tuple(last)]
    return 0.5 * (K + nxt)


def operators(shape, spacing, dt, d_ref):
    """(kappa_d, -|k|^2 kappa_d) on the reduced grid (Nz, Ny, Nx / 2 + 1) in float64"""
    nz, ny, nx = shape
    dz, dy, dx = spacing
    kx, ky, kz = kvec(nx, dx)[:nx // 2 + 1], kvec(ny, dy), kvec(nz, dz)
    k2 = kz[:, None, None] ** 2 + ky[None, :, None] ** 2 + kx[None, None, :] ** 2
    e = d_ref * k2 * dt
    with np.errstate(invalid="ignore", divide="ignore"):
        kd = np.where(e == 0.0, 1.0, -np.expm1(-e) / np.where(e == 0.0, 1.0, e))
    return kd, -k2 * kd


class Reference:
    def __init__(self, pr, dtype=np.float64):
        self.dtype = dtype
        nx, ny, nz = (int(np.asarray(pr[k]).ravel()[0]) for k in ("Nx", "Ny", "Nz"))
        self.shape = (nz, ny, nx)
        self.spacing = tuple(_scalar(pr, k) for k in ("dz", "dy", "dx"))
        self.dt = _scalar(pr, "dt")
        full = lambda v: np.broadcast_to(v, self.shape).copy()  # noqa: E731
        K = _f64(pr, "thermal_conductivity")
        a = 1.0 / (_f64(pr, "density") * _f64(pr, "specific_heat"))
        if "perfusion_coeff" in pr:
            P = _f64(pr, "perfusion_coeff")
        elif "blood_perfusion_rate" in pr:
            P = _f64(pr, "blood_density") * _f64(pr, "blood_specific_heat") * _f64(pr, "blood_perfusion_rate") * a
        else:
            P = np.zeros(1)
        Ta = _f64(pr, "blood_ambient_temperature") if "blood_ambient_temperature" in pr else np.zeros(1)
        self.flux = K.size > 1
        self.d_ref = _scalar(pr, "diffusion_coeff_ref") if "diffusion_coeff_ref" in pr else float(np.max(K * a))
        kd, lap = operators(self.shape, self.spacing, self.dt, self.d_ref)
        c = lambda v: np.asarray(v).astype(dtype)  # noqa: E731  (rounded once)
        self.a, self.P, self.Ta, self.K = c(a), c(P), c(Ta), c(K)
        self.kd, self.lap = c(kd), c(lap)
        if self.flux:
            K = full(K)
            sg = [_f64(pr, f"thermal_conductivity_sg{ax}") if f"thermal_conductivity_sg{ax}" in pr else None for ax in "zyx"]
            self.K_sg = [c(sg[i] if sg[i] is not None else staggered(K, i)) for i in range(3)]  # axes 0, 1, 2 = z, y, x
            ctype = np.complex64 if dtype == F32 else np.complex128
            self.pos, self.neg = [], []
            for axis, (n, d) in enumerate(zip(self.shape, self.spacing)):
                k = kvec(n, d)[:n // 2 + 1] if axis == 2 else kvec(n, d)
                bshape = [1, 1, 1]
                bshape[axis] = k.size
                self.pos.append((1j * k * np.exp(1j * k * d / 2)).astype(ctype).reshape(bshape))
                self.neg.append((1j * k * np.exp(-1j * k * d / 2)).astype(ctype).reshape(bshape))
        self.Q = c(full(_f64(pr, "Q"))) if "Q" in pr else None
        self.T = c(full(_f64(pr, "T0")))
        self.cem43 = np.zeros(self.shape, dtype=dtype)
        self.T_max = self.T.copy()
        self.t = 0

    def _fwd(self, v):
        s = np.fft.rfftn(v, axes=(0, 1, 2))
        if self.dtype == F32:
            assert s.dtype == np.complex64, "the float32 twin needs single-precision FFTs"
        return s

    def _inv(self, s):
        return np.fft.irfftn(s, s=self.shape, axes=(0, 1, 2)).astype(self.dtype, copy=False)

    def diffusion_term(self):
        if not self.flux:
            return self.K * self.a * self._inv(self.lap * self._fwd(self.T))
        S = self.kd * self._fwd(self.T)
        div = None
        for i in range(3):
            flux = self.K_sg[i] * self._inv(self.pos[i] * S)
            term = self._inv(self.neg[i] * self._fwd(flux))
            div = term if div is None else div + term
        return self.a * div

    def step(self, heat_on=True):
        dt = self.dtype(self.dt)
        rate = self.diffusion_term() - self.P * (self.T - self.Ta)
        if heat_on and self.Q is not None:
            rate = rate + self.a * self.Q
        self.T = (self.T + dt * rate).astype(self.dtype)
        self.cem43 = (self.cem43 + dose_increment(self.T, self.dt, self.dtype)).astype(self.dtype)
        self.T_max = np.maximum(self.T_max, self.T)
        self.t += 1

    def run(self, n, heat_on=True):
        for _ in range(n):
            self.step(heat_on)
        return self


def dose_increment(T, dt, dtype=np.float64):
    """(dt / 60) R^(43 - T): R = 0.5 for T >= 43, 0.25 for 37 <= T < 43, nothing below 37"""
    T = np.asarray(T, dtype=dtype)
    s = np.where(T >= 43, 1.0, 2.0).astype(dtype)
    inc = dtype(dt) / dtype(60) * np.exp2(s * (T - dtype(43)))
    return np.where(T >= 37, inc, 0).astype(dtype)


# ---- the problems the tests share -------------------------------------------------------------------------------------
FUSED_GRID = (16, 32, 48)     # (Nx, Ny, Nz): every side a fast-path length of the hand-written FFT pipeline
ROCFFT_GRID = (24, 20, 18)    # none of them is
SPACING = (1.0e-3, 1.25e-3, 0.75e-3)  # dx, dy, dz: the sides of both grids then have three different lengths
K0, RHO0, C0 = 0.5, 1000.0, 3600.0  # soft tissue


def grid_datasets(dims, dt):
    nx, ny, nz = dims
    pr = {"Nx": np.array([[[nx]]], U64), "Ny": np.array([[[ny]]], U64), "Nz": np.array([[[nz]]], U64)}
    for name, v in zip(("dx", "dy", "dz"), SPACING):
        pr[name] = np.array([[[v]]], F32)
    pr["dt"] = np.array([[[dt]]], F32)
    return pr


def k2_max(dims):
    return sum((math.pi / d) ** 2 for d in SPACING)


def euler_limit(dims, diffusivity):
    """the largest stable step of explicit Euler without the k-space correction: 2 / (D k_max^2)"""
    return 2.0 / (diffusivity * k2_max(dims))


MODE = (1, 2, 1)  # periods along x, y, z; with the side lengths, a different wavenumber on every axis


def mode_problem(dims, flux, dt):
    """ambient 0, no perfusion, no source, T0 = one Fourier mode of amplitude 1; flux: the same K as a constant array"""
    nx, ny, nz = dims
    pr = grid_datasets(dims, dt)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pr["T0"] = np.cos(2 * math.pi * (MODE[0] * x / nx + MODE[1] * y / ny + MODE[2] * z / nz)).astype(F32)
    pr["thermal_conductivity"] = np.full((nz, ny, nx), K0, F32) if flux else np.array([[[K0]]], F32)
    pr["density"] = np.array([[[RHO0]]], F32)
    pr["specific_heat"] = np.array([[[C0]]], F32)
    return pr


def mode_decay(pr, n_steps):
    """the closed form of mode_problem after n steps: T0 exp(-D |k|^2 dt n), from the float32 datasets, in float64"""
    nx, ny, nz = (int(pr[k].ravel()[0]) for k in ("Nx", "Ny", "Nz"))
    k2 = sum((2 * math.pi * m / (n * _scalar(pr, d))) ** 2 for m, n, d in zip(MODE, (nx, ny, nz), ("dx", "dy", "dz")))
    D = float(_f64(pr, "thermal_conductivity").ravel()[0]) / (_scalar(pr, "density") * _scalar(pr, "specific_heat"))
    return pr["T0"].astype(np.float64) * math.exp(-D * k2 * _scalar(pr, "dt") * n_steps)


def _bump(dims, centre, width):
    """a smooth periodic bump of height 1 at `centre` (fractions of the sides): exp(-sum sin^2(pi (r - c)) / w^2)"""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
    s = sum(np.sin(math.pi * (r - c)) ** 2 for r, c in zip((x, y, z), centre))
    return np.exp(-s / width ** 2)


HET_CONTRAST = 3.0
HET_STEPS = 10


def heterogeneous_problem(dims):
    """K, rho, C in three smooth-edged regions (the background and two bumps) with contrast HET_CONTRAST each, array
    perfusion, a Gaussian Q, a smooth T0 of order 1 about ambient 0; dt with D_max k_max^2 dt = 0.5"""
    up, down = math.sqrt(HET_CONTRAST) - 1.0, 1.0 - 1.0 / math.sqrt(HET_CONTRAST)
    b1, b2 = _bump(dims, (0.3, 0.35, 0.4), 0.55), _bump(dims, (0.7, 0.6, 0.75), 0.5)
    K = K0 * (1 + up * b1) * (1 - down * b2)
    rho = RHO0 * (1 - down * b1) * (1 + up * b2)
    C = C0 * (1 + up * b2) * (1 - down * _bump(dims, (0.5, 0.1, 0.2), 0.6))
    K, rho, C = K.astype(F32), rho.astype(F32), C.astype(F32)
    d_max = float(np.max(K.astype(np.float64) / (rho.astype(np.float64) * C.astype(np.float64))))
    pr = grid_datasets(dims, 0.5 / (d_max * k2_max(dims)))
    pr.update({"thermal_conductivity": K, "density": rho, "specific_heat": C})
    pr["blood_density"] = np.array([[[1060.0]]], F32)
    pr["blood_specific_heat"] = np.array([[[3600.0]]], F32)
    pr["blood_perfusion_rate"] = (0.01 * (1 + b1 - 0.5 * b2)).astype(F32)
    pr["blood_ambient_temperature"] = np.array([[[0.0]]], F32)
    pr["Q"] = (2.0e6 * _bump(dims, (0.5, 0.5, 0.5), 0.4)).astype(F32)
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
    pr["T0"] = (np.cos(2 * math.pi * x) * np.sin(2 * math.pi * (y + z)) + 0.5 * np.cos(4 * math.pi * y) * b2).astype(F32)
    return pr


HEAT_STEPS = 10  # heating, then as many cooling


def heating_problem(dims):
    """T0 = T_a = 37 in a homogeneous perfused medium (scalar K: the Laplacian form), a Gaussian Q that takes the focus past
    43 degC within HEAT_STEPS steps of 0.2 s"""
    pr = grid_datasets(dims, 0.2)
    for name, v in (("T0", 37.0), ("thermal_conductivity", K0), ("density", RHO0), ("specific_heat", C0),
                    ("blood_density", 1060.0), ("blood_specific_heat", 3600.0), ("blood_perfusion_rate", 0.01),
                    ("blood_ambient_temperature", 37.0)):
        pr[name] = np.array([[[v]]], F32)
    pr["Q"] = (2.0e7 * _bump(dims, (0.5, 0.5, 0.5), 0.35)).astype(F32)
    return pr


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
