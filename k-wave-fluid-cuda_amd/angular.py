"""Angular-spectrum CW projector front-end (include/kwave_host.h "Angular-spectrum CW projector" -> lib/libkwave_host.so).

`AngularSpectrum` carries a complex pressure plane — a measured hologram, or the plane just in front of a simulated
array — to a stack of parallel planes z_j = z0 + j dz in a homogeneous medium that may absorb, what k-Wave's
angularSpectrumCW computes: one 2-D FFT of the plane, then one multiply and one inverse 2-D FFT per output plane, in
chunks of planes.  Next to `cw.FieldPropagator` (a volume source, lossless) it is the acoustic link of the planning chain
for plane sources and absorbing media; `heat()` is the `Q` of `thermal.ThermalSolver`.  No CPU fallback: a missing library
or device raises.

`AngularSpectrumTime` does the same for a time-varying plane p(x, y, t) — a pulsed hydrophone scan, a `--p_raw` cuboid of
a time-loop run, a nonlinear waveform — what k-Wave's angularSpectrum computes: one 3-D FFT of the record over (t, y, x),
then per output plane one multiply by H(kx, ky, w; z) and one inverse transform, giving the peak positive and peak
negative pressure of every plane and, on request, the record of one.

Not built: heterogeneous media, reverse projection (z < 0), non-uniform plane spacing of the CW projector,
2-D (line -> plane), Z-slabs, HDF5 files and the command line, graphs.  Time domain: dispersion, several output planes per
z-pass, the x- and y-inverse restricted to the crop, band limits other than DC / Nyquist.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Tuple

import numpy as np

from .solver import Options, _check, load_host

_bound = False
NEPER_PER_DB = math.log(10.0) / 20.0


class Config(C.Structure):
    """struct kwh_angular_config"""
    _fields_ = [("nx", C.c_uint64), ("ny", C.c_uint64), ("dx", C.c_double), ("dy", C.c_double),
                ("c0", C.c_double), ("f0", C.c_double), ("z0", C.c_double), ("dz", C.c_double),
                ("planes", C.c_uint64), ("alpha_np", C.c_double), ("ex", C.c_uint64), ("ey", C.c_uint64),
                ("chunk_planes", C.c_uint64), ("angular_restriction", C.c_int32), ("pad_", C.c_int32)]


class TimeConfig(C.Structure):
    """struct kwh_angular_time_config"""
    _fields_ = [("nx", C.c_uint64), ("ny", C.c_uint64), ("nt", C.c_uint64), ("dx", C.c_double), ("dy", C.c_double),
                ("dt", C.c_double), ("c0", C.c_double), ("alpha_coeff", C.c_double), ("alpha_power", C.c_double),
                ("ex", C.c_uint64), ("ey", C.c_uint64), ("lt", C.c_uint64), ("n_planes", C.c_uint64),
                ("z", C.POINTER(C.c_double)), ("angular_restriction", C.c_int32), ("retarded_time", C.c_int32)]


def alpha_np(alpha_coeff_db_mhz_cm: float, alpha_power: float, f0: float) -> float:
    """absorption in Np/m at f0 [Hz] of the power law alpha_coeff [dB / (MHz^y cm)] f^y"""
    return float(alpha_coeff_db_mhz_cm) * (float(f0) * 1e-6) ** float(alpha_power) * 100.0 * NEPER_PER_DB


def _lib() -> C.CDLL:
    global _bound
    L = load_host()
    if not _bound:
        L.kwh_angular_plan.argtypes = [C.POINTER(Config), C.POINTER(Options), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_int32)]
        L.kwh_angular_create.argtypes = [C.POINTER(Config), C.POINTER(Options), C.POINTER(C.c_void_p)]
        L.kwh_angular_destroy.argtypes = [C.c_void_p]
        L.kwh_angular_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.kwh_angular_get.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
        L.kwh_angular_heat.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_uint64]
        L.kwh_angular_project.argtypes = [C.c_void_p]
        L.kwh_angular_get_scalar.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        L.kwh_angular_context.restype = C.c_void_p
        L.kwh_angular_context.argtypes = [C.c_void_p]
        L.kwh_angular_time_plan.argtypes = [C.POINTER(TimeConfig), C.POINTER(Options), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
        L.kwh_angular_time_create.argtypes = [C.POINTER(TimeConfig), C.POINTER(Options), C.POINTER(C.c_void_p)]
        L.kwh_angular_time_destroy.argtypes = [C.c_void_p]
        L.kwh_angular_time_set_input.argtypes = [C.c_void_p, C.c_void_p]
        L.kwh_angular_time_run.argtypes = [C.c_void_p, C.c_void_p]
        L.kwh_angular_time_get.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
        L.kwh_angular_time_series.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        L.kwh_angular_time_project.argtypes = [C.c_void_p]
        L.kwh_angular_time_get_scalar.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        L.kwh_angular_time_context.restype = C.c_void_p
        L.kwh_angular_time_context.argtypes = [C.c_void_p]
        _bound = True
    return L


def _config(dims, spacing, c0, f0, z0, dz, planes, alpha, angular_restriction, expanded, chunk_planes) -> Config:
    dims = tuple(int(v) for v in dims)
    spacing = tuple(float(v) for v in spacing)
    if len(dims) != 2 or len(spacing) != 2:
        raise ValueError("dims = (Nx, Ny) and spacing = (dx, dy)")
    if min(dims) < 0 or int(planes) < 0:
        raise ValueError(f"dims and planes must not be negative, got {dims}, {planes}")
    c = Config()
    c.nx, c.ny = dims
    c.dx, c.dy = spacing
    c.c0, c.f0, c.z0, c.dz = float(c0), float(f0), float(z0), float(dz)
    c.planes = int(planes)
    c.alpha_np = float(alpha)
    c.angular_restriction = int(bool(angular_restriction))
    if expanded is not None:
        expanded = tuple(int(v) for v in expanded)
        if len(expanded) != 2 or min(expanded) < 0:
            raise ValueError("expanded = (Ex, Ey)")
        c.ex, c.ey = expanded
    if chunk_planes is not None:
        if int(chunk_planes) <= 0:
            raise ValueError(f"chunk_planes must be positive, got {chunk_planes}")
        c.chunk_planes = int(chunk_planes)
    return c


def plan(dims, spacing, c0, f0, z0, dz, planes, alpha_np=0.0, angular_restriction=True, expanded=None, chunk_planes=None,
         fused_kernels=True) -> Tuple[Tuple[int, int], int, bool]:
    """((Ex, Ey), chunk_planes, fast path) of a projection, validated as AngularSpectrum would, without a device"""
    L = _lib()
    c = _config(dims, spacing, c0, f0, z0, dz, planes, alpha_np, angular_restriction, expanded, chunk_planes)
    o = Options()
    o.fused_kernels = int(bool(fused_kernels))
    e, zc, fast = (C.c_uint64 * 2)(), C.c_uint64(), C.c_int32()
    _check(L.kwh_angular_plan(C.byref(c), C.byref(o), e, C.byref(zc), C.byref(fast)))
    return (int(e[0]), int(e[1])), int(zc.value), bool(fast.value)


class AngularSpectrum:
    """Projection of an Nx x Ny pressure plane (arrays are (Ny, Nx), x fastest) to `planes` planes z0 + j dz; results are
    (Nz, Ny, Nx).

    dims = (Nx, Ny), spacing = (dx, dy) [m], c0 [m/s], f0 [Hz], z0 >= 0 and dz > 0 [m], planes <= 4096.  alpha_np: absorption
    [Np/m] at f0 (`alpha_np()` converts a power law).  angular_restriction: drop the components that would wrap around the
    expanded grid by plane z.  expanded = (Ex, Ey): default the smallest fast-path sides >= 2 N (2 N on rocFFT with
    fused_kernels=False).  chunk_planes: planes computed per launch; default the smallest of 16, 32, 48,
    64 that holds them all, 64 beyond that (memory: about 20 bytes per expanded point and plane of the chunk)."""

    def __init__(self, dims, spacing, c0, f0, z0, dz, planes, alpha_np=0.0, angular_restriction=True, expanded=None,
                 chunk_planes=None, fused_kernels=True, device_idx=-1):
        L = _lib()
        c = _config(dims, spacing, c0, f0, z0, dz, planes, alpha_np, angular_restriction, expanded, chunk_planes)
        o = Options()
        o.device_idx = int(device_idx)
        o.fused_kernels = int(bool(fused_kernels))
        self.L, self._h = L, None
        h = C.c_void_p()
        _check(L.kwh_angular_create(C.byref(c), C.byref(o), C.byref(h)))
        self._h = h
        self.nx, self.ny, self.nz = int(c.nx), int(c.ny), int(c.planes)
        self.spacing = (float(c.dx), float(c.dy))
        self.c0, self.f0, self.z0, self.dz = float(c.c0), float(c.f0), float(c.z0), float(c.dz)

    def _scalar(self, name: str) -> float:
        v = C.c_double()
        _check(self.L.kwh_angular_get_scalar(self._h, name.encode(), C.byref(v)))
        return float(v.value)

    @property
    def shape(self):
        return (self.nz, self.ny, self.nx)

    @property
    def expanded(self) -> Tuple[int, int]:
        return tuple(int(self._scalar(n)) for n in ("Ex", "Ey"))

    @property
    def chunk_planes(self) -> int:
        return int(self._scalar("chunk_planes"))

    @property
    def fused(self) -> bool:
        return self._scalar("fused_pipeline") != 0.0

    @property
    def runs(self) -> int:
        return int(self._scalar("runs"))

    @property
    def ctx(self):
        return C.c_void_p(self.L.kwh_angular_context(self._h))

    def _plane(self, v) -> np.ndarray:
        a = np.asarray(v, dtype=np.float32)
        if a.shape != (self.ny, self.nx):
            a = np.broadcast_to(a, (self.ny, self.nx))
        return np.ascontiguousarray(a)

    def _get(self, name: str) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float32)
        _check(self.L.kwh_angular_get(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def _result(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.complex64)
        out.real = self._get("re")
        out.imag = self._get("im")
        return out

    def run(self, amp, phase) -> np.ndarray:
        """P for the plane amp * exp(i phase) (phase in radians): complex64 (Nz, Ny, Nx)"""
        a, b = self._plane(amp), self._plane(phase)
        _check(self.L.kwh_angular_run(self._h, a.ctypes.data, b.ctypes.data, 0))
        return self._result()

    def run_parts(self, re, im) -> np.ndarray:
        """P for the plane re + i im"""
        a, b = self._plane(re), self._plane(im)
        _check(self.L.kwh_angular_run(self._h, a.ctypes.data, b.ctypes.data, 1))
        return self._result()

    def amplitude(self) -> np.ndarray:
        """|P| of the last run, float32"""
        return self._get("amplitude")

    def phase(self) -> np.ndarray:
        """arg P of the last run [rad], float32"""
        return self._get("phase")

    def heat(self, alpha_np, rho0) -> np.ndarray:
        """Plane-wave volume rate of heat deposition Q = alpha |P|^2 / (rho0 c0) [W/m^3] of the last run: alpha_np [Np/m]
        and rho0 [kg/m^3] scalars or (Nz, Ny, Nx) arrays.  The `Q` of thermal.ThermalSolver."""
        q = np.asarray(alpha_np, dtype=np.float64) / (np.asarray(rho0, dtype=np.float64) * self.c0)
        out = np.empty(self.shape, dtype=np.float32)
        if q.ndim == 0:
            _check(self.L.kwh_angular_heat(self._h, None, float(q), out.ctypes.data, out.size))
        else:
            qa = np.ascontiguousarray(np.broadcast_to(np.asarray(q, dtype=np.float32), self.shape))
            _check(self.L.kwh_angular_heat(self._h, qa.ctypes.data, 0.0, out.ctypes.data, out.size))
        return out

    def project(self):
        """the chunks alone, from the source spectra as they stand (timing)"""
        _check(self.L.kwh_angular_project(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self.L.kwh_angular_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _time_config(dims, spacing, dt, nt, c0, z, alpha_coeff, alpha_power, angular_restriction, retarded_time, expanded,
                 time_length):
    """(TimeConfig, the z array it points to)"""
    dims = tuple(int(v) for v in dims)
    spacing = tuple(float(v) for v in spacing)
    if len(dims) != 2 or len(spacing) != 2:
        raise ValueError("dims = (Nx, Ny) and spacing = (dx, dy)")
    if min(dims) < 0 or int(nt) < 0:
        raise ValueError(f"dims and nt must not be negative, got {dims}, {nt}")
    za = np.ascontiguousarray(np.atleast_1d(np.asarray(z, dtype=np.float64)).reshape(-1))
    c = TimeConfig()
    c.nx, c.ny = dims
    c.nt = int(nt)
    c.dx, c.dy = spacing
    c.dt, c.c0 = float(dt), float(c0)
    c.alpha_coeff, c.alpha_power = float(alpha_coeff), float(alpha_power)
    c.angular_restriction = int(bool(angular_restriction))
    c.retarded_time = int(bool(retarded_time))
    c.n_planes = int(za.size)
    c.z = za.ctypes.data_as(C.POINTER(C.c_double)) if za.size else None
    if expanded is not None:
        expanded = tuple(int(v) for v in expanded)
        if len(expanded) != 2 or min(expanded) < 0:
            raise ValueError("expanded = (Ex, Ey)")
        c.ex, c.ey = expanded
    if time_length is not None:
        if int(time_length) <= 0:
            raise ValueError(f"time_length must be positive, got {time_length}")
        c.lt = int(time_length)
    return c, za


def plan_time(dims, spacing, dt, nt, c0, z, alpha_coeff=0.0, alpha_power=1.5, angular_restriction=True, retarded_time=False,
              expanded=None, time_length=None, fused_kernels=True) -> Tuple[Tuple[int, int], int, bool]:
    """((Ex, Ey), Lt, fast path) of a time-domain projection, validated as AngularSpectrumTime would, without a device"""
    L = _lib()
    c, _z = _time_config(dims, spacing, dt, nt, c0, z, alpha_coeff, alpha_power, angular_restriction, retarded_time, expanded,
                         time_length)
    o = Options()
    o.fused_kernels = int(bool(fused_kernels))
    e, fast = (C.c_uint64 * 3)(), C.c_int32()
    _check(L.kwh_angular_time_plan(C.byref(c), C.byref(o), e, C.byref(fast)))
    return (int(e[0]), int(e[1])), int(e[2]), bool(fast.value)


class AngularSpectrumTime:
    """Projection of a pressure record p0 (Nt, Ny, Nx) (x fastest) on a plane to the parallel planes at the distances z [m]
    (a scalar or a sequence, each >= 0, at most 4096): `run(p0)` gives the peak positive pressure (Nz, Ny, Nx), `p_min()` the
    peak negative one, `series(j)` the record (Nt, Ny, Nx) of plane j.

    dims = (Nx, Ny), spacing = (dx, dy) [m], dt [s], nt = Nt, c0 [m/s].  alpha_coeff [dB / (MHz^y cm)] and alpha_power: power-law
    absorption without dispersion.  angular_restriction: drop the components that would wrap around the expanded grid by
    plane z.  retarded_time: plane z is reported at the times t_n + z / c0, so that a pulse stays inside the record.
    expanded = (Ex, Ey): default the smallest fast-path sides >= 2 N.  time_length = Lt: the zero-padded record length,
    default the smallest fast-path length >= Nt (even, >= Nt when given).  The temporal mean of the record is dropped.
    Memory: about 36 bytes per point of Ex Ey Lt on the fast path."""

    def __init__(self, dims, spacing, dt, nt, c0, z, alpha_coeff=0.0, alpha_power=1.5, angular_restriction=True,
                 retarded_time=False, expanded=None, time_length=None, fused_kernels=True, device_idx=-1):
        L = _lib()
        c, za = _time_config(dims, spacing, dt, nt, c0, z, alpha_coeff, alpha_power, angular_restriction, retarded_time,
                             expanded, time_length)
        o = Options()
        o.device_idx = int(device_idx)
        o.fused_kernels = int(bool(fused_kernels))
        self.L, self._h = L, None
        h = C.c_void_p()
        _check(L.kwh_angular_time_create(C.byref(c), C.byref(o), C.byref(h)))
        self._h = h
        self.nx, self.ny, self.nt, self.nz = int(c.nx), int(c.ny), int(c.nt), int(za.size)
        self.spacing = (float(c.dx), float(c.dy))
        self.dt, self.c0 = float(c.dt), float(c.c0)
        self.z = za.copy()

    def _scalar(self, name: str) -> float:
        v = C.c_double()
        _check(self.L.kwh_angular_time_get_scalar(self._h, name.encode(), C.byref(v)))
        return float(v.value)

    @property
    def shape(self):
        return (self.nz, self.ny, self.nx)

    @property
    def expanded(self) -> Tuple[int, int]:
        return tuple(int(self._scalar(n)) for n in ("Ex", "Ey"))

    @property
    def time_length(self) -> int:
        return int(self._scalar("Lt"))

    @property
    def fused(self) -> bool:
        return self._scalar("fused_pipeline") != 0.0

    @property
    def runs(self) -> int:
        return int(self._scalar("runs"))

    @property
    def ctx(self):
        return C.c_void_p(self.L.kwh_angular_time_context(self._h))

    def _record(self, p0) -> np.ndarray:
        a = np.asarray(p0, dtype=np.float32)
        if a.shape != (self.nt, self.ny, self.nx):
            raise ValueError(f"p0 must be (Nt, Ny, Nx) = {(self.nt, self.ny, self.nx)}, got {a.shape}")
        return np.ascontiguousarray(a)

    def _get(self, name: str) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float32)
        _check(self.L.kwh_angular_time_get(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def set_input(self, p0):
        """embed, transform and keep the record (run() does this itself)"""
        a = self._record(p0)
        _check(self.L.kwh_angular_time_set_input(self._h, a.ctypes.data))

    def run(self, p0) -> np.ndarray:
        """max_t p on every plane for the record p0: float32 (Nz, Ny, Nx)"""
        a = self._record(p0)
        _check(self.L.kwh_angular_time_run(self._h, a.ctypes.data))
        return self._get("p_max")

    def p_max(self) -> np.ndarray:
        """max_t p of the last run"""
        return self._get("p_max")

    def p_min(self) -> np.ndarray:
        """min_t p of the last run"""
        return self._get("p_min")

    def series(self, j: int) -> np.ndarray:
        """the record of plane j, recomputed from the kept spectrum: float32 (Nt, Ny, Nx)"""
        out = np.empty((self.nt, self.ny, self.nx), dtype=np.float32)
        _check(self.L.kwh_angular_time_series(self._h, int(j), out.ctypes.data, out.size))
        return out

    def project(self):
        """the planes alone, from the kept spectrum as it stands (timing)"""
        _check(self.L.kwh_angular_time_project(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self.L.kwh_angular_time_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
