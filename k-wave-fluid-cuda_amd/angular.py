"""Angular-spectrum CW projector front-end (include/kwave_host.h "Angular-spectrum CW projector" -> lib/libkwave_host.so).

`AngularSpectrum` carries a complex pressure plane — a measured hologram, or the plane just in front of a simulated
array — to a stack of parallel planes z_j = z0 + j dz in a homogeneous medium that may absorb, what k-Wave's
angularSpectrumCW computes: one 2-D FFT of the plane, then one multiply and one inverse 2-D FFT per output plane, in
chunks of planes.  Next to `cw.FieldPropagator` (a volume source, lossless) it is the acoustic link of the planning chain
for plane sources and absorbing media; `heat()` is the `Q` of `thermal.ThermalSolver`.  No CPU fallback: a missing library
or device raises.

Not built: heterogeneous media, reverse projection (z < 0), non-uniform plane spacing, the time-domain angularSpectrum,
2-D (line -> plane), Z-slabs, HDF5 files and the command line, graphs.
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
