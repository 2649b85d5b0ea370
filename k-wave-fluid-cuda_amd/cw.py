"""CW field propagator front-end (include/kwave_host.h "CW field propagator" -> lib/libkwave_host.so).

`FieldPropagator` gives the steady-state complex pressure amplitude of a continuous-wave source in a homogeneous lossless
medium from one forward and one inverse 3-D FFT on an expanded grid — what k-Wave's acousticFieldPropagator computes —
instead of a time loop run until steady.  It sits between the array builders (`arrays.offgrid_elements`) and the bioheat
solver (`thermal.ThermalSolver`, whose `Q` is `heat()`).  No CPU fallback: a missing library or device raises.

Not built: heterogeneous media, 2-D, Z-slabs, HDF5 files and the command line, graphs.  Absorbing media and sources given
as a pressure plane: `angular.AngularSpectrum`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import arrays
from .solver import Options, _check, load_host

_bound = False


class Config(C.Structure):
    """struct kwh_cw_config"""
    _fields_ = [("nx", C.c_uint64), ("ny", C.c_uint64), ("nz", C.c_uint64),
                ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double),
                ("c0", C.c_double), ("f0", C.c_double), ("t", C.c_double),
                ("ex", C.c_uint64), ("ey", C.c_uint64), ("ez", C.c_uint64),
                ("source_scale_re", C.c_double), ("source_scale_im", C.c_double),
                ("source_scale_kwave", C.c_int32), ("pad_", C.c_int32)]


def _lib() -> C.CDLL:
    global _bound
    L = load_host()
    if not _bound:
        L.kwh_cw_plan.argtypes = [C.POINTER(Config), C.POINTER(Options), C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_int32)]
        L.kwh_cw_create.argtypes = [C.POINTER(Config), C.POINTER(Options), C.POINTER(C.c_void_p)]
        L.kwh_cw_destroy.argtypes = [C.c_void_p]
        L.kwh_cw_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.kwh_cw_get.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
        L.kwh_cw_heat.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_uint64]
        L.kwh_cw_propagate.argtypes = [C.c_void_p]
        L.kwh_cw_get_scalar.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        L.kwh_cw_context.restype = C.c_void_p
        L.kwh_cw_context.argtypes = [C.c_void_p]
        _bound = True
    return L


def _config(dims, spacing, c0, f0, t, expanded, source_scale) -> Config:
    dims = tuple(int(v) for v in dims)
    spacing = tuple(float(v) for v in spacing)
    if len(dims) != 3 or len(spacing) != 3:
        raise ValueError("dims = (Nx, Ny, Nz) and spacing = (dx, dy, dz)")
    if min(dims) < 0:
        raise ValueError(f"dims must not be negative, got {dims}")
    c = Config()
    c.nx, c.ny, c.nz = dims
    c.dx, c.dy, c.dz = spacing
    c.c0, c.f0, c.t = float(c0), float(f0), 0.0 if t is None else float(t)
    if expanded is not None:
        expanded = tuple(int(v) for v in expanded)
        if len(expanded) != 3 or min(expanded) < 0:
            raise ValueError("expanded = (Ex, Ey, Ez)")
        c.ex, c.ey, c.ez = expanded
    if isinstance(source_scale, str):
        if source_scale != "kwave":
            raise ValueError(f'source_scale must be a number or "kwave", got {source_scale!r}')
        c.source_scale_kwave = 1
    else:
        s = complex(source_scale)
        if s == 0:
            raise ValueError("source_scale must not be 0")
        if s != 1:
            c.source_scale_re, c.source_scale_im = s.real, s.imag
    return c


def plan(dims, spacing, c0, f0, t=None, expanded=None, fused_kernels=True, source_scale=1) -> Tuple[float, Tuple[int, int, int], bool]:
    """(T, (Ex, Ey, Ez), fast path) of a propagation, validated as FieldPropagator would, without a device"""
    L = _lib()
    c = _config(dims, spacing, c0, f0, t, expanded, source_scale)
    o = Options()
    o.fused_kernels = int(bool(fused_kernels))
    tt, e, fast = C.c_double(), (C.c_uint64 * 3)(), C.c_int32()
    _check(L.kwh_cw_plan(C.byref(c), C.byref(o), C.byref(tt), e, C.byref(fast)))
    return float(tt.value), (int(e[0]), int(e[1]), int(e[2])), bool(fast.value)


class FieldPropagator:
    """Steady-state field of a CW source on an Nx x Ny x Nz domain (arrays are (Nz, Ny, Nx), x fastest).

    dims = (Nx, Ny, Nz), spacing = (dx, dy, dz) [m], c0 [m/s], f0 [Hz].  t: evaluation time [s], default the domain
    diagonal over c0.  expanded = (Ex, Ey, Ez): default the smallest fast-path sides that keep the periodic images out of
    the domain until t (even sides on rocFFT with fused_kernels=False).  source_scale: a complex factor on the source, or
    "kwave" for 2 i w c0 / dx, with which an amplitude p_s reproduces the time loop's additive pressure source
    p_s sin(w t)."""

    def __init__(self, dims, spacing, c0, f0, t=None, expanded=None, fused_kernels=True, source_scale=1, device_idx=-1):
        L = _lib()
        c = _config(dims, spacing, c0, f0, t, expanded, source_scale)
        o = Options()
        o.device_idx = int(device_idx)
        o.fused_kernels = int(bool(fused_kernels))
        self.L, self._h = L, None
        h = C.c_void_p()
        _check(L.kwh_cw_create(C.byref(c), C.byref(o), C.byref(h)))
        self._h = h
        self.nx, self.ny, self.nz = int(c.nx), int(c.ny), int(c.nz)
        self.spacing = (float(c.dx), float(c.dy), float(c.dz))
        self.c0, self.f0 = float(c.c0), float(c.f0)

    def _scalar(self, name: str) -> float:
        v = C.c_double()
        _check(self.L.kwh_cw_get_scalar(self._h, name.encode(), C.byref(v)))
        return float(v.value)

    @property
    def shape(self):
        return (self.nz, self.ny, self.nx)

    @property
    def expanded(self) -> Tuple[int, int, int]:
        return tuple(int(self._scalar(n)) for n in ("Ex", "Ey", "Ez"))

    @property
    def t(self) -> float:
        return self._scalar("t")

    @property
    def fused(self) -> bool:
        return self._scalar("fused_pipeline") != 0.0

    @property
    def runs(self) -> int:
        return int(self._scalar("runs"))

    @property
    def source_scale(self) -> complex:
        return complex(self._scalar("source_scale_re"), self._scalar("source_scale_im"))

    @property
    def ctx(self):
        return C.c_void_p(self.L.kwh_cw_context(self._h))

    def _field(self, v, what: str) -> np.ndarray:
        a = np.asarray(v, dtype=np.float32)
        if a.shape != self.shape:
            a = np.broadcast_to(a, self.shape)
        return np.ascontiguousarray(a)

    def _get(self, name: str) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float32)
        _check(self.L.kwh_cw_get(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def _result(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.complex64)
        out.real = self._get("re")
        out.imag = self._get("im")
        return out

    def run(self, amp, phase) -> np.ndarray:
        """P for the source amp * exp(i phase) (phase in radians): complex64 (Nz, Ny, Nx)"""
        a, b = self._field(amp, "amp"), self._field(phase, "phase")
        _check(self.L.kwh_cw_run(self._h, a.ctypes.data, b.ctypes.data, 0))
        return self._result()

    def run_parts(self, re, im) -> np.ndarray:
        """P for the source re + i im"""
        a, b = self._field(re, "re"), self._field(im, "im")
        _check(self.L.kwh_cw_run(self._h, a.ctypes.data, b.ctypes.data, 1))
        return self._result()

    def run_elements(self, elements: Sequence, amplitudes, phases) -> np.ndarray:
        """P for an array of weighted elements (arrays.offgrid_elements, or any [(grid indices, weights), ...] on this
        domain), element e driven with amplitudes[e] * exp(i phases[e]): the source is the elements' weights times the two
        rows Re and Im of the drive, expanded point by point as arrays.weighted_source / expand_source do."""
        amplitudes = np.asarray(amplitudes, dtype=np.float64).reshape(-1)
        phases = np.asarray(phases, dtype=np.float64).reshape(-1)
        if amplitudes.size != len(elements) or phases.size != len(elements):
            raise ValueError(f"{len(elements)} elements need as many amplitudes and phases")
        drive = np.stack([amplitudes * np.cos(phases), amplitudes * np.sin(phases)]).astype(np.float32)
        ds = arrays.weighted_source(elements, drive)
        rows = arrays.expand_source(ds).reshape(2, -1)
        index = ds["p_source_index"].reshape(-1).astype(np.int64) - 1
        n = self.nx * self.ny * self.nz
        if index.size and int(index.max()) >= n:
            raise ValueError(f"an element holds grid index {int(index.max())}, the domain has {n} points")
        re, im = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        re[index], im[index] = rows[0], rows[1]
        return self.run_parts(re.reshape(self.shape), im.reshape(self.shape))

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
            _check(self.L.kwh_cw_heat(self._h, None, float(q), out.ctypes.data, out.size))
        else:
            qa = self._field(q, "alpha_np / (rho0 c0)")
            _check(self.L.kwh_cw_heat(self._h, qa.ctypes.data, 0.0, out.ctypes.data, out.size))
        return out

    def propagate(self):
        """the FFT round trip alone on the expanded pair as it stands (timing)"""
        _check(self.L.kwh_cw_propagate(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self.L.kwh_cw_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
