"""Bioheat solver front-end (include/kwave_host.h "Bioheat solver" -> lib/libkwave_host.so).

`ThermalSolver` runs the C++ `ThermalSolver` (k-wave-fluid-cuda_amd/host/) on an MI355X: explicit k-space time stepping of
the Pennes equation on a periodic grid with the CEM43 thermal dose accumulated on the GPU — what k-Wave's kWaveDiffusion
computes.  `heat_source` turns the acoustic solver's Q_term / Q_term_c stream into its full-grid heat source `Q`.
No CPU fallback: a missing library or device raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np

from . import capi
from .solver import Dataset, Options, _check, load_host

_bound = False


def _lib() -> C.CDLL:
    global _bound
    L = load_host()
    if not _bound:
        L.kwh_thermal_create.argtypes = [C.POINTER(Dataset), C.c_size_t, C.POINTER(Options), C.POINTER(C.c_void_p)]
        L.kwh_thermal_destroy.argtypes = [C.c_void_p]
        L.kwh_thermal_run.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
        L.kwh_thermal_time_index.restype = C.c_uint64
        L.kwh_thermal_time_index.argtypes = [C.c_void_p]
        L.kwh_thermal_context.restype = C.c_void_p
        L.kwh_thermal_context.argtypes = [C.c_void_p]
        L.kwh_thermal_get_matrix.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
        L.kwh_thermal_set_matrix.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
        L.kwh_thermal_lesion_volume.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_double)]
        L.kwh_thermal_stream_read.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64)]
        L.kwh_thermal_get_scalar.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_float)]
        _bound = True
    return L


def heat_source(values, sensor_mask_index, shape) -> np.ndarray:
    """The full-grid heat source Q [W/m^3], float32 of `shape` = (Nz, Ny, Nx), from the Q_term / Q_term_c values of an
    acoustic run (HostSolver.stream("Q_term") or the dataset of an output file) and the 1-based sensor_mask_index they
    were sampled at; points outside the mask get 0."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3:
        raise ValueError(f"shape must be (Nz, Ny, Nx), got {shape}")
    n = shape[0] * shape[1] * shape[2]
    values = np.asarray(values, dtype=np.float32).reshape(-1)
    index = np.asarray(sensor_mask_index).reshape(-1)
    if index.size != values.size:
        raise ValueError(f"{values.size} values for {index.size} sensor points")
    index = index.astype(np.int64)
    if index.size and (index.min() < 1 or index.max() > n):
        raise ValueError(f"sensor_mask_index lies outside 1..{n}")
    if np.unique(index).size != index.size:
        raise ValueError("sensor_mask_index names a point twice")
    q = np.zeros(n, dtype=np.float32)
    q[index - 1] = values
    return q.reshape(shape)


class ThermalSolver:
    """One bioheat simulation on the GPU.  `pr`: dict of NumPy arrays keyed by the dataset names of kwh_thermal_create
    (arrays as (Nz, Ny, Nx)).  Options: device_idx, fused_kernels (default True), t_max (keep the running maximum)."""

    def __init__(self, pr: Dict[str, np.ndarray], **opts):
        L = _lib()
        self._keep = []
        sets = (Dataset * len(pr))()
        for i, (name, a) in enumerate(pr.items()):
            a = np.asarray(a)
            if a.dtype == np.uint64:
                arr, dt = np.ascontiguousarray(a, dtype=np.uint64), 1
            else:
                arr, dt = np.ascontiguousarray(a, dtype=np.float32), 0
            shp = list(arr.shape)[::-1]
            while len(shp) < 3:
                shp.append(1)
            if len(shp) > 3:
                raise ValueError(f"{name}: more than three dimensions")
            nm = name.encode()
            self._keep += [arr, nm]
            sets[i].name, sets[i].data, sets[i].dtype = nm, arr.ctypes.data, dt
            sets[i].nx, sets[i].ny, sets[i].nz = shp
        o = Options()
        o.device_idx = int(opts.pop("device_idx", -1))
        o.fused_kernels = int(opts.pop("fused_kernels", True))
        o.slab_ranks = int(opts.pop("slab_ranks", 1))
        t_max = bool(opts.pop("t_max", False))
        if opts:
            raise TypeError(f"unknown option {sorted(opts)[0]}")
        self.L, self._h = L, None
        h = C.c_void_p()
        _check(L.kwh_thermal_create(sets, len(pr), C.byref(o), C.byref(h)))
        self._h = h
        self.nx, self.ny, self.nz = (int(np.asarray(pr[k]).ravel()[0]) for k in ("Nx", "Ny", "Nz"))
        if t_max:
            self.set("T_max", self.T)

    def run(self, n_steps: int, heat_on: bool = True):
        _check(self.L.kwh_thermal_run(self._h, int(n_steps), int(bool(heat_on))))

    @property
    def t(self) -> int:
        return int(self.L.kwh_thermal_time_index(self._h))

    @property
    def ctx(self):
        return C.c_void_p(self.L.kwh_thermal_context(self._h))

    @property
    def fused(self) -> bool:
        v = C.c_float()
        _check(self.L.kwh_thermal_get_scalar(self._h, b"fused_pipeline", C.byref(v)))
        return v.value != 0.0

    def field(self, name: str) -> np.ndarray:
        out = np.empty((self.nz, self.ny, self.nx), dtype=np.float32)
        _check(self.L.kwh_thermal_get_matrix(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def set(self, name: str, values):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.float32), (self.nz, self.ny, self.nx)))
        _check(self.L.kwh_thermal_set_matrix(self._h, name.encode(), a.ctypes.data, a.size))

    T = property(lambda self: self.field("T"))
    cem43 = property(lambda self: self.field("cem43"))
    T_max = property(lambda self: self.field("T_max"))

    def lesion_volume(self, threshold_minutes: float = 240.0) -> float:
        """volume [m^3] of the points with cem43 >= threshold_minutes"""
        v = C.c_double()
        _check(self.L.kwh_thermal_lesion_volume(self._h, float(threshold_minutes), C.byref(v)))
        return float(v.value)

    def series(self, name: str = "T_raw") -> np.ndarray:
        """T at the sensor points after every step so far: (steps, points)"""
        size, steps = C.c_uint64(), C.c_uint64()
        _check(self.L.kwh_thermal_stream_read(self._h, name.encode(), None, 0, C.byref(size), C.byref(steps)))
        out = np.empty((steps.value, size.value), dtype=np.float32)
        _check(self.L.kwh_thermal_stream_read(self._h, name.encode(), out.ctypes.data, out.size, C.byref(size), C.byref(steps)))
        return out

    def time_steps(self, n_steps: int, heat_on: bool = True) -> float:
        """milliseconds of n steps between two HIP events on the solver's stream"""
        hip, ctx = capi.load(), self.ctx
        e0, e1 = C.c_void_p(), C.c_void_p()
        capi.check(hip.kw_event_create(ctx, C.byref(e0)))
        capi.check(hip.kw_event_create(ctx, C.byref(e1)))
        capi.check(hip.kw_event_record(ctx, e0))
        self.run(n_steps, heat_on)
        capi.check(hip.kw_event_record(ctx, e1))
        capi.check(hip.kw_event_synchronize(ctx, e1))
        ms = C.c_float()
        capi.check(hip.kw_event_elapsed_ms(ctx, e0, e1, C.byref(ms)))
        hip.kw_event_destroy(ctx, e0)
        hip.kw_event_destroy(ctx, e1)
        return float(ms.value)

    def close(self):
        if getattr(self, "_h", None):
            self.L.kwh_thermal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
