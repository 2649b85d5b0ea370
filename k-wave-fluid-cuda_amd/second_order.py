"""Exact k-space propagator front-end (include/kwave_host.h "Exact k-space propagator" -> lib/libkwave_host.so).

`SecondOrder` carries an initial pressure p0(x, y, z) in a homogeneous medium, lossless or power-law absorbing, to the
pressure at any time t, what k-Wave's kspaceSecondOrder computes: one 3-D FFT of p0, then per output time one multiply by
the real H(|k|; t) and one inverse transform.  There is no time loop, so there is no CFL limit and no stepping error: a
snapshot at t = 40 us costs two transforms, a sensor record three passes per sample at any sampling interval.  The box is
periodic; `t_free` is the time up to which the result inside the domain is the free-space one.  No CPU fallback: a missing
library or device raises.  With `plane` set, `plane_record(times)` gives what a planar sensor at z = plane dz records,
(n_times, Ny, Nx) — `recon.PlaneRecon`'s input — in one call: per time and (kx, ky) one sum over the kz bins and one 2-D
inverse over the record itself, no 3-D round trip per time.

`SecondOrderFrames` is its batched 2-D form (kwave_host.h "Exact k-space propagator on frames"): F independent images
p0(x, y) that share the medium, the expanded plane, the output times and the sensor points, each carried to any time by one
2-D round trip — what a linear array records for many phantoms, the forward side of `recon.LineRecon`.  With `line_row`
set, `line_record(times)` gives that record for one row of the plane, (F, n_times, Nx), in one call: per time and kx one sum
over the ky bins and one 1-D inverse over the record itself, no 2-D round trip per time.

`set_dp0dt(v)` on either gives dp/dt at t = 0 [Pa/s] as a second initial condition (k-Wave's source.dp0dt): per mode
p^(t) = Hc P0 + Hs V0, so dp0dt = -c0 df/dx with p0 = f(x) launches a one-way wave, and a snapshot (p, dp/dt) continues a
field.  It is independent of `set_p0`; `None` clears it.

Not built: dp0/dt in `line_record` and `plane_record`, time-varying sources, heterogeneous media, Z-slabs, chunks of frames and
frames over several GPUs, HDF5 files and the command line, graphs, several output times per pass and inverse passes
restricted to the crop, to the sensor points or to the rows that hold sensors (but for the one row of `line_record` and the
one plane of `plane_record`),
several rows, columns or arbitrary points in `line_record`, planes normal to x or y and several planes in `plane_record`,
particle velocity outputs.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

from .solver import Options, _check, load_host

_bound = False
FLAGS = {"p_max": 1, "p_min": 2, "p_rms": 4, "p_final": 8}   # KWH_SECOND_ORDER_P_*
RECORDS = ("p_raw",) + tuple(FLAGS)


class Config(C.Structure):
    """struct kwh_second_order_config"""
    _fields_ = [("nx", C.c_uint64), ("ny", C.c_uint64), ("nz", C.c_uint64), ("dx", C.c_double), ("dy", C.c_double),
                ("dz", C.c_double), ("c0", C.c_double), ("alpha_coeff", C.c_double), ("alpha_power", C.c_double),
                ("t_max", C.c_double), ("ex", C.c_uint64), ("ey", C.c_uint64), ("ez", C.c_uint64), ("n_sensor", C.c_uint64),
                ("sensor_index", C.POINTER(C.c_uint64)), ("flags", C.c_int32), ("pad_", C.c_int32)]


class FramesConfig(C.Structure):
    """struct kwh_second_order_frames_config"""
    _fields_ = [("nx", C.c_uint64), ("ny", C.c_uint64), ("frames", C.c_uint64), ("dx", C.c_double), ("dy", C.c_double),
                ("c0", C.c_double), ("alpha_coeff", C.c_double), ("alpha_power", C.c_double), ("t_max", C.c_double),
                ("ex", C.c_uint64), ("ey", C.c_uint64), ("n_sensor", C.c_uint64), ("sensor_index", C.POINTER(C.c_uint64)),
                ("flags", C.c_int32), ("pad_", C.c_int32)]


def _lib() -> C.CDLL:
    global _bound
    L = load_host()
    if not _bound:
        for name, cfg in (("kwh_second_order", Config), ("kwh_second_order_frames", FramesConfig)):
            fn = lambda what: getattr(L, name + "_" + what)
            fn("plan").argtypes = [C.POINTER(cfg), C.POINTER(Options), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
            fn("create").argtypes = [C.POINTER(cfg), C.POINTER(Options), C.POINTER(C.c_void_p)]
            fn("destroy").argtypes = [C.c_void_p]
            fn("set_p0").argtypes = [C.c_void_p, C.c_void_p]
            fn("set_dp0dt").argtypes = [C.c_void_p, C.c_void_p]
            fn("field").argtypes = [C.c_void_p, C.c_double, C.c_void_p]
            fn("run").argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint64]
            fn("get").argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
            fn("get_scalar").argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
            fn("context").restype = C.c_void_p
            fn("context").argtypes = [C.c_void_p]
        L.kwh_second_order_plane_plan.argtypes = [C.POINTER(Config), C.POINTER(Options), C.c_int64, C.c_uint64, C.c_uint64,
                                                  C.POINTER(C.c_uint64)]
        L.kwh_second_order_set_plane.argtypes = [C.c_void_p, C.c_int64]
        L.kwh_second_order_set_plane_chunk_times.argtypes = [C.c_void_p, C.c_uint64]
        L.kwh_second_order_plane_record.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint64, C.c_void_p]
        L.kwh_second_order_frames_line_plan.argtypes = [C.POINTER(FramesConfig), C.POINTER(Options), C.c_int64, C.c_uint64,
                                                        C.c_uint64, C.POINTER(C.c_uint64)]
        L.kwh_second_order_frames_set_line_row.argtypes = [C.c_void_p, C.c_int64]
        L.kwh_second_order_frames_set_line_chunk_times.argtypes = [C.c_void_p, C.c_uint64]
        L.kwh_second_order_frames_line_record.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint64, C.c_void_p]
        _bound = True
    return L


def _config(n, d, c0, alpha_coeff, alpha_power, t_max, expanded, sensor_index, record, frames=None):
    """the 3-D config, or with `frames` the batched 2-D one; the sensor indices are returned to keep them alive"""
    n = tuple(int(v) for v in n)
    d = tuple(float(v) for v in d)
    axes = 3 if frames is None else 2
    if len(n) != axes or len(d) != axes:
        raise ValueError("n = (Nx, Ny, Nz) and d = (dx, dy, dz)" if axes == 3 else "n = (Nx, Ny) and d = (dx, dy)")
    if min(n) < 0:
        raise ValueError(f"n must not be negative, got {n}")
    record = (record,) if isinstance(record, str) else tuple(record)
    unknown = [r for r in record if r not in RECORDS]
    if unknown:
        raise ValueError(f"record: {unknown} not among {RECORDS}")
    if axes == 3:
        c = Config()
        c.nx, c.ny, c.nz = n
        c.dx, c.dy, c.dz = d
    else:
        if int(frames) < 0:
            raise ValueError(f"frames must not be negative, got {frames}")
        c = FramesConfig()
        c.nx, c.ny = n
        c.dx, c.dy = d
        c.frames = int(frames)
    c.c0 = float(c0)
    c.alpha_coeff, c.alpha_power = float(alpha_coeff), float(alpha_power)
    c.t_max = 0.0 if t_max is None else float(t_max)
    if expanded is not None:
        expanded = tuple(int(v) for v in expanded)
        if len(expanded) != axes or min(expanded) < 0:
            raise ValueError("expanded = (Ex, Ey, Ez)" if axes == 3 else "expanded = (Ex, Ey)")
        if axes == 3:
            c.ex, c.ey, c.ez = expanded
        else:
            c.ex, c.ey = expanded
    idx = np.zeros(0, dtype=np.uint64)
    if sensor_index is not None and "p_raw" in record:
        s = np.asarray(sensor_index).reshape(-1)
        if s.size and s.min() < 0:
            raise ValueError("sensor_index must not be negative")
        idx = np.ascontiguousarray(s.astype(np.uint64))
    c.n_sensor = int(idx.size)
    c.sensor_index = idx.ctypes.data_as(C.POINTER(C.c_uint64)) if idx.size else None
    c.flags = sum(FLAGS[r] for r in set(record) if r in FLAGS)
    return c, idx


class _Propagator:
    """What SecondOrder and SecondOrderFrames share: the handle and its scalars, dp0dt, field, run, the aggregates of a run.
    `_ENTRY` is the C entry points' common name."""

    def _create(self, c, idx, fused_kernels, device_idx):
        self.L, self._h = _lib(), None
        o = Options()
        o.device_idx = int(device_idx)
        o.fused_kernels = int(bool(fused_kernels))
        h = C.c_void_p()
        _check(self._fn("create")(C.byref(c), C.byref(o), C.byref(h)))
        self._h = h
        self.n_sensor = int(idx.size)
        self.n_times = 0

    @classmethod
    def _fn(cls, what: str):
        return getattr(_lib(), cls._ENTRY + "_" + what)

    def _scalar(self, name: str) -> float:
        v = C.c_double()
        _check(self._fn("get_scalar")(self._h, name.encode(), C.byref(v)))
        return float(v.value)

    @property
    def t_free(self) -> float:
        """[s]: up to this time nothing has wrapped around the periodic box into the domain"""
        return self._scalar("t_free")

    @property
    def fused(self) -> bool:
        return self._scalar("fused_pipeline") != 0.0

    @property
    def runs(self) -> int:
        return int(self._scalar("runs"))

    @property
    def ctx(self):
        return C.c_void_p(self._fn("context")(self._h))

    def _get(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.float32)
        _check(self._fn("get")(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def _set_dp0dt(self, v, name):
        if v is None:
            _check(self._fn("set_dp0dt")(self._h, None))
            return
        a = np.asarray(v, dtype=np.float32)
        if a.shape != self.shape:
            raise ValueError(f"dp0dt must be {name} = {self.shape}, got {a.shape}")
        a = np.ascontiguousarray(a)
        _check(self._fn("set_dp0dt")(self._h, a.ctypes.data))

    @property
    def has_dp0dt(self) -> bool:
        return self._scalar("has_dp0dt") != 0.0

    def field(self, t: float) -> np.ndarray:
        """the pressure at time t [s] on the domain: float32 (Nz, Ny, Nx)"""
        out = np.empty(self.shape, dtype=np.float32)
        _check(self._fn("field")(self._h, float(t), out.ctypes.data))
        return out

    def run(self, times) -> np.ndarray:
        """every time of `times` [s] in the given order; returns the record float32 (n_times, n_sensor)"""
        ta = np.ascontiguousarray(np.asarray(times, dtype=np.float64).reshape(-1))
        _check(self._fn("run")(self._h, ta.ctypes.data_as(C.POINTER(C.c_double)), ta.size))
        self.n_times = int(ta.size)
        shape = self._record_shape()
        return self._get("p_raw", shape) if self.n_sensor != 0 else np.empty(shape, dtype=np.float32)

    def _record_shape(self):
        return (self.n_times, self.n_sensor)

    def p_max(self) -> np.ndarray:
        """max over the output times of the last run"""
        return self._get("p_max", self.shape)

    def p_min(self) -> np.ndarray:
        """min over the output times of the last run"""
        return self._get("p_min", self.shape)

    def p_rms(self) -> np.ndarray:
        """root mean square over the output times of the last run"""
        return self._get("p_rms", self.shape)

    def p_final(self) -> np.ndarray:
        """the field at the last output time of the last run"""
        return self._get("p_final", self.shape)

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SecondOrder(_Propagator):
    """The pressure at any time from an initial pressure p0 (Nz, Ny, Nx) (x fastest) in a homogeneous medium.

    n = (Nx, Ny, Nz), d = (dx, dy, dz) [m], c0 [m/s].  alpha_coeff [dB / (MHz^y cm)] (0: lossless) and alpha_power y: power-law
    absorption with its dispersion, underdamped modes only (a coefficient that damps a mode of the grid beyond B = 1/4 is
    refused).  t_max [s] sizes the default expanded grid: per axis the smallest fast-path length >= N + ceil(c0 t_max / d);
    expanded = (Ex, Ey, Ez) gives the sides instead (expanded = n: the periodic box).  sensor_index: 0-based flat indices
    into the (Nz, Ny, Nx) array, sampled by run(); record: which of "p_raw", "p_max", "p_min", "p_rms", "p_final" run() keeps.

    set_p0(p0), then field(t) -> (Nz, Ny, Nx) or run(times) -> the record (n_times, n_sensor); times in any order.
    set_dp0dt(v) adds dp/dt at t = 0 (Nz, Ny, Nx) [Pa/s]; None clears it (has_dp0dt).

    plane: a plane 0 ... Nz - 1 of the domain (None: none) whose record plane_record(times) -> (n_times, Ny, Nx) gives without
    a 3-D round trip per time — `recon.PlaneRecon`'s input when times = n dt.  It is prepared by set_p0; plane_chunk_times
    bounds the output times of one pass (None: by a byte budget).  field, run and plane_record may be interleaved."""

    _ENTRY = "kwh_second_order"   # the C entry points' common name (SecondOrderFrames: its own)

    def __init__(self, n, d, c0, alpha_coeff=0.0, alpha_power=1.5, t_max=None, expanded=None, sensor_index=None,
                 record=("p_raw",), fused_kernels=True, device_idx=-1, plane=None, plane_chunk_times=None):
        c, idx = _config(n, d, c0, alpha_coeff, alpha_power, t_max, expanded, sensor_index, record)
        self._create(c, idx, fused_kernels, device_idx)
        self.nx, self.ny, self.nz = int(c.nx), int(c.ny), int(c.nz)
        try:
            if plane is not None:
                self.plane = plane
            if plane_chunk_times is not None:
                self.plane_chunk_times = plane_chunk_times
        except Exception:
            self.close()
            raise

    @staticmethod
    def plan(n, d, c0, alpha_coeff=0.0, alpha_power=1.5, t_max=None, expanded=None, sensor_index=None, record=("p_raw",),
             fused_kernels=True) -> Tuple[Tuple[int, int, int], bool]:
        """((Ex, Ey, Ez), fast path), validated as the constructor would, without a device"""
        L = _lib()
        c, _idx = _config(n, d, c0, alpha_coeff, alpha_power, t_max, expanded, sensor_index, record)
        o = Options()
        o.fused_kernels = int(bool(fused_kernels))
        e, fast = (C.c_uint64 * 3)(), C.c_int32()
        _check(L.kwh_second_order_plan(C.byref(c), C.byref(o), e, C.byref(fast)))
        return (int(e[0]), int(e[1]), int(e[2])), bool(fast.value)

    @property
    def shape(self):
        return (self.nz, self.ny, self.nx)

    @property
    def expanded(self) -> Tuple[int, int, int]:
        return tuple(int(self._scalar(n)) for n in ("Ex", "Ey", "Ez"))

    def set_p0(self, p0):
        """embed, transform and keep the initial pressure; may be called again"""
        a = np.asarray(p0, dtype=np.float32)
        if a.shape != self.shape:
            raise ValueError(f"p0 must be (Nz, Ny, Nx) = {self.shape}, got {a.shape}")
        a = np.ascontiguousarray(a)
        _check(self._fn("set_p0")(self._h, a.ctypes.data))

    def set_dp0dt(self, v):
        """dp/dt at t = 0 [Pa/s], (Nz, Ny, Nx), as a second initial condition; None clears it.  Independent of set_p0
        (which stays required, and may be all zeros): either may be called again in any order."""
        self._set_dp0dt(v, "(Nz, Ny, Nx)")

    @staticmethod
    def plane_plan(n, d, c0, plane, n_times, plane_chunk_times=None, **kw) -> Tuple[int, int, int]:
        """(output times of one pass, passes for n_times, complex values of Q), checked as the plane setter, the chunk setter
        and plane_record would, without a device; kw: the constructor's other arguments"""
        o = Options()
        o.fused_kernels = int(bool(kw.pop("fused_kernels", True)))
        c, _idx = _config(n, d, c0, kw.pop("alpha_coeff", 0.0), kw.pop("alpha_power", 1.5), kw.pop("t_max", None),
                          kw.pop("expanded", None), kw.pop("sensor_index", None), kw.pop("record", ("p_raw",)))
        if kw:
            raise TypeError(f"unknown arguments {sorted(kw)}")
        out = (C.c_uint64 * 3)()
        _check(_lib().kwh_second_order_plane_plan(C.byref(c), C.byref(o), -1 if plane is None else int(plane),
                                                  int(plane_chunk_times or 0), int(n_times), out))
        return int(out[0]), int(out[1]), int(out[2])

    @property
    def plane(self):
        """the plane that plane_record records (None: none); setting it takes effect at the next set_p0"""
        r = int(self._scalar("plane"))
        return None if r < 0 else r

    @plane.setter
    def plane(self, plane):
        _check(_lib().kwh_second_order_set_plane(self._h, -1 if plane is None else int(plane)))

    @property
    def plane_chunk_times(self) -> int:
        """output times per pass of plane_record; set None or 0 for the default"""
        return int(self._scalar("plane_chunk_times"))

    @plane_chunk_times.setter
    def plane_chunk_times(self, times):
        if times is not None and int(times) < 0:
            raise ValueError(f"plane_chunk_times must not be negative, got {times}")
        _check(_lib().kwh_second_order_set_plane_chunk_times(self._h, int(times or 0)))

    def plane_record(self, times) -> np.ndarray:
        """the pressure on the plane z = plane dz at every time of `times` [s], in the given order: float32 (n_times, Ny, Nx)"""
        ta = np.ascontiguousarray(np.asarray(times, dtype=np.float64).reshape(-1))
        out = np.empty((int(ta.size), self.ny, self.nx), dtype=np.float32)
        _check(_lib().kwh_second_order_plane_record(self._h, ta.ctypes.data_as(C.POINTER(C.c_double)), ta.size,
                                                    out.ctypes.data))
        return out


class SecondOrderFrames(_Propagator):
    """The pressure at any time from F independent initial pressures p0 (F, Ny, Nx) (x fastest) in one homogeneous medium:
    SecondOrder in 2-D, batched — one pass serves all frames.

    n = (Nx, Ny), d = (dx, dy) [m], c0 [m/s], frames = F (at most 65535).  alpha_coeff, alpha_power, t_max, record: as
    SecondOrder, the B rule on the 2-D grid.  expanded = (Ex, Ey) gives the sides of the periodic plane (default: per axis the
    smallest fast-path length >= N + ceil(c0 t_max / d)).  sensor_index: 0-based flat indices into ONE (Ny, Nx) plane,
    sampled in every frame by run() — a row of the plane is a linear array.

    set_p0(p0) takes (F, Ny, Nx), or (Ny, Nx) when frames == 1; field(t) -> (F, Ny, Nx); run(times) -> the record
    (n_times, F, n_sensor), times in any order; p_max() / p_min() / p_rms() / p_final() -> (F, Ny, Nx).  set_dp0dt(v) adds
    dp/dt at t = 0 of every frame (F, Ny, Nx) [Pa/s]; None clears it.

    line_row: a row 0 ... Ny - 1 of the plane (None: none) whose record line_record(times) -> (F, n_times, Nx) gives without
    a 2-D round trip per time — `recon.LineRecon`'s order "ty" with x as the array axis.  It is prepared by set_p0;
    line_chunk_times bounds the output times of one pass (None: by a byte budget).  field, run and line_record may be
    interleaved."""

    _ENTRY = "kwh_second_order_frames"

    def __init__(self, n, d, c0, frames, alpha_coeff=0.0, alpha_power=1.5, t_max=None, expanded=None, sensor_index=None,
                 record=("p_raw",), fused_kernels=True, device_idx=-1, line_row=None, line_chunk_times=None):
        c, idx = _config(n, d, c0, alpha_coeff, alpha_power, t_max, expanded, sensor_index, record, frames=frames)
        self._create(c, idx, fused_kernels, device_idx)
        self.nx, self.ny, self.frames = int(c.nx), int(c.ny), int(c.frames)
        try:
            if line_row is not None:
                self.line_row = line_row
            if line_chunk_times is not None:
                self.line_chunk_times = line_chunk_times
        except Exception:
            self.close()
            raise

    @staticmethod
    def plan(n, d, c0, frames, alpha_coeff=0.0, alpha_power=1.5, t_max=None, expanded=None, sensor_index=None,
             record=("p_raw",), fused_kernels=True) -> Tuple[Tuple[int, int], bool]:
        """((Ex, Ey), fast path), validated as the constructor would, without a device"""
        c, _idx = _config(n, d, c0, alpha_coeff, alpha_power, t_max, expanded, sensor_index, record, frames=frames)
        o = Options()
        o.fused_kernels = int(bool(fused_kernels))
        e, fast = (C.c_uint64 * 2)(), C.c_int32()
        _check(SecondOrderFrames._fn("plan")(C.byref(c), C.byref(o), e, C.byref(fast)))
        return (int(e[0]), int(e[1])), bool(fast.value)

    @property
    def shape(self):
        return (self.frames, self.ny, self.nx)

    @property
    def expanded(self) -> Tuple[int, int]:
        return tuple(int(self._scalar(n)) for n in ("Ex", "Ey"))

    def set_p0(self, p0):
        """embed, transform and keep the initial pressures (F, Ny, Nx); (Ny, Nx) for a single frame; may be called again"""
        a = np.asarray(p0, dtype=np.float32)
        if self.frames == 1 and a.shape == self.shape[1:]:
            a = a[None]
        if a.shape != self.shape:
            raise ValueError(f"p0 must be (F, Ny, Nx) = {self.shape}, got {a.shape}")
        a = np.ascontiguousarray(a)
        _check(self._fn("set_p0")(self._h, a.ctypes.data))

    def set_dp0dt(self, v):
        """dp/dt at t = 0 of every frame [Pa/s], (F, Ny, Nx), as a second initial condition; None clears it.  Independent
        of set_p0.  line_record is refused while one is set."""
        self._set_dp0dt(v, "(F, Ny, Nx)")

    def _record_shape(self):
        return (self.n_times, self.frames, self.n_sensor)

    @staticmethod
    def line_plan(n, d, c0, frames, line_row, n_times, line_chunk_times=None, **kw) -> Tuple[int, int, int]:
        """(output times of one pass, passes for n_times, complex values of Q), checked as set_line_row, the chunk setter and
        line_record would, without a device; kw: the constructor's other arguments"""
        o = Options()
        o.fused_kernels = int(bool(kw.pop("fused_kernels", True)))
        c, _idx = _config(n, d, c0, kw.pop("alpha_coeff", 0.0), kw.pop("alpha_power", 1.5), kw.pop("t_max", None),
                          kw.pop("expanded", None), kw.pop("sensor_index", None), kw.pop("record", ("p_raw",)), frames=frames)
        if kw:
            raise TypeError(f"unknown arguments {sorted(kw)}")
        out = (C.c_uint64 * 3)()
        _check(_lib().kwh_second_order_frames_line_plan(C.byref(c), C.byref(o), -1 if line_row is None else int(line_row),
                                                        int(line_chunk_times or 0), int(n_times), out))
        return int(out[0]), int(out[1]), int(out[2])

    @property
    def line_row(self):
        """the row that line_record records (None: none); setting it takes effect at the next set_p0"""
        r = int(self._scalar("line_row"))
        return None if r < 0 else r

    @line_row.setter
    def line_row(self, row):
        _check(_lib().kwh_second_order_frames_set_line_row(self._h, -1 if row is None else int(row)))

    @property
    def line_chunk_times(self) -> int:
        """output times per pass of line_record; set None or 0 for the default"""
        return int(self._scalar("line_chunk_times"))

    @line_chunk_times.setter
    def line_chunk_times(self, times):
        if times is not None and int(times) < 0:
            raise ValueError(f"line_chunk_times must not be negative, got {times}")
        _check(_lib().kwh_second_order_frames_set_line_chunk_times(self._h, int(times or 0)))

    def line_record(self, times) -> np.ndarray:
        """the pressure on row line_row of every frame at every time of `times` [s], in the given order: float32
        (F, n_times, Nx)"""
        ta = np.ascontiguousarray(np.asarray(times, dtype=np.float64).reshape(-1))
        out = np.empty((self.frames, int(ta.size), self.nx), dtype=np.float32)
        _check(_lib().kwh_second_order_frames_line_record(self._h, ta.ctypes.data_as(C.POINTER(C.c_double)), ta.size,
                                                          out.ctypes.data))
        return out
