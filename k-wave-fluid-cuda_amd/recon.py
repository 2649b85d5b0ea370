"""k-space reconstruction front-ends (include/kwave_host.h "k-space plane reconstruction" and "Batched k-space line
reconstruction" -> lib/libkwave_host.so).

`PlaneRecon` takes the record p(x, y, t) of a planar sensor — a photoacoustic measurement, or the sensor plane of a
time-loop run — and recovers the initial pressure p0(x, y, z) that produced it, what k-Wave's kspacePlaneRecon computes:
one 3-D FFT of the record mirrored in time, a re-gridding of every (kx, ky) line from w to
kz = sqrt((w / c)^2 - kx^2 - ky^2) with a weight, and one inverse 3-D FFT.  It is the inverse problem for the data that
`angular.AngularSpectrumTime` carries forward.  On fast-path sizes the whole reconstruction is one round trip of the fused
pipeline, the re-gridding done along the line its z-pass holds in LDS.  No CPU fallback: a missing library or device raises.

`LineRecon` is its 2-D form for a linear array, what k-Wave's kspaceLineRecon computes, batched: a stream of frames
p(t, y) to the images p0(x, y), F frames in one round trip of the pipeline (a context whose z axis is the batch).

Not built: heterogeneous media, Z-slabs, HDF5 files and the command line, graphs, the 2-D forms of the three projectors,
frames spread over several GPUs; a half-length (DCT) time transform that would use the evenness of the mirrored record, the
x- and y-inverse restricted to the crop, other interpolants.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

from .solver import Options, _check, load_host

_bound = False
INTERP = {"linear": 0, "nearest": 1}


class Config(C.Structure):
    """struct kwh_plane_recon_config"""
    _fields_ = [("nx", C.c_uint64), ("ny", C.c_uint64), ("nt", C.c_uint64), ("dx", C.c_double), ("dy", C.c_double),
                ("dt", C.c_double), ("c0", C.c_double), ("ex", C.c_uint64), ("ey", C.c_uint64), ("lt", C.c_uint64),
                ("planes", C.c_uint64), ("interp", C.c_int32), ("positivity", C.c_int32)]


class LineConfig(C.Structure):
    """struct kwh_line_recon_config"""
    _fields_ = [("ny", C.c_uint64), ("nt", C.c_uint64), ("frames", C.c_uint64), ("dy", C.c_double), ("dt", C.c_double),
                ("c0", C.c_double), ("ey", C.c_uint64), ("lt", C.c_uint64), ("depth", C.c_uint64),
                ("chunk_frames", C.c_uint64), ("interp", C.c_int32), ("positivity", C.c_int32)]


def _lib() -> C.CDLL:
    global _bound
    L = load_host()
    if not _bound:
        L.kwh_plane_recon_plan.argtypes = [C.POINTER(Config), C.POINTER(Options), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
        L.kwh_plane_recon_create.argtypes = [C.POINTER(Config), C.POINTER(Options), C.POINTER(C.c_void_p)]
        L.kwh_plane_recon_destroy.argtypes = [C.c_void_p]
        L.kwh_plane_recon_run.argtypes = [C.c_void_p, C.c_void_p]
        L.kwh_plane_recon_get.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
        L.kwh_plane_recon_get_scalar.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        L.kwh_plane_recon_context.restype = C.c_void_p
        L.kwh_plane_recon_context.argtypes = [C.c_void_p]
        L.kwh_line_recon_plan.argtypes = [C.POINTER(LineConfig), C.POINTER(Options), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
        L.kwh_line_recon_create.argtypes = [C.POINTER(LineConfig), C.POINTER(Options), C.POINTER(C.c_void_p)]
        L.kwh_line_recon_destroy.argtypes = [C.c_void_p]
        L.kwh_line_recon_run.argtypes = [C.c_void_p, C.c_void_p]
        L.kwh_line_recon_get.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
        L.kwh_line_recon_get_scalar.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        L.kwh_line_recon_context.restype = C.c_void_p
        L.kwh_line_recon_context.argtypes = [C.c_void_p]
        _bound = True
    return L


def _config(dims, spacing, dt, nt, c0, planes, interp, positivity, expanded, time_length) -> Config:
    dims = tuple(int(v) for v in dims)
    spacing = tuple(float(v) for v in spacing)
    if len(dims) != 2 or len(spacing) != 2:
        raise ValueError("dims = (Nx, Ny) and spacing = (dx, dy)")
    if min(dims) < 0 or int(nt) < 0:
        raise ValueError(f"dims and nt must not be negative, got {dims}, {nt}")
    if interp not in INTERP:
        raise ValueError(f"interp must be one of {sorted(INTERP)}, got {interp!r}")
    c = Config()
    c.nx, c.ny = dims
    c.nt = int(nt)
    c.dx, c.dy = spacing
    c.dt, c.c0 = float(dt), float(c0)
    c.interp = INTERP[interp]
    c.positivity = int(bool(positivity))
    if planes is not None:
        if int(planes) <= 0:
            raise ValueError(f"planes must be positive, got {planes}")
        c.planes = int(planes)
    if expanded is not None:
        expanded = tuple(int(v) for v in expanded)
        if len(expanded) != 2 or min(expanded) < 0:
            raise ValueError("expanded = (Ex, Ey)")
        c.ex, c.ey = expanded
    if time_length is not None:
        if int(time_length) <= 0:
            raise ValueError(f"time_length must be positive, got {time_length}")
        c.lt = int(time_length)
    return c


def plan_recon(dims, spacing, dt, nt, c0, planes=None, interp="linear", positivity=False, expanded=None, time_length=None,
               fused_kernels=True) -> Tuple[Tuple[int, int], int, bool]:
    """((Ex, Ey), Lt, fast path) of a reconstruction, validated as PlaneRecon would, without a device"""
    L = _lib()
    c = _config(dims, spacing, dt, nt, c0, planes, interp, positivity, expanded, time_length)
    o = Options()
    o.fused_kernels = int(bool(fused_kernels))
    e, fast = (C.c_uint64 * 3)(), C.c_int32()
    _check(L.kwh_plane_recon_plan(C.byref(c), C.byref(o), e, C.byref(fast)))
    return (int(e[0]), int(e[1])), int(e[2]), bool(fast.value)


class PlaneRecon:
    """Reconstruction of the initial pressure from the record p (Nt, Ny, Nx) (x fastest) of a planar sensor sampled at
    t_n = n dt: `run(p)` gives p0 on the planes z_j = j c0 dt, float32 (planes, Ny, Nx).

    dims = (Nx, Ny), spacing = (dx, dy) [m], dt [s], nt = Nt, c0 [m/s].  planes: default Nt.  interp: "linear" or "nearest",
    the interpolant of the re-gridding from w to kz.  positivity: clamp the result at 0.  expanded = (Ex, Ey): default
    (Nx, Ny), k-Wave's choice.  time_length = Lt >= 2 Nt - 1, the length of the record mirrored in time: default the
    smallest fast-path length at or above 2 Nt - 1 (a finer w grid than k-Wave's, and a smaller interpolation error), or
    2 Nt - 1 itself with fused_kernels=False or above 1024.  The fused stage runs when Ex, Ey and Lt are all fast-path
    lengths, the rocFFT twin otherwise.  Memory: about 28 bytes per point of Ex Ey Lt on the fast path."""

    def __init__(self, dims, spacing, dt, nt, c0, planes=None, interp="linear", positivity=False, expanded=None,
                 time_length=None, fused_kernels=True, device_idx=-1):
        L = _lib()
        c = _config(dims, spacing, dt, nt, c0, planes, interp, positivity, expanded, time_length)
        o = Options()
        o.device_idx = int(device_idx)
        o.fused_kernels = int(bool(fused_kernels))
        self.L, self._h = L, None
        h = C.c_void_p()
        _check(L.kwh_plane_recon_create(C.byref(c), C.byref(o), C.byref(h)))
        self._h = h
        self.nx, self.ny, self.nt = int(c.nx), int(c.ny), int(c.nt)
        self.spacing = (float(c.dx), float(c.dy))
        self.dt, self.c0 = float(c.dt), float(c.c0)
        self.interp, self.positivity = interp, bool(positivity)
        self.planes = int(self._scalar("planes"))

    def _scalar(self, name: str) -> float:
        v = C.c_double()
        _check(self.L.kwh_plane_recon_get_scalar(self._h, name.encode(), C.byref(v)))
        return float(v.value)

    @property
    def shape(self):
        return (self.planes, self.ny, self.nx)

    @property
    def dz(self) -> float:
        """plane spacing c0 dt [m]"""
        return self._scalar("dz")

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
        return C.c_void_p(self.L.kwh_plane_recon_context(self._h))

    def run(self, p) -> np.ndarray:
        """p0 for the record p: float32 (planes, Ny, Nx)"""
        a = np.asarray(p, dtype=np.float32)
        if a.shape != (self.nt, self.ny, self.nx):
            raise ValueError(f"p must be (Nt, Ny, Nx) = {(self.nt, self.ny, self.nx)}, got {a.shape}")
        a = np.ascontiguousarray(a)
        _check(self.L.kwh_plane_recon_run(self._h, a.ctypes.data))
        out = np.empty(self.shape, dtype=np.float32)
        _check(self.L.kwh_plane_recon_get(self._h, b"p0", out.ctypes.data, out.size))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.L.kwh_plane_recon_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _line_config(ny, dy, dt, nt, c0, frames, depth, interp, positivity, expanded, time_length, chunk_frames) -> LineConfig:
    if int(ny) < 0 or int(nt) < 0 or int(frames) < 0:
        raise ValueError(f"ny, nt and frames must not be negative, got {ny}, {nt}, {frames}")
    if interp not in INTERP:
        raise ValueError(f"interp must be one of {sorted(INTERP)}, got {interp!r}")
    c = LineConfig()
    c.ny, c.nt, c.frames = int(ny), int(nt), int(frames)
    c.dy, c.dt, c.c0 = float(dy), float(dt), float(c0)
    c.interp = INTERP[interp]
    c.positivity = int(bool(positivity))
    for name, field, value in (("depth", "depth", depth), ("expanded", "ey", expanded), ("time_length", "lt", time_length),
                               ("chunk_frames", "chunk_frames", chunk_frames)):
        if value is not None:
            if int(value) <= 0:
                raise ValueError(f"{name} must be positive, got {value}")
            setattr(c, field, int(value))
    return c


def plan_line_recon(ny, dy, dt, nt, c0, frames=1, depth=None, interp="linear", positivity=False, expanded=None,
                    time_length=None, chunk_frames=None, fused_kernels=True) -> Tuple[int, int, int, int, bool]:
    """(Ey, Lt, depth, chunk_frames, fast path) of a line reconstruction, validated as LineRecon would, without a device"""
    L = _lib()
    c = _line_config(ny, dy, dt, nt, c0, frames, depth, interp, positivity, expanded, time_length, chunk_frames)
    o = Options()
    o.fused_kernels = int(bool(fused_kernels))
    e, fast = (C.c_uint64 * 4)(), C.c_int32()
    _check(L.kwh_line_recon_plan(C.byref(c), C.byref(o), e, C.byref(fast)))
    return int(e[0]), int(e[1]), int(e[2]), int(e[3]), bool(fast.value)


class LineRecon:
    """Reconstruction of `frames` images from the records p (F, Nt, Ny) (y fastest) of a linear array sampled at
    t_n = n dt: `run(p)` gives p0 on the rows x_j = j c0 dt, float32 (F, depth, Ny).  With frames == 1, (Nt, Ny) gives
    (depth, Ny).  order="yt" takes the transposed records (F, Ny, Nt), as k-Wave's sensor_data(y, t).

    ny = Ny, dy [m], dt [s], nt = Nt, c0 [m/s].  depth: default Nt.  interp: "linear" or "nearest".  positivity: clamp the
    result at 0.  expanded = Ey: default Ny.  time_length = Lt >= 2 Nt - 1: default the smallest fast-path length at or above
    2 Nt - 1, or 2 Nt - 1 itself with fused_kernels=False or above 1024.  chunk_frames: the frames that go through the pipeline
    at once (default all, capped at 65535 frames and at 4 GiB of spectrum, 2^29 padded bins); a run goes chunk by chunk on one context, and a frame's result
    does not depend on the chunking on the fused path.  The fused stage runs when Ey and Lt are fast-path lengths (and, for the
    ten lengths of Ey without masked x kernels, Lt chunk_frames is a multiple of 16), the rocFFT twin otherwise."""

    def __init__(self, ny, dy, dt, nt, c0, frames=1, depth=None, interp="linear", positivity=False, expanded=None,
                 time_length=None, chunk_frames=None, order="ty", fused_kernels=True, device_idx=-1):
        if order not in ("ty", "yt"):
            raise ValueError(f"order must be 'ty' or 'yt', got {order!r}")
        L = _lib()
        c = _line_config(ny, dy, dt, nt, c0, frames, depth, interp, positivity, expanded, time_length, chunk_frames)
        o = Options()
        o.device_idx = int(device_idx)
        o.fused_kernels = int(bool(fused_kernels))
        self.L, self._h = L, None
        h = C.c_void_p()
        _check(L.kwh_line_recon_create(C.byref(c), C.byref(o), C.byref(h)))
        self._h = h
        self.ny, self.nt, self.frames = int(c.ny), int(c.nt), int(c.frames)
        self.dy, self.dt, self.c0 = float(c.dy), float(c.dt), float(c.c0)
        self.interp, self.positivity, self.order = interp, bool(positivity), order
        self.depth = int(self._scalar("depth"))

    def _scalar(self, name: str) -> float:
        v = C.c_double()
        _check(self.L.kwh_line_recon_get_scalar(self._h, name.encode(), C.byref(v)))
        return float(v.value)

    @property
    def shape(self):
        return (self.frames, self.depth, self.ny)

    @property
    def dx(self) -> float:
        """row spacing c0 dt [m]"""
        return self._scalar("dx")

    @property
    def expanded(self) -> int:
        return int(self._scalar("Ey"))

    @property
    def time_length(self) -> int:
        return int(self._scalar("Lt"))

    @property
    def chunk_frames(self) -> int:
        return int(self._scalar("chunk_frames"))

    @property
    def fused(self) -> bool:
        return self._scalar("fused_pipeline") != 0.0

    @property
    def runs(self) -> int:
        return int(self._scalar("runs"))

    @property
    def ctx(self):
        return C.c_void_p(self.L.kwh_line_recon_context(self._h))

    def run(self, p) -> np.ndarray:
        """p0 for the records p: float32 (F, depth, Ny), or (depth, Ny) for one frame handed in as a 2-D array"""
        a = np.asarray(p, dtype=np.float32)
        single = a.ndim == 2 and self.frames == 1
        if single:
            a = a[None]
        want = (self.frames, self.nt, self.ny) if self.order == "ty" else (self.frames, self.ny, self.nt)
        if a.shape != want:
            raise ValueError(f"p must be {'(F, Nt, Ny)' if self.order == 'ty' else '(F, Ny, Nt)'} = {want}, got {a.shape}")
        if self.order == "yt":
            a = a.transpose(0, 2, 1)
        a = np.ascontiguousarray(a)
        _check(self.L.kwh_line_recon_run(self._h, a.ctypes.data))
        out = np.empty(self.shape, dtype=np.float32)
        _check(self.L.kwh_line_recon_get(self._h, b"p0", out.ctypes.data, out.size))
        return out[0] if single else out

    def close(self):
        if getattr(self, "_h", None):
            self.L.kwh_line_recon_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
