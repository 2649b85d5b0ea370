"""Weighted transducer arrays: the input datasets of a k-Wave kWaveArray-style array, built from per-element weights.

An array element (off-grid, curved or finite-size) is a set of grid points with band-limited interpolation weights.
The solver takes the array in this weighted form (include/kwave_host.h):

* source: `p_source_element_input` (one signal per element) and a point-major CSR matrix (`p_source_element_ptr`,
  `p_source_element_index`, `p_source_element_weight`) over the points of `p_source_index`;
* velocity source: the same with `u_source_element_ptr/_index/_weight` over the points of `u_source_index`, shared by
  the components, and `ux_/uy_/uz_source_element_input` (one signal per element and component);
* sensor (`--p_elements`): an element-major CSR matrix (`sensor_element_ptr`, `sensor_element_index`,
  `sensor_element_weight`) whose rows give one value per element and step, `p_elements[t][e] = sum_j w_j p[index_j]`.

Every entry of the three CSR matrices may carry an integer time delay in steps (`p_source_element_delay`,
`u_source_element_delay`, `sensor_element_delay`, built from the `delays=` argument of the three builders): point k gets
`sum_j w_j s[t - d_j][e_j]`, element e records `sum_j w_j p^(t - d_j)[index_j]`.  `focus_delays` gives the delays that
focus an array at a point.

Elements are given as `[(flat grid indices, weights), ...]`, one pair per element, with 0-based linear grid indices in
the x-fastest order of `sensor_mask_index` (`np.ravel` of a `[nz][ny][nx]` array).  Weights are used as given: any
element-area normalisation belongs in them.

`offgrid_elements` builds those pairs from geometry, on the GPU (kw_offgrid_build): an element is a set of integration
points on its surface, its weights their band-limited interpolant.  `line_element`, `rect_element`, `disc_element` and
`bowl_element` place the points of the usual shapes; any (P, 3) array of points in metres serves as well.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np

U64 = np.uint64
Element = Tuple[Sequence[int], Sequence[float]]
Shape = Tuple[np.ndarray, float, int]     # (points (P, 3) float64 in metres, measure in m^dim, dim)
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))
MAX_DELAY = 65535                         # KW_ELEMENT_MAX_DELAY of include/kwave_hip.h


class Grid(NamedTuple):
    """The grid an array sits on.  Point i of an axis of N points lies at (i - N // 2) * d (k-Wave's kgrid.x_vec); a 2-D
    grid has nz == 1."""
    nx: int
    ny: int
    nz: int
    dx: float
    dy: float
    dz: float


# ---- element shapes: integration points, pure NumPy in float64 ---------------------------------------------------------------
def _vec3(v, what: str) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size == 2:
        v = np.append(v, 0.0)
    if v.size != 3 or not np.all(np.isfinite(v)):
        raise ValueError(f"{what} must be 2 or 3 finite coordinates, got {v}")
    return v


def _spacing(grid: Grid) -> float:
    """the one spacing the shape helpers count their points by"""
    if grid.dx != grid.dy or (grid.nz > 1 and grid.dz != grid.dx):
        raise ValueError("the shape helpers need dx == dy == dz; pass your own points on other grids")
    return float(grid.dx)


def _count(measure: float, d: float, dim: int, upsampling: float) -> int:
    if not (measure > 0.0 and math.isfinite(measure)):
        raise ValueError(f"an element needs a positive size, got a measure of {measure}")
    return int(math.ceil(upsampling * measure / d ** dim))


def _plane_basis(normal: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """unit vectors (e1, e2, n) with e1 x e2 = n: e1 is the coordinate axis least aligned with n, made normal to it"""
    length = np.linalg.norm(normal)
    if not length > 0.0:
        raise ValueError("the normal / axis of an element must not be zero")
    n = normal / length
    e1 = np.zeros(3)
    e1[int(np.argmin(np.abs(n)))] = 1.0
    e1 -= n * (e1 @ n)
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(n, e1), n


def _rotation(rotation) -> np.ndarray:
    r = np.asarray(rotation, dtype=np.float64)
    if r.ndim == 0:                                        # an angle in radians about z
        c, s = math.cos(float(r)), math.sin(float(r))
        return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    if r.shape != (3, 3) or not np.allclose(r @ r.T, np.eye(3), atol=1e-12):
        raise ValueError("rotation is an angle about z in radians or a 3 x 3 rotation matrix")
    return r


def line_element(grid: Grid, a, b, upsampling: float = 10.0) -> Shape:
    """The segment from a to b: the midpoints of P = ceil(upsampling * |b - a| / dx) equal pieces; measure |b - a|, dim 1."""
    a, b = _vec3(a, "a"), _vec3(b, "b")
    length = float(np.linalg.norm(b - a))
    p = _count(length, _spacing(grid), 1, upsampling)
    t = (np.arange(p) + 0.5) / p
    return a + t[:, None] * (b - a), length, 1


def rect_element(grid: Grid, centre, Lx: float, Ly: float, rotation=0.0, upsampling: float = 10.0) -> Shape:
    """The Lx x Ly rectangle about `centre`, in the xy-plane turned by `rotation` (an angle about z in radians, or a 3 x 3
    rotation matrix): the centres of an n_x x n_y lattice of equal cells, n_x = ceil(sqrt(P Lx / Ly)) and
    n_y = ceil(sqrt(P Ly / Lx)) with P = ceil(upsampling * Lx Ly / dx^2), so n_x n_y >= P; measure Lx Ly, dim 2."""
    centre, rot = _vec3(centre, "centre"), _rotation(rotation)
    area = float(Lx) * float(Ly)
    p = _count(area, _spacing(grid), 2, upsampling)
    n_x = max(1, int(math.ceil(math.sqrt(p * Lx / Ly))))
    n_y = max(1, int(math.ceil(math.sqrt(p * Ly / Lx))))
    x = ((np.arange(n_x) + 0.5) / n_x - 0.5) * Lx
    y = ((np.arange(n_y) + 0.5) / n_y - 0.5) * Ly
    local = np.zeros((n_y, n_x, 3))
    local[..., 0], local[..., 1] = x[None, :], y[:, None]
    return centre + local.reshape(-1, 3) @ rot.T, area, 2


def disc_element(grid: Grid, centre, radius: float, normal=(0.0, 0.0, 1.0), upsampling: float = 10.0) -> Shape:
    """The disc of `radius` about `centre` in the plane normal to `normal`: the sunflower set r_k = radius
    sqrt((k + 1/2) / P), theta_k = k pi (3 - sqrt 5), P = ceil(upsampling * pi radius^2 / dx^2) points of equal area;
    measure pi radius^2, dim 2."""
    centre = _vec3(centre, "centre")
    e1, e2, _ = _plane_basis(_vec3(normal, "normal"))
    area = math.pi * float(radius) ** 2
    p = _count(area, _spacing(grid), 2, upsampling)
    k = np.arange(p)
    r, theta = radius * np.sqrt((k + 0.5) / p), k * GOLDEN_ANGLE
    return centre + (r * np.cos(theta))[:, None] * e1 + (r * np.sin(theta))[:, None] * e2, area, 2


def bowl_element(grid: Grid, apex, radius_of_curvature: float, diameter: float, focus, upsampling: float = 10.0) -> Shape:
    """The spherical cap with its rear point at `apex`, opening towards `focus` (which only gives the direction of the
    axis): radius of curvature Rc, aperture `diameter` <= 2 Rc, height h = Rc - sqrt(Rc^2 - (diameter / 2)^2).  The
    golden-angle set of the disc with equal steps in the height above the apex, t_k = h (k + 1/2) / P — equal areas on a
    sphere; measure 2 pi Rc h, dim 2.  3-D grids only."""
    if grid.nz == 1:
        raise ValueError("a bowl needs a 3-D grid")
    apex = _vec3(apex, "apex")
    e1, e2, axis = _plane_basis(_vec3(focus, "focus") - apex)
    rc, half = float(radius_of_curvature), 0.5 * float(diameter)
    if not 0.0 < half <= rc:
        raise ValueError(f"a bowl needs 0 < diameter <= 2 * radius_of_curvature, got {diameter} and {rc}")
    h = rc - math.sqrt(rc * rc - half * half)
    area = 2.0 * math.pi * rc * h
    p = _count(area, _spacing(grid), 2, upsampling)
    k = np.arange(p)
    t, theta = h * (k + 0.5) / p, k * GOLDEN_ANGLE
    rho = np.sqrt(t * (2.0 * rc - t))                      # distance from the axis at height t: sqrt(Rc^2 - (Rc - t)^2)
    return apex + t[:, None] * axis + (rho * np.cos(theta))[:, None] * e1 + (rho * np.sin(theta))[:, None] * e2, area, 2


def grid_units(grid: Grid, points) -> np.ndarray:
    """points (P, 3) in metres -> grid units, u = x / d + N // 2 per axis, float64"""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] not in (2, 3):
        raise ValueError(f"points must be (P, 3), got {pts.shape}")
    if pts.shape[1] == 2:
        pts = np.concatenate([pts, np.zeros((pts.shape[0], 1))], axis=1)
    return pts / np.array([grid.dx, grid.dy, grid.dz]) + np.array([grid.nx // 2, grid.ny // 2, grid.nz // 2], dtype=np.float64)


def offgrid_elements(device, grid: Grid, elements: Sequence[Shape], bli_tolerance: float = 0.05,
                     normalise: bool = False, scratch_bytes: int = 0) -> List[Element]:
    """Elements from geometry, their weights computed on the GPU (capi.offgrid_build): the list weighted_source,
    weighted_velocity_source and weighted_sensor take.

    device: a capi.Device, or None to open one for the call.  grid: a Grid (or anything with nx .. dz).  elements: one
    (points (P, 3) float64 in metres, measure, dim) per element, as the shape helpers return.  Each point carries
    scale = m_grid / P with m_grid = measure / dx^dim, k-Wave's source convention; normalise=True divides by m_grid, which
    gives the element average that kWaveArray.combineSensorData forms (for sensors)."""
    from . import capi
    grid = Grid(*(getattr(grid, n) for n in Grid._fields))
    coords, counts, scale = [], [], []
    for e, (pts, measure, dim) in enumerate(elements):
        u = grid_units(grid, pts) if len(pts) else np.zeros((0, 3))
        if dim not in (1, 2, 3):
            raise ValueError(f"element {e}: dim must be 1, 2 or 3, got {dim}")
        m_grid = float(measure) / grid.dx ** dim
        coords.append(u)
        counts.append(u.shape[0])
        scale.append((1.0 if normalise else m_grid) / u.shape[0] if u.shape[0] else 0.0)
    point_ptr = np.zeros(len(counts) + 1, dtype=U64)
    point_ptr[1:] = np.cumsum(counts)
    coords = np.concatenate(coords) if coords else np.zeros((0, 3))
    own = device is None
    dev = capi.Device() if own else device
    try:
        ptr, index, weight = capi.offgrid_build(dev, coords, point_ptr, scale, (grid.nx, grid.ny, grid.nz), bli_tolerance,
                                                scratch_bytes)
    finally:
        if own:
            dev.close()
    ptr = ptr.astype(np.int64)
    return [(index[ptr[e]:ptr[e + 1]].astype(np.int64), weight[ptr[e]:ptr[e + 1]]) for e in range(len(counts))]


def _check(elements: Sequence[Element]):
    out = []
    for e, (idx, w) in enumerate(elements):
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        w = np.asarray(w, dtype=np.float32).reshape(-1)
        if idx.shape != w.shape:
            raise ValueError(f"element {e}: {idx.size} indices but {w.size} weights")
        if idx.size and idx.min() < 0:
            raise ValueError(f"element {e}: negative grid index")
        out.append((idx, w))
    return out


def _check_delays(els, delays):
    """one integer array per element, aligned with its points -> the concatenated uint64 delays"""
    if len(delays) != len(els):
        raise ValueError(f"delays must hold one array per element ({len(els)}), got {len(delays)}")
    out = []
    for e, ((idx, _), d) in enumerate(zip(els, delays)):
        d = np.asarray(d).reshape(-1)
        if d.shape != idx.shape:
            raise ValueError(f"element {e}: {idx.size} indices but {d.size} delays")
        if d.size and (np.any(d != np.round(d)) or d.min() < 0 or d.max() > MAX_DELAY):
            raise ValueError(f"element {e}: delays must be integers in 0..{MAX_DELAY}")
        out.append(d.astype(np.int64))
    return np.concatenate(out).astype(U64) if out else np.zeros(0, U64)


def focus_delays(grid: Grid, elements: Sequence[Element], focus, sound_speed: float, dt: float,
                 per_element: bool = False) -> List[np.ndarray]:
    """Per-point delays that focus an array at `focus` (metres), one int64 array per element aligned with its points:
    round((r_max - r_j) / (sound_speed * dt)), r_j the distance of grid point j from the focus.  r_max is the largest
    distance over the whole array, so the farthest point fires first (delay 0) and all arrivals coincide; with
    per_element=True it is taken inside each element, which focuses every element on its own (an elevation focus) and
    leaves steering between elements to the signals."""
    grid = Grid(*(getattr(grid, n) for n in Grid._fields))
    f = _vec3(focus, "focus")
    if not (sound_speed > 0.0 and dt > 0.0):
        raise ValueError("sound_speed and dt must be positive")
    dist = []
    for idx, _ in _check(elements):
        pos = np.stack([(idx % grid.nx - grid.nx // 2) * grid.dx, (idx // grid.nx % grid.ny - grid.ny // 2) * grid.dy,
                        (idx // (grid.nx * grid.ny) - grid.nz // 2) * grid.dz], axis=1).astype(np.float64)
        dist.append(np.sqrt(((pos - f) ** 2).sum(axis=1)))
    whole = max((float(r.max()) for r in dist if r.size), default=0.0)
    return [np.round(((float(r.max()) if per_element and r.size else whole) - r) / (sound_speed * dt)).astype(np.int64)
            for r in dist]


def weighted_source(elements: Sequence[Element], signals: np.ndarray, delays=None) -> Dict[str, np.ndarray]:
    """Datasets of a weighted pressure source.  signals: (Nt_src, E) array, row t = the element signals of step t.
    delays: None, or one integer array per element aligned with its points (time steps, e.g. focus_delays); they follow
    their entries through the transpose into p_source_element_delay, and the source then acts for Nt_src + max delay steps.

    The source points are the union of the elements' points in ascending grid order; point k's CSR row holds one entry
    per element that covers it, in element order (the point-major transpose of the element lists).  Sets
    p_source_flag = Nt_src; p_source_mode is left to the caller."""
    els = _check(elements)
    sig = np.asarray(signals, dtype=np.float32)
    if sig.ndim != 2 or sig.shape[1] != len(els):
        raise ValueError(f"signals must be (Nt, E={len(els)}), got {sig.shape}")
    pts = np.concatenate([i for i, _ in els]) if els else np.zeros(0, np.int64)
    elem = np.concatenate([np.full(i.size, e, dtype=np.int64) for e, (i, _) in enumerate(els)]) if els else pts
    wts = np.concatenate([w for _, w in els]) if els else np.zeros(0, np.float32)
    order = np.lexsort((elem, pts))                      # by point, then element: a stable point-major order
    pts, elem, wts = pts[order], elem[order], wts[order]
    points, counts = np.unique(pts, return_counts=True)
    ptr = np.zeros(points.size + 1, dtype=U64)
    ptr[1:] = np.cumsum(counts)
    extra = {} if delays is None else {"p_source_element_delay": _check_delays(els, delays)[order].reshape(1, 1, -1)}
    return {
        **extra,
        "p_source_flag": np.array([[[sig.shape[0]]]], dtype=U64),
        "p_source_index": (points + 1).astype(U64).reshape(1, 1, -1),
        "p_source_element_input": np.ascontiguousarray(sig).reshape(1, sig.shape[0], sig.shape[1]),
        "p_source_element_ptr": ptr.reshape(1, 1, -1),
        "p_source_element_index": (elem + 1).astype(U64).reshape(1, 1, -1),
        "p_source_element_weight": wts.astype(np.float32).reshape(1, 1, -1),
    }


def weighted_velocity_source(elements: Sequence[Element], signals_x=None, signals_y=None, signals_z=None, delays=None
                             ) -> Dict[str, np.ndarray]:
    """Datasets of a weighted velocity source.  signals_x / _y / _z: (Nt_src, E) arrays or None; a component left out is
    not driven (its flag is 0).  The components may differ in Nt_src.  The points and the CSR are those of
    weighted_source and are shared by the components; u_source_many is 1 and u_source_mode is left to the caller.
    delays: as in weighted_source, into u_source_element_delay, shared by the components."""
    given = {c: np.asarray(s, dtype=np.float32) for c, s in (("x", signals_x), ("y", signals_y), ("z", signals_z))
             if s is not None}
    if not given:
        raise ValueError("a weighted velocity source needs the signals of at least one component")
    for c, sig in given.items():
        if sig.ndim != 2 or sig.shape[1] != len(elements):
            raise ValueError(f"signals_{c} must be (Nt, E={len(elements)}), got {sig.shape}")
    csr = weighted_source(elements, next(iter(given.values())), delays)
    out = {"u_source_index": csr["p_source_index"], "u_source_many": np.array([[[1]]], dtype=U64)}
    for part in ("ptr", "index", "weight") + (("delay",) if delays is not None else ()):
        out["u_source_element_" + part] = csr["p_source_element_" + part]
    for c in "xyz":
        out[f"u{c}_source_flag"] = np.array([[[given[c].shape[0] if c in given else 0]]], dtype=U64)
        if c in given:
            out[f"u{c}_source_element_input"] = np.ascontiguousarray(given[c]).reshape(1, *given[c].shape)
    return out


def weighted_sensor(elements: Sequence[Element], delays=None) -> Dict[str, np.ndarray]:
    """Datasets of a weighted sensor (record it with --p_elements / HostSolver(..., p_elements=1)): element e's row holds
    its points and weights in the order given.  delays: None, or one integer array per element aligned with its points,
    into sensor_element_delay: element e then records sum_j w_j p^(t - d_j)[index_j] (delay-and-sum on receive)."""
    els = _check(elements)
    ptr = np.zeros(len(els) + 1, dtype=U64)
    ptr[1:] = np.cumsum([i.size for i, _ in els])
    idx = np.concatenate([i for i, _ in els]) if els else np.zeros(0, np.int64)
    w = np.concatenate([w for _, w in els]) if els else np.zeros(0, np.float32)
    extra = {} if delays is None else {"sensor_element_delay": _check_delays(els, delays).reshape(1, 1, -1)}
    return {
        **extra,
        "sensor_element_ptr": ptr.reshape(1, 1, -1),
        "sensor_element_index": (idx + 1).astype(U64).reshape(1, 1, -1),
        "sensor_element_weight": w.astype(np.float32).reshape(1, 1, -1),
    }


def expand_source(ds: Dict[str, np.ndarray]) -> np.ndarray:
    """The expanded (p_source_many = 1) series of a weighted source, (1, Nt_src, Npts) float32: every point's series
    summed in float64 from the element signals and weights, then rounded once.  With p_source_element_delay the series
    has Nt_src + max delay rows, row t = sum_j w_j s[t - d_j][e_j] over the entries whose signal row exists: the
    expanded problem's p_source_flag is that row count (capped by Nt)."""
    sig = np.asarray(ds["p_source_element_input"], dtype=np.float64)
    sig = sig.reshape(sig.shape[-2], sig.shape[-1])
    ptr = np.asarray(ds["p_source_element_ptr"]).reshape(-1).astype(np.int64)
    col = np.asarray(ds["p_source_element_index"]).reshape(-1).astype(np.int64) - 1
    w = np.asarray(ds["p_source_element_weight"], dtype=np.float64).reshape(-1)
    rows = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    if "p_source_element_delay" in ds:
        d = np.asarray(ds["p_source_element_delay"]).reshape(-1).astype(np.int64)
        nt = sig.shape[0] + (int(d.max()) if d.size else 0)
        out = np.zeros((nt, ptr.size - 1), dtype=np.float64)
        for delay in np.unique(d):                        # entries in CSR order inside a delay, delays ascending
            j = np.nonzero(d == delay)[0]
            np.add.at(out[delay:delay + sig.shape[0]].T, rows[j], (w[j, None] * sig[:, col[j]].T))
        return out.astype(np.float32).reshape(1, nt, -1)
    out = np.zeros((sig.shape[0], ptr.size - 1), dtype=np.float64)
    np.add.at(out.T, rows, (w[:, None] * sig[:, col].T))
    return out.astype(np.float32).reshape(1, sig.shape[0], -1)


def expand_velocity_source(ds: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The expanded (u_source_many = 1) series of a weighted velocity source: {"ux_source_input": (1, Nt_src, Npts)
    float32, ...} for the components that `ds` drives, each as expand_source gives it (with u_source_element_delay:
    its Nt_src + max delay rows)."""
    out = {}
    for c in "xyz":
        name = f"u{c}_source_element_input"
        if name in ds:
            one = {"p_source_element_input": ds[name]}
            for part in ("ptr", "index", "weight") + (("delay",) if "u_source_element_delay" in ds else ()):
                one["p_source_element_" + part] = ds["u_source_element_" + part]
            out[f"u{c}_source_input"] = expand_source(one)
    return out


def sensor_matrix(ds: Dict[str, np.ndarray], n_grid: int) -> np.ndarray:
    """The weighted sensor as a dense float64 (E, n_grid) matrix W (p_elements[t] = W @ p[t].ravel()).  A delayed sensor is
    no single matrix: it is refused here, delayed_sensor_matrices gives one matrix per delay."""
    if "sensor_element_delay" in ds:
        raise ValueError("sensor_matrix: the sensor carries sensor_element_delay; use delayed_sensor_matrices")
    ptr = np.asarray(ds["sensor_element_ptr"]).reshape(-1).astype(np.int64)
    idx = np.asarray(ds["sensor_element_index"]).reshape(-1).astype(np.int64) - 1
    w = np.asarray(ds["sensor_element_weight"], dtype=np.float64).reshape(-1)
    W = np.zeros((ptr.size - 1, n_grid), dtype=np.float64)
    np.add.at(W, (np.repeat(np.arange(ptr.size - 1), np.diff(ptr)), idx), w)
    return W


def delayed_sensor_matrices(ds: Dict[str, np.ndarray], n_grid: int) -> Dict[int, np.ndarray]:
    """A delayed weighted sensor as {delay: dense float64 (E, n_grid) matrix W_d}: p_elements[t] = sum_d W_d @ p[t - d].ravel()
    over the delays with t - d at or after the sampling start.  Without sensor_element_delay: {0: sensor_matrix(ds)}."""
    ptr = np.asarray(ds["sensor_element_ptr"]).reshape(-1).astype(np.int64)
    idx = np.asarray(ds["sensor_element_index"]).reshape(-1).astype(np.int64) - 1
    w = np.asarray(ds["sensor_element_weight"], dtype=np.float64).reshape(-1)
    d = np.asarray(ds["sensor_element_delay"]).reshape(-1).astype(np.int64) if "sensor_element_delay" in ds else np.zeros(idx.size, np.int64)
    rows = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    out = {}
    for delay in np.unique(d) if d.size else [0]:
        j = np.nonzero(d == delay)[0]
        W = np.zeros((ptr.size - 1, n_grid), dtype=np.float64)
        np.add.at(W, (rows[j], idx[j]), w[j])
        out[int(delay)] = W
    return out
