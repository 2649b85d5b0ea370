"""Weighted transducer arrays: the input datasets of a k-Wave kWaveArray-style array, built from per-element weights.

An array element (off-grid, curved or finite-size) is a set of grid points with band-limited interpolation weights.
The solver takes the array in this weighted form (include/kwave_host.h):

* source: `p_source_element_input` (one signal per element) and a point-major CSR matrix (`p_source_element_ptr`,
  `p_source_element_index`, `p_source_element_weight`) over the points of `p_source_index`;
* velocity source: the same with `u_source_element_ptr/_index/_weight` over the points of `u_source_index`, shared by
  the components, and `ux_/uy_/uz_source_element_input` (one signal per element and component);
* sensor (`--p_elements`): an element-major CSR matrix (`sensor_element_ptr`, `sensor_element_index`,
  `sensor_element_weight`) whose rows give one value per element and step, `p_elements[t][e] = sum_j w_j p[index_j]`.

Elements are given as `[(flat grid indices, weights), ...]`, one pair per element, with 0-based linear grid indices in
the x-fastest order of `sensor_mask_index` (`np.ravel` of a `[nz][ny][nx]` array).  Weights are used as given: any
element-area normalisation belongs in them.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

U64 = np.uint64
Element = Tuple[Sequence[int], Sequence[float]]


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


def weighted_source(elements: Sequence[Element], signals: np.ndarray) -> Dict[str, np.ndarray]:
    """Datasets of a weighted pressure source.  signals: (Nt_src, E) array, row t = the element signals of step t.

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
    return {
        "p_source_flag": np.array([[[sig.shape[0]]]], dtype=U64),
        "p_source_index": (points + 1).astype(U64).reshape(1, 1, -1),
        "p_source_element_input": np.ascontiguousarray(sig).reshape(1, sig.shape[0], sig.shape[1]),
        "p_source_element_ptr": ptr.reshape(1, 1, -1),
        "p_source_element_index": (elem + 1).astype(U64).reshape(1, 1, -1),
        "p_source_element_weight": wts.astype(np.float32).reshape(1, 1, -1),
    }


def weighted_velocity_source(elements: Sequence[Element], signals_x=None, signals_y=None, signals_z=None
                             ) -> Dict[str, np.ndarray]:
    """Datasets of a weighted velocity source.  signals_x / _y / _z: (Nt_src, E) arrays or None; a component left out is
    not driven (its flag is 0).  The components may differ in Nt_src.  The points and the CSR are those of
    weighted_source and are shared by the components; u_source_many is 1 and u_source_mode is left to the caller."""
    given = {c: np.asarray(s, dtype=np.float32) for c, s in (("x", signals_x), ("y", signals_y), ("z", signals_z))
             if s is not None}
    if not given:
        raise ValueError("a weighted velocity source needs the signals of at least one component")
    for c, sig in given.items():
        if sig.ndim != 2 or sig.shape[1] != len(elements):
            raise ValueError(f"signals_{c} must be (Nt, E={len(elements)}), got {sig.shape}")
    csr = weighted_source(elements, next(iter(given.values())))
    out = {"u_source_index": csr["p_source_index"], "u_source_many": np.array([[[1]]], dtype=U64)}
    for part in ("ptr", "index", "weight"):
        out["u_source_element_" + part] = csr["p_source_element_" + part]
    for c in "xyz":
        out[f"u{c}_source_flag"] = np.array([[[given[c].shape[0] if c in given else 0]]], dtype=U64)
        if c in given:
            out[f"u{c}_source_element_input"] = np.ascontiguousarray(given[c]).reshape(1, *given[c].shape)
    return out


def weighted_sensor(elements: Sequence[Element]) -> Dict[str, np.ndarray]:
    """Datasets of a weighted sensor (record it with --p_elements / HostSolver(..., p_elements=1)): element e's row holds
    its points and weights in the order given."""
    els = _check(elements)
    ptr = np.zeros(len(els) + 1, dtype=U64)
    ptr[1:] = np.cumsum([i.size for i, _ in els])
    idx = np.concatenate([i for i, _ in els]) if els else np.zeros(0, np.int64)
    w = np.concatenate([w for _, w in els]) if els else np.zeros(0, np.float32)
    return {
        "sensor_element_ptr": ptr.reshape(1, 1, -1),
        "sensor_element_index": (idx + 1).astype(U64).reshape(1, 1, -1),
        "sensor_element_weight": w.astype(np.float32).reshape(1, 1, -1),
    }


def expand_source(ds: Dict[str, np.ndarray]) -> np.ndarray:
    """The expanded (p_source_many = 1) series of a weighted source, (1, Nt_src, Npts) float32: every point's series
    summed in float64 from the element signals and weights, then rounded once."""
    sig = np.asarray(ds["p_source_element_input"], dtype=np.float64)
    sig = sig.reshape(sig.shape[-2], sig.shape[-1])
    ptr = np.asarray(ds["p_source_element_ptr"]).reshape(-1).astype(np.int64)
    col = np.asarray(ds["p_source_element_index"]).reshape(-1).astype(np.int64) - 1
    w = np.asarray(ds["p_source_element_weight"], dtype=np.float64).reshape(-1)
    rows = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    out = np.zeros((sig.shape[0], ptr.size - 1), dtype=np.float64)
    np.add.at(out.T, rows, (w[:, None] * sig[:, col].T))
    return out.astype(np.float32).reshape(1, sig.shape[0], -1)


def expand_velocity_source(ds: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The expanded (u_source_many = 1) series of a weighted velocity source: {"ux_source_input": (1, Nt_src, Npts)
    float32, ...} for the components that `ds` drives, each as expand_source gives it."""
    out = {}
    for c in "xyz":
        name = f"u{c}_source_element_input"
        if name in ds:
            one = {"p_source_element_input": ds[name]}
            for part in ("ptr", "index", "weight"):
                one["p_source_element_" + part] = ds["u_source_element_" + part]
            out[f"u{c}_source_input"] = expand_source(one)
    return out


def sensor_matrix(ds: Dict[str, np.ndarray], n_grid: int) -> np.ndarray:
    """The weighted sensor as a dense float64 (E, n_grid) matrix W (p_elements[t] = W @ p[t].ravel())."""
    ptr = np.asarray(ds["sensor_element_ptr"]).reshape(-1).astype(np.int64)
    idx = np.asarray(ds["sensor_element_index"]).reshape(-1).astype(np.int64) - 1
    w = np.asarray(ds["sensor_element_weight"], dtype=np.float64).reshape(-1)
    W = np.zeros((ptr.size - 1, n_grid), dtype=np.float64)
    np.add.at(W, (np.repeat(np.arange(ptr.size - 1), np.diff(ptr)), idx), w)
    return W
