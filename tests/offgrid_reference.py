"""The off-grid element weights restated in float64 NumPy (a plain module, imported by name from tests/): the reference
of tests/test_gpu_offgrid.py and the subject of one property test in tests/test_offgrid_host.py.

W[e][g] = sum over the points p of element e of scale_e * sinc(d_x - f_x) * sinc(d_y - f_y) * sinc(d_z - f_z) for the
grid points g = n + d with |d| <= R per axis inside the grid, n = floor(u + 0.5), f = u - n, R = ceil(1 / (pi * tol));
an axis of one point has d = 0 and the factor 1."""
import math

import numpy as np


def radius(bli_tolerance):
    return int(math.ceil(1.0 / (math.pi * bli_tolerance)))


def reference_weights(coords, point_ptr, scale, dims, bli_tolerance):
    """dense float64 (E, n_grid) arrays W and A = sum over the points of |c| (the magnitude the error bound scales with)"""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    point_ptr = np.asarray(point_ptr).astype(np.int64)
    scale = np.asarray(scale, dtype=np.float32).astype(np.float64)  # the build takes fp32 scales: the same numbers here
    R = radius(bli_tolerance)
    W = np.zeros((scale.size, int(np.prod(dims))))
    A = np.zeros_like(W)
    nearest = np.floor(coords + 0.5)
    offset = coords - nearest
    for e in range(scale.size):
        for p in range(point_ptr[e], point_ptr[e + 1]):
            idx, fac = [], []
            for a in range(3):
                d = np.arange(-R, R + 1) if dims[a] > 1 else np.zeros(1, dtype=np.int64)
                g = int(nearest[p, a]) + d
                keep = (g >= 0) & (g < dims[a])
                idx.append(g[keep])
                fac.append(np.sinc(d[keep] - offset[p, a]) if dims[a] > 1 else np.ones(1))
            c = scale[e] * fac[2][:, None, None] * fac[1][None, :, None] * fac[0][None, None, :]
            g = idx[0][None, None, :] + dims[0] * (idx[1][None, :, None] + dims[1] * idx[2][:, None, None])
            W[e, g.ravel()] += c.ravel()       # the cells of one stencil are distinct
            A[e, g.ravel()] += np.abs(c).ravel()
    return W, A
