"""Off-grid elements, host side: the shape helpers of kwave_amd.arrays (point counts, measures, every point on its surface,
deterministic), offgrid_elements without a device, and one property of the float64 reference the GPU test compares
against (tests/offgrid_reference.py).  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from offgrid_reference import radius, reference_weights  # noqa: E402

DX = 2.0e-4
REL = 1e-12


@pytest.fixture(scope="module")
def arrays():
    import kwave_amd  # noqa: F401
    from kwave_amd import arrays
    return arrays


@pytest.fixture(scope="module")
def grid(arrays):
    return arrays.Grid(64, 64, 64, DX, DX, DX)


def test_line_element(arrays, grid):
    a, b = np.array([-1.3e-3, 0.4e-3, 0.2e-3]), np.array([2.1e-3, -0.7e-3, 1.1e-3])
    pts, measure, dim = arrays.line_element(grid, a, b)
    length = np.linalg.norm(b - a)
    assert dim == 1 and measure == pytest.approx(length, rel=REL)
    assert pts.shape == (math.ceil(10 * length / DX), 3) and pts.dtype == np.float64
    t = (pts - a) @ (b - a) / length ** 2
    assert np.all((t > 0) & (t < 1))
    assert np.max(np.linalg.norm(pts - (a + t[:, None] * (b - a)), axis=1)) <= REL * length   # on the segment
    assert np.allclose(np.diff(t), 1.0 / len(pts), rtol=0, atol=1e-12) and t[0] == pytest.approx(0.5 / len(pts))
    assert arrays.line_element(grid, a, b, upsampling=4)[0].shape[0] == math.ceil(4 * length / DX)
    # 2-D: two coordinates, z = 0
    p2 = arrays.line_element(arrays.Grid(64, 64, 1, DX, DX, DX), (0.0, 0.0), (1.0e-3, 0.0))[0]
    assert p2.shape == (50, 3) and np.all(p2[:, 2] == 0.0)


def test_rect_element(arrays, grid):
    Lx, Ly, angle = 3.1e-3, 1.2e-3, 0.4
    centre = np.array([0.2e-3, -0.5e-3, 0.9e-3])
    pts, measure, dim = arrays.rect_element(grid, centre, Lx, Ly, angle)
    P = math.ceil(10 * Lx * Ly / DX ** 2)
    n_x, n_y = math.ceil(math.sqrt(P * Lx / Ly)), math.ceil(math.sqrt(P * Ly / Lx))
    assert dim == 2 and measure == pytest.approx(Lx * Ly, rel=REL)
    assert pts.shape == (n_x * n_y, 3) and n_x * n_y >= P
    ex = np.array([math.cos(angle), math.sin(angle), 0.0])
    ey = np.array([-math.sin(angle), math.cos(angle), 0.0])
    rel = pts - centre
    assert np.max(np.abs(rel[:, 2])) <= REL * Lx                        # in the plane
    assert np.max(np.abs(rel @ ex)) < Lx / 2 and np.max(np.abs(rel @ ey)) < Ly / 2   # inside the rectangle
    # cell centres: the lattice is symmetric about the centre and as wide as the rectangle less one cell
    assert np.allclose(rel.mean(axis=0), 0.0, atol=REL * Lx)
    assert np.ptp(rel @ ex) == pytest.approx(Lx * (1 - 1 / n_x), rel=1e-9)
    assert np.ptp(rel @ ey) == pytest.approx(Ly * (1 - 1 / n_y), rel=1e-9)
    # a rotation matrix in place of the angle: the rectangle in the yz-plane
    rot = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    q = arrays.rect_element(grid, centre, Lx, Ly, rot)[0] - centre
    assert np.max(np.abs(q[:, 0])) <= REL * Lx and np.ptp(q[:, 1]) == pytest.approx(Lx * (1 - 1 / n_x), rel=1e-9)


def test_disc_element(arrays, grid):
    centre, radius_, normal = np.array([0.3e-3, 0.1e-3, -0.4e-3]), 1.7e-3, np.array([1.0, -2.0, 0.5])
    pts, measure, dim = arrays.disc_element(grid, centre, radius_, normal)
    P = math.ceil(10 * math.pi * radius_ ** 2 / DX ** 2)
    assert dim == 2 and measure == pytest.approx(math.pi * radius_ ** 2, rel=REL) and pts.shape == (P, 3)
    rel = pts - centre
    assert np.max(np.abs(rel @ (normal / np.linalg.norm(normal)))) <= REL * radius_   # in the plane
    r = np.linalg.norm(rel, axis=1)
    assert np.allclose(r, radius_ * np.sqrt((np.arange(P) + 0.5) / P), rtol=1e-12, atol=0)   # the sunflower radii
    assert r.max() < radius_
    # equal areas: the points inside half the radius are a quarter of the set
    assert abs(np.count_nonzero(r < radius_ / 2) - P / 4) <= 1
    # the golden angle between consecutive points
    e1 = rel[0] / r[0]
    e2 = np.cross(normal / np.linalg.norm(normal), e1)
    theta = np.arctan2(rel @ e2, rel @ e1)
    step = np.mod(np.diff(theta), 2 * math.pi)
    assert np.allclose(step, np.mod(arrays.GOLDEN_ANGLE, 2 * math.pi), atol=1e-9)


def test_bowl_element(arrays, grid):
    apex, focus = np.array([-2.0e-3, 0.5e-3, 0.0]), np.array([3.0e-3, 1.5e-3, 1.0e-3])
    rc, diameter = 4.0e-3, 5.0e-3
    pts, measure, dim = arrays.bowl_element(grid, apex, rc, diameter, focus)
    h = rc - math.sqrt(rc ** 2 - (diameter / 2) ** 2)
    P = math.ceil(10 * 2 * math.pi * rc * h / DX ** 2)
    assert dim == 2 and measure == pytest.approx(2 * math.pi * rc * h, rel=REL) and pts.shape == (P, 3)
    axis = (focus - apex) / np.linalg.norm(focus - apex)
    centre = apex + rc * axis
    assert np.max(np.abs(np.linalg.norm(pts - centre, axis=1) - rc)) <= REL * rc      # on the sphere
    t = (pts - apex) @ axis                                                           # height above the apex
    assert np.all((t > 0) & (t < h))                                                   # within the cap ...
    off_axis = np.linalg.norm((pts - apex) - t[:, None] * axis, axis=1)
    assert off_axis.max() < diameter / 2                                               # ... and its aperture
    assert np.allclose(t, h * (np.arange(P) + 0.5) / P, rtol=1e-9, atol=0)            # equal steps in height = equal areas
    with pytest.raises(ValueError):
        arrays.bowl_element(arrays.Grid(64, 64, 1, DX, DX, DX), apex, rc, diameter, focus)
    with pytest.raises(ValueError):
        arrays.bowl_element(grid, apex, rc, 2.5 * rc, focus)


def test_point_sets_are_deterministic_and_need_one_spacing(arrays, grid):
    for make in (lambda: arrays.line_element(grid, (0, 0, 0), (1e-3, 2e-3, 0.5e-3)),
                 lambda: arrays.rect_element(grid, (0, 0, 0), 2e-3, 1e-3, 0.3),
                 lambda: arrays.disc_element(grid, (0, 0, 0), 1e-3, (0.2, 0.3, 1.0)),
                 lambda: arrays.bowl_element(grid, (0, 0, 0), 3e-3, 2e-3, (0, 0, 1e-3))):
        a, b = make(), make()
        assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    with pytest.raises(ValueError, match="dx == dy == dz"):
        arrays.disc_element(arrays.Grid(64, 64, 64, DX, 2 * DX, DX), (0, 0, 0), 1e-3)


def test_grid_units_follow_kgrid(arrays):
    g = arrays.Grid(24, 21, 1, 1.0e-3, 2.0e-3, 1.0)
    u = arrays.grid_units(g, [[0.0, 0.0, 0.0], [-12.0e-3, 20.0e-3, 0.0], [0.5e-3, -1.0e-3, 0.0]])
    assert np.array_equal(u, [[12.0, 10.0, 0.0], [0.0, 20.0, 0.0], [12.5, 9.5, 0.0]])


def test_offgrid_elements_needs_a_device(arrays, grid):
    """the weights are computed on the GPU and nowhere else: without one the call raises the library's error"""
    from kwave_amd import capi
    shapes = [arrays.disc_element(grid, (0, 0, 0), 1e-3)]
    try:
        capi.Device().close()
    except capi.KWaveError:
        with pytest.raises(capi.KWaveError):
            arrays.offgrid_elements(None, grid, shapes)
        return
    (index, weight), = arrays.offgrid_elements(None, grid, shapes)   # a GPU is present: the call opens it itself
    assert index.size == weight.size > 0


def test_reference_weights_of_one_point_sum_to_one_within_the_truncation():
    """The untruncated interpolant sums to 1.  With f = 0.3 and R = 7 the pairs d = +-m left out add up to
    (sin(pi f) / pi) * sum_{m > R} (-1)^m (-2 f) / (m^2 - f^2), an alternating series bounded by its first term,
    2 f sin(pi f) / (pi ((R + 1)^2 - f^2)) = 2.42e-3; the sum computed in float64 is 1.0013578597043173."""
    f, tol = 0.3, 0.05
    R = radius(tol)
    assert R == 7 and radius(0.1) == 4
    W, A = reference_weights([[32 + f, 0.0, 0.0]], [0, 1], [1.0], (64, 1, 1), tol)
    assert np.count_nonzero(W) == 2 * R + 1 and np.flatnonzero(W)[0] == 32 - R
    total = W.sum()
    assert abs(total - 1.0013578597043173) < 1e-12
    assert abs(total - 1.0) <= 2 * f * math.sin(math.pi * f) / (math.pi * ((R + 1) ** 2 - f ** 2))
    assert W[0, 32] == pytest.approx(np.sinc(f), rel=1e-15) and np.all(A >= np.abs(W))
