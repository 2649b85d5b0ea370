"""Off-grid elements on the GPU: kw_offgrid_build against the float64 restatement of its definition
(tests/offgrid_reference.py), its determinism (run to run, under permutations of the points, under translation, under
reflection, under the scratch budget), its input checks, and a disc source with an off-grid point sensor run end to end
against the oracle.

Bound per entry of the densified CSR (values only: a contribution below the fixed-point step may vanish, so membership is
not compared):  |W_gpu - W_ref| <= 32 * 2^-24 * A + P_e * 2^-41 + 2^-24 * |W_ref|,  A = sum over the points of |c|.
Each 1-D factor carries about 5.5 roundings of 2^-24 (pi * f, sinf within 2 ulp, f - d, pi * (f - d), the divide), the
fp32 offset one more, three factors and three products about 20: the bound takes 32; every contribution is rounded once to
a multiple of 2^-40 and the sum once to fp32.  The worst err / bound is printed (pytest -s); measured: 0.176 on the
3-D case, 0.184 in 2-D and 0.145 at R = 4."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_l2

sys.path.insert(0, os.path.join(ROOT, "tests"))
from offgrid_reference import radius, reference_weights  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TOL = 1e-5
CELL_BYTES = 20  # scratch per box cell (kwave_hip.h)


@pytest.fixture(scope="module")
def mods():
    import kwave_amd  # noqa: F401
    from kwave_amd import arrays, capi
    from kwave_amd.solver import HostSolver
    return arrays, capi, HostSolver


@pytest.fixture(scope="module")
def dev(mods):
    d = mods[1].Device()
    yield d
    d.close()


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _draw(rng, lo, hi, count):
    """`count` points uniform in the box lo .. hi (grid units), redrawn while an offset is within 1e-3 of +-0.5: the
    reference's own choice of the nearest index is then never on a knife edge"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    u = rng.uniform(lo, hi, (count, 3))
    while True:
        bad = np.any(np.abs(np.abs(u - np.floor(u + 0.5)) - 0.5) < 1e-3, axis=1)
        if not bad.any():
            return u
        u[bad] = rng.uniform(lo, hi, (int(bad.sum()), 3))


def _case(dims, seed=20):
    """One build with: no point, one point, 5 000 points (many blocks), two elements on shared grid points, points at both
    ends of every axis (a box clipped on all six faces), an offset of exactly -0.5, and a point on the grid."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    flat = nz == 1
    zlo, zhi = (-0.4, 0.4) if flat else (4.0, nz - 5.0)
    z_of = (lambda z: 0.0) if flat else (lambda z: z)
    parts = [
        np.zeros((0, 3)),
        _draw(rng, (9, 8, zlo if flat else 7.6), (12, 11, zhi if flat else 9.4), 1),   # its stencil is not clipped
        _draw(rng, (6, 5, zlo), (nx - 7.0, ny - 6.0, zhi), 5000),
        _draw(rng, (8, 7, zlo), (13, 12, zhi), 40),
        _draw(rng, (10, 9, zlo), (15, 14, zhi), 40),
        np.array([[0.2, 0.3, z_of(-0.1)], [nx - 1.2, ny - 0.8, z_of(nz - 0.7)]]),   # n = 0 and n = N - 1 on every axis
        np.array([[10.5, 8.0, z_of(7.25)]]),                                         # n_x = 11, f_x = -0.5 exactly
        np.array([[12.0, 9.0, z_of(8.0)]]),                                          # on the grid: one entry
    ]
    counts = [len(p) for p in parts]
    point_ptr = np.zeros(len(parts) + 1, dtype=np.uint64)
    point_ptr[1:] = np.cumsum(counts)
    scale = (rng.uniform(0.5, 1.5, len(parts)) / np.maximum(counts, 1)).astype(np.float32)
    return np.concatenate(parts), point_ptr, scale


CASES = {"3d": ((24, 20, 18), 0.05), "2d": ((24, 20, 1), 0.05), "r4": ((24, 20, 18), 0.1)}
_cache = {}


def _reference(name):
    """inputs and float64 reference of a case, computed once and shared"""
    if name not in _cache:
        dims, tol = CASES[name]
        coords, point_ptr, scale = _case(dims)
        W, A = reference_weights(coords, point_ptr, scale, dims, tol)
        for a in (coords, point_ptr, scale, W, A):
            a.setflags(write=False)
        _cache[name] = (dims, tol, coords, point_ptr, scale, W, A)
    return _cache[name]


def _dense(ptr, index, weight, n_grid):
    W = np.zeros((ptr.size - 1, n_grid), dtype=np.float32)
    rows = np.repeat(np.arange(ptr.size - 1), np.diff(ptr.astype(np.int64)))
    assert np.unique(rows * n_grid + index.astype(np.int64)).size == index.size, "a grid point twice in one row"
    W[rows, index.astype(np.int64)] = weight
    return W


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1, 2. against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_weights_against_fp64(mods, dev, name):
    _, capi, _ = mods
    dims, tol, coords, point_ptr, scale, W_ref, A = _reference(name)
    before = [a.copy() for a in (coords, point_ptr, scale)]
    ptr, index, weight = capi.offgrid_build(dev, coords, point_ptr, scale, dims, tol)
    assert _same(before, (coords, point_ptr, scale)), "an input array was written"
    n_grid = int(np.prod(dims))
    assert ptr.dtype == np.uint64 and index.dtype == np.uint64 and weight.dtype == np.float32
    assert ptr.size == scale.size + 1 and ptr[0] == 0 and ptr[-1] == index.size == weight.size
    assert np.all(np.diff(ptr.astype(np.int64)) >= 0) and index.max() < n_grid
    assert np.all(weight != 0.0) and np.all(np.isfinite(weight))
    W = _dense(ptr, index, weight, n_grid).astype(np.float64)
    counts = np.diff(point_ptr.astype(np.int64)).astype(np.float64)[:, None]
    bound = 32 * U * A + counts * 2.0 ** -41 + U * np.abs(W_ref)
    err = np.abs(W - W_ref)
    ratio = np.max(err[bound > 0] / bound[bound > 0])
    print(f"\noffgrid {name}: worst err / bound = {ratio:.3f}, {index.size} entries, largest |W| = {np.abs(W_ref).max():.3g}")
    assert np.all(err <= bound), ratio
    # no point: an empty row; outside the reference's support nothing is emitted
    assert ptr[1] == ptr[0]
    assert np.all(W[A == 0.0] == 0.0)
    # the point on the grid: exactly one entry, the scale
    on_grid = slice(int(ptr[7]), int(ptr[8]))
    n = np.floor(coords[-1] + 0.5).astype(np.int64)
    assert index[on_grid].tolist() == [n[0] + dims[0] * (n[1] + dims[1] * n[2])]
    assert abs(float(weight[on_grid][0]) - float(scale[7])) <= bound[7, index[on_grid][0]]
    # the stencil of the one-point element: (2R + 1) points per axis of more than one point, none thresholded away
    R = radius(tol)
    assert ptr[2] - ptr[1] == (2 * R + 1) ** (2 if dims[2] == 1 else 3)


# ---- 3. determinism ----------------------------------------------------------------------------------------------------
def test_build_is_bitwise_reproducible_and_order_independent(mods, dev):
    _, capi, _ = mods
    dims, tol, coords, point_ptr, scale, _, _ = _reference("3d")
    first = capi.offgrid_build(dev, coords, point_ptr, scale, dims, tol)
    again = capi.offgrid_build(dev, coords, point_ptr, scale, dims, tol)
    assert _same(first, again), "two builds of one input differ"
    rng = np.random.default_rng(4)
    shuffled = coords.copy()
    for e in range(scale.size):
        lo, hi = int(point_ptr[e]), int(point_ptr[e + 1])
        shuffled[lo:hi] = coords[lo:hi][rng.permutation(hi - lo)]
    assert not np.array_equal(shuffled, coords)
    assert _same(first, capi.offgrid_build(dev, shuffled, point_ptr, scale, dims, tol)), "the order of the points shows"
    ptr, index, _ = first
    for e in range(scale.size):
        row = index[int(ptr[e]):int(ptr[e + 1])].astype(np.int64)
        assert np.all(np.diff(row) > 0), e


# ---- 4. translation ----------------------------------------------------------------------------------------------------
def test_translation_by_whole_cells_moves_the_indices_only(mods, dev):
    _, capi, _ = mods
    dims, tol, shift = (40, 36, 34), 0.05, np.array([5, 3, -2])
    rng = np.random.default_rng(8)
    # offsets with ten fractional bits: u + shift is exact in float64, so both builds see the same offsets; nearest
    # indices 10 .. 14 keep every box (radius 7) inside the grid before and after the shift
    counts = [300, 1, 17]
    coords = rng.integers(10, 15, (sum(counts), 3)) + rng.integers(-500, 500, (sum(counts), 3)) / 1024.0
    point_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    scale = np.array([0.01, 0.7, 0.05], dtype=np.float32)
    ptr0, index0, weight0 = capi.offgrid_build(dev, coords, point_ptr, scale, dims, tol)
    ptr1, index1, weight1 = capi.offgrid_build(dev, coords + shift, point_ptr, scale, dims, tol)
    assert ptr0.tobytes() == ptr1.tobytes() and weight0.tobytes() == weight1.tobytes()
    moved = index0.astype(np.int64) + shift[0] + dims[0] * (shift[1] + dims[1] * shift[2])
    assert np.array_equal(moved, index1.astype(np.int64))
    assert ptr0[2] - ptr0[1] == 15 ** 3   # nothing clipped


# ---- 5. symmetry -------------------------------------------------------------------------------------------------------
def test_half_cell_offset_gives_mirror_weights(mods, dev):
    _, capi, _ = mods
    dims, i, y, z = (24, 20, 18), 11, 9, 8
    ptr, index, weight = capi.offgrid_build(dev, [[i + 0.5, y, z]], [0, 1], [0.73], dims, 0.05)
    W = _dense(ptr, index, weight, int(np.prod(dims)))[0].reshape(dims[2], dims[1], dims[0])
    assert index.size == 2 * 7 + 1 and np.count_nonzero(W[z, y]) == index.size   # on the grid in y and z: one line of x
    for k in range(7):
        a, b = W[z, y, i - k], W[z, y, i + 1 + k]
        assert a != 0.0 and a.tobytes() == b.tobytes(), (k, a, b)
    assert abs(float(W[z, y, i]) - 0.73 * 2 / np.pi) < 1e-6


# ---- 6. batching -------------------------------------------------------------------------------------------------------
def _box_bytes(coords, point_ptr, dims, tol):
    """scratch of each element's box: the nearest indices, dilated by R, clipped, padded to 256 cells, 20 bytes per cell"""
    R, out = radius(tol), []
    n = np.floor(coords + 0.5).astype(np.int64)
    for e in range(point_ptr.size - 1):
        pts = n[int(point_ptr[e]):int(point_ptr[e + 1])]
        cells = 0
        if len(pts):
            cells = 1
            for a in range(3):
                r = R if dims[a] > 1 else 0
                cells *= min(pts[:, a].max() + r, dims[a] - 1) - max(pts[:, a].min() - r, 0) + 1
        out.append((cells + 255) // 256 * 256 * CELL_BYTES)
    return out


def test_scratch_budget_changes_the_rounds_not_the_result(mods, dev):
    _, capi, _ = mods
    dims, tol, coords, point_ptr, scale, _, _ = _reference("3d")
    need = _box_bytes(coords, point_ptr, dims, tol)
    largest = max(need)
    # a budget of the largest box: the eight elements take several rounds, some of one box (elements 2 .. 5: any two of
    # their boxes exceed it) and some of two (the small boxes of the one-point elements 6 and 7 fit together)
    assert sum(need) > 3 * largest and need[6] + need[7] <= largest
    default = capi.offgrid_build(dev, coords, point_ptr, scale, dims, tol)
    tight = capi.offgrid_build(dev, coords, point_ptr, scale, dims, tol, scratch_bytes=largest)
    assert _same(default, tight)
    # only one box fits at a time: elements 2 .. 5 alone, every round one element
    lo, hi = int(point_ptr[2]), int(point_ptr[6])
    sub = (coords[lo:hi], point_ptr[2:7] - point_ptr[2], scale[2:6])
    assert all(a + b > largest for i, a in enumerate(need[2:6]) for b in need[2:6][i + 1:])
    one_by_one = capi.offgrid_build(dev, *sub, dims, tol, scratch_bytes=largest)
    assert _same(capi.offgrid_build(dev, *sub, dims, tol), one_by_one)
    # ... and their rows are the rows of the whole build
    ptr, index, weight = default
    a, b = int(ptr[2]), int(ptr[6])
    assert _same((ptr[2:7] - ptr[2], index[a:b], weight[a:b]), one_by_one)
    with pytest.raises(capi.KWaveError, match=rf"kw_status 4.*element {need.index(largest)}\b.*{largest} bytes"):
        capi.offgrid_build(dev, coords, point_ptr, scale, dims, tol, scratch_bytes=largest - 1)
    # the budget of kw_tuning is the default: a context whose tuning allows less refuses the same build
    t = capi.default_tuning()
    assert t.offgrid_scratch_bytes == 256 << 20
    d2 = capi.Device()
    try:
        t.offgrid_scratch_bytes = largest - 1
        capi.check(d2.L.kw_set_tuning(d2.ctx, capi.C.byref(t)))
        with pytest.raises(capi.KWaveError, match="kw_status 4"):
            capi.offgrid_build(d2, coords, point_ptr, scale, dims, tol)
    finally:
        d2.close()


# ---- 7. input checks ---------------------------------------------------------------------------------------------------
def test_bad_inputs_are_refused_by_name(mods, dev):
    _, capi, _ = mods
    dims = (24, 20, 18)
    coords = np.array([[5.0, 5.0, 5.0], [6.2, 7.1, 8.3], [7.0, 7.0, 7.0], [9.5, 3.25, 4.0]])
    point_ptr, scale = np.array([0, 1, 4], dtype=np.uint64), np.array([1.0, 0.5], dtype=np.float32)
    good = capi.offgrid_build(dev, coords, point_ptr, scale, dims, 0.05)
    assert good[0].size == 3

    def edit(row, col, value):
        c = coords.copy()
        c[row, col] = value
        return c

    bad = [
        ("element 1, point 1.*outside the grid", edit(2, 0, 23.5), point_ptr, 0.05),     # n_x = 24
        ("element 1, point 2.*outside the grid", edit(3, 2, -0.6), point_ptr, 0.05),     # n_z = -1
        ("element 0, point 0.*not finite", edit(0, 1, np.nan), point_ptr, 0.05),
        ("element 1, point 0.*not finite", edit(1, 2, np.inf), point_ptr, 0.05),
        ("not monotone at element 1", coords, np.array([0, 3, 2], dtype=np.uint64), 0.05),
        ("bli_tolerance", coords, point_ptr, 0.0),
        ("bli_tolerance", coords, point_ptr, 1.0),
        ("bli_tolerance", coords, point_ptr, -0.05),
        ("bli_tolerance", coords, point_ptr, float("nan")),
    ]
    for what, c, pp, tol in bad:
        with pytest.raises(capi.KWaveError, match="kw_status 1.*" + what):
            capi.offgrid_build(dev, c, pp, scale, dims, tol)
    # the fixed-point sum cannot overflow: |scale| summed over the points stays below 2^22
    with pytest.raises(capi.KWaveError, match="kw_status 1.*element 1.*2\\^22"):
        capi.offgrid_build(dev, coords, point_ptr, np.array([1.0, 2.0 ** 22 / 3], dtype=np.float32), dims, 0.05)
    assert _same(good, capi.offgrid_build(dev, coords, point_ptr, scale, dims, 0.05)), "a refused call left something behind"


def test_empty_builds(mods, dev):
    _, capi, _ = mods
    ptr, index, weight = capi.offgrid_build(dev, np.zeros((0, 3)), [0], [], (24, 20, 18))
    assert ptr.tolist() == [0] and index.size == 0 and weight.size == 0
    ptr, index, weight = capi.offgrid_build(dev, np.zeros((0, 3)), [0, 0, 0], [1.0, 2.0], (24, 20, 18))
    assert ptr.tolist() == [0, 0, 0] and index.size == 0 and weight.size == 0


# ---- 9. end to end -----------------------------------------------------------------------------------------------------
def test_disc_source_and_point_sensor_match_the_oracle(mods, dev, syn, orc):
    arrays, _, HostSolver = mods
    n, nt = 32, 40
    pr = syn.make_problem(n, heterogeneous=False, nonlinear=False, absorbing=False, source="none", nt=nt, pml_size=4)
    dx = float(np.asarray(pr["dx"]).ravel()[0])
    grid = arrays.Grid(n, n, n, dx, dx, dx)
    disc = arrays.disc_element(grid, (-2.3 * dx, 1.4 * dx, 0.6 * dx), 4.0 * dx, normal=(1.0, 0.5, 0.2))
    source = arrays.offgrid_elements(dev, grid, [disc])
    point = (np.array([[3.3 * dx, 2.6 * dx, -1.7 * dx]]), 1.0, 3)
    sensor = arrays.offgrid_elements(dev, grid, [point], normalise=True)
    assert source[0][0].size > 15 ** 3 and sensor[0][0].size == 15 ** 3
    assert abs(float(np.sum(sensor[0][1], dtype=np.float64)) - 1.0) < 0.02       # an interpolation: weights sum to ~1
    m_grid = disc[1] / dx ** 2
    assert abs(float(np.sum(source[0][1], dtype=np.float64)) / m_grid - 1.0) < 0.02
    t = np.arange(nt)[:, None]
    sig = (2.0e4 * np.sin(0.5 * t) * np.minimum(1.0, t / 6.0)).astype(np.float32)
    ds = arrays.weighted_source(source, sig)
    ds_sensor = arrays.weighted_sensor(sensor)
    pr.update(ds)
    pr.update(ds_sensor)
    pr["p_source_mode"] = np.array([[[2]]], dtype=np.uint64)
    exp = {k: v for k, v in pr.items() if not k.startswith("p_source_element_")}
    exp["p_source_input"] = arrays.expand_source(ds)
    exp["p_source_many"] = np.array([[[1]]], dtype=np.uint64)
    g = HostSolver(pr, p_elements=1)
    g.run(nt)
    g.finish()
    got = g.stream("p_elements")
    g.close()
    W = arrays.sensor_matrix(ds_sensor, n ** 3)
    o = orc.OracleSim(exp)
    ref = []
    for _ in range(nt):
        o.step()
        ref.append(W @ o.field("p").reshape(-1).astype(np.float64))
    o.close()
    ref = np.array(ref)
    assert got.shape == ref.shape == (nt, 1) and np.abs(ref).max() > 0
    err = rel_l2(got, ref)
    print(f"\noffgrid end to end: rel-L2 of the element series = {err:.3e}")
    assert err < TOL
