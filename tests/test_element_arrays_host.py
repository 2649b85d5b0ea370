"""Weighted transducer arrays, host side: the dataset builder (point-major transpose of the source, element-major sensor),
the slab partition of both CSR matrices, and the HDF5 round trip of the new datasets.  No GPU."""
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mods():
    import kwave_amd  # noqa: F401
    from kwave_amd import arrays, dist
    return arrays, dist


def _dense(ptr, col, w, ncols):
    ptr = np.asarray(ptr).reshape(-1).astype(np.int64)
    M = np.zeros((ptr.size - 1, ncols))
    np.add.at(M, (np.repeat(np.arange(ptr.size - 1), np.diff(ptr)), np.asarray(col).reshape(-1).astype(np.int64) - 1),
              np.asarray(w, dtype=np.float64).reshape(-1))
    return M


ELEMENTS = [(np.array([40, 7, 12]), np.array([0.5, 1.0, 0.25])),
            (np.array([12, 99]), np.array([2.0, -1.0])),
            (np.zeros(0, np.int64), np.zeros(0)),
            (np.array([7, 12, 3000]), np.array([0.1, 0.2, 0.3]))]


def test_source_builder_is_the_point_major_transpose(mods):
    arrays, _ = mods
    sig = np.arange(12, dtype=np.float32).reshape(3, 4)
    ds = arrays.weighted_source(ELEMENTS, sig)
    points = ds["p_source_index"].reshape(-1).astype(np.int64) - 1
    assert list(points) == [7, 12, 40, 99, 3000]
    assert ds["p_source_element_input"].shape == (1, 3, 4) and int(ds["p_source_flag"].ravel()[0]) == 3
    # point x element matrix == transpose of the element x point lists
    S = _dense(ds["p_source_element_ptr"], ds["p_source_element_index"], ds["p_source_element_weight"], 4)
    E = np.zeros((4, 5))
    for e, (idx, w) in enumerate(ELEMENTS):
        for i, wi in zip(idx, w):
            E[e, list(points).index(i)] += wi
    assert np.array_equal(S, E.T.astype(np.float32))
    # rows in element order: point 12 is covered by elements 1, 2, 4 (1-based)
    ptr = ds["p_source_element_ptr"].reshape(-1)
    assert list(ds["p_source_element_index"].reshape(-1)[ptr[1]:ptr[2]]) == [1, 2, 4]
    exp = arrays.expand_source(ds)
    assert exp.shape == (1, 3, 5)
    assert np.allclose(exp[0], sig.astype(np.float64) @ E, rtol=1e-6)


def test_sensor_builder_and_matrix(mods):
    arrays, _ = mods
    ds = arrays.weighted_sensor(ELEMENTS)
    assert list(ds["sensor_element_ptr"].reshape(-1)) == [0, 3, 5, 5, 8]
    assert list(ds["sensor_element_index"].reshape(-1)) == [41, 8, 13, 13, 100, 8, 13, 3001]
    W = arrays.sensor_matrix(ds, 4000)
    assert W.shape == (4, 4000) and W[0, 40] == 0.5 and W[3, 3000] == np.float32(0.3) and not W[2].any()


def test_partition_reproduces_the_global_csr(mods, syn):
    arrays, dist = mods
    pr = syn.make_problem(8, 8, 16, heterogeneous=False, nonlinear=False, absorbing=False, source="none", nt=4, pml_size=2)
    rng = np.random.default_rng(1)
    els = [(np.sort(rng.choice(8 * 8 * 16, 30, replace=False)), rng.uniform(0.1, 1.0, 30)) for _ in range(5)]
    src = arrays.weighted_source(els, rng.standard_normal((4, 5)).astype(np.float32))
    sen = arrays.weighted_sensor(els[:3] + [(np.arange(64, 128), np.ones(64))])  # the last lies wholly in plane 1
    pr.update(src)
    pr.update(sen)
    pr["p_source_mode"] = np.array([[[0]]], dtype=np.uint64)
    n = 8 * 8 * 16
    for nranks in (2, 4):
        S = np.zeros((n, 5))
        W = np.zeros((4, n))
        for rank in range(nranks):
            loc, info = dist.partition_problem(pr, rank, nranks)
            off = info["z0"] * 64
            assert np.array_equal(loc["p_source_element_input"], pr["p_source_element_input"])  # replicated
            pts = loc["p_source_index"].reshape(-1).astype(np.int64) - 1 + off
            S[pts] += _dense(loc["p_source_element_ptr"], loc["p_source_element_index"], loc["p_source_element_weight"], 5)
            assert loc["sensor_element_ptr"].size == 5  # all E rows stay
            cols = loc["sensor_element_index"].reshape(-1).astype(np.int64)
            assert np.all((cols >= 1) & (cols <= 64 * (info["z1"] - info["z0"])))
            W[:, off:off + 64 * (info["z1"] - info["z0"])] += _dense(loc["sensor_element_ptr"], cols, loc["sensor_element_weight"],
                                                                      64 * (info["z1"] - info["z0"]))
        gpts = src["p_source_index"].reshape(-1).astype(np.int64) - 1
        Sg = np.zeros((n, 5))
        Sg[gpts] = _dense(src["p_source_element_ptr"], src["p_source_element_index"], src["p_source_element_weight"], 5)
        assert np.array_equal(S, Sg)
        assert np.array_equal(W, _dense(sen["sensor_element_ptr"], sen["sensor_element_index"], sen["sensor_element_weight"], n))


def test_h5io_writes_and_reads_the_element_datasets(mods, syn, tmp_path):
    arrays, _ = mods
    from kwave_amd import h5io
    if not os.path.exists(h5io.H5_LIB_PATH):
        pytest.skip("HDF5 component not built")
    pr = syn.make_problem(8, heterogeneous=False, nonlinear=False, absorbing=False, source="none", nt=4, pml_size=2)
    pr.update(arrays.weighted_source(ELEMENTS, np.ones((4, 4), np.float32)))
    pr.update(arrays.weighted_sensor(ELEMENTS))
    path = str(tmp_path / "in.h5")
    h5io.write_input_file(pr, path)
    back = h5io.read_problem(path)
    for name in ("p_source_element_input", "p_source_element_ptr", "p_source_element_index", "p_source_element_weight",
                 "sensor_element_ptr", "sensor_element_index", "sensor_element_weight"):
        assert name in back, name
        assert back[name].dtype == pr[name].dtype, name
        assert np.array_equal(back[name].reshape(-1), pr[name].reshape(-1)), name
    assert h5io.dataset_info(path, "p_source_element_input")[0] == (4, 4, 1)
