"""Per-entry time delays of the weighted transducer arrays, host side: the builders carry the delays through the
point-major transpose, focus_delays against its formula, the slab partition, the HDF5 round trip, and a stand-alone host
program built with AddressSanitizer and UBSan that exercises the regrouping of a delayed sensor and the create-time
checks of Parameters::init.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

U64 = np.uint64


@pytest.fixture(scope="module")
def mods():
    import kwave_amd  # noqa: F401
    from kwave_amd import arrays, dist
    return arrays, dist


ELEMENTS = [(np.array([40, 7, 12]), np.array([0.5, 1.0, 0.25])),
            (np.array([12, 99]), np.array([2.0, -1.0])),
            (np.zeros(0, np.int64), np.zeros(0)),
            (np.array([7, 12, 3000]), np.array([0.1, 0.2, 0.3]))]
DELAYS = [np.array([3, 0, 1]), np.array([2, 5]), np.zeros(0, np.int64), np.array([4, 0, 6])]


def test_builders_carry_delays_through_the_transpose(mods):
    arrays, _ = mods
    sig = np.arange(12, dtype=np.float32).reshape(3, 4)
    plain, ds = arrays.weighted_source(ELEMENTS, sig), arrays.weighted_source(ELEMENTS, sig, delays=DELAYS)
    assert "p_source_element_delay" not in plain
    for name, a in plain.items():
        assert np.array_equal(ds[name], a) and ds[name].dtype == a.dtype, name
    d = ds["p_source_element_delay"]
    assert d.dtype == U64 and d.shape == ds["p_source_element_index"].shape
    # every (point, element) entry carries the delay its element gave that point
    want = {(int(i), e): int(x) for e, ((idx, _), dl) in enumerate(zip(ELEMENTS, DELAYS)) for i, x in zip(idx, dl)}
    points = ds["p_source_index"].reshape(-1).astype(np.int64) - 1
    ptr = ds["p_source_element_ptr"].reshape(-1).astype(np.int64)
    col = ds["p_source_element_index"].reshape(-1).astype(np.int64) - 1
    got = {(int(points[k]), int(col[j])): int(d.reshape(-1)[j]) for k in range(points.size) for j in range(ptr[k], ptr[k + 1])}
    assert got == want
    vs = arrays.weighted_velocity_source(ELEMENTS, signals_x=sig, signals_z=sig[:2], delays=DELAYS)
    assert np.array_equal(vs["u_source_element_delay"], d)
    assert "u_source_element_delay" not in arrays.weighted_velocity_source(ELEMENTS, signals_x=sig)
    ss = arrays.weighted_sensor(ELEMENTS, delays=DELAYS)
    assert list(ss["sensor_element_delay"].reshape(-1)) == [3, 0, 1, 2, 5, 4, 0, 6] and ss["sensor_element_delay"].dtype == U64
    for name, a in arrays.weighted_sensor(ELEMENTS).items():
        assert np.array_equal(ss[name], a), name
    for bad in (DELAYS[:3], [np.array([1, 2])] + DELAYS[1:], [np.array([0, -1, 0])] + DELAYS[1:],
                [np.array([0, 65536, 0])] + DELAYS[1:], [np.array([0, 0.5, 0])] + DELAYS[1:]):
        with pytest.raises(ValueError):
            arrays.weighted_sensor(ELEMENTS, delays=bad)


def test_expansions_honour_the_delays(mods):
    arrays, _ = mods
    rng = np.random.default_rng(4)
    sig = rng.standard_normal((3, 4)).astype(np.float32)
    ds = arrays.weighted_source(ELEMENTS, sig, delays=DELAYS)
    exp = arrays.expand_source(ds)
    points = list(ds["p_source_index"].reshape(-1).astype(np.int64) - 1)
    assert exp.shape == (1, 3 + 6, 5)
    ref = np.zeros((9, 5))
    for e, ((idx, w), dl) in enumerate(zip(ELEMENTS, DELAYS)):
        for i, wi, di in zip(idx, w, dl):
            ref[di:di + 3, points.index(i)] += np.float32(wi).astype(np.float64) * sig[:, e]
    assert np.allclose(exp[0], ref, rtol=1e-6, atol=1e-7)
    vs = arrays.weighted_velocity_source(ELEMENTS, signals_x=sig, signals_z=sig[:2], delays=DELAYS)
    ev = arrays.expand_velocity_source(vs)
    assert np.array_equal(ev["ux_source_input"], exp) and ev["uz_source_input"].shape == (1, 2 + 6, 5)
    # without delays nothing changes; with them the sensor is no single matrix
    assert np.array_equal(arrays.expand_source(arrays.weighted_source(ELEMENTS, sig))[0],
                          (sig.astype(np.float64) @ _dense_source(arrays, sig).T).astype(np.float32))
    ss = arrays.weighted_sensor(ELEMENTS, delays=DELAYS)
    with pytest.raises(ValueError, match="sensor_element_delay"):
        arrays.sensor_matrix(ss, 4000)
    mats = arrays.delayed_sensor_matrices(ss, 4000)
    assert sorted(mats) == [0, 1, 2, 3, 4, 5, 6]
    assert np.array_equal(sum(mats.values()), arrays.sensor_matrix(arrays.weighted_sensor(ELEMENTS), 4000))
    assert mats[5][1, 99] == -1.0 and np.count_nonzero(mats[5]) == 1


def _dense_source(arrays, sig):
    ds = arrays.weighted_source(ELEMENTS, sig)
    ptr = ds["p_source_element_ptr"].reshape(-1).astype(np.int64)
    S = np.zeros((ptr.size - 1, 4))
    np.add.at(S, (np.repeat(np.arange(ptr.size - 1), np.diff(ptr)), ds["p_source_element_index"].reshape(-1).astype(np.int64) - 1),
              ds["p_source_element_weight"].reshape(-1).astype(np.float64))
    return S


def test_focus_delays_follow_the_formula(mods):
    arrays, _ = mods
    grid = arrays.Grid(32, 16, 8, 1e-3, 1e-3, 1e-3)
    c, dt = 1500.0, 1e-7
    # a line array of three elements of four points each along x, at y index 3, z index 2
    els = [(np.array([x + 32 * (3 + 16 * 2) for x in range(4 * e + 2, 4 * e + 6)]), np.ones(4)) for e in range(3)]
    focus = (2e-3, 4e-3, 1e-3)
    r = [np.sqrt(((np.arange(4 * e + 2, 4 * e + 6) - 16) * 1e-3 - focus[0]) ** 2 + ((3 - 8) * 1e-3 - focus[1]) ** 2 +
                 ((2 - 4) * 1e-3 - focus[2]) ** 2) for e in range(3)]
    whole = arrays.focus_delays(grid, els, focus, c, dt)
    r_max = max(x.max() for x in r)
    for e in range(3):
        assert whole[e].dtype == np.int64 and np.array_equal(whole[e], np.round((r_max - r[e]) / (c * dt)).astype(np.int64))
    flat = np.concatenate(whole)
    assert flat.min() == 0 and np.all(flat >= 0) and np.count_nonzero(flat == 0) >= 1
    assert flat.max() > 10                                      # millimetres at 0.15 mm per step
    per = arrays.focus_delays(grid, els, focus, c, dt, per_element=True)
    for e in range(3):
        assert np.array_equal(per[e], np.round((r[e].max() - r[e]) / (c * dt)).astype(np.int64))
        assert per[e].min() == 0
    # they are what the builders take
    ds = arrays.weighted_sensor(els, delays=whole)
    assert np.array_equal(ds["sensor_element_delay"].reshape(-1).astype(np.int64), flat)


def _delayed_problem(syn, arrays):
    pr = syn.make_problem(8, 8, 16, heterogeneous=False, nonlinear=False, absorbing=False, source="none", nt=4, pml_size=2)
    rng = np.random.default_rng(1)
    n = 8 * 8 * 16
    els = [(np.sort(rng.choice(n, 30, replace=False)), rng.uniform(0.1, 1.0, 30)) for _ in range(5)]
    delays = [rng.integers(0, 9, 30) for _ in range(5)]
    pr.update(arrays.weighted_source(els, rng.standard_normal((4, 5)).astype(np.float32), delays=delays))
    pr["p_source_mode"] = np.array([[[0]]], dtype=U64)
    pr.update(arrays.weighted_velocity_source(els[:3], signals_x=rng.standard_normal((3, 3)).astype(np.float32),
                                              delays=[d + 1 for d in delays[:3]]))
    pr["u_source_mode"] = np.array([[[0]]], dtype=U64)
    pr.update(arrays.weighted_sensor(els, delays=delays[::-1]))
    return pr, n


def _triples(index1, ptr, col1, w, d, offset=0):
    """the delayed CSR as a sorted list of (global row key, column, weight, delay)"""
    ptr = np.asarray(ptr).reshape(-1).astype(np.int64)
    rows = np.repeat(np.asarray(index1).reshape(-1).astype(np.int64) - 1 + offset, np.diff(ptr))
    return sorted(zip(rows.tolist(), np.asarray(col1).reshape(-1).astype(np.int64).tolist(),
                      np.asarray(w).reshape(-1).tolist(), np.asarray(d).reshape(-1).astype(np.int64).tolist()))


def test_partition_reproduces_the_global_delayed_csr(mods, syn):
    arrays, dist = mods
    pr, n = _delayed_problem(syn, arrays)
    whole = {q: _triples(pr[q + "_source_index"], pr[q + "_source_element_ptr"], pr[q + "_source_element_index"],
                         pr[q + "_source_element_weight"], pr[q + "_source_element_delay"]) for q in "pu"}
    n_el = pr["sensor_element_ptr"].size - 1
    sensor = _triples(np.arange(1, n_el + 1), pr["sensor_element_ptr"], pr["sensor_element_index"],
                      pr["sensor_element_weight"], pr["sensor_element_delay"])
    for nranks in (2, 4):
        got = {"p": [], "u": []}
        got_sensor = []
        for rank in range(nranks):
            loc, info = dist.partition_problem(pr, rank, nranks)
            for q in "pu":
                assert loc[q + "_source_element_delay"].dtype == U64
                assert loc[q + "_source_element_delay"].size == loc[q + "_source_element_index"].size
                got[q] += _triples(loc[q + "_source_index"], loc[q + "_source_element_ptr"], loc[q + "_source_element_index"],
                                   loc[q + "_source_element_weight"], loc[q + "_source_element_delay"], offset=info["z0"] * 64)
                # every rank keeps the source active for the same steps: the largest delay of the whole array
                assert int(loc[q + "_source_element_delay_max"].ravel()[0]) == int(pr[q + "_source_element_delay"].max())
            assert loc["sensor_element_delay"].dtype == U64 and loc["sensor_element_ptr"].size == n_el + 1
            part = _triples(np.arange(1, n_el + 1), loc["sensor_element_ptr"], loc["sensor_element_index"],
                            loc["sensor_element_weight"], loc["sensor_element_delay"])
            got_sensor += [(e, c + info["z0"] * 64, w, d) for e, c, w, d in part]
        assert sorted(got["p"]) == whole["p"] and sorted(got["u"]) == whole["u"]
        assert sorted(got_sensor) == sensor


def test_h5io_writes_and_reads_the_delay_datasets(mods, syn, tmp_path):
    arrays, _ = mods
    from kwave_amd import h5io
    if not os.path.exists(h5io.H5_LIB_PATH):
        pytest.skip("HDF5 component not built")
    pr, _ = _delayed_problem(syn, arrays)
    path = str(tmp_path / "in.h5")
    h5io.write_input_file(pr, path)
    back = h5io.read_problem(path)
    for name in ("p_source_element_delay", "u_source_element_delay", "sensor_element_delay"):
        assert name in back, name
        assert back[name].dtype == U64, name
        assert np.array_equal(back[name].reshape(-1), pr[name].reshape(-1)), name
        assert h5io.dataset_info(path, name)[0] == (pr[name].size, 1, 1)
    assert "p_source_element_delay_max" not in back


EXPECTED = {
    # {2, 0, 2, 0, 1}: by delay, CSR order inside a group; an empty row; one group; every entry a group of its own
    "mixed": "ok order=1,3,4,0,2,5,6,7,10,9,8 gptr=0,2,3,5,8,9,10,11 gdelay=0,1,2,4,1,2,3 egp=0,3,3,4,7 chunks=0,1,2,3,4,5,6,7",
    "empty": "ok order= gptr=0 gdelay= egp=0,0,0 chunks=0",
    "long": "ok stable=1 gptr=0,1250,2500 gdelay=0,1 egp=0,2,2 chunks=0,2,4",
    "good": "ok delayed=111 max=4,7,6 length=14,27,0,19",
    "none": "ok delayed=000 max=0,0,0 length=10,20,0,12",
    "capped": "ok delayed=111 max=4,15,6 length=14,30,0,27",
    "p_length": "p_source_element_delay: has 4 entries, but p_source_element_index has 5",
    "u_length": "u_source_element_delay: has 6 entries, but u_source_element_index has 5",
    "s_length": "sensor_element_delay: has 2 entries, but sensor_element_index has 3",
    "p_high": "p_source_element_delay: entry 1 = 65536 lies above the largest delay 65535",
    "u_high": "u_source_element_delay: entry 4 = 1099511627776 lies above the largest delay 65535",
    "s_high": "sensor_element_delay: entry 2 = 65536 lies above the largest delay 65535",
    "s_top": "ok delayed=111 max=4,7,65535 length=14,27,0,19",
    "p_lone": "p_source_element_delay: present without p_source_element_index",
    "u_lone": "u_source_element_delay: present without u_source_element_index",
    "s_lone": "sensor_element_delay: present without sensor_element_index",
    "s_unused": "ok delayed=110 max=4,7,0 length=14,27,0,19",
    "horizon": "ok delayed=111 max=9,8,6 length=19,28,0,20",
    "horizon_low": "p_source_element_delay_max: 3 lies outside 4..65535",
    "horizon_lone": "u_source_element_delay_max: present without u_source_element_delay",
}


def test_regrouping_and_delay_checks_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/element_delay_check.cpp: ElementCsr::regroup and Parameters::init on in-memory inputs, in a stand-alone
    program that runs directly"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "element_delay_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "element_delay_check.cpp"), os.path.join(host, "Parameters.cpp"),
           os.path.join(host, "CompressHelper.cpp"), os.path.join(host, "ElementGroups.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
    lines = dict(line.split(": ", 1) for line in r.stdout.strip().splitlines())
    assert sorted(lines) == sorted(EXPECTED)
    for case, what in EXPECTED.items():
        assert lines[case].startswith(what), (case, lines[case])
