"""Weighted transducer arrays for the velocity, host side: the dataset builder and its expansion, the slab partition of
the shared CSR, the HDF5 round trip of the new datasets, the option fields of the host library, the create-time checks
(Parameters::init refuses before a device is opened), and those checks again in a stand-alone host program built with
AddressSanitizer and UBSan.  No GPU."""
import ctypes
import os
import re
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


def test_velocity_source_builder_round_trips(mods):
    arrays, _ = mods
    sx = np.arange(12, dtype=np.float32).reshape(3, 4)
    sz = -np.arange(20, dtype=np.float32).reshape(5, 4)          # another number of steps
    ds = arrays.weighted_velocity_source(ELEMENTS, signals_x=sx, signals_z=sz)
    assert list(ds["u_source_index"].reshape(-1).astype(np.int64) - 1) == [7, 12, 40, 99, 3000]
    assert [int(ds[f"u{c}_source_flag"].ravel()[0]) for c in "xyz"] == [3, 0, 5]
    assert int(ds["u_source_many"].ravel()[0]) == 1
    assert "uy_source_element_input" not in ds and ds["uz_source_element_input"].shape == (1, 5, 4)
    # the CSR is the one weighted_source builds for the pressure
    ps = arrays.weighted_source(ELEMENTS, sx)
    for part in ("ptr", "index", "weight"):
        assert np.array_equal(ds["u_source_element_" + part], ps["p_source_element_" + part])
    S = _dense(ds["u_source_element_ptr"], ds["u_source_element_index"], ds["u_source_element_weight"], 4)
    exp = arrays.expand_velocity_source(ds)
    assert sorted(exp) == ["ux_source_input", "uz_source_input"]
    assert exp["ux_source_input"].shape == (1, 3, 5) and exp["uz_source_input"].shape == (1, 5, 5)
    assert np.allclose(exp["ux_source_input"][0], sx.astype(np.float64) @ S.T, rtol=1e-6)
    assert np.allclose(exp["uz_source_input"][0], sz.astype(np.float64) @ S.T, rtol=1e-6)
    assert np.array_equal(exp["ux_source_input"], arrays.expand_source(ps))
    with pytest.raises(ValueError):
        arrays.weighted_velocity_source(ELEMENTS)
    with pytest.raises(ValueError):
        arrays.weighted_velocity_source(ELEMENTS, signals_y=np.zeros((3, 5), np.float32))


def test_partition_reproduces_the_global_velocity_csr(mods, syn):
    arrays, dist = mods
    pr = syn.make_problem(8, 8, 16, heterogeneous=False, nonlinear=False, absorbing=False, source="none", nt=4, pml_size=2)
    rng = np.random.default_rng(1)
    els = [(np.sort(rng.choice(8 * 8 * 16, 30, replace=False)), rng.uniform(0.1, 1.0, 30)) for _ in range(5)]
    src = arrays.weighted_velocity_source(els, signals_x=rng.standard_normal((4, 5)).astype(np.float32),
                                          signals_y=rng.standard_normal((3, 5)).astype(np.float32))
    pr.update(src)
    pr["u_source_mode"] = np.array([[[0]]], dtype=U64)
    n = 8 * 8 * 16
    gpts = src["u_source_index"].reshape(-1).astype(np.int64) - 1
    Sg = np.zeros((n, 5))
    Sg[gpts] = _dense(src["u_source_element_ptr"], src["u_source_element_index"], src["u_source_element_weight"], 5)
    for nranks in (2, 4):
        S = np.zeros((n, 5))
        for rank in range(nranks):
            loc, info = dist.partition_problem(pr, rank, nranks)
            for c in "xy":
                assert np.array_equal(loc[f"u{c}_source_element_input"], pr[f"u{c}_source_element_input"])  # replicated
            pts = loc["u_source_index"].reshape(-1).astype(np.int64) - 1 + info["z0"] * 64
            assert loc["u_source_element_ptr"].size == pts.size + 1
            S[pts] += _dense(loc["u_source_element_ptr"], loc["u_source_element_index"], loc["u_source_element_weight"], 5)
        assert np.array_equal(S, Sg)


def test_h5io_writes_and_reads_the_velocity_element_datasets(mods, syn, tmp_path):
    arrays, _ = mods
    from kwave_amd import h5io
    if not os.path.exists(h5io.H5_LIB_PATH):
        pytest.skip("HDF5 component not built")
    pr = syn.make_problem(8, heterogeneous=False, nonlinear=False, absorbing=False, source="none", nt=4, pml_size=2)
    pr.update(arrays.weighted_velocity_source(ELEMENTS, signals_x=np.ones((4, 4), np.float32), signals_z=np.ones((2, 4), np.float32)))
    pr["u_source_mode"] = np.array([[[1]]], dtype=U64)
    path = str(tmp_path / "in.h5")
    h5io.write_input_file(pr, path)
    back = h5io.read_problem(path)
    for name in ("ux_source_element_input", "uz_source_element_input", "u_source_element_ptr", "u_source_element_index",
                 "u_source_element_weight"):
        assert name in back, name
        assert back[name].dtype == pr[name].dtype, name
        assert np.array_equal(back[name].reshape(-1), pr[name].reshape(-1)), name
    assert "uy_source_element_input" not in back
    assert h5io.dataset_info(path, "uz_source_element_input")[0] == (4, 2, 1)


def test_option_fields_follow_the_header():
    """solver.Options mirrors kwh_options field by field: the new flags sit at the end of both, in the same order, and
    the command-line program and the slab launcher know them"""
    import kwave_amd  # noqa: F401
    from kwave_amd import run_slab, solver
    header = open(os.path.join(ROOT, "include", "kwave_host.h")).read()
    body = header[header.index("typedef struct kwh_options"):header.index("} kwh_options;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = [m.group(1) for m in re.finditer(r"(\w+)(?:\[\d+\])?\s*;", body)]
    py_fields = [f[0] for f in solver.Options._fields_]
    assert c_fields[-3:] == ["p_elements", "u_elements", "u_non_staggered_elements"]
    assert [f for f in py_fields if f not in ("pad_", "reserved_")][-3:] == c_fields[-3:]
    o = solver.Options()
    o.u_elements, o.u_non_staggered_elements = 1, 1
    assert ctypes.sizeof(solver.Options) % 8 == 0
    assert {"u_elements", "u_non_staggered_elements"} <= set(run_slab.STREAM_FLAGS)
    main = open(os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host", "h5", "main.cpp")).read()
    assert '"--u_elements"' in main and '"--u_non_staggered_elements"' in main


# ---- create-time checks: Parameters::init runs before the device is opened, so a refusal needs no GPU -------------------
def _problem(syn, arrays):
    pr = syn.make_problem(16, heterogeneous=False, nonlinear=False, absorbing=False, source="none", nt=30, pml_size=2)
    rng = np.random.default_rng(3)
    els = [(np.sort(rng.choice(16 ** 3, 20, replace=False)), rng.uniform(0.2, 1.0, 20)) for _ in range(5)]
    pr.update(arrays.weighted_velocity_source(els, signals_x=np.ones((20, 5), np.float32), signals_z=np.ones((12, 5), np.float32)))
    pr["u_source_mode"] = np.array([[[2]]], dtype=U64)
    pr.update(arrays.weighted_sensor(els[:3]))
    return pr


REFUSALS = [
    ("uy_source_element_input: present, but uy_source_flag is 0", lambda pr, n: {"uy_source_element_input": np.zeros((1, 20, 5), np.float32)}),
    ("ux_source_input and ux_source_element_input cannot both be present", lambda pr, n: {"ux_source_input": np.zeros((1, 20, n), np.float32)}),
    ("uy_source_element_input: missing, although uy_source_flag is above 0", lambda pr, n: {"uy_source_flag": np.array([[[20]]], dtype=U64),
                                               "uy_source_input": np.zeros((1, 20, n), np.float32)}),
    ("u_source_many: must be 1 with", lambda pr, n: {"u_source_many": np.array([[[0]]], dtype=U64)}),
    ("uz_source_element_input: has 4 elements, but ux_source_element_input has 5", lambda pr, n: {"uz_source_element_input": np.zeros((1, 12, 4), np.float32)}),
    ("weighted velocity source cannot be combined with transducer_source_flag", lambda pr, n: {"transducer_source_flag": np.array([[[5]]], dtype=U64),
                                              "transducer_source_input": np.zeros((1, 1, 64), np.float32),
                                              "delay_mask": np.ones((1, 1, n), dtype=U64)}),
    ("u_source_element_ptr: has [0-9]+ entries, expected", lambda pr, n: {"u_source_element_ptr": pr["u_source_element_ptr"].reshape(-1)[:-1].reshape(1, 1, -1)}),
    ("u_source_element_index: entry 0 = [0-9]+ lies outside 1..5", lambda pr, n: {"u_source_element_index": pr["u_source_element_index"] + U64(5)}),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_malformed_velocity_elements_are_refused_without_a_device(mods, syn, case):
    arrays, _ = mods
    from kwave_amd import capi
    from kwave_amd.solver import HOST_LIB_PATH, HostSolver
    if not os.path.exists(HOST_LIB_PATH):
        pytest.skip("host library not built")
    pr = _problem(syn, arrays)
    message, edit = REFUSALS[case]
    pr.update(edit(pr, pr["u_source_index"].size))
    with pytest.raises(capi.KWaveError, match=message):
        HostSolver(pr, u_elements=1)


@pytest.mark.parametrize("flag", ["u_elements", "u_non_staggered_elements"])
def test_built_host_library_reads_the_new_option_fields(mods, syn, flag):
    """The header text alone would not show a library built from a stale kwh_options: with the sensor datasets missing, the
    built library must refuse each new flag on its own, by name (a library that does not read the field accepts the input
    and goes on to open a device)."""
    arrays, _ = mods
    from kwave_amd import capi
    from kwave_amd.solver import HOST_LIB_PATH, HostSolver
    if not os.path.exists(HOST_LIB_PATH):
        pytest.skip("host library not built")
    pr = {k: v for k, v in _problem(syn, arrays).items() if not k.startswith("sensor_element_")}
    with pytest.raises(capi.KWaveError, match=f"--{flag} needs the datasets sensor_element_ptr"):
        HostSolver(pr, **{flag: 1})


EXPECTED = {
    "good": "ok E=3 nnz=5 sensor=2 shifted=1",
    "flag0": "uy_source_element_input", "both": "ux_source_input", "mixed": "uy_source_element_input",
    "many": "u_source_many", "elements": "uz_source_element_input", "transducer": "transducer_source_flag",
    "points": "u_source_index: more than 2^32 - 1 points", "entries": "u_source_element_index: more than 2^32 - 1 entries",
    "monotone": "u_source_element_ptr", "last": "u_source_element_ptr", "column": "u_source_element_index",
    "zero": "u_source_element_index", "missing": "u_source_element_ptr", "grid": "sensor_element_index",
}


def test_element_array_checks_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/element_arrays_check.cpp: Parameters::init on an in-memory input, the good one and each bad one
    (among them the two a real array cannot reach: more than 2^32 - 1 points or entries), in a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "element_arrays_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "element_arrays_check.cpp"), os.path.join(host, "Parameters.cpp"),
           os.path.join(host, "CompressHelper.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
    lines = dict(line.split(": ", 1) for line in r.stdout.strip().splitlines())
    assert sorted(lines) == sorted(EXPECTED)
    for case, what in EXPECTED.items():
        assert what in lines[case], (case, lines[case])
