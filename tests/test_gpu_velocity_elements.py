"""Weighted transducer arrays for the velocity, on the GPU: kw_element_source_rows and kw_sample_elements_multi alone
against the one-field kernels (bit for bit) and fp64, the weighted velocity source against the expanded one (CPU oracle
and GPU), u*_elements against W @ u_raw, the output file and a checkpointed restart, a slab run, and the create-time
checks of the new datasets.

Element-wise bound of both kernels: |gpu - fp64| <= (k + 1) 2^-24 sum_j |w_j x_j|, k = the row's entry count."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_l2

sys.path.insert(0, ROOT)
from gpu_buffers import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TOL = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64


@pytest.fixture(scope="module")
def mods():
    import kwave_amd  # noqa: F401
    from kwave_amd import arrays, capi, h5io
    from kwave_amd.solver import HostSolver
    return arrays, capi, h5io, HostSolver


def _scalar(v):
    return np.array([[[v]]], dtype=U64)


def _bound_check(gpu, ptr, cols, w, x):
    k = np.diff(ptr)
    rows = np.repeat(np.arange(k.size), k)
    terms = w.astype(np.float64) * x.astype(np.float64)[cols]
    ref = np.bincount(rows, weights=terms, minlength=k.size)
    mag = np.bincount(rows, weights=np.abs(terms), minlength=k.size)
    err = np.abs(gpu.astype(np.float64) - ref)
    assert np.all(err <= (k + 1) * U * mag), (np.max(err / np.maximum((k + 1) * U * mag, 1e-300)))
    assert np.all(gpu[k == 0] == 0.0)


def _pointers(values):
    return (C.c_void_p * len(values))(*values)


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 3000, 64, 1024, 1025, 0, 7, 50000]   # the edge cases of the one-field kernel test


def _csr(rng, ncols):
    ptr = np.zeros(len(LENGTHS) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(LENGTHS)
    return ptr, rng.integers(0, ncols, ptr[-1]), rng.uniform(-1.5, 1.5, ptr[-1]).astype(np.float32)


def test_sample_elements_multi_equals_the_one_field_kernel(mods):
    _, capi, _, _ = mods
    rng = np.random.default_rng(17)
    n_grid, n_el = 40000, len(LENGTHS)
    ptr, cols, w = _csr(rng, n_grid)
    host_fields = [rng.standard_normal(n_grid).astype(np.float32) for _ in range(3)]
    cp = capi.element_chunk_ptr(ptr)
    n_chunks = int(cp[-1])
    d = capi.Device()
    try:
        fields = [Guarded(d, f) for f in host_fields]
        csr = [Guarded(d, ptr.astype(np.uint32), dtype=np.uint32), Guarded(d, capi.csr_entries(cols, w), dtype=np.uint32),
               Guarded(d, cp, dtype=np.uint32)]
        single = []
        part1 = Guarded(d, np.zeros(n_chunks, np.float32))
        for f in fields:
            out = Guarded(d, np.full(n_el, np.nan, np.float32))
            capi.check(d.L.kw_sample_elements(d.ctx, out.ptr, f.ptr, csr[0].ptr, csr[1].ptr, n_el, int(ptr[-1]), csr[2].ptr,
                                              n_chunks, part1.ptr))
            single.append(out.read())
        for nf in (1, 2, 3):
            part = Guarded(d, np.full(nf * n_chunks, np.nan, np.float32))
            runs = []
            for _ in range(2):
                outs = [Guarded(d, np.full(n_el, np.nan, np.float32)) for _ in range(nf)]
                capi.check(d.L.kw_sample_elements_multi(d.ctx, nf, _pointers([o.ptr for o in outs]),
                                                        _pointers([f.ptr for f in fields[:nf]]), csr[0].ptr, csr[1].ptr, n_el,
                                                        int(ptr[-1]), csr[2].ptr, n_chunks, part.ptr))
                runs.append([o.read() for o in outs])
            for f in range(nf):
                assert np.array_equal(runs[0][f].view(np.uint32), runs[1][f].view(np.uint32)), "two launches differ"
                assert np.array_equal(runs[0][f].view(np.uint32), single[f].view(np.uint32)), (nf, f)
                _bound_check(runs[0][f], ptr, cols, w, host_fields[f])
            assert not np.isnan(part.read()).any()  # guard bands intact, every partial written
        for g, h in zip(fields + csr, host_fields + [ptr.astype(np.uint32), capi.csr_entries(cols, w), cp]):
            assert np.array_equal(g.read().view(np.uint8), np.ascontiguousarray(h).view(np.uint8)), "input changed"
    finally:
        d.close()


def test_element_source_rows_equals_the_one_row_kernel(mods):
    _, capi, _, _ = mods
    rng = np.random.default_rng(19)
    n_el, nt, t = 6, 5, 3
    # every point is covered by 0 .. 3 elements, plus one long row; more than one block (703 points)
    lengths = list(rng.integers(0, 4, 700)) + [0, 1, 300]
    n_pts = len(lengths)
    ptr = np.zeros(n_pts + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(lengths)
    cols = np.concatenate([rng.choice(n_el, size=k, replace=k > n_el) for k in lengths]).astype(np.int64)
    w = rng.uniform(-2.0, 2.0, ptr[-1]).astype(np.float32)
    host_sig = [rng.standard_normal((nt, n_el)).astype(np.float32) for _ in range(3)]
    d = capi.Device()
    try:
        sigs = [Guarded(d, s) for s in host_sig]
        csr = [Guarded(d, ptr.astype(np.uint32), dtype=np.uint32), Guarded(d, capi.csr_entries(cols, w), dtype=np.uint32)]
        single = []
        for s in sigs:
            row = Guarded(d, np.full(n_pts, np.nan, np.float32))
            capi.check(d.L.kw_element_source_row(d.ctx, row.ptr, s.ptr, csr[0].ptr, csr[1].ptr, n_pts, n_el, t))
            single.append(row.read())
        # x only; x and z; all three.  A skipped component gets NULL for its row and its input, and a NaN-filled buffer
        # that no pointer leads to must still hold NaN afterwards
        for active in ((0,), (0, 2), (0, 1, 2)):
            runs = []
            for _ in range(2):
                rows = [Guarded(d, np.full(n_pts, np.nan, np.float32)) for _ in range(3)]
                capi.check(d.L.kw_element_source_rows(
                    d.ctx, _pointers([rows[c].ptr if c in active else None for c in range(3)]),
                    _pointers([sigs[c].ptr if c in active else None for c in range(3)]), csr[0].ptr, csr[1].ptr, n_pts, n_el, t))
                runs.append([r.read() for r in rows])
            for c in range(3):
                if c not in active:
                    assert np.isnan(runs[0][c]).all(), (active, c)
                    continue
                assert np.array_equal(runs[0][c].view(np.uint32), runs[1][c].view(np.uint32)), "two launches differ"
                assert np.array_equal(runs[0][c].view(np.uint32), single[c].view(np.uint32)), (active, c)
                _bound_check(runs[0][c], ptr, cols, w, host_sig[c][t])
        for g, h in zip(sigs + csr, host_sig + [ptr.astype(np.uint32), capi.csr_entries(cols, w)]):
            assert np.array_equal(g.read().view(np.uint8), np.ascontiguousarray(h).view(np.uint8)), "input changed"
    finally:
        d.close()


# ---- problems ----------------------------------------------------------------------------------------------------------
def _elements(rng, dims, n_el, per, lo=(6, 6, 6), span=10):
    """n_el overlapping elements of `per` points each, drawn from one span^3 box of the (nx, ny, nz) grid"""
    nx, ny, nz = dims
    zs = range(lo[2], min(lo[2] + span, nz)) if nz > 1 else [0]
    pool = np.array([x + nx * (y + ny * z) for z in zs for y in range(lo[1], lo[1] + span) for x in range(lo[0], lo[0] + span)])
    return [(np.sort(rng.choice(pool, per, replace=False)), rng.uniform(0.2, 1.0, per)) for _ in range(n_el)]


NT_X, NT_Z = 20, 12   # the z component runs out mid-run, before the x component


def _weighted(syn, arrays, mode, n=32, nt=30, seed=3, lo=(6, 6, 6)):
    """five overlapping elements driving ux (20 steps) and uz (12 steps); uy is not driven"""
    pr = syn.make_problem(n, heterogeneous=True, nonlinear=False, absorbing=True, source="none", nt=nt, pml_size=4)
    rng = np.random.default_rng(seed)
    els = _elements(rng, (n, n, n), 5, 60, lo=lo)

    def sig(steps, phase):
        t = np.arange(steps)[:, None]
        return (1.0e-2 * np.sin(0.5 * t + phase + np.arange(5)[None, :]) * (1 + 0.3 * np.arange(5)[None, :])).astype(np.float32)
    ds = arrays.weighted_velocity_source(els, signals_x=sig(NT_X, 0.0), signals_z=sig(NT_Z, 0.7))
    pr.update(ds)
    pr["u_source_mode"] = _scalar(mode)
    return pr, ds


def _expanded(pr, series):
    exp = {k: v for k, v in pr.items() if "_source_element_" not in k}
    exp.update(series)
    exp["u_source_many"] = _scalar(1)
    return exp


def _fma_series(ds):
    """the series the kernel forms: fp32 fma in CSR order (the product is exact in fp64)"""
    ptr = ds["u_source_element_ptr"].reshape(-1).astype(np.int64)
    col = ds["u_source_element_index"].reshape(-1).astype(np.int64) - 1
    w = ds["u_source_element_weight"].reshape(-1).astype(np.float64)
    out = {}
    for c in "xyz":
        if f"u{c}_source_element_input" not in ds:
            continue
        sig = ds[f"u{c}_source_element_input"]
        sig = sig.reshape(-1, sig.shape[-1])
        acc = np.zeros((sig.shape[0], ptr.size - 1), dtype=np.float32)
        for j in range(int(np.diff(ptr).max())):
            rows = np.nonzero(np.diff(ptr) > j)[0]
            e = ptr[rows] + j
            acc[:, rows] = (w[e] * sig[:, col[e]].astype(np.float64) + acc[:, rows]).astype(np.float32)
        out[f"u{c}_source_input"] = acc.reshape(1, sig.shape[0], -1)
    return out


# ---- 2. weighted velocity source = expanded source ---------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_weighted_velocity_source_matches_expanded(mods, syn, orc, mode, fused):
    arrays, _, _, HostSolver = mods
    pr, ds = _weighted(syn, arrays, mode)
    assert int(pr["ux_source_flag"].ravel()[0]) == NT_X and int(pr["uz_source_flag"].ravel()[0]) == NT_Z
    assert int(pr["uy_source_flag"].ravel()[0]) == 0 and "uy_source_element_input" not in pr
    nt = 30
    g = HostSolver(pr, fused_kernels=fused)
    # the GPU's own expanded run gets the series the kernel forms: near-cancelling element sums would otherwise put
    # their fp32 rounding (<= (k + 1) ulp of sum |w s|, large relative to a small v) into the additive modes' density
    e = HostSolver(_expanded(pr, _fma_series(ds)), fused_kernels=fused)
    o = orc.OracleSim(_expanded(pr, arrays.expand_velocity_source(ds)))
    g.run(nt)
    assert g.scalar("fused_pipeline") == fused
    e.run(nt)
    o.step(nt)
    for f in ("p", "ux", "uy", "uz", "rhox"):
        a = g.field(f)
        assert np.any(a != 0.0), f
        assert rel_l2(a, o.field(f)) < TOL, f
        assert rel_l2(a, e.field(f)) < 1e-6, f
    g.close(), e.close(), o.close()


# ---- 3. u*_elements = W @ u_raw ----------------------------------------------------------------------------------------
def _sensor_problem(syn, arrays, dims, nt):
    nx, ny, nz = dims
    pr = syn.make_problem(nx, ny, nz, heterogeneous=True, nonlinear=True, absorbing=True, source="p0", nt=nt, pml_size=4)
    if nz == 1:
        pr = syn.as_2d_file(pr)
    rng = np.random.default_rng(5)
    els = _elements(rng, dims, 4, 40, lo=(8, 8, 8 if nz > 1 else 0), span=8)
    els.append((np.zeros(0, np.int64), np.zeros(0)))  # an empty element
    if nz > 1:
        several = (np.arange(0, nx * ny * nz, 7), rng.uniform(-1, 1, len(range(0, nx * ny * nz, 7))))
    else:  # 2-D: the plane has 1 024 points, so the element visits each three times; one sign, so that |W| = sum |w|
        several = (np.tile(np.arange(nx * ny), 3), rng.uniform(0.1, 1, 3 * nx * ny))
    els.append(several)  # several chunks
    ds = arrays.weighted_sensor(els)
    pr.update(ds)
    union = np.unique(np.concatenate([i for i, _ in els]))
    pr["sensor_mask_type"] = _scalar(0)
    pr["sensor_mask_index"] = (union + 1).astype(U64).reshape(1, 1, -1)
    return pr, ds, union


@pytest.mark.parametrize("case", ["fused", "rocfft", "2d"])
def test_u_elements_match_weighted_u_raw(mods, syn, case):
    arrays, capi, _, HostSolver = mods
    dims = (32, 32, 1) if case == "2d" else (32, 32, 32)
    nt, start = 24, 5
    pr, ds, union = _sensor_problem(syn, arrays, dims, nt)
    k = np.diff(ds["sensor_element_ptr"].reshape(-1).astype(np.int64))
    assert k[5] > 2 * capi.ELEMENT_CHUNK and k[4] == 0
    g = HostSolver(pr, fused_kernels=int(case != "rocfft"), u_raw=1, u_non_staggered_raw=1, u_elements=1,
                   u_non_staggered_elements=1, sampling_start=start)
    g.run(nt)
    if case != "2d":
        assert g.scalar("fused_pipeline") == int(case == "fused")
    g.finish()
    names = g.stream_names()
    comps = "xy" if case == "2d" else "xyz"
    got = {n: g.stream(n) for c in comps for n in (f"u{c}", f"u{c}_elements", f"u{c}_non_staggered",
                                                   f"u{c}_non_staggered_elements")}
    g.close()
    if case == "2d":
        assert "uz_elements" not in names and "uz_non_staggered_elements" not in names
    W = arrays.sensor_matrix(ds, int(np.prod(dims)))[:, union]
    for c in comps:
        for raw_name in (f"u{c}", f"u{c}_non_staggered"):
            raw, el = got[raw_name], got[raw_name + "_elements"]
            assert raw.shape == (nt - start, union.size) and el.shape == (nt - start, 6), raw_name
            for t in range(nt - start):
                x = raw[t].astype(np.float64)
                ref, mag = W @ x, np.abs(W) @ np.abs(x)
                assert np.all(np.abs(el[t] - ref) <= (k + 1) * U * mag), (raw_name, t)
            assert np.all(el[:, 4] == 0.0), raw_name
            assert np.all(np.any(el[:, [0, 1, 2, 3, 5]] != 0.0, axis=0)), raw_name


# ---- 4. output file and checkpointed restart ---------------------------------------------------------------------------
ELEMENT_STREAMS = tuple(f"u{c}{kind}_elements" for kind in ("", "_non_staggered") for c in "xyz")


def test_u_elements_output_file_and_restart(mods, syn, tmp_path):
    arrays, _, h5io, HostSolver = mods
    if not os.path.exists(h5io.H5_LIB_PATH):
        pytest.skip("HDF5 component not built")
    nt, split, start = 30, 13, 4
    pr, _ = _weighted(syn, arrays, 2, nt=nt)
    pr.update(arrays.weighted_sensor(_elements(np.random.default_rng(9), (32, 32, 32), 3, 50, lo=(14, 14, 14))))
    flags = dict(u_elements=1, u_non_staggered_elements=1, u_raw=1, sampling_start=start)
    mem = HostSolver(pr, **flags)
    mem.run(nt)
    mem.finish()
    ref = {n: mem.stream(n) for n in ELEMENT_STREAMS}
    mem.close()
    path_in, whole, legs, ckpt = (str(tmp_path / n) for n in ("in.h5", "whole.h5", "legs.h5", "ckpt.h5"))
    h5io.write_input_file(pr, path_in)
    fs = h5io.FileSolver(path_in, output=whole, **flags)
    fs.run(nt)
    fs.finish()
    fs.write_output(whole)
    fs.close()
    for n in ELEMENT_STREAMS:
        got = h5io.read_dataset(whole, n)
        assert got.shape[-2:] == (nt - start, 3), n
        assert np.array_equal(got.reshape(ref[n].shape), ref[n]), n
        assert np.any(got != 0.0), n
    a = h5io.FileSolver(path_in, output=legs, **flags)
    a.run(split)
    a.write_checkpoint(ckpt)
    a.close()
    b = h5io.FileSolver(path_in, output=legs, reopen_output=True, **flags)
    b.read_checkpoint(ckpt)
    assert b.t == split
    b.run(nt)
    b.finish()
    b.write_output(legs)
    b.close()
    for name in ELEMENT_STREAMS + ("ux", "uy", "uz"):
        assert np.array_equal(h5io.read_dataset(legs, name), h5io.read_dataset(whole, name)), name


# ---- 5. slab run -------------------------------------------------------------------------------------------------------
def test_slab_run_with_weighted_velocity_source_and_sensor(mods, syn, tmp_path):
    arrays, _, h5io, _ = mods
    if not os.path.exists(h5io.H5_LIB_PATH):
        pytest.skip("HDF5 component not built")
    world, nt, start = 2, 18, 3
    pr, ds = _weighted(syn, arrays, 2, nt=nt, lo=(6, 6, 10))   # source box z = 10..19: crosses the slab boundary at 16
    z = (ds["u_source_index"].reshape(-1).astype(np.int64) - 1) // (32 * 32)
    assert z.min() < 16 <= z.max()
    rng = np.random.default_rng(13)
    straddle = _elements(rng, (32, 32, 32), 2, 80, lo=(12, 12, 12), span=8)   # z = 12..19 crosses z = 16
    inside = _elements(rng, (32, 32, 32), 1, 30, lo=(4, 4, 1), span=6)        # z = 1..6: rank 0 alone
    for idx, _ in straddle:
        assert (idx // 1024).min() < 16 <= (idx // 1024).max()
    pr.update(arrays.weighted_sensor(straddle + inside))
    union = np.unique(np.concatenate([i for i, _ in straddle + inside]))
    pr["sensor_mask_type"] = _scalar(0)
    pr["sensor_mask_index"] = (union + 1).astype(U64).reshape(1, 1, -1)
    path_in, one, many = (str(tmp_path / n) for n in ("in.h5", "one.h5", f"slab{world}.h5"))
    h5io.write_input_file(pr, path_in)
    flags = dict(u_raw=1, u_elements=1, u_non_staggered_elements=1)
    fs = h5io.FileSolver(path_in, sampling_start=start - 1, **flags)
    fs.run(nt)
    fs.finish()
    fs.write_output(one)
    fs.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", "29871", "-m", "kwave_amd.run_slab", "-i", path_in, "-o", many,
           "-s", str(start), "--backend", "gloo"] + ["--" + f for f in flags]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       cwd=os.path.dirname(HERE), env=dict(os.environ, OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout[-4000:]
    for name in ELEMENT_STREAMS + ("ux", "uy", "uz"):
        a, b = h5io.read_dataset(many, name), h5io.read_dataset(one, name)
        assert a.shape == b.shape, name
        assert np.any(b != 0.0), name
        assert rel_l2(a, b) < TOL, name


# ---- 6. create-time checks ---------------------------------------------------------------------------------------------
def _bad_inputs(pr):
    def edit(**kv):
        q = dict(pr)
        for k, v in kv.items():
            if v is None:
                q.pop(k)
            else:
                q[k] = v
        return q
    npts = pr["u_source_index"].size
    sp = pr["u_source_element_ptr"].reshape(-1)
    nonmono = sp.copy(); nonmono[2], nonmono[3] = nonmono[3], nonmono[2]  # noqa: E702
    last = sp.copy(); last[-1] -= 1  # noqa: E702
    bad_el = pr["u_source_element_index"].copy(); bad_el.reshape(-1)[5] = 6  # noqa: E702
    zeros = lambda steps, n: np.zeros((1, steps, n), np.float32)  # noqa: E731
    return [
        # the refusal list of the weighted velocity source
        ("flag 0", "uy_source_element_input: present, but uy_source_flag is 0", edit(uy_source_element_input=zeros(NT_X, 5))),
        ("both", "ux_source_input and ux_source_element_input cannot both be present", edit(ux_source_input=zeros(NT_X, npts))),
        ("mixed", "uy_source_element_input: missing, although uy_source_flag is above 0", edit(uy_source_flag=_scalar(NT_X), uy_source_input=zeros(NT_X, npts))),
        ("many", "u_source_many: must be 1 with", edit(u_source_many=_scalar(0))),
        ("E differs", "uz_source_element_input: has 4 elements, but ux_source_element_input has 5", edit(uz_source_element_input=zeros(NT_Z, 4))),
        ("transducer", "weighted velocity source cannot be combined with transducer_source_flag", edit(transducer_source_flag=_scalar(5), transducer_source_input=zeros(1, 64)[0],
                                                      delay_mask=np.ones((1, 1, npts), dtype=U64))),
        ("steps", "ux_source_element_input: expected .1, ux_source_flag = 20, E.", edit(ux_source_element_input=zeros(NT_X - 1, 5))),
        # the CSR checks, shared with the pressure source, name the velocity datasets
        ("not monotone", "u_source_element_ptr: offsets are not monotone at row 2", edit(u_source_element_ptr=nonmono.reshape(1, 1, -1))),
        ("last offset", "u_source_element_ptr: last offset", edit(u_source_element_ptr=last.reshape(1, 1, -1))),
        ("length", "u_source_element_ptr: has [0-9]+ entries, expected", edit(u_source_element_ptr=sp[:-1].reshape(1, 1, -1))),
        ("element", "u_source_element_index: entry 5 = 6 lies outside 1..5", edit(u_source_element_index=bad_el)),
        ("weights", "u_source_element_weight: has [0-9]+ entries, but u_source_element_index has", edit(u_source_element_weight=pr["u_source_element_weight"].reshape(-1)[:-1].reshape(1, 1, -1))),
        ("no csr", "u_source_element_ptr: dataset is missing", edit(u_source_element_ptr=None)),
        ("no sensor", "--u_elements needs the datasets sensor_element_ptr", edit(sensor_element_ptr=None)),
    ]


def test_malformed_velocity_element_datasets_fail_at_create(mods, syn):
    """The refusal of more than 2^32 - 1 points or entries cannot be reached from real arrays (32 GiB of indices); the
    stand-alone host program of tests/test_velocity_elements_host.py covers it with an input that only reports sizes."""
    arrays, capi, _, HostSolver = mods
    pr, _ = _weighted(syn, arrays, 0, nt=10)
    pr.update(arrays.weighted_sensor(_elements(np.random.default_rng(2), (32, 32, 32), 3, 20)))
    for flags in (dict(u_elements=1), dict(u_non_staggered_elements=1), dict(u_elements=1, u_non_staggered_elements=1, p_elements=1)):
        g = HostSolver(pr, **flags)  # the well-formed input is accepted
        g.close()
    for what, message, bad in _bad_inputs(pr):   # each case is matched by the message of its own check
        with pytest.raises(capi.KWaveError, match=message):
            HostSolver(bad, u_elements=1)
