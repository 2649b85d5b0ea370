"""Weighted transducer arrays on the GPU: kw_element_source_row and kw_sample_elements alone against fp64, the weighted
source against the expanded one (CPU oracle and GPU), p_elements against W @ p_raw, the output file and a checkpointed
restart, slab runs, and the create-time checks of the CSR datasets.

Element-wise bound of both kernels: |gpu - fp64| <= (k + 1) 2^-24 sum_j |w_j x_j|, k = the row's entry count."""
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


@pytest.fixture(scope="module")
def mods():
    import kwave_amd  # noqa: F401
    from kwave_amd import arrays, capi, h5io
    from kwave_amd.solver import HostSolver
    return arrays, capi, h5io, HostSolver


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------
def _csr(rng, lengths, ncols, shared_cols=None):
    ptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(lengths)
    cols = rng.integers(0, ncols, ptr[-1]) if shared_cols is None else shared_cols
    w = rng.uniform(-1.5, 1.5, ptr[-1]).astype(np.float32)
    return ptr, cols, w


def _bound_check(gpu, ptr, cols, w, x):
    k = np.diff(ptr)
    rows = np.repeat(np.arange(k.size), k)
    terms = w.astype(np.float64) * x.astype(np.float64)[cols]
    ref = np.bincount(rows, weights=terms, minlength=k.size)
    mag = np.bincount(rows, weights=np.abs(terms), minlength=k.size)
    err = np.abs(gpu.astype(np.float64) - ref)
    assert np.all(err <= (k + 1) * U * mag), (np.max(err / np.maximum((k + 1) * U * mag, 1e-300)))
    assert np.all(gpu[k == 0] == 0.0)


def test_sample_elements_kernel_against_fp64(mods):
    _, capi, _, _ = mods
    rng = np.random.default_rng(7)
    n_grid = 40000
    # empty rows, one entry, several chunks (3000 > 2 x 1024), exactly one chunk, one past it
    lengths = [0, 1, 3000, 64, 1024, 1025, 0, 7, 50000]
    ptr, cols, w = _csr(rng, lengths, n_grid)
    p = rng.standard_normal(n_grid).astype(np.float32)
    cp = capi.element_chunk_ptr(ptr)
    assert cp[-1] == 0 + 1 + 3 + 1 + 1 + 2 + 0 + 1 + 49
    d = capi.Device()
    try:
        ins = [Guarded(d, p), Guarded(d, ptr.astype(np.uint32), dtype=np.uint32),
               Guarded(d, capi.csr_entries(cols, w), dtype=np.uint32), Guarded(d, cp, dtype=np.uint32)]
        part = Guarded(d, np.zeros(int(cp[-1]), np.float32))
        outs = []
        for _ in range(2):
            out = Guarded(d, np.full(len(lengths), np.nan, np.float32))
            capi.check(d.L.kw_sample_elements(d.ctx, out.ptr, ins[0].ptr, ins[1].ptr, ins[2].ptr, len(lengths), int(ptr[-1]),
                                              ins[3].ptr, int(cp[-1]), part.ptr))
            outs.append(out.read())
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "two launches differ"
        _bound_check(outs[0], ptr, cols, w, p)
        for g, h in zip(ins, (p, ptr.astype(np.uint32), capi.csr_entries(cols, w), cp)):
            assert np.array_equal(g.read().view(np.uint8), np.ascontiguousarray(h).view(np.uint8)), "input changed"
        part.read()  # guard bands intact
    finally:
        d.close()


def test_element_source_row_kernel_against_fp64(mods):
    _, capi, _, _ = mods
    rng = np.random.default_rng(11)
    n_el, nt, t = 6, 5, 3
    # every point is covered by 0 .. 3 elements (points shared by up to 3), plus one long row
    lengths = list(rng.integers(0, 4, 700)) + [0, 1, 300]
    ptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(lengths)
    cols = np.concatenate([rng.choice(n_el, size=k, replace=k > n_el) for k in lengths]).astype(np.int64)
    w = rng.uniform(-2.0, 2.0, ptr[-1]).astype(np.float32)
    sig = rng.standard_normal((nt, n_el)).astype(np.float32)
    d = capi.Device()
    try:
        ins = [Guarded(d, sig), Guarded(d, ptr.astype(np.uint32), dtype=np.uint32),
               Guarded(d, capi.csr_entries(cols, w), dtype=np.uint32)]
        outs = []
        for _ in range(2):
            row = Guarded(d, np.full(len(lengths), np.nan, np.float32))
            capi.check(d.L.kw_element_source_row(d.ctx, row.ptr, ins[0].ptr, ins[1].ptr, ins[2].ptr, len(lengths), n_el, t))
            outs.append(row.read())
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
        _bound_check(outs[0], ptr, cols, w, sig[t])
        for g, h in zip(ins, (sig, ptr.astype(np.uint32), capi.csr_entries(cols, w))):
            assert np.array_equal(g.read().view(np.uint8), np.ascontiguousarray(h).view(np.uint8))
    finally:
        d.close()


# ---- problems ----------------------------------------------------------------------------------------------------------
def _elements(rng, dims, n_el, per, lo=(6, 6, 6), span=10):
    """n_el overlapping elements of `per` points each, drawn from one span^3 box of the (nx, ny, nz) grid"""
    nx, ny, nz = dims
    zs = range(lo[2], min(lo[2] + span, nz)) if nz > 1 else [0]
    pool = np.array([x + nx * (y + ny * z) for z in zs for y in range(lo[1], lo[1] + span) for x in range(lo[0], lo[0] + span)])
    return [(np.sort(rng.choice(pool, per, replace=False)), rng.uniform(0.2, 1.0, per)) for _ in range(n_el)]


def _weighted(syn, arrays, mode, n=32, nt=30, nt_src=20, seed=3):
    pr = syn.make_problem(n, heterogeneous=True, nonlinear=False, absorbing=True, source="none", nt=nt, pml_size=4)
    rng = np.random.default_rng(seed)
    els = _elements(rng, (n, n, n), 5, 60)
    t = np.arange(nt_src)[:, None]
    sig = (2.0e4 * np.sin(0.5 * t + np.arange(5)[None, :]) * (1 + 0.3 * np.arange(5)[None, :])).astype(np.float32)
    ds = arrays.weighted_source(els, sig)
    pr.update(ds)
    pr["p_source_mode"] = np.array([[[mode]]], dtype=np.uint64)
    exp = {k: v for k, v in pr.items() if not k.startswith("p_source_element_")}
    exp["p_source_input"] = arrays.expand_source(ds)
    exp["p_source_many"] = np.array([[[1]]], dtype=np.uint64)
    return pr, exp


def _fma_expanded(pr):
    """the expanded problem with the series the kernel forms: fp32 fma in CSR order (the product is exact in fp64)"""
    sig = pr["p_source_element_input"].reshape(-1, pr["p_source_element_input"].shape[-1])
    ptr = pr["p_source_element_ptr"].reshape(-1).astype(np.int64)
    col = pr["p_source_element_index"].reshape(-1).astype(np.int64) - 1
    w = pr["p_source_element_weight"].reshape(-1).astype(np.float64)
    acc = np.zeros((sig.shape[0], ptr.size - 1), dtype=np.float32)
    for j in range(int(np.diff(ptr).max())):
        rows = np.nonzero(np.diff(ptr) > j)[0]
        e = ptr[rows] + j
        acc[:, rows] = (w[e] * sig[:, col[e]].astype(np.float64) + acc[:, rows]).astype(np.float32)
    exp = {k: v for k, v in pr.items() if not k.startswith("p_source_element_")}
    exp["p_source_input"] = acc.reshape(1, sig.shape[0], -1)
    exp["p_source_many"] = np.array([[[1]]], dtype=np.uint64)
    return exp


# ---- 2. weighted source = expanded source ------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_weighted_source_matches_expanded(mods, syn, orc, mode, fused):
    arrays, _, _, HostSolver = mods
    pr, exp = _weighted(syn, arrays, mode)
    nt = 30
    g = HostSolver(pr, fused_kernels=fused)
    # the GPU's own expanded run gets the series the kernel forms: near-cancelling element sums would otherwise put
    # their fp32 rounding (<= (k + 1) ulp of sum |w s|, large relative to a small v) into the additive modes' density
    e = HostSolver(_fma_expanded(pr), fused_kernels=fused)
    o = orc.OracleSim(exp)
    g.run(nt)
    assert g.scalar("fused_pipeline") == fused
    e.run(nt)
    o.step(nt)
    for f in ("p", "ux", "uy", "uz", "rhox"):
        a = g.field(f)
        assert rel_l2(a, o.field(f)) < TOL, f
        assert rel_l2(a, e.field(f)) < 1e-6, f
    g.close(), e.close(), o.close()


# ---- 3. p_elements = W @ p_raw -----------------------------------------------------------------------------------------
def _sensor_problem(syn, arrays, dims, nt):
    nx, ny, nz = dims
    pr = syn.make_problem(nx, ny, nz, heterogeneous=True, nonlinear=True, absorbing=True, source="p0", nt=nt, pml_size=4)
    if nz == 1:
        pr = syn.as_2d_file(pr)
    rng = np.random.default_rng(5)
    els = _elements(rng, dims, 4, 40, lo=(8, 8, 8 if nz > 1 else 0), span=8)
    els.append((np.zeros(0, np.int64), np.zeros(0)))  # an empty element
    els.append((np.arange(0, nx * ny * nz, 7), rng.uniform(-1, 1, len(range(0, nx * ny * nz, 7)))))  # several chunks
    ds = arrays.weighted_sensor(els)
    pr.update(ds)
    union = np.unique(np.concatenate([i for i, _ in els]))
    pr["sensor_mask_type"] = np.array([[[0]]], dtype=np.uint64)
    pr["sensor_mask_index"] = (union + 1).astype(np.uint64).reshape(1, 1, -1)
    return pr, ds, union


@pytest.mark.parametrize("case", ["fused", "rocfft", "2d"])
def test_p_elements_matches_weighted_p_raw(mods, syn, case):
    arrays, _, _, HostSolver = mods
    dims = (32, 32, 1) if case == "2d" else (32, 32, 32)
    nt, start = 24, 5
    pr, ds, union = _sensor_problem(syn, arrays, dims, nt)
    g = HostSolver(pr, fused_kernels=int(case != "rocfft"), p_raw=1, p_elements=1, sampling_start=start)
    g.run(nt)
    if case != "2d":
        assert g.scalar("fused_pipeline") == int(case == "fused")
    g.finish()
    raw, el = g.stream("p"), g.stream("p_elements")
    g.close()
    assert raw.shape == (nt - start, union.size) and el.shape == (nt - start, 6)
    W = arrays.sensor_matrix(ds, int(np.prod(dims)))[:, union]
    k = np.diff(ds["sensor_element_ptr"].reshape(-1).astype(np.int64))
    for t in range(nt - start):
        x = raw[t].astype(np.float64)
        ref, mag = W @ x, np.abs(W) @ np.abs(x)
        assert np.all(np.abs(el[t] - ref) <= (k + 1) * U * mag), t
    assert np.all(el[:, 4] == 0.0) and np.any(el[:, :4] != 0.0)


# ---- 4. output file and checkpointed restart ---------------------------------------------------------------------------
def test_p_elements_output_file_and_restart(mods, syn, tmp_path):
    arrays, _, h5io, HostSolver = mods
    if not os.path.exists(h5io.H5_LIB_PATH):
        pytest.skip("HDF5 component not built")
    nt, split, start = 30, 13, 4
    pr, _ = _weighted(syn, arrays, 2, nt=nt)
    pr.update(arrays.weighted_sensor(_elements(np.random.default_rng(9), (32, 32, 32), 3, 50, lo=(14, 14, 14))))
    flags = dict(p_elements=1, p_raw=1, sampling_start=start)
    mem = HostSolver(pr, **flags)
    mem.run(nt)
    mem.finish()
    ref = mem.stream("p_elements")
    mem.close()
    path_in, whole, legs, ckpt = (str(tmp_path / n) for n in ("in.h5", "whole.h5", "legs.h5", "ckpt.h5"))
    h5io.write_input_file(pr, path_in)
    fs = h5io.FileSolver(path_in, output=whole, **flags)
    fs.run(nt)
    fs.finish()
    fs.write_output(whole)
    fs.close()
    got = h5io.read_dataset(whole, "p_elements")
    assert got.shape[-2:] == (nt - start, 3)
    assert np.array_equal(got.reshape(ref.shape), ref)
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
    for name in ("p_elements", "p"):
        assert np.array_equal(h5io.read_dataset(legs, name), h5io.read_dataset(whole, name)), name


# ---- 5. slab runs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
def test_slab_run_with_weighted_source_and_sensor(mods, syn, tmp_path, world):
    arrays, _, h5io, _ = mods
    if not os.path.exists(h5io.H5_LIB_PATH):
        pytest.skip("HDF5 component not built")
    nt, start = 18, 3
    pr, _ = _weighted(syn, arrays, 2, nt=nt)   # source box z = 6..15: crosses the slab boundaries at 8 and 16
    rng = np.random.default_rng(13)
    straddle = _elements(rng, (32, 32, 32), 2, 80, lo=(12, 12, 12), span=8)   # z = 12..19 crosses z = 16
    inside = _elements(rng, (32, 32, 32), 1, 30, lo=(4, 4, 1), span=6)        # z = 1..6: rank 0 alone
    pr.update(arrays.weighted_sensor(straddle + inside))
    path_in, one, many = (str(tmp_path / n) for n in ("in.h5", "one.h5", f"slab{world}.h5"))
    h5io.write_input_file(pr, path_in)
    flags = dict(p_raw=1, p_elements=1)
    fs = h5io.FileSolver(path_in, sampling_start=start - 1, **flags)
    fs.run(nt)
    fs.finish()
    fs.write_output(one)
    fs.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29850 + world), "-m", "kwave_amd.run_slab", "-i", path_in, "-o", many,
           "-s", str(start), "--backend", "gloo"] + ["--" + f for f in flags]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       cwd=os.path.dirname(HERE), env=dict(os.environ, OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout[-4000:]
    for name in ("p", "p_elements"):
        a, b = h5io.read_dataset(many, name), h5io.read_dataset(one, name)
        assert a.shape == b.shape, name
        assert rel_l2(a, b) < TOL, name


# ---- 6. create-time checks ---------------------------------------------------------------------------------------------
def _bad_inputs(pr):
    u = np.uint64
    def edit(**kv):
        q = dict(pr)
        for k, v in kv.items():
            if v is None:
                q.pop(k)
            else:
                q[k] = v
        return q
    sp = pr["p_source_element_ptr"].reshape(-1)
    se = pr["sensor_element_ptr"].reshape(-1)
    nonmono = sp.copy(); nonmono[2], nonmono[3] = nonmono[3], nonmono[2]  # noqa: E702
    bad_el = pr["p_source_element_index"].copy(); bad_el.reshape(-1)[5] = 6  # noqa: E702
    bad_grid = pr["sensor_element_index"].copy(); bad_grid.reshape(-1)[0] = 32 ** 3 + 1  # noqa: E702
    short = se[:-1]
    last = sp.copy(); last[-1] -= 1  # noqa: E702
    return [
        ("not monotone", "p_source_element_ptr", edit(p_source_element_ptr=nonmono.reshape(1, 1, -1)), {}),
        ("last offset", "p_source_element_ptr", edit(p_source_element_ptr=last.reshape(1, 1, -1)), {}),
        ("length", "p_source_element_ptr", edit(p_source_element_ptr=sp[:-1].reshape(1, 1, -1)), {}),
        ("last offset", "sensor_element_ptr", edit(sensor_element_ptr=short.reshape(1, 1, -1)), {}),
        ("element", "p_source_element_index", edit(p_source_element_index=bad_el), {}),
        ("grid", "sensor_element_index", edit(sensor_element_index=bad_grid), {}),
        ("both", "p_source_input", edit(p_source_input=np.zeros((1, 20, 1), np.float32)), {}),
        ("no sensor", "sensor_element_ptr", edit(sensor_element_ptr=None), {}),
        ("many", "p_source_many", edit(p_source_many=np.array([[[0]]], dtype=u)), {}),
    ]


def test_malformed_element_datasets_fail_at_create(mods, syn):
    arrays, capi, _, HostSolver = mods
    pr, _ = _weighted(syn, arrays, 0, nt=10)
    pr.update(arrays.weighted_sensor(_elements(np.random.default_rng(2), (32, 32, 32), 3, 20)))
    g = HostSolver(pr, p_elements=1)  # the well-formed input is accepted
    g.close()
    for what, name, bad, _ in _bad_inputs(pr):
        with pytest.raises(capi.KWaveError, match=name):
            HostSolver(bad, p_elements=1)
