"""Per-entry time delays of the weighted transducer arrays, on the GPU: kw_sample_elements_delayed and
kw_element_source_rows_delayed alone against bit-exact twins built from the undelayed kernels and against fp64, delayed
sources against the expanded problem (CPU oracle and GPU), delayed sensors against the delayed weighted sum of the raw
series, the output file and a checkpointed restart with a non-empty ring, a slab run, and the create-time checks.

Bounds: the source kernel |gpu - fp64| <= (k + 1) 2^-24 sum |w s| (k = the row's entries, one fma chain); the sensor
|gpu - fp64| <= (k + G + 1) 2^-24 sum |w x| (G = the row's delay groups: the bound of kw_sample_elements per group plus
one rounding per addition into the ring)."""
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


def _pointers(values):
    return (C.c_void_p * len(values))(*values)


def _u64s(values):
    return (C.c_uint64 * len(values))(*values)


# ---- the regrouping, as the header states it: per row by ascending delay, stable --------------------------------------------
def _regroup(ptr, delays):
    """order (regrouped position -> CSR entry), group_ptr, group_delay, element_group_ptr"""
    order, group_ptr, group_delay, egp = [], [0], [], [0]
    for r in range(len(ptr) - 1):
        d = delays[ptr[r]:ptr[r + 1]]
        o = np.argsort(d, kind="stable")
        order.append(ptr[r] + o)
        ds = d[o]
        for j in range(len(ds)):
            if j + 1 == len(ds) or ds[j + 1] != ds[j]:
                group_delay.append(int(ds[j]))
                group_ptr.append(int(ptr[r]) + j + 1)
        egp.append(len(group_delay))
    order = np.concatenate(order).astype(np.int64) if order else np.zeros(0, np.int64)
    return order, np.array(group_ptr, np.int64), np.array(group_delay, np.int64), np.array(egp, np.int64)


class _Delayed:
    """device copies of a regrouped CSR and one call of kw_sample_elements_delayed per step"""

    def __init__(self, capi, d, ptr, cols, w, delays, n_fields, ring_rows):
        self.capi, self.d, self.nf, self.rows = capi, d, n_fields, ring_rows
        self.n_el = len(ptr) - 1
        self.order, self.gptr, self.gdelay, self.egp = _regroup(ptr, delays)
        self.cols, self.w = cols[self.order], w[self.order]
        self.cp = capi.element_chunk_ptr(self.gptr)
        self.n_chunks = int(self.cp[-1])
        self.host = [self.gptr.astype(np.uint32), capi.csr_entries(self.cols, self.w), self.gdelay.astype(np.uint32),
                     self.egp.astype(np.uint32), self.cp]
        self.dev = [Guarded(d, h, dtype=np.uint32) for h in self.host]
        self.part = Guarded(d, np.full(max(n_fields * self.n_chunks, 1), np.nan, np.float32))
        self.rings = [Guarded(d, np.zeros((ring_rows, self.n_el), np.float32)) for _ in range(n_fields)]

    def step(self, fields, n):
        outs = [Guarded(self.d, np.full(self.n_el, np.nan, np.float32)) for _ in range(self.nf)]
        g = self.dev
        self.capi.check(self.d.L.kw_sample_elements_delayed(
            self.d.ctx, self.nf, _pointers([o.ptr for o in outs]), _pointers([f.ptr for f in fields[:self.nf]]), g[0].ptr,
            g[1].ptr, g[2].ptr, g[3].ptr, self.n_el, len(self.gdelay), len(self.cols), g[4].ptr, self.n_chunks, self.part.ptr,
            _pointers([r.ptr for r in self.rings]), self.rows, n))
        got = [o.read() for o in outs]
        for o in outs:
            o.free()
        return got

    def check_inputs(self):
        for g, h in zip(self.dev, self.host):
            assert np.array_equal(g.read().view(np.uint8), np.ascontiguousarray(h).view(np.uint8)), "input changed"
        self.part.read()
        for r in self.rings:
            r.read()  # guard bands intact


# ---- 1. the delayed sampler alone ---------------------------------------------------------------------------------------------
def _seven_elements(rng, n_grid):
    d3 = np.array([0] * 500 + [1] * 2100 + [5] * 400)
    rng.shuffle(d3)
    d4 = np.array([2] * 600 + [3] * 425)
    rng.shuffle(d4)
    per = [np.zeros(0, np.int64), np.array([0]), np.full(64, 5), d3, d4, np.array([0, 1, 2, 3, 4, 5, 3]), np.zeros(50, np.int64)]
    lengths = [len(x) for x in per]
    assert lengths == [0, 1, 64, 3000, 1025, 7, 50]
    ptr = np.zeros(8, dtype=np.int64)
    ptr[1:] = np.cumsum(lengths)
    delays = np.concatenate(per).astype(np.int64)
    return ptr, rng.integers(0, n_grid, ptr[-1]), rng.uniform(-1.5, 1.5, ptr[-1]).astype(np.float32), delays


@pytest.mark.parametrize("n_fields", [1, 3])
def test_delayed_sampler_against_twin_and_fp64(mods, n_fields):
    _, capi, _, _ = mods
    rng = np.random.default_rng(23)
    n_grid, steps, max_delay = 4096, 14, 5
    ptr, cols, w, delays = _seven_elements(rng, n_grid)
    n_el = 7
    noise = rng.standard_normal((steps, n_fields, n_grid)).astype(np.float32)
    d = capi.Device()
    try:
        fields = [Guarded(d, noise[0, f]) for f in range(n_fields)]
        runs = {}
        for ring_rows in (6, 6, 9):
            s = _Delayed(capi, d, ptr, cols, w, delays, n_fields, ring_rows)
            assert len(s.gdelay) == 0 + 1 + 1 + 3 + 2 + 6 + 1 and s.n_chunks == len(s.gdelay) + 2  # the 2100-entry group: 3 chunks
            out = np.zeros((steps, n_fields, n_el), np.float32)
            for t in range(steps):
                for f in range(n_fields):
                    fields[f].write(noise[t, f])
                out[t] = np.stack(s.step(fields, t))
            s.check_inputs()
            runs.setdefault(ring_rows, []).append(out)
        for f in range(n_fields):
            assert np.array_equal(fields[f].read(), noise[-1, f]), "field changed"
        got = runs[6][0]
        assert np.array_equal(got.view(np.uint32), runs[6][1].view(np.uint32)), "two runs differ"
        assert np.array_equal(got.view(np.uint32), runs[9][0].view(np.uint32)), "a ring of 9 rows gives other bits"
        # the twin: the groups as the rows of kw_sample_elements, the ring replayed in fp32
        s = _Delayed(capi, d, ptr, cols, w, delays, 1, 6)
        n_groups = len(s.gdelay)
        twin = np.zeros((steps, n_fields, n_el), np.float32)
        ring = np.zeros((n_fields, 6, n_el), np.float32)
        gsum = Guarded(d, np.full(n_groups, np.nan, np.float32))
        for t in range(steps):
            for f in range(n_fields):
                fields[0].write(noise[t, f])
                capi.check(d.L.kw_sample_elements(d.ctx, gsum.ptr, fields[0].ptr, s.dev[0].ptr, s.dev[1].ptr, n_groups,
                                                  len(s.cols), s.dev[4].ptr, s.n_chunks, s.part.ptr))
                gs = gsum.read()
                for e in range(n_el):
                    for g in range(s.egp[e], s.egp[e + 1]):
                        slot = (t + s.gdelay[g]) % 6
                        ring[f, slot, e] = np.float32(ring[f, slot, e] + gs[g])
                twin[t, f] = ring[f, t % 6]
                ring[f, t % 6] = 0.0
        assert np.array_equal(got.view(np.uint32), twin.view(np.uint32)), "the delayed sampler differs from its twin"
        # fp64, and the rows before a slot's first contribution
        k = np.diff(ptr)
        groups = np.diff(s.egp)
        rows = np.repeat(np.arange(n_el), k)
        for f in range(n_fields):
            for t in range(steps):
                live = delays <= t
                x = noise[np.maximum(t - delays, 0), f, cols].astype(np.float64)
                terms = np.where(live, w.astype(np.float64) * x, 0.0)
                ref = np.bincount(rows, weights=terms, minlength=n_el)
                mag = np.bincount(rows, weights=np.abs(terms), minlength=n_el)
                assert np.all(np.abs(got[t, f] - ref) <= (k + groups + 1) * U * mag), (f, t)
            assert np.all(got[:5, f, 2].view(np.uint32) == 0) and got[5, f, 2] != 0.0   # element 2: all at d = 5
            assert np.all(got[:2, f, 4].view(np.uint32) == 0) and got[2, f, 4] != 0.0   # element 4: {2, 3}
            assert np.all(got[:, f, 0].view(np.uint32) == 0)                            # the empty row
        assert max_delay == int(delays.max())
    finally:
        d.close()


# ---- 2. all delays zero = kw_sample_elements(_multi) -------------------------------------------------------------------------
LENGTHS = [0, 1, 3000, 64, 1024, 1025, 0, 7, 50000]   # the lengths of test_sample_elements_kernel_against_fp64


@pytest.mark.parametrize("n_fields", [1, 3])
def test_zero_delays_equal_the_undelayed_kernels(mods, n_fields):
    _, capi, _, _ = mods
    rng = np.random.default_rng(29)
    n_grid, n_el = 40000, len(LENGTHS)
    ptr = np.zeros(n_el + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(LENGTHS)
    cols, w = rng.integers(0, n_grid, ptr[-1]), rng.uniform(-1.5, 1.5, ptr[-1]).astype(np.float32)
    host_fields = [rng.standard_normal(n_grid).astype(np.float32) for _ in range(n_fields)]
    cp = capi.element_chunk_ptr(ptr)
    d = capi.Device()
    try:
        fields = [Guarded(d, f) for f in host_fields]
        csr = [Guarded(d, ptr.astype(np.uint32), dtype=np.uint32), Guarded(d, capi.csr_entries(cols, w), dtype=np.uint32),
               Guarded(d, cp, dtype=np.uint32)]
        part = Guarded(d, np.full(n_fields * int(cp[-1]), np.nan, np.float32))
        outs = [Guarded(d, np.full(n_el, np.nan, np.float32)) for _ in range(n_fields)]
        if n_fields == 1:
            capi.check(d.L.kw_sample_elements(d.ctx, outs[0].ptr, fields[0].ptr, csr[0].ptr, csr[1].ptr, n_el, int(ptr[-1]),
                                              csr[2].ptr, int(cp[-1]), part.ptr))
        else:
            capi.check(d.L.kw_sample_elements_multi(d.ctx, n_fields, _pointers([o.ptr for o in outs]),
                                                    _pointers([f.ptr for f in fields]), csr[0].ptr, csr[1].ptr, n_el,
                                                    int(ptr[-1]), csr[2].ptr, int(cp[-1]), part.ptr))
        want = np.stack([o.read() for o in outs])
        s = _Delayed(capi, d, ptr, cols, w, np.zeros(ptr[-1], np.int64), n_fields, 1)
        assert np.array_equal(s.order, np.arange(ptr[-1])) and len(s.gdelay) == n_el - 2  # one group per non-empty row
        for n in range(3):   # the one ring row is emitted and cleared every step
            got = np.stack(s.step(fields, n))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
        s.check_inputs()
        for g, h in zip(fields, host_fields):
            assert np.array_equal(g.read(), h), "field changed"
    finally:
        d.close()


# ---- 3. the delayed source kernel alone ------------------------------------------------------------------------------------
def test_delayed_source_rows_against_twin_and_fp64(mods):
    _, capi, _, _ = mods
    rng = np.random.default_rng(31)
    n_el, nt, max_delay = 6, 5, 4
    lengths = list(rng.integers(0, 4, 700)) + [0, 1, 300]
    n_pts = len(lengths)
    ptr = np.zeros(n_pts + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(lengths)
    nnz = int(ptr[-1])
    cols = np.concatenate([rng.choice(n_el, size=k, replace=k > n_el) for k in lengths]).astype(np.int64)
    w = rng.uniform(-2.0, 2.0, nnz).astype(np.float32)
    delays = rng.integers(0, max_delay + 1, nnz)
    delays[-300:-295] = [0, 1, 2, 3, 4]
    rows_of = np.repeat(np.arange(n_pts), lengths)
    cases = [((0,), (nt, 0, 0)), ((1, 2), (0, nt, nt)), ((0, 1, 2), (nt, 3, 4))]
    d = capi.Device()
    try:
        csr = [Guarded(d, ptr.astype(np.uint32), dtype=np.uint32), Guarded(d, capi.csr_entries(cols, w), dtype=np.uint32),
               Guarded(d, delays.astype(np.uint32), dtype=np.uint32)]
        # the twin's CSR: the same rows and weights, the columns are the entry numbers
        twin_entries = Guarded(d, capi.csr_entries(np.arange(nnz), w), dtype=np.uint32)
        twin_signal = Guarded(d, np.zeros(nnz, np.float32))
        for active, steps in cases:
            host_sig = {c: rng.standard_normal((steps[c], n_el)).astype(np.float32) for c in active}
            sigs = {c: Guarded(d, host_sig[c]) for c in active}
            for t in (0, 2, 4, 6, 9):
                runs = []
                for _ in range(2):
                    rows = [Guarded(d, np.full(n_pts, np.nan, np.float32)) for _ in range(3)]
                    capi.check(d.L.kw_element_source_rows_delayed(
                        d.ctx, _pointers([rows[c].ptr if c in active else None for c in range(3)]),
                        _pointers([sigs[c].ptr if c in active else None for c in range(3)]), _u64s(list(steps)), csr[0].ptr,
                        csr[1].ptr, csr[2].ptr, n_pts, n_el, t))
                    runs.append([r.read() for r in rows])
                    for r in rows:
                        r.free()
                for c in range(3):
                    if c not in active:
                        assert np.isnan(runs[0][c]).all(), (active, c)
                        continue
                    got = runs[0][c]
                    assert np.array_equal(got.view(np.uint32), runs[1][c].view(np.uint32)), "two launches differ"
                    live = (delays <= t) & (t - delays < steps[c])
                    s = np.where(live, host_sig[c][np.clip(t - delays, 0, steps[c] - 1), cols], np.float32(0.0)).astype(np.float32)
                    twin_signal.write(s)
                    twin = Guarded(d, np.full(n_pts, np.nan, np.float32))
                    capi.check(d.L.kw_element_source_row(d.ctx, twin.ptr, twin_signal.ptr, csr[0].ptr, twin_entries.ptr, n_pts,
                                                         nnz, 0))
                    assert np.array_equal(got.view(np.uint32), twin.read().view(np.uint32)), (active, c, t)
                    twin.free()
                    terms = w.astype(np.float64) * s.astype(np.float64)
                    ref = np.bincount(rows_of, weights=terms, minlength=n_pts)
                    mag = np.bincount(rows_of, weights=np.abs(terms), minlength=n_pts)
                    assert np.all(np.abs(got - ref) <= (np.array(lengths) + 1) * U * mag), (active, c, t)
                    if t >= steps[c] + max_delay:
                        assert np.all(got.view(np.uint32) == 0), (active, c, t)   # past flag + max delay: rows of +0
                    elif t == 2:
                        assert np.any(got != 0.0)
            for c in active:
                assert np.array_equal(sigs[c].read(), host_sig[c]), "signal changed"
        for g, h in zip(csr, (ptr.astype(np.uint32), capi.csr_entries(cols, w), delays.astype(np.uint32))):
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


def _delays(rng, els, top):
    out = [rng.integers(0, top + 1, i.size) for i, _ in els]
    out[0][:2] = [0, top]   # the whole range is there
    return out


def _signal(steps, scale, phase=0.0):
    t = np.arange(steps)[:, None]
    return (scale * np.sin(0.5 * t + phase + np.arange(5)[None, :]) * (1 + 0.3 * np.arange(5)[None, :])).astype(np.float32)


def _pressure_problem(syn, arrays, mode, nt=30, nt_src=20, n=32):
    """_weighted of test_gpu_element_arrays.py with delays 0..7 per entry"""
    pr = syn.make_problem(n, heterogeneous=True, nonlinear=False, absorbing=True, source="none", nt=nt, pml_size=4)
    rng = np.random.default_rng(3)
    els = _elements(rng, (n, n, n), 5, 60)
    ds = arrays.weighted_source(els, _signal(nt_src, 2.0e4), delays=_delays(rng, els, 7))
    pr.update(ds)
    pr["p_source_mode"] = _scalar(mode)
    return pr, ds


def _fma_rows(sig, ptr, col, w, delays):
    """the rows the delayed kernel forms, steps + max delay of them: fp32 fma in CSR order, skipped entries left out"""
    steps, top = sig.shape[0], int(delays.max())
    t = np.arange(steps + top)[:, None]
    acc = np.zeros((steps + top, ptr.size - 1), dtype=np.float32)
    for j in range(int(np.diff(ptr).max())):
        rows = np.nonzero(np.diff(ptr) > j)[0]
        e = ptr[rows] + j
        src = t - delays[e][None, :]
        live = (src >= 0) & (src < steps)
        s = sig[np.clip(src, 0, steps - 1), col[e][None, :]].astype(np.float64)
        acc[:, rows] = np.where(live, (w[e].astype(np.float64) * s + acc[:, rows]).astype(np.float32), acc[:, rows])
    return acc


def _csr_of(ds, q):
    return (ds[q + "_source_element_ptr"].reshape(-1).astype(np.int64), ds[q + "_source_element_index"].reshape(-1).astype(np.int64) - 1,
            ds[q + "_source_element_weight"].reshape(-1), ds[q + "_source_element_delay"].reshape(-1).astype(np.int64))


def _expanded_p(pr, series, rows=None):
    exp = {k: v for k, v in pr.items() if not k.startswith("p_source_element_")}
    series = series.reshape(-1, series.shape[-1])[:rows]
    exp["p_source_input"] = np.ascontiguousarray(series).reshape(1, series.shape[0], -1)
    exp["p_source_flag"] = _scalar(series.shape[0])
    exp["p_source_many"] = _scalar(1)
    return exp


# ---- 4. delayed sources = the expanded problem ------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_delayed_source_matches_expanded(mods, syn, orc, mode, fused):
    arrays, _, _, HostSolver = mods
    nt = 30
    pr, ds = _pressure_problem(syn, arrays, mode, nt=nt)
    sig = ds["p_source_element_input"].reshape(-1, 5)
    exact = arrays.expand_source(ds)
    assert exact.shape[1] == 20 + 7
    g = HostSolver(pr, fused_kernels=fused)
    e = HostSolver(_expanded_p(pr, _fma_rows(sig, *_csr_of(ds, "p"))), fused_kernels=fused)
    o = orc.OracleSim(_expanded_p(pr, exact))
    g.run(nt)
    assert g.scalar("fused_pipeline") == fused
    e.run(nt)
    o.step(nt)
    for f in ("p", "ux", "uy", "uz", "rhox"):
        a = g.field(f)
        assert rel_l2(a, o.field(f)) < TOL, f
        assert rel_l2(a, e.field(f)) < 1e-6, f
    g.close(), e.close(), o.close()


@pytest.mark.parametrize("fused", [0, 1])
def test_delayed_source_acts_past_its_flag(mods, syn, fused):
    """flag = 12, max delay 7: the source acts during steps 12..18.  The run equals the expanded one of 19 rows; the
    expanded input cut at row 12 gives another field (the rows 12..18 carry signals of the amplitude of the first 12)."""
    arrays, _, _, HostSolver = mods
    nt = 22
    pr, ds = _pressure_problem(syn, arrays, 2, nt=nt, nt_src=12)
    rows = _fma_rows(ds["p_source_element_input"].reshape(-1, 5), *_csr_of(ds, "p"))
    assert rows.shape[0] == 19 and np.any(rows[18] != 0.0)
    runs = []
    for problem in (pr, _expanded_p(pr, rows), _expanded_p(pr, rows, rows=12)):
        s = HostSolver(problem, fused_kernels=fused)
        s.run(nt)
        runs.append({f: s.field(f) for f in ("p", "ux", "rhox")})
        s.close()
    for f in ("p", "ux", "rhox"):
        assert rel_l2(runs[0][f], runs[1][f]) < 1e-6, f
        assert rel_l2(runs[0][f], runs[2][f]) > 100 * TOL, f


def _velocity_problem(syn, arrays, mode, nt, steps_x, steps_z, n=32):
    pr = syn.make_problem(n, heterogeneous=True, nonlinear=False, absorbing=True, source="none", nt=nt, pml_size=4)
    rng = np.random.default_rng(3)
    els = _elements(rng, (n, n, n), 5, 60)
    ds = arrays.weighted_velocity_source(els, signals_x=_signal(steps_x, 1.0e-2), signals_z=_signal(steps_z, 1.0e-2, 0.7),
                                         delays=_delays(rng, els, 7))
    pr.update(ds)
    pr["u_source_mode"] = _scalar(mode)
    return pr, ds


def _expanded_u(pr, series, cut=None):
    exp = {k: v for k, v in pr.items() if "_source_element_" not in k}
    for c, rows in series.items():
        rows = rows.reshape(-1, rows.shape[-1])[:(cut or {}).get(c)]
        exp[f"u{c}_source_input"] = np.ascontiguousarray(rows).reshape(1, rows.shape[0], -1)
        exp[f"u{c}_source_flag"] = _scalar(rows.shape[0])
    exp["u_source_many"] = _scalar(1)
    return exp


@pytest.mark.parametrize("mode,fused", [(0, 0), (2, 1), (0, 1), (1, 1)])
def test_delayed_velocity_source_with_two_flags(mods, syn, orc, mode, fused):
    """ux: flag 12, uz: flag 8, delays up to 7: each component acts for its own flag + 7 steps"""
    arrays, _, _, HostSolver = mods
    nt = 22
    pr, ds = _velocity_problem(syn, arrays, mode, nt, 12, 8)
    csr = _csr_of(ds, "u")
    fma = {c: _fma_rows(ds[f"u{c}_source_element_input"].reshape(-1, 5), *csr) for c in "xz"}
    assert fma["x"].shape[0] == 19 and fma["z"].shape[0] == 15
    exact = {c[1]: v for c, v in arrays.expand_velocity_source(ds).items()}
    assert exact["x"].shape[1] == 19 and exact["z"].shape[1] == 15
    g = HostSolver(pr, fused_kernels=fused)
    e = HostSolver(_expanded_u(pr, fma), fused_kernels=fused)
    cut = HostSolver(_expanded_u(pr, fma, cut={"x": 12, "z": 8}), fused_kernels=fused)
    o = orc.OracleSim(_expanded_u(pr, exact))
    for s in (g, e, cut):
        s.run(nt)
    o.step(nt)
    assert g.scalar("fused_pipeline") == fused
    for f in ("p", "ux", "uy", "uz", "rhox"):
        a = g.field(f)
        assert rel_l2(a, o.field(f)) < TOL, f
        assert rel_l2(a, e.field(f)) < 1e-6, f
        assert rel_l2(a, cut.field(f)) > 100 * TOL, f
    g.close(), e.close(), cut.close(), o.close()


# ---- 5. delayed sensors = the delayed weighted sum of the raw series -------------------------------------------------------
def _sensor_problem(syn, arrays, dims, nt, delayed=True, zero=False):
    """_sensor_problem of test_gpu_element_arrays.py plus delays 0..6"""
    nx, ny, nz = dims
    pr = syn.make_problem(nx, ny, nz, heterogeneous=True, nonlinear=True, absorbing=True, source="p0", nt=nt, pml_size=4)
    if nz == 1:
        pr = syn.as_2d_file(pr)
    rng = np.random.default_rng(5)
    els = _elements(rng, dims, 4, 40, lo=(8, 8, 8 if nz > 1 else 0), span=8)
    els.append((np.zeros(0, np.int64), np.zeros(0)))  # an empty element
    els.append((np.arange(0, nx * ny * nz, 7), rng.uniform(-1, 1, len(range(0, nx * ny * nz, 7)))))  # several chunks in 3-D
    delays = _delays(rng, els, 6)
    if zero:
        delays = [np.zeros_like(x) for x in delays]
    ds = arrays.weighted_sensor(els, delays=delays if delayed else None)
    pr.update(ds)
    union = np.unique(np.concatenate([i for i, _ in els]))
    pr["sensor_mask_type"] = _scalar(0)
    pr["sensor_mask_index"] = (union + 1).astype(U64).reshape(1, 1, -1)
    return pr, ds, union


@pytest.mark.parametrize("case", ["fused", "rocfft", "2d"])
def test_delayed_elements_match_delayed_weighted_raw(mods, syn, case):
    arrays, _, _, HostSolver = mods
    dims = (32, 32, 1) if case == "2d" else (32, 32, 32)
    nt, start = 24, 5
    pr, ds, union = _sensor_problem(syn, arrays, dims, nt)
    g = HostSolver(pr, fused_kernels=int(case != "rocfft"), p_raw=1, p_elements=1, u_raw=1, u_elements=1, sampling_start=start)
    g.run(nt)
    if case != "2d":
        assert g.scalar("fused_pipeline") == int(case == "fused")
    g.finish()
    pairs = [("p", "p_elements")] + [(f"u{c}", f"u{c}_elements") for c in ("xy" if case == "2d" else "xyz")]
    got = {n: g.stream(n) for pair in pairs for n in pair}
    g.close()
    mats = {d: W[:, union] for d, W in arrays.delayed_sensor_matrices(ds, int(np.prod(dims))).items()}
    assert sorted(mats) == list(range(7))
    k = np.diff(ds["sensor_element_ptr"].reshape(-1).astype(np.int64))
    groups = np.array([np.unique(ds["sensor_element_delay"].reshape(-1)[a:b]).size
                       for a, b in zip(np.cumsum(k) - k, np.cumsum(k))])
    for raw_name, el_name in pairs:
        raw, el = got[raw_name].astype(np.float64), got[el_name]
        assert raw.shape == (nt - start, union.size) and el.shape == (nt - start, 6), el_name
        for t in range(nt - start):
            ref, mag = np.zeros(6), np.zeros(6)
            for d, W in mats.items():
                if t - d >= 0:   # the field is not looked at before sampling starts
                    ref += W @ raw[t - d]
                    mag += np.abs(W) @ np.abs(raw[t - d])
            assert np.all(np.abs(el[t] - ref) <= (k + groups + 1) * U * mag), (el_name, t)
        assert np.all(el[:, 4] == 0.0) and np.all(np.any(el[:, [0, 1, 2, 3, 5]] != 0.0, axis=0)), el_name


def test_zero_sensor_delays_equal_the_run_without_them(mods, syn):
    arrays, _, _, HostSolver = mods
    nt, start = 16, 3
    flags = dict(p_elements=1, u_elements=1, u_non_staggered_elements=1, sampling_start=start)
    names = ["p_elements"] + [f"u{c}{kind}_elements" for kind in ("", "_non_staggered") for c in "xyz"]
    runs = []
    for delayed in (False, True):
        pr, ds, _ = _sensor_problem(syn, arrays, (32, 32, 32), nt, delayed=delayed, zero=True)
        assert ("sensor_element_delay" in pr) == delayed
        g = HostSolver(pr, **flags)
        g.run(nt)
        g.finish()
        runs.append({n: g.stream(n) for n in names})
        g.close()
    for n in names:
        assert runs[0][n].shape == (nt - start, 6) and np.any(runs[0][n] != 0.0), n
        assert np.array_equal(runs[0][n].view(np.uint32), runs[1][n].view(np.uint32)), n


# ---- 6. output file and checkpointed restart ------------------------------------------------------------------------------
def _file_problem(syn, arrays, nt):
    pr, _ = _pressure_problem(syn, arrays, 2, nt=nt)
    rng = np.random.default_rng(9)
    els = _elements(rng, (32, 32, 32), 3, 50, lo=(14, 14, 14))
    pr.update(arrays.weighted_sensor(els, delays=_delays(rng, els, 6)))
    return pr


def test_delayed_elements_output_file_and_restart(mods, syn, tmp_path):
    arrays, _, h5io, HostSolver = mods
    if not os.path.exists(h5io.H5_LIB_PATH):
        pytest.skip("HDF5 component not built")
    nt, split, start = 30, 13, 4
    pr = _file_problem(syn, arrays, nt)
    flags = dict(p_elements=1, u_elements=1, p_raw=1, sampling_start=start)
    streams = ("p_elements", "ux_elements", "uy_elements", "uz_elements")
    mem = HostSolver(pr, **flags)
    mem.run(nt)
    mem.finish()
    ref = {n: mem.stream(n) for n in streams}
    mem.close()
    # the file-less checkpoint: the ring travels behind the series
    a = HostSolver(pr, **flags)
    a.run(split)
    state = a.checkpoint_state()
    a.close()
    b = HostSolver(pr, **flags)
    b.restore_state(state)
    b.run(nt)
    b.finish()
    for n in streams:
        assert np.array_equal(b.stream(n).view(np.uint32), ref[n].view(np.uint32)), n
    b.close()
    path_in, whole, legs, ckpt = (str(tmp_path / n) for n in ("in.h5", "whole.h5", "legs.h5", "ckpt.h5"))
    h5io.write_input_file(pr, path_in)
    fs = h5io.FileSolver(path_in, output=whole, **flags)
    fs.run(nt)
    fs.finish()
    fs.write_output(whole)
    fs.close()
    for n in streams:
        got = h5io.read_dataset(whole, n)
        assert got.shape[-2:] == (nt - start, 3), n
        assert np.array_equal(got.reshape(ref[n].shape), ref[n]), n
    a = h5io.FileSolver(path_in, output=legs, **flags)
    a.run(split)
    a.write_checkpoint(ckpt)
    a.close()
    ring = h5io.read_dataset(ckpt, "Temp_p_elements").reshape(7, 3)   # 6 + 1 rows, the next row to emit first
    assert np.any(ring[:6] != 0.0) and np.all(ring[6] == 0.0)          # row 6 waits for step split + 6 alone: still +0
    b = h5io.FileSolver(path_in, output=legs, reopen_output=True, **flags)
    b.read_checkpoint(ckpt)
    assert b.t == split
    b.run(nt)
    b.finish()
    b.write_output(legs)
    b.close()
    for name in streams + ("p",):
        assert np.array_equal(h5io.read_dataset(legs, name), h5io.read_dataset(whole, name)), name


# ---- 7. slab run --------------------------------------------------------------------------------------------------------
def test_slab_run_with_delayed_source_and_sensor(mods, syn, tmp_path):
    arrays, _, h5io, _ = mods
    if not os.path.exists(h5io.H5_LIB_PATH):
        pytest.skip("HDF5 component not built")
    world, nt, start = 2, 18, 3
    pr = syn.make_problem(32, heterogeneous=True, nonlinear=False, absorbing=True, source="none", nt=nt, pml_size=4)
    rng = np.random.default_rng(13)
    box = _elements(rng, (32, 32, 32), 5, 60, lo=(10, 10, 12), span=8)   # z = 12..19: the source box straddles z = 16
    pr.update(arrays.weighted_source(box, _signal(8, 2.0e4), delays=_delays(rng, box, 7)))
    pr["p_source_mode"] = _scalar(2)
    sens = _elements(rng, (32, 32, 32), 2, 80, lo=(12, 12, 12), span=8) + _elements(rng, (32, 32, 32), 1, 30, lo=(4, 4, 1), span=6)
    pr.update(arrays.weighted_sensor(sens, delays=_delays(rng, sens, 6)))
    path_in, one, many = (str(tmp_path / n) for n in ("in.h5", "one.h5", f"slab{world}.h5"))
    h5io.write_input_file(pr, path_in)
    flags = dict(p_raw=1, p_elements=1)
    fs = h5io.FileSolver(path_in, sampling_start=start - 1, **flags)
    fs.run(nt)
    fs.finish()
    fs.write_output(one)
    fs.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29870 + world), "-m", "kwave_amd.run_slab", "-i", path_in, "-o", many,
           "-s", str(start), "--backend", "gloo"] + ["--" + f for f in flags]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       cwd=os.path.dirname(HERE), env=dict(os.environ, OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout[-4000:]
    for name in ("p", "p_elements"):
        a, b = h5io.read_dataset(many, name), h5io.read_dataset(one, name)
        assert a.shape == b.shape, name
        assert np.any(b != 0.0), name
        assert rel_l2(a, b) < TOL, name


# ---- 8. create-time refusals -----------------------------------------------------------------------------------------------
def _refusal_problem(syn, arrays):
    pr, _ = _pressure_problem(syn, arrays, 0, nt=10)
    rng = np.random.default_rng(2)
    els = _elements(rng, (32, 32, 32), 5, 30, lo=(16, 16, 16), span=8)
    pr.update(arrays.weighted_velocity_source(els, signals_x=_signal(6, 1.0e-2), delays=_delays(rng, els, 5)))
    pr["u_source_mode"] = _scalar(0)
    sens = _elements(rng, (32, 32, 32), 3, 20)
    pr.update(arrays.weighted_sensor(sens, delays=_delays(rng, sens, 6)))
    return pr


def _refusals(pr):
    def edit(drop=(), **kv):
        q = {k: v for k, v in pr.items() if not any(k.startswith(p) for p in drop)}
        q.update(kv)
        return q
    out = []
    for name in ("p_source_element_delay", "u_source_element_delay", "sensor_element_delay"):
        d = pr[name].reshape(-1)
        high = d.copy()
        high[3] = 65536
        out.append((name, "length", edit(**{name: d[:-1].reshape(1, 1, -1)})))
        out.append((name, "above the maximum", edit(**{name: high.reshape(1, 1, -1)})))
    n_p, n_u = pr["p_source_index"].size, pr["u_source_index"].size
    out.append(("p_source_element_delay", "without its CSR",
                edit(drop=("p_source_element_i", "p_source_element_p", "p_source_element_w"),
                     p_source_input=np.zeros((1, 20, n_p), np.float32), p_source_many=_scalar(1))))
    out.append(("u_source_element_delay", "without its CSR",
                edit(drop=("u_source_element_i", "u_source_element_p", "u_source_element_w", "ux_source_element_input"),
                     ux_source_input=np.zeros((1, 6, n_u), np.float32), u_source_many=_scalar(1))))
    out.append(("sensor_element_delay", "without its CSR",
                edit(drop=("sensor_element_i", "sensor_element_p", "sensor_element_w"))))
    return out


def test_malformed_delay_datasets_fail_at_create(mods, syn):
    arrays, capi, _, HostSolver = mods
    pr = _refusal_problem(syn, arrays)
    g = HostSolver(pr, p_elements=1)   # the well-formed input is accepted
    g.close()
    cases = _refusals(pr)
    assert len(cases) == 9
    for name, what, bad in cases:
        flags = {} if (name, what) == ("sensor_element_delay", "without its CSR") else {"p_elements": 1}
        with pytest.raises(capi.KWaveError, match=name):
            HostSolver(bad, **flags)
