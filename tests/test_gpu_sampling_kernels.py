"""The compression, intensity, Q-term and divide kernels of csrc/kw_sampling_kernels.hip, each called on its own.

  * kw_sample_index_compress against fp64 accumulation in the statement order of IndexOutputStream.cpp:373-470, per
    element |gpu - fp64| <= (k + 1) 2^-24 M (k roundings on the longest path, M the same sums on absolute values);
  * the device 40-bit codec of kw_sample_index_compress_40b bit for bit against the host codec (kwh_pack_complex_40b /
    kwh_unpack_complex_40b, pinned to the reference by tests/golden/compress_ref*.npz).  The multipliers are taken from
    {0, +-1, +-2, +-0.5} and x keeps b x exact, so the device's fused multiply-add equals the host's multiply-then-add;
  * the same kernel with the real bases over one full series: one 17-bit code step of tolerance per step (the device may
    contract into an FMA where the host rounds the product);
  * kw_intensity_avg_c_accumulate (and _40b) per element against fp64, kw_q_term_sum and kw_divide bit for bit.
n reaches past the sampler grid's cap (CU count x 8 blocks of 256: 524 288 threads on an MI355X), so the grid-stride
step runs.  Arrays sit between NaN guard bands (gpu_buffers.Guarded); read-only inputs must come back unchanged.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
from gpu_buffers import Guarded, check_bound, check_exact, report_worst, run  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG_N = 600001  # > 524 288: past the grid-stride cap, ragged


@pytest.fixture(scope="module")
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    report_worst(("sample_index_compress", "intensity_avg_c"))
    d.close()


@pytest.fixture(scope="module")
def host():
    import kwave_amd  # noqa: F401
    from kwave_amd import solver
    L = solver.load_host()
    L.kwh_pack_complex_40b.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32]
    L.kwh_unpack_complex_40b.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32]
    return L


def host_pack(L, v, e):
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = np.zeros(v.shape[:-1] + (5,), np.uint8)
    assert L.kwh_pack_complex_40b(v.ctypes.data, v.size // 2, out.ctypes.data, e) == 0
    return out


def host_unpack(L, codes, e):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.zeros(codes.shape[:-1] + (2,), np.float32)
    assert L.kwh_unpack_complex_40b(codes.ctypes.data, codes.size // 5, out.ctypes.data, e) == 0
    return out


def field_and_mask(rng, n, values=None):
    """a field of 2n + 7 elements and a mask of n distinct indices in random order; src[mask] = values (or noise)"""
    size = 2 * n + 7
    src = rng.standard_normal(size).astype(np.float32)
    mask = rng.permutation(size)[:n].astype(np.uint64)
    if values is not None:
        src[mask.astype(np.int64)] = values
    return src, mask


# ---- kw_sample_index_compress (float accumulators) ----------------------------------------------------------------------
def compress_ref(c1, c2, x, b0, b1, mirror, alias):
    """IndexOutputStream.cpp:373-470 per (point, harmonic): c1 += bE x; c2 += bE_1 x; mirror: c2 += c1 (after the store
    of c1, so with c1 == c2 the second update starts from the first).  k: c1 2, c2 2 (+1 mirror, +1 alias)."""
    v1 = c1 + b0[None] * x[:, None, None]
    v2 = (v1 if alias else c2) + b1[None] * x[:, None, None]
    if mirror:
        v2 = v2 + v1
    return v1, v2


CASES = [(h, n, mirror, step, alias) for h in (1, 2, 5) for n in (1, 257) for mirror in (0, 1) for step in ("first", "last")
         for alias in (False, True)] + [(h, BIG_N, m, s, a) for h in (1, 2, 5) for m, s, a in ((0, "first", False), (1, "last", True))]


@pytest.mark.parametrize("harm,n,mirror,step,alias", CASES,
                         ids=[f"h{c[0]}-n{c[1]}-mirror{c[2]}-{c[3]}-{'c1==c2' if c[4] else 'c1!=c2'}" for c in CASES])
def test_sample_index_compress(dev, orc, harm, n, mirror, step, alias):
    rng = np.random.default_rng(n + 10 * harm + 100 * mirror + 1000 * alias)
    bE, bE1 = orc.compress_basis(20.0, 1, harm, False)
    bs = bE.shape[1]
    sl = 0 if step == "first" else bs - 1
    src, mask = field_and_mask(rng, n)
    x = src[mask.astype(np.int64)]
    c1 = rng.standard_normal((n, harm, 2)).astype(np.float32)
    c2 = c1.copy() if alias else rng.standard_normal((n, harm, 2)).astype(np.float32)
    common = [("src", src, True), ("mask", mask, True), n, harm, ("bE", bE, True), ("bE1", bE1, True), bs, sl, mirror]
    if alias:  # --no_overlap: one buffer passed as both c1 and c2
        g = Guarded(dev, c1)
        ins = [Guarded(dev, a, 0, a.dtype) for a in (src, mask, bE, bE1)]
        dev.call("sample_index_compress", g.ptr, g.ptr, ins[0].ptr, ins[1].ptr, n, harm, ins[2].ptr, ins[3].ptr, bs, sl, mirror)
        got1 = got2 = g.read()
        for a, h in zip(ins, (src, mask, bE, bE1)):
            assert np.array_equal(a.read().view(np.uint8), h.view(np.uint8))
            a.free()
        g.free()
    else:
        out = run(dev, "sample_index_compress", [("c1", c1, False), ("c2", c2, False)] + common)
        got1, got2 = out["c1"], out["c2"]
    b0, b1 = bE[:, sl].astype(np.float64), bE1[:, sl].astype(np.float64)
    v1, v2 = compress_ref(c1.astype(np.float64), c2.astype(np.float64), x.astype(np.float64), b0, b1, mirror, alias)
    M1, M2 = compress_ref(np.abs(c1.astype(np.float64)), np.abs(c2.astype(np.float64)), np.abs(x.astype(np.float64)),
                          np.abs(b0), np.abs(b1), mirror, alias)
    k2 = 2 + mirror + int(alias)
    if not alias:
        check_bound("sample_index_compress", "c1", got1, v1, M1, 2)
    check_bound("sample_index_compress", "c2", got2, v2, M2, k2)


# ---- device 40-bit codec, bit for bit ----------------------------------------------------------------------------------
MULTS = np.array([0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5], np.float32)


def codec_x(rng):
    """finite x for which 2x and x/2 stay normal and finite: random bit patterns over every such exponent, both signs,
    the golden edge values, +-0"""
    bits = rng.integers(0, 2 ** 32, 120000, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    ex = (bits >> 23) & 0xFF
    x = x[(ex >= 2) & (ex <= 253)]
    edges = np.load(os.path.join(GOLD, "compress_ref_edges.npz"))["edges_in"].reshape(-1)
    ee = (edges.view(np.uint32) >> 23) & 0xFF
    edges = edges[(ee >= 2) & (ee <= 253) | (edges == 0)]
    return rng.permutation(np.concatenate([x, edges, np.array([0.0, -0.0], np.float32)]))


def codec_x_denormal(rng):
    """denormal x (every exponent-less pattern scale), +-0 and some normal values: only multipliers 0 and +-1 apply"""
    m = rng.integers(1, 2 ** 23, 20000, dtype=np.uint64).astype(np.uint32)
    m[:23] = 1 << np.arange(23, dtype=np.uint32)
    den = (m | (rng.integers(0, 2, m.size).astype(np.uint32) << 31)).view(np.float32)
    return rng.permutation(np.concatenate([den, np.array([0.0, -0.0, 1.0, -3.5e-38, 2.5e38], np.float32)]))


def start_codes(rng, count, e):
    """zeros, random 5-byte patterns (every exponent nibble, some with all-zero mantissa fields) and the golden tables"""
    g = np.load(os.path.join(GOLD, "compress_ref.npz"))
    ge = np.load(os.path.join(GOLD, "compress_ref_edges.npz"))
    rnd = rng.integers(0, 256, (count, 5), dtype=np.uint64).astype(np.uint8)
    rnd[: count // 8, 0] &= 0xCF  # no top mantissa bits ...
    rnd[: count // 16, 1:] = 0    # ... and zero low fields: signed zeros with every exponent
    rnd[count // 16: count // 8, 1:3] = 0
    pool = np.concatenate([np.zeros((count // 8, 5), np.uint8), rnd, g[f"codec{e}_packed"], g[f"codec{138 if e == 114 else 114}_packed"],
                           ge[f"edges{e}_packed"], ge[f"codec{e}_repacked"]])
    return pool[rng.integers(0, len(pool), count)]


def emulate_40b(L, c1, c2, x, b0, b1, mirror, no_overlap, e):
    """host_pack(host_unpack(c) + b x) in float32 in the statement order of k_sample_index_compress_40b (sums of large x
    may overflow to +-Inf, which saturates like any value above the range)"""
    f = np.float32
    xx = x[:, None, None]
    u1 = host_unpack(L, c1, e)
    with np.errstate(over="ignore"):
        if no_overlap:
            return host_pack(L, (u1 + ((b0[None] * xx).astype(f) + (b1[None] * xx).astype(f)).astype(f)).astype(f), e), None
        u2 = host_unpack(L, c2, e)
        v1 = (u1 + (b0[None] * xx).astype(f)).astype(f)
        v2 = (u2 + (b1[None] * xx).astype(f)).astype(f)
        if mirror:
            v2 = (v2 + v1).astype(f)
    return host_pack(L, v1, e), host_pack(L, v2, e)


MODES_40B = [(0, 0), (1, 0), (0, 1)]


@pytest.mark.parametrize("e", [138, 114])
@pytest.mark.parametrize("mirror,no_overlap", MODES_40B, ids=["plain", "mirror", "no_overlap"])
@pytest.mark.parametrize("xs", ["normal", "denormal"])
def test_device_codec_bit_exact(dev, host, e, mirror, no_overlap, xs):
    rng = np.random.default_rng(e + 10 * mirror + 100 * no_overlap + (1000 if xs == "denormal" else 0))
    x = codec_x(rng) if xs == "normal" else codec_x_denormal(rng)
    n, harm, bs = x.size, 4, 6
    mults = MULTS if xs == "normal" else MULTS[:3]
    bE = mults[rng.integers(0, mults.size, (harm, bs, 2))]
    bE1 = mults[rng.integers(0, mults.size, (harm, bs, 2))]
    bE[0, :, 0], bE1[0, :, 1] = mults[1], mults[-1]  # every x meets a non-zero multiplier
    src, mask = field_and_mask(rng, n, x)
    c1 = start_codes(rng, n * harm, e).reshape(n, harm, 5)
    c2 = start_codes(rng, n * harm, e).reshape(n, harm, 5)
    for sl in (0, 2, bs - 1):
        out = run(dev, "sample_index_compress_40b",
                  [("c1", c1, False), ("c2", None if no_overlap else c2, False), ("src", src, True), ("mask", mask, True), n,
                   harm, ("bE", bE, True), ("bE1", bE1, True), bs, sl, mirror, no_overlap, e])
        w1, w2 = emulate_40b(host, c1, c2, x, bE[:, sl], bE1[:, sl], mirror, no_overlap, e)
        check_exact(f"c1 step {sl}", out["c1"], w1)
        if not no_overlap:
            check_exact(f"c2 step {sl}", out["c2"], w2)
            c2 = out["c2"]
        c1 = out["c1"]


@pytest.mark.parametrize("e", [138, 114])
@pytest.mark.parametrize("mirror,no_overlap", MODES_40B, ids=["plain", "mirror", "no_overlap"])
def test_compress_40b_real_bases_one_series(dev, host, orc, e, mirror, no_overlap):
    """one full b_size series of the real bases on random inputs; at every step the decoded device result and the host
    emulation from the device's previous codes differ by at most one 17-bit code step of the element's shared exponent"""
    rng = np.random.default_rng(e + mirror + 7 * no_overlap)
    harm, n = 3, 3001
    bE, bE1 = orc.compress_basis(12.0, 1, harm, True)
    bs = bE.shape[1]
    scale = 1.0e4 if e == 138 else 1.0e-2
    c1 = np.zeros((n, harm, 5), np.uint8)
    c2 = c1.copy()
    for sl in range(bs):
        src, mask = field_and_mask(rng, n)
        src *= np.float32(scale)
        x = src[mask.astype(np.int64)]
        out = run(dev, "sample_index_compress_40b",
                  [("c1", c1, False), ("c2", None if no_overlap else c2, False), ("src", src, True), ("mask", mask, True), n,
                   harm, ("bE", bE, True), ("bE1", bE1, True), bs, sl, mirror, no_overlap, e])
        w1, w2 = emulate_40b(host, c1, c2, x, bE[:, sl], bE1[:, sl], mirror, no_overlap, e)
        for name, want in (("c1", w1), ("c2", w2)):
            if want is None:
                continue
            got = out[name]
            step = np.exp2(np.maximum(got[..., 0] & 0xF, want[..., 0] & 0xF).astype(np.float64) + e - 143)[..., None]
            d = np.abs(host_unpack(host, got, e).astype(np.float64) - host_unpack(host, want, e).astype(np.float64))
            assert np.all(d <= step), (name, sl, float(np.max(d / step)))
        c1 = out["c1"]
        if not no_overlap:
            c2 = out["c2"]


# ---- intensity ------------------------------------------------------------------------------------------------------------
def intensity_ref(iavg, P, Uf):
    """IndexOutputStream.cpp:315-339: acc = iavg; acc += (p.re u.re + p.im u.im) / 2 per harmonic in order, k = 3 + H"""
    acc, accM = iavg.astype(np.float64), np.abs(iavg.astype(np.float64))
    P, Uf = P.astype(np.float64), Uf.astype(np.float64)
    for h in range(P.shape[1]):
        acc = acc + (P[:, h, 0] * Uf[:, h, 0] + P[:, h, 1] * Uf[:, h, 1]) / 2.0
        accM = accM + (np.abs(P[:, h, 0] * Uf[:, h, 0]) + np.abs(P[:, h, 1] * Uf[:, h, 1])) / 2.0
    return acc, accM


@pytest.mark.parametrize("harm", [1, 2, 3, 4])
def test_intensity_avg_c_accumulate(dev, harm):
    rng = np.random.default_rng(harm)
    n = BIG_N
    iavg = rng.standard_normal(n).astype(np.float32)
    P = rng.standard_normal((n, harm, 2)).astype(np.float32)
    Uf = rng.standard_normal((n, harm, 2)).astype(np.float32)
    out = run(dev, "intensity_avg_c_accumulate", [("iavg", iavg, False), ("P", P, True), ("U", Uf, True), n, harm])
    ref, M = intensity_ref(iavg, P, Uf)
    check_bound("intensity_avg_c", f"I_avg_c h={harm}", out["iavg"], ref, M, 3 + harm)


@pytest.mark.parametrize("harm", [1, 2, 3, 4])
def test_intensity_avg_c_accumulate_40b(dev, host, harm):
    rng = np.random.default_rng(10 + harm)
    n = BIG_N
    iavg = rng.standard_normal(n).astype(np.float32)
    P = host_pack(host, (1.0e3 * rng.standard_normal((n, harm, 2))).astype(np.float32), 138)
    Uf = host_pack(host, (1.0e-3 * rng.standard_normal((n, harm, 2))).astype(np.float32), 114)
    out = run(dev, "intensity_avg_c_accumulate_40b", [("iavg", iavg, False), ("P", P, True), ("U", Uf, True), n, harm, 138, 114])
    ref, M = intensity_ref(iavg, host_unpack(host, P, 138), host_unpack(host, Uf, 114))
    check_bound("intensity_avg_c_40b", f"I_avg_c 40-bit h={harm}", out["iavg"], ref, M, 3 + harm)


# ---- Q term and divide --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000, BIG_N])
@pytest.mark.parametrize("three_d", [True, False], ids=["3-D", "2-D"])
def test_q_term_sum(dev, n, three_d):
    """KSpaceFirstOrderSolver.cpp:2014-2026, exact: -((a + b) + c), 2-D (c = NULL) -(a + b)"""
    rng = np.random.default_rng(n + three_d)
    a, b, c = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    out = run(dev, "q_term_sum", [("out", rng.standard_normal(n).astype(np.float32), False), ("a", a, True), ("b", b, True),
                                  ("c", c if three_d else None, True), n])
    check_exact("Q", out["out"], -((a + b) + c) if three_d else -(a + b))


@pytest.mark.parametrize("n", [1, 1000, BIG_N])
def test_divide(dev, n):
    """exact: buf / divisor"""
    rng = np.random.default_rng(n)
    buf = rng.standard_normal(n).astype(np.float32)
    for divisor in (3.0, 7.3e-3, 1.0e30):
        out = run(dev, "divide", [("buf", buf, False), np.float32(divisor), n])
        check_exact(f"divide by {divisor}", out["buf"], buf / np.float32(divisor))
        buf = out["buf"]
