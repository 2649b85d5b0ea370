"""The raw sampling kernels of csrc/kw_sampling_kernels.hip and the series shift of csrc/kw_fft.hip, each entry point
called on its own: kw_sample_index, kw_sample_index_multi, kw_sample_cuboid, kw_sample_all, kw_post_processing_rms,
kw_intensity_avg and kw_time_shift_series.

  * gather, max, min, the RMS step fma(v, v, buf) and sqrtf(buf * scale) bit for bit against the NumPy definitions of
    tests/sampling_reference.py (max / min are CUDA's fmaxf / fminf, the FMA and the square root are correctly rounded),
    on white noise and on fields of +-0, denormals, +-FLT_MIN, +-1, +-FLT_MAX, +-inf and NaN, over three "time steps",
    from the host's initial buffer values (0, 0, -FLT_MAX, +FLT_MAX) and from special values.  Where the reference
    result is NaN any NaN is accepted; nothing else is left out of a comparison;
  * kw_intensity_avg and kw_time_shift_series per element against fp64, |gpu - fp64| <= (k + 1) 2^-24 M.
Sizes are 1, 255, 256, 257 and n_big = cap + 257 + 1 with cap = CU count x 8 x 256 threads of the sampler grid, so the
grid-stride step runs and its last pass is partial.  Arrays sit between NaN guard bands (gpu_buffers.Guarded); read-only
inputs must come back byte-identical.
"""
import ctypes as C
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
from gpu_buffers import Guarded, check_bound, check_exact, report_worst, run  # noqa: E402
from sampling_reference import (DEN_MAX, DEN_MIN, FLT_MAX, FLT_MIN, INIT, SPECIAL, SPECIAL_NO_NAN, check_bits,  # noqa: E402
                                post_rms_ref, reduce_ref, special_field)

pytestmark = pytest.mark.gpu

F32 = np.float32
KW_OK, KW_ERR_INVALID = 0, 1
SIZES = [1, 255, 256, 257, "n_big"]
OPS = [0, 1, 2, 3]
OP_NAMES = {0: "none", 1: "rms", 2: "max", 3: "min"}
STEPS = 3  # "time steps" per case, each with another field


@pytest.fixture(scope="module")
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    report_worst(("raw ",))
    d.close()


def size_of(dev, n):
    """n_big: past the sampler grid's cap of CU count x 8 blocks of 256 threads, ragged, with a partial last pass"""
    if n != "n_big":
        return n
    cap = dev.info().compute_units * 8 * 256
    n_big = cap + 257 + 1
    assert n_big > cap
    return n_big


def rng_of(*parts):
    """a generator seeded by the case (strings by their characters: hash() is salted per process)"""
    return np.random.default_rng([sum(ord(c) * (i + 1) for i, c in enumerate(p)) if isinstance(p, str) else int(p)
                                  for p in parts])


def make_field(rng, kind, shape, op, step):
    """white noise (another scale at every step, so max / min / RMS move) or a field of special values (without NaN as an
    RMS input: every square is then finite in exact arithmetic or exactly inf)"""
    if kind == "noise":
        return (rng.standard_normal(shape) * (1.5 - step)).astype(F32)
    return special_field(rng, shape, SPECIAL_NO_NAN if op == 1 else SPECIAL)


def first_buffer(rng, start, op, n):
    """what the host gives a fresh stream buffer (0, 0, -FLT_MAX, +FLT_MAX), or special values"""
    return np.full(n, INIT[op], F32) if start == "host" else special_field(rng, n)


PASSES = [(kind, start) for kind in ("noise", "special") for start in ("host", "special")]


# ---- kw_sample_index --------------------------------------------------------------------------------------------------
def index_mask(rng, n):
    """(field size, mask): n indices in random order that include the first and the last field element; from n = 4 on a
    quarter of them appears twice (the kernel does not need unique indices)"""
    if n == 1:
        return 1, np.zeros(1, np.uint64)
    size = 2 * n + 7
    twice = n // 4 if n >= 4 else 0
    distinct = np.concatenate([[0, size - 1], 1 + rng.permutation(size - 2)[:n - twice - 2]])
    mask = np.concatenate([distinct, rng.permutation(distinct)[:twice]])
    assert mask.size == n and np.unique(mask).size == n - twice
    return size, rng.permutation(mask).astype(np.uint64)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", OPS, ids=OP_NAMES.get)
def test_sample_index(dev, orc, op, n):
    n = size_of(dev, n)
    rng = rng_of("index", op, n)
    size, mask = index_mask(rng, n)
    for kind, start in PASSES:
        buf = first_buffer(rng, start, op, n)
        for step in range(STEPS):
            src = make_field(rng, kind, size, op, step)
            out = run(dev, "sample_index", [op, ("buf", buf, False), ("src", src, True), ("mask", mask, True), n])
            want = reduce_ref(op, buf, src[mask.astype(np.int64)])
            if op == 1:  # the test's own FMA against glibc's correctly rounded fmaf: a difference is a bug in the test
                glibc = buf.copy()
                orc.sample_index(1, glibc, src, mask)
                check_bits(f"NumPy FMA against fmaf, {kind} from {start} step {step}", glibc, want)
            check_bits(f"{OP_NAMES[op]} n={n} {kind} from {start} step {step}", out["buf"], want)
            buf = out["buf"]


# ---- kw_sample_index_multi --------------------------------------------------------------------------------------------
OP_LISTS = [(0,), (2, 3), (1, 0), (3, 1, 2), (0, 1, 2, 3), (3, 2, 1, 0), (1, 1)]


def call_multi(dev, ops, bufs, src, mask, n, n_ops=None, null=None):
    """kw_sample_index_multi through guarded buffers: (status, buffers after the call); src and mask must be unchanged"""
    g_bufs = [Guarded(dev, b) for b in bufs]
    g_src, g_mask = Guarded(dev, src), Guarded(dev, mask, 0, np.uint64)
    c_ops = (C.c_int * len(ops))(*ops)
    c_ptrs = (C.c_void_p * len(ops))(*[None if i == null else g.ptr for i, g in enumerate(g_bufs)])
    status = dev.L.kw_sample_index_multi(dev.ctx, len(ops) if n_ops is None else n_ops, c_ops, c_ptrs, g_src.ptr, g_mask.ptr, n)
    outs = [g.read() for g in g_bufs]
    check_exact("multi: src", g_src.read(), src)
    check_exact("multi: mask", g_mask.read(), mask)
    for g in g_bufs + [g_src, g_mask]:
        g.free()
    return status, outs


@pytest.mark.parametrize("n", [257, "n_big"])
@pytest.mark.parametrize("ops", OP_LISTS, ids=["-".join(OP_NAMES[o] for o in ops) for ops in OP_LISTS])
def test_sample_index_multi(dev, ops, n):
    """1 to 4 operators in the orders OutputStreamContainer::sampleStreams can hand over (and rms twice, into two
    buffers): every buffer equals the reference and, bit for bit, what the single-operator entry point writes"""
    n = size_of(dev, n)
    rng = rng_of("multi", len(ops), *ops, n)
    size, mask = index_mask(rng, n)
    for kind, start in PASSES:
        bufs = [first_buffer(rng, start, op, n) for op in ops]
        for step in range(STEPS):
            src = make_field(rng, kind, size, 1 if 1 in ops else 0, step)
            status, outs = call_multi(dev, ops, bufs, src, mask, n)
            assert status == KW_OK
            for o, op in enumerate(ops):
                label = f"{OP_NAMES[op]} (buffer {o}) n={n} {kind} from {start} step {step}"
                check_bits(label, outs[o], reduce_ref(op, bufs[o], src[mask.astype(np.int64)]))
                single = run(dev, "sample_index", [op, ("buf", bufs[o], False), ("src", src, True), ("mask", mask, True), n])
                check_exact(label + " against kw_sample_index", outs[o], single["buf"])
            bufs = outs


# ---- kw_sample_cuboid -------------------------------------------------------------------------------------------------
GRID = (310, 12, 9)
MANY_ROWS = ((4, 259, 258), (1, 1, 1), (2, 257, 256))  # cy cz = 65 792 rows > 65 535: grid.y is clamped, the row loop runs


def box(tl, extent):
    return tuple(tl), tuple(t + e - 1 for t, e in zip(tl, extent))


# name -> (grid, top-left, bottom-right), 0-based inclusive (x, y, z)
CUBOIDS = {f"cx{cx}": (GRID,) + box((3, 2, 1), (cx, 8, 6)) for cx in (1, 255, 256, 257, 300)}
CUBOIDS.update({
    "whole-grid": (GRID, (0, 0, 0), (309, 11, 8)),
    "voxel-first": (GRID, (0, 0, 0), (0, 0, 0)),
    "voxel-last": (GRID, (309, 11, 8), (309, 11, 8)),
    "face-x-low": (GRID,) + box((0, 3, 2), (41, 6, 4)),
    "face-x-high": (GRID,) + box((269, 3, 2), (41, 6, 4)),
    "face-y-low": (GRID,) + box((5, 0, 2), (41, 5, 4)),
    "face-y-high": (GRID,) + box((5, 7, 2), (41, 5, 4)),
    "face-z-low": (GRID,) + box((5, 3, 0), (41, 6, 3)),
    "face-z-high": (GRID,) + box((5, 3, 6), (41, 6, 3)),
    "nz1": ((310, 12, 1), (4, 1, 0), (303, 10, 0)),
    "many-rows": (MANY_ROWS[0],) + box(MANY_ROWS[1], MANY_ROWS[2]),
})
PARTIAL = ("cx300", "many-rows")  # also run with n = product - 1, cx + 1 and 1 (test_sample_cuboid_partial)


def cuboid_slice(field, tl, br):
    return field[tl[2]:br[2] + 1, tl[1]:br[1] + 1, tl[0]:br[0] + 1].reshape(-1)


def u32(v):
    return np.array(v, np.uint32)


def run_cuboid(dev, op, name, count):
    """one cuboid at output pointers 4 and 12 bytes past a 256-byte boundary; count(product, cx) is n"""
    grid, tl, br = CUBOIDS[name]
    nx, ny, nz = grid
    cx, product = br[0] - tl[0] + 1, int(np.prod([b - t + 1 for t, b in zip(tl, br)]))
    n = count(product, cx)
    assert 1 <= n <= product
    rng = rng_of("cuboid", name, op, n)
    corners = [u32(tl), u32(br), u32(grid)]  # host arrays
    for offset in (4, 12):
        for kind, start in PASSES:
            buf = first_buffer(rng, start, op, product)
            for step in range(STEPS):
                src = make_field(rng, kind, (nz, ny, nx), op, step)
                out = run(dev, "sample_cuboid", [op, ("buf", buf, False, offset), ("src", src, True)]
                          + [c.ctypes.data for c in corners] + [n])
                want = buf.copy()
                want[:n] = reduce_ref(op, buf[:n], cuboid_slice(src, tl, br)[:n])
                label = f"{name} {OP_NAMES[op]} n={n} offset {offset} {kind} from {start} step {step}"
                check_bits(label, out["buf"], want)
                check_exact(label + ": elements from n on", out["buf"][n:], buf[n:])
                buf = out["buf"]


@pytest.mark.parametrize("name", list(CUBOIDS))
@pytest.mark.parametrize("op", OPS, ids=OP_NAMES.get)
def test_sample_cuboid(dev, op, name):
    """every shape, whole (n = the cuboid's size), against the NumPy slice field[z0:z1+1, y0:y1+1, x0:x1+1]; the output
    pointer is only 4-byte aligned, as CuboidOutputStream::sample hands it over (dst + the sizes of the cuboids before)"""
    run_cuboid(dev, op, name, lambda product, cx: product)


PARTIAL_COUNTS = {"product-1": lambda product, cx: product - 1, "cx+1": lambda product, cx: cx + 1, "one": lambda product, cx: 1}


@pytest.mark.parametrize("count", list(PARTIAL_COUNTS))
@pytest.mark.parametrize("name", PARTIAL)
@pytest.mark.parametrize("op", OPS, ids=OP_NAMES.get)
def test_sample_cuboid_partial(dev, op, name, count):
    """n below the cuboid's size (the kernel's i >= n exit): the elements from n on keep their bytes"""
    run_cuboid(dev, op, name, PARTIAL_COUNTS[count])


@pytest.mark.parametrize("op", OPS, ids=OP_NAMES.get)
def test_sample_cuboid_back_to_back(dev, op):
    """two cuboids into one buffer at the host's offsets (CuboidOutputStream::sample): the first has an odd size, so the
    second starts 4 bytes off an 8-byte boundary"""
    rng = rng_of("back-to-back", op)
    nx, ny, nz = GRID
    cuboids = [box((2, 3, 1), (7, 5, 3)), box((5, 0, 2), (300, 4, 2))]
    sizes = [int(np.prod([b - t + 1 for t, b in zip(tl, br)])) for tl, br in cuboids]
    assert sizes[0] % 2 == 1
    for kind, start in PASSES:
        buf = first_buffer(rng, start, op, sum(sizes))
        for step in range(STEPS):
            src = make_field(rng, kind, (nz, ny, nx), op, step)
            g_buf, g_src = Guarded(dev, buf, 4), Guarded(dev, src)
            want, at = buf.copy(), 0
            for (tl, br), n in zip(cuboids, sizes):
                c_tl, c_br, c_size = u32(tl), u32(br), u32(GRID)
                dev.call("sample_cuboid", op, g_buf.ptr + 4 * at, g_src.ptr, c_tl.ctypes.data, c_br.ctypes.data, c_size.ctypes.data, n)
                want[at:at + n] = reduce_ref(op, buf[at:at + n], cuboid_slice(src, tl, br))
                at += n
            got = g_buf.read()
            check_exact("back to back: src", g_src.read(), src)
            g_buf.free()
            g_src.free()
            check_bits(f"back to back {OP_NAMES[op]} {kind} from {start} step {step}", got, want)
            buf = got


# ---- kw_sample_all and kw_post_processing_rms ---------------------------------------------------------------------------
RMS_SCALES = [F32(1.0) / F32(3.0), F32(1.0), F32(2.0 ** -149) * F32(2.0 ** 23)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", OPS, ids=OP_NAMES.get)
def test_sample_all(dev, op, n):
    """operators 0-3 over the whole array; the RMS accumulator then goes through kw_post_processing_rms at every scale"""
    n = size_of(dev, n)
    rng = rng_of("all", op, n)
    for kind, start in PASSES:
        buf = first_buffer(rng, start, op, n)
        for step in range(STEPS):
            src = make_field(rng, kind, n, op, step)
            out = run(dev, "sample_all", [op, ("buf", buf, False), ("src", src, True), n])
            check_bits(f"{OP_NAMES[op]} n={n} {kind} from {start} step {step}", out["buf"], reduce_ref(op, buf, src))
            buf = out["buf"]
        if op == 1:
            for scale in RMS_SCALES:
                out = run(dev, "post_processing_rms", [("buf", buf, False), scale, n])
                check_bits(f"post_rms n={n} {kind} from {start} scale {scale!r}", out["buf"], post_rms_ref(buf, scale))


def test_post_processing_rms_hand_made(dev):
    """sqrtf(buf * scale) where a correctly rounded and an approximate square root differ: zeros, denormals, exact squares
    and their neighbours, 3.0, the largest finite value, and n_big values over every exponent.

    The reference is numpy.sqrt in float64 of the float32 product, rounded to float32: the argument has at most 24
    significant bits, and the float64 square root of such a number rounded to float32 is the correctly rounded float32
    square root, because double rounding cannot occur for sqrt of a 24-bit argument."""
    n_big = size_of(dev, "n_big")
    rng = rng_of("post_rms")
    squares = (np.arange(1, 4097, dtype=np.float64) ** 2).astype(F32)
    hand = np.concatenate([
        np.array([0.0, -0.0, DEN_MIN, 2 * DEN_MIN, 3 * DEN_MIN, DEN_MAX, FLT_MIN, 2 * FLT_MIN, 3.0, 2.0, 0.5, FLT_MAX, np.inf], F32),
        squares, np.nextafter(squares, F32(0)), np.nextafter(squares, F32(np.inf)),
        (squares * F32(2.0 ** -140)).astype(F32), (squares * F32(2.0 ** 100)).astype(F32)])
    with np.errstate(over="ignore"):  # a few values land on inf: sqrt(inf) = inf is part of the check
        wide = np.abs(rng.standard_normal(n_big) * np.exp2(rng.uniform(-149, 127, n_big))).astype(F32)
    buf = np.concatenate([hand, wide])
    out = run(dev, "post_processing_rms", [("buf", buf, False), F32(1.0), buf.size])
    check_bits("post_rms hand-made, scale 1", out["buf"], post_rms_ref(buf, 1.0))
    for scale in RMS_SCALES:
        out = run(dev, "post_processing_rms", [("buf", hand, False), scale, hand.size])
        check_bits(f"post_rms hand-made, scale {scale!r}", out["buf"], post_rms_ref(hand, scale))


# ---- kw_intensity_avg ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps,n", [(1, 1), (2, 257), (37, 513), (9, "n_big")])
def test_intensity_avg(dev, steps, n):
    """iavg[i] = (sum over the steps, in order, of u p) / steps against fp64 per element: k = steps + 1 (one rounding per
    product or fma and one per add, which is `steps` for the sum, and one for the divide), M the same sum on absolute
    values; p and u are read-only"""
    n = size_of(dev, n)
    rng = rng_of("intensity", steps, n)
    p = rng.standard_normal((steps, n)).astype(F32)
    u = rng.standard_normal((steps, n)).astype(F32)
    out = run(dev, "intensity_avg", [("iavg", rng.standard_normal(n).astype(F32), False), ("p", p, True), ("u", u, True), steps, n])
    prod = u.astype(np.float64) * p.astype(np.float64)
    ref, M = prod.sum(axis=0) / steps, np.abs(prod).sum(axis=0) / steps
    check_bound("raw intensity_avg", f"I_avg steps={steps} n={n}", out["iavg"], ref, M, steps + 1)
    ratio = float(np.max(np.abs(out["iavg"] - ref) / M)) / 2.0 ** -24
    print(f"\nkw_intensity_avg steps={steps} n={n}: worst |gpu - fp64| / (2^-24 M) = {ratio:.3f} (bound {steps + 2})")


# ---- kw_time_shift_series --------------------------------------------------------------------------------------------------
def half_step_shift(steps):
    """exp(i pi s(k) / steps), k = 0..steps/2, as the host computes it (KSpaceFirstOrderSolver.cpp:1253-1260), complex64"""
    k = np.arange(steps // 2 + 1)
    return np.exp(1j * np.pi * (((k + steps // 2) % steps) - steps // 2) / steps).astype(np.complex64)


@pytest.mark.parametrize("steps,n", [(2, 1), (3, 257), (16, 1000), (128, 70000), (37, 513)])
def test_time_shift_series(dev, steps, n):
    """series[step][i] through its spectrum along the step axis, X[k] *= shift[k] / steps, against
    irfft(rfft(u, axis=0) shift[:, None], steps, axis=0) in fp64.

    Power-of-two and small-prime lengths: per element |gpu - fp64| <= (k + 1) 2^-24 M in the form of
    test_gpu_unfused_kernels.py::test_fft_1d, k = 2 * 6 ceil(log2 steps) + 4 (two transforms, the complex multiply and
    the divider), M the DFT sum on absolute values carried through both transforms: each part of X[k] is bounded by
    S = sum over the steps of |u|, each part of X[k] shift[k] / steps by S (|Re shift| + |Im shift|) / steps, and the
    inverse adds both parts of every bin, the bins with a conjugate partner twice.
    steps = 37 takes another rocFFT algorithm whose rounding chain cannot be derived from this project: the tolerance is
    the one the project states for this kernel, 1e-5 of the series' maximum (tests/test_postprocess.py), and the ratio
    err / (2^-24 M) is printed for the record."""
    rng = rng_of("time_shift", steps, n)
    u = rng.standard_normal((steps, n)).astype(F32)
    shift = half_step_shift(steps)
    out = run(dev, "time_shift_series", [("series", u, False), ("shift", shift.view(F32), True), steps, n])
    s64 = shift.astype(np.complex128)
    ref = np.fft.irfft(np.fft.rfft(u.astype(np.float64), axis=0) * s64[:, None], steps, axis=0)
    w = np.full(steps // 2 + 1, 2.0)
    w[0] = 1.0
    if steps % 2 == 0:
        w[-1] = 1.0
    per_bin = (np.abs(s64.real) + np.abs(s64.imag)) / steps
    M = np.abs(u.astype(np.float64)).sum(axis=0, keepdims=True) * float(np.sum(w * 2.0 * per_bin)) * np.ones((steps, 1))
    err = np.abs(out["series"].astype(np.float64) - ref)
    ratio = float(np.max(err / M)) / 2.0 ** -24
    k = 2 * 6 * int(np.ceil(np.log2(steps))) + 4
    print(f"\nkw_time_shift_series steps={steps} n={n}: worst |gpu - fp64| / (2^-24 M) = {ratio:.3f}"
          + (f" (bound {k + 1})" if steps != 37 else f"; worst error / series maximum = {err.max() / np.abs(ref).max():.3e}"))
    if steps == 37:
        assert err.max() < 1e-5 * np.abs(ref).max()
    else:
        check_bound("raw time_shift_series", f"time shift steps={steps} n={n}", out["series"], ref, M, k)


# ---- argument checks -----------------------------------------------------------------------------------------------------
class Untouched:
    """guarded buffers that a refused call must leave as they are: bands and contents"""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def __call__(self, host, dtype=F32):
        host = np.ascontiguousarray(host, dtype=dtype)
        g = Guarded(self.dev, host, 0, dtype)
        self.items.append((g, host))
        return g.ptr

    def check(self):
        for g, host in self.items:
            check_exact("buffer of a refused call", g.read(), host)
            g.free()
        self.items = []


def test_invalid_arguments_write_nothing(dev):
    """every refused call returns KW_ERR_INVALID and writes nothing: cuboid corners out of order or outside the grid, n
    above the cuboid's size, 0 or 5 operators, a NULL buffer among several, operators outside the enum, no steps, a series
    of one step, and a series of 131 070 steps (65 536 spectrum rows, one above the launch's limit: refused before
    anything is allocated or launched)"""
    rng = rng_of("invalid")
    L, ctx, keep = dev.L, dev.ctx, Untouched(dev)
    noise = lambda n: rng.standard_normal(n).astype(F32)  # noqa: E731
    grid = (16, 12, 10)
    for tl, br, extra in [((5, 4, 3), (4, 6, 5), 0), ((5, 4, 3), (7, 3, 5), 0), ((5, 4, 3), (7, 6, 2), 0),   # br < tl
                          ((5, 4, 3), (16, 6, 5), 0), ((5, 4, 3), (7, 12, 5), 0), ((5, 4, 3), (7, 6, 10), 0),  # br == size
                          ((5, 4, 3), (7, 6, 5), 1)]:                                                          # n = product + 1
        n = max(1, int(np.prod([b - t + 1 for t, b in zip(tl, br)]))) + extra
        c_tl, c_br, c_size = u32(tl), u32(br), u32(grid)
        for op in OPS:
            status = L.kw_sample_cuboid(ctx, op, keep(noise(128)), keep(noise(int(np.prod(grid)))), c_tl.ctypes.data,
                                        c_br.ctypes.data, c_size.ctypes.data, n)
            assert status == KW_ERR_INVALID, (tl, br, n, op)
            keep.check()
    src, mask = noise(100), rng.permutation(100)[:40].astype(np.uint64)
    for ops, n_ops, null in [((0, 1, 2, 3), 0, None), ((0, 1, 2, 3), 5, None), ((0, 1, 2), None, 1), ((0, 4), None, None),
                             ((-1,), None, None)]:
        bufs = [noise(40) for _ in ops]
        status, outs = call_multi(dev, ops, bufs, src, mask, 40, n_ops=n_ops, null=null)
        assert status == KW_ERR_INVALID, (ops, n_ops, null)
        for got, b in zip(outs, bufs):
            check_exact("buffer of a refused kw_sample_index_multi", got, b)
    for op in (7, 4, -1):
        assert L.kw_sample_all(ctx, op, keep(noise(300)), keep(noise(300)), 300) == KW_ERR_INVALID
        assert L.kw_sample_index(ctx, op, keep(noise(40)), keep(src), keep(mask, np.uint64), 40) == KW_ERR_INVALID
        keep.check()
    assert L.kw_intensity_avg(ctx, keep(noise(50)), keep(noise(50)), keep(noise(50)), 0, 50) == KW_ERR_INVALID
    keep.check()
    for steps in (1, 131070):
        assert L.kw_time_shift_series(ctx, keep(noise(64)), keep(noise(64)), steps, 1) == KW_ERR_INVALID, steps
        keep.check()


def test_nothing_to_sample_is_not_an_error(dev):
    """n = 0 with NULL pointers returns KW_OK for every entry point"""
    L, ctx = dev.L, dev.ctx
    one_op = (C.c_int * 1)(0)
    for op in OPS:
        assert L.kw_sample_index(ctx, op, None, None, None, 0) == KW_OK
        assert L.kw_sample_cuboid(ctx, op, None, None, None, None, None, 0) == KW_OK
        assert L.kw_sample_all(ctx, op, None, None, 0) == KW_OK
    assert L.kw_sample_index_multi(ctx, 1, one_op, None, None, None, 0) == KW_OK
    assert L.kw_sample_index_multi(ctx, 1, None, None, None, None, 0) == KW_OK
    assert L.kw_post_processing_rms(ctx, None, 1.0, 0) == KW_OK
    assert L.kw_intensity_avg(ctx, None, None, None, 3, 0) == KW_OK
    assert L.kw_time_shift_series(ctx, None, None, 4, 0) == KW_OK
