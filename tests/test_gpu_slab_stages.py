"""The fused stages on Z-slabs (kw_fused_set_slab*) against the fp64 stage functions of oracle/kwave_np.py, with the ranks
as threads of this process (tests/slab_ranks.py): one capi.Device() per rank, host-staged exchange callbacks that meet at
a barrier, no RCCL, no P2P, no torch.distributed, and no kernel that waits for another rank.

A SlabGrid is test_gpu_stages.Grid spread over P ranks: the same random streams give the same global operators, fields and
media whatever P is; every real array goes to the ranks as z-slices between guard bands, the reduced operators as each
rank's ky rows of the symmetry-broken global operator (the transposed layout [nz_global][ny / P][nx/2 + 1]), the
derivative vectors whole, pml_z sliced.  A stage call runs on all ranks at once; outputs are stacked along z and compared
with the GLOBAL fp64 reference under the four bounds of test_gpu_stages.py (whole array, worst line, upper half of the
spectrum, x-Nyquist component), unchanged.  Read-only inputs are checked unchanged on every rank.  Only the C ABI is
used (no HostSolver).

Families (test_slab_*): the side array with packed y lines (96, L, 16) and transposed z lines (96, 16, L) on two ranks at
the nine RAGGED_LENGTHS; ragged (32, 72, L) / (32, L, 72) on four ranks (nyl = 18 resp. nz_local = 18, masked x tiles);
(100, 196, 72) on four (nyl = 49, no side array); (140, 252, 48) on three; (32, 16, 128) on eight (nyl = 2); one rank
exchanging with itself.  Each runs run_stages and one chained sequence under callback form 3 with the library's default
tuning, which the exchange log must show to be the batched schedule.

Schedules (test_slab_schedules): (96, 48, 64) on two ranks and (32, 72, 100) on four under S1 form 1, S2 form 2,
S3 form 3 batched, S4 unbatched one chunk, S5 two chunks, S6 four chunks, S7 slab_pipeline = 0, S8 batched without the
side array; stages and all three chained sequences; the log must show the schedule (chunk count by the library's rule:
(32, 72, 100) / 4 has 25 planes per rank and stays at one chunk).  Chained output equals unchained output bit for bit.
test_slab_abandoned_forward_exchange: a chained producer whose consumer never comes (drain_ahead), then
kw_fused_destroy / kw_fused_create / a stage.

Further entry points: kw_fused_shift_velocity on all three axes (axis 2 crosses the slabs) with the random Hermitian
filter and bounds of test_gpu_shift_lengths.py; kw_fused_density(terms 4, 5, 6) and kw_fused_absorption_pressure_one with
the bodies, references and TOL_P of test_gpu_absorption_lengths.py.

Two bit-level comparisons are printed per case on lines that start with SLABBITS (elements that differ in any bit): the
stacked slab result against a one-context run of the same global grid (every family case is followed by a case of its
own for it), and every schedule against the first schedule run on that grid.

Measured on an MI355X (worst whole array / worst line / upper half / x-Nyquist; bounds 2.2e-6 / 5e-6 / 2.1e-6 / 1.9e-6):
  (96, L, 16) on two ranks          4.5e-7 / 2.4e-6 / 4.5e-7 / 3.8e-7
  (96, 16, L) on two ranks          4.6e-7 / 2.4e-6 / 4.6e-7 / 3.7e-7
  ragged on four ranks              5.1e-7 / 1.8e-6 / 5.0e-7 / 4.2e-7
  (100, 196, 72) on four            4.4e-7 / 8.1e-7 / 4.3e-7 / -
  (140, 252, 48) on three           3.1e-7 / 1.1e-6 / 3.1e-7 / -
  (32, 16, 128) on eight            3.0e-7 / 1.6e-6 / 3.1e-7 / 3.0e-7
  one rank, (16, 16, 16)            3.2e-7 / 1.1e-6 / 3.1e-7 / -;  (96, 48, 64) 3.3e-7 / 8.2e-7 / 3.4e-7 / 3.6e-7
  S1-S8, (96, 48, 64) on two        4.7e-7 / 9.5e-7 / 4.7e-7 / 4.2e-7 (the same under every schedule)
  S1-S8, (32, 72, 100) on four      3.8e-7 / 1.2e-6 / 3.8e-7 / 3.5e-7 (the same under every schedule)
  abandoned forward exchange        2.4e-7 / 4.9e-7 / 2.6e-7 / 2.4e-7
  shift, all axes and grids         1.8e-7 / 2.7e-7 / 1.8e-7
  absorption epilogues              6.4e-7 / 1.7e-6 / 7.1e-7;  p under TOL_P = 1e-5: 6.5e-7
Every slab case lies within the bounds the same global grid meets on one context; none was changed.
Schedules against each other: 0 elements differ in all 14 comparisons (25.7 M and 30.2 M elements per grid): asserted
(BITS_BETWEEN_SCHEDULES).  Slabs against one context: 0 elements differ on 33 of the 40 grids; about 80 % of the elements
differ on the seven whose y lines are 48, 256, 512 or 1024 points long, (96, 256 | 512 | 1024, 16), (32, 256 | 512, 72),
(96, 48, 64) on one rank and on two, whatever the rank count.  The x kernels and the z-pass are the same instantiations
in both runs; the y-pass is not: one context runs k_ypass<L, DIR, false, false> / k_ypass_split<512, DIR, false, false>
(natural rows), a slab k_ypass<L, kFwd, false, true> and <L, kInv, true, false> (packed rows), separately compiled from
the same source, and at those four lengths the two come out with differently contracted arithmetic.  So that comparison
is printed, not asserted (BITS_VS_ONE_CONTEXT), and the fp64 bounds are the check.

Durations on the same machine: the slowest case 9.6 s ((96, 16, 1024) against fp64), the slowest one-context case 8.8 s;
the slowest stage test of the parent, mixed 140 x 252 x 48, took 12.4 s there.  No case lost its chained sequence or a
rank.  The whole file: 112 cases in about five minutes.

Mutations of csrc/kw_fused_main.hip (scratch builds, a subset of 34 cases of this file: every rank-count grid, both
schedule grids under S1-S8, the abandoned exchanges, two absorption cases, seven family grids, one shift case):
  (a) a.ky0 = 0 in launch_zfused: 29 of the 34 fail, every grid with more than one rank, errors of order 1 (velocity
      gradient du1 whole-array 1.03 on (96, 16, 16));
  (b) the side piece's offset 0 in xpieces_start: the 5 cases with plane chunks fail (S5, S6, both abandoned S5, absorption
      S5): 0.06 whole-array, 0.3 worst line in the velocity of (96, 48, 64);
  (c) z0 = 0 in the y-inverse of pslab_tail: the same 5 cases, errors of order 50.
tests/test_gpu_dist.py notices all three as well: test_slab_ranks_match_oracle[2-dims6-p0-0] fails under (a) only,
test_slab_schedules_agree[p0-...] in 5 of 8 cases under (a) and in the 3 chunked ones under (b) and (c).

Found by S7 here and fixed: with a piece callback that has a wait callback, the whole-array schedule (slab_pipeline = 0)
started the side array's piece on slot + KW_COMM_SLOTS and never waited for it (xwait of csrc/kw_fused_main.hip).
"""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
from gpu_buffers import Guarded, set_constants  # noqa: E402
from slab_ranks import COMM_SLOTS, RankGroup, device_copies, install  # noqa: E402
from test_gpu_stages import (CHAIN_KINDS, CHAIN_P, CHAIN_U, RAGGED_LENGTHS, TOL_LINE, TOL_UPPER, TOL_WHOLE, Checker,  # noqa: E402
                             Grid, metrics, run_chain, run_stages)
from test_gpu_absorption_lengths import BOTH, TOL_P, Recorder  # noqa: E402
from test_gpu_shift_lengths import random_hermitian_filter  # noqa: E402
import test_gpu_alpha_mode as one_term  # noqa: E402
import test_gpu_stokes as stokes  # noqa: E402

pytestmark = pytest.mark.gpu

# set from the first measurement on an MI355X (module docstring): assert the counts printed as SLABBITS to be zero
BITS_VS_ONE_CONTEXT = False
BITS_BETWEEN_SCHEDULES = True

gid = lambda d: "x".join(map(str, d))  # noqa: E731
ZSHIFT_SLOT = COMM_SLOTS - 1


def _nl_x_table():
    src = open(os.path.join(ROOT, "k-wave-fluid-cuda_amd", "csrc", "kw_fused.hip")).read()
    body = re.search(r"#else\nconstexpr int nl_x\(int L\)\n\{(.*?)\n\}\n", src, re.S).group(1)
    table = {}
    for cases, value in re.findall(r"((?:case \d+: ?)+)return (\d+);", body):
        for n in re.findall(r"case (\d+):", cases):
            table[int(n)] = int(value)
    assert re.search(r"default: return L >= 400 \? 8 : 16;", body)
    return table


NL_X = _nl_x_table()


def nl_x(n):
    return NL_X.get(n, 8 if n >= 400 else 16)


def chunk_rule(dims, P, asked):
    """the plane chunks create_impl grants: whole planes and whole x tiles per chunk, at most four"""
    nx, ny, nz = dims
    nzl, nch = nz // P, min(max(asked, 1), 4)
    while nch > 1 and (nzl % nch != 0 or (nzl // nch * ny) % (2 * nl_x(nx)) != 0):
        nch -= 1
    return nch


# ---- ranks ----------------------------------------------------------------------------------------------------------------
class SlabArray:
    """one array of every rank: "z" slices stacked along z, "same" a replica per rank, "own" per-rank data never read"""

    def __init__(self, parts, kind):
        self.parts, self.kind = parts, kind

    @property
    def ptr(self):
        return self  # SlabDev.call turns it into the rank's own pointer

    def read(self):
        got = [p.read() for p in self.parts]  # (checks every rank's guard bands)
        if self.kind == "z":
            return np.concatenate(got, axis=0)
        assert self.kind == "same"
        for x in got[1:]:
            assert np.array_equal(x.view(np.uint32), got[0].view(np.uint32)), "the ranks' replicas differ"
        return got[0]


class SlabDev:
    """stands where Grid has its one capi.Device: a call runs on every rank at once"""

    def __init__(self, grid):
        self.grid = grid

    def call(self, name, *args):
        devs = self.grid.devs

        def rank(r):
            devs[r].call(name, *[a.parts[r].ptr if isinstance(a, SlabArray) else a for a in args])
        self.grid.group.run(rank)

    def set_constants(self, k):
        """k describes the global grid (gpu_buffers.set_constants): every rank gets its own plane count"""
        from kwave_amd import capi
        g = self.grid
        assert (k.nx, k.ny, k.nz) == (g.nx, g.ny, g.nz)
        loc = capi.Constants.from_buffer_copy(k)
        loc.nz = loc.nz_complex = g.nzl
        loc.n_elements, loc.n_elements_complex = g.nx * g.ny * g.nzl, (g.nx // 2 + 1) * g.ny * g.nzl
        for d in g.devs:
            d.set_constants(loc)

    def sync(self):
        for d in self.grid.devs:
            d.sync()

    def close(self):
        for d in self.grid.devs:
            d.close()


class SlabGrid(Grid):
    def __init__(self, syn, dims, P, form=3, tuning=None, seed=0):
        self.P, self.form, self.tuning = P, form, dict(tuning or {})
        assert dims[1] % P == 0 and dims[2] % P == 0, (dims, P)
        self.nyl, self.nzl = dims[1] // P, dims[2] // P
        self._zvecs = []
        super().__init__(syn, dims, 1, seed)

    def open(self, plane_kernels):
        from kwave_amd import capi
        self.devs = [capi.Device() for _ in range(self.P)]
        self.group = RankGroup(self.P, *device_copies(self.devs))
        self.dev = SlabDev(self)
        return self.create()

    def create(self):
        from kwave_amd import capi
        nx, ny, nz = self.nx, self.ny, self.nz
        ok, n, sizes = C.c_int(), C.c_size_t(), set()
        for d in self.devs:
            set_constants(d, nx, ny, self.nzl, nz_global=nz)
            t = capi.default_tuning()
            for k, v in self.tuning.items():
                setattr(t, k, v)
            d.call("set_tuning", C.addressof(t))
        install(self.group, self.devs, self.form, nz)
        for d in self.devs:
            d.call("fused_supported", C.byref(ok))
            assert ok.value == 1, (nx, ny, nz, self.P)
            d.call("fused_create")
            d.call("fused_angular_elems", C.byref(n))
            sizes.add(n.value)
            d.call("fused_reduced_elems", C.byref(n))
        assert len(sizes) == 1 and sizes <= {(nx // 2 + 1) * ny, (nx // 2 + 1 + 15) // 16 * 16 * ny}, sizes
        self.side = sizes == {(nx // 2 + 1) * ny} and (nx // 2 + 1) % 16 != 0
        return n.value

    def recreate(self):
        """kw_fused_destroy forgets the slab description with everything else: set it again, as a new run would"""
        for d in self.devs:
            d.call("fused_destroy")
        self.group.forget_in_flight()
        self.create()

    def _array(self, host):
        sliced = any(host is z for z in self._zvecs)
        host = np.ascontiguousarray(host, dtype=np.float32)
        if host.shape == self.shape or sliced:
            return SlabArray([Guarded(d, host[r * self.nzl:(r + 1) * self.nzl]) for r, d in enumerate(self.devs)], "z")
        assert host.ndim <= 2, host.shape  # derivative vectors (complex as [n][2]), x / y PML, shift filters: whole on every rank
        return SlabArray([Guarded(d, host) for d in self.devs], "same")

    def import_reduced(self, host, n):
        parts = []
        for r, d in enumerate(self.devs):
            src = Guarded(d, host[:, r * self.nyl:(r + 1) * self.nyl, :])  # [nz_global][ny / P][nx/2 + 1]
            dst = Guarded(d, np.full(n, np.nan, dtype=np.float32))
            d.call("fused_import_reduced", dst.ptr, src.ptr)
            assert np.array_equal(src.read(), host[:, r * self.nyl:(r + 1) * self.nyl, :])
            parts.append(dst)
        return SlabArray(parts, "own")

    def vector(self, host):
        return self._array(host)

    def field(self, host):
        return self._array(host)

    def ro(self, host):
        g = self._array(host)
        self.readonly.append((g, np.asarray(host, dtype=np.float32).copy()))
        return g

    def pml_vectors(self):
        v = [np.ascontiguousarray(x, dtype=np.float32) for x in super().pml_vectors()]
        self._zvecs.append(v[2])  # (kept alive: recognised by identity when it is handed to ro())
        return v

    def starts(self):
        return self.group.starts(0)


class Keeper(Checker):
    """Checker that keeps every device result by its label, for the bit-level comparisons"""

    def __init__(self, axes, nyquist=False):
        super().__init__(axes, nyquist)
        self.got = {}

    def __call__(self, label, got, ref):
        assert label not in self.got, label
        self.got[label] = got
        super().__call__(label, got, ref)


class Collector(Keeper):
    """keeps the results and compares nothing: the one-context run's own fp64 check is test_gpu_stages.py"""

    def __call__(self, label, got, ref):
        self.got[label] = got

    def chain(self, label, chained, unchained):
        pass


def differing(a, b):
    """(elements that differ in any bit, elements) over the results two runs kept under the same labels"""
    assert a.keys() == b.keys()
    return (sum(int(np.count_nonzero(a[k].view(np.uint32) != b[k].view(np.uint32))) for k in a), sum(v.size for v in a.values()))


def report(tag, chk, t0):
    print("\nSLAB %s: worst whole %.3e line %.3e upper %.3e x-Nyquist %.3e; %.1f s" % ((tag,) + chk.worst() + (time.monotonic() - t0,)))
    bad = chk.failures()
    assert not bad, (tag, (TOL_WHOLE, TOL_LINE, TOL_UPPER), bad[:8])


# ---- what the exchange log must show --------------------------------------------------------------------------------------
def assert_schedule(g, name, chunks=1):
    """rank 0's log of a run of stages under schedule `name` (S1..S8 of the module docstring)"""
    starts = g.starts()
    waits = [e for e in g.group.log[0] if e[0] == "wait"]
    assert starts, "no exchange ran"
    for r in range(1, g.P):  # every rank ran the same sequence
        assert g.group.log[r] == g.group.log[0], f"rank {r} logged another sequence than rank 0"
    assert not any(g.group.in_flight), g.group.in_flight
    forms = {e[0] for e in starts}
    base = {e[1] % COMM_SLOTS for e in starts} - {ZSHIFT_SLOT}
    pieces = max(e[1] // COMM_SLOTS for e in starts) + 1          # pieces of the largest exchange
    strides = {e[2] for e in starts}
    per_array = 2 if g.side else 1
    whole = all(e[3] == 0 and e[4] == e[2] for e in starts)
    assert len(strides) == per_array, (name, strides)               # rows, and the side array's rows where there is one
    if name == "S1":
        assert forms == {1} and whole and not waits
        return
    assert len(waits) == len(starts), (name, len(waits), len(starts))
    if name == "S2":
        assert forms == {2} and whole and base <= {0, 1, 2} and pieces == per_array, (name, forms, base, pieces)
        return
    assert forms == {3}, (name, forms)
    if name == "S7":      # whole-array schedule: the arrays' own numbers as slots
        assert whole and base == {0, 1, 2} and pieces == per_array, (name, base, pieces)
    elif name in ("S3", "S8", "default"):  # batched: all arrays of a stage in one exchange per direction
        assert whole and base == {0, 12} and pieces == 3 * per_array, (name, base, pieces)
        assert (name == "S8") <= (not g.side)
    else:                 # S4, S5, S6: one exchange per array and chunk
        assert base >= {0, 4, 8, 12, 16, 20} and pieces == per_array, (name, base, pieces)
        part = [e for e in starts if e[4] != e[2]]
        if chunks == 1:
            assert whole
        else:
            assert part and all(e[4] * chunks == e[2] and e[3] % e[4] == 0 for e in part), (name, chunks)
            assert {e[3] // e[4] for e in part} == set(range(chunks)), name
            assert {e[1] % COMM_SLOTS for e in part} >= {12 + c for c in range(chunks)}, name  # chunk c of array 0 on its way back


# ---- families -------------------------------------------------------------------------------------------------------------
ONE_CONTEXT = {}  # dims -> results of a one-context run of the same global grid (kept for the cases that share a grid)


def one_context(syn, dims, chains):
    key = (dims, tuple(chains))
    if key not in ONE_CONTEXT:
        ONE_CONTEXT.clear()  # one grid's results at a time
        g = Grid(syn, dims)
        try:
            chk = Collector((0, 1, 2))
            run_stages(g, chk)
            for kind in chains:
                run_chain(g, chk, kind)
        finally:
            g.close()
        ONE_CONTEXT[key] = chk.got
    return ONE_CONTEXT[key]


def check_slab(syn, dims, P, chains, side=None, form=3, tuning=None, schedule="default", chunks=1):
    t0 = time.monotonic()
    g = SlabGrid(syn, dims, P, form, tuning)
    try:
        assert side is None or g.side == side, (dims, g.side)
        chk = Keeper((0, 1, 2), nyquist=g.side)
        run_stages(g, chk)
        for kind in chains:
            run_chain(g, chk, kind)
        g.check_readonly()
        assert_schedule(g, schedule, chunks)
    finally:
        g.close()
    report(f"{gid(dims)} P={P} {schedule}", chk, t0)
    return chk


def against_one_context(syn, dims, P, chains, got):
    n, of = differing(got, one_context(syn, dims, chains))
    print(f"\nSLABBITS {gid(dims)} P={P} against one context: {n} of {of} elements differ")
    if BITS_VS_ONE_CONTEXT:
        assert n == 0, (dims, P, n)


LAST_SLAB = {}  # (dims, P, chains) -> what the "fp64" case kept for the "one-context" case that follows it
# every family case is two: the slab run against fp64, then its kept results against a one-context run of the same grid
WHAT = pytest.mark.parametrize("what", ["fp64", "one-context"])


def family(syn, dims, P, chains, side, what):
    key = (dims, P, tuple(chains))
    if what == "fp64":
        LAST_SLAB.clear()
        LAST_SLAB[key] = check_slab(syn, dims, P, chains, side=side).got
        return
    got = LAST_SLAB.pop(key, None)
    if got is None:  # (run on its own)
        got = check_slab(syn, dims, P, chains, side=side).got
    against_one_context(syn, dims, P, chains, got)


SIDE_Y = [(96, n, 16) for n in RAGGED_LENGTHS]
SIDE_Z = [(96, 16, n) for n in RAGGED_LENGTHS]
RAGGED = [(32, 72, n) for n in RAGGED_LENGTHS if n != 1024] + [(32, n, 72) for n in RAGGED_LENGTHS if n not in (72, 1024)]


@pytest.mark.parametrize("dims", SIDE_Y, ids=gid)
@WHAT
def test_slab_side_array_packed_y_lines(syn, dims, what):
    """(96, L, 16) on two ranks: k_ypass / k_ypass_split with PIN / POUT at each length class, nyl = L / 2, the side piece"""
    family(syn, dims, 2, (CHAIN_KINDS[SIDE_Y.index(dims) % 3],), True, what)


@pytest.mark.parametrize("dims", SIDE_Z, ids=gid)
@WHAT
def test_slab_side_array_transposed_z_lines(syn, dims, what):
    """(96, 16, L) on two ranks: k_zfused* on exchanged rows with ky0 = 8, 32-column tiles at 240 / 400, the split at 512"""
    family(syn, dims, 2, (CHAIN_KINDS[(SIDE_Z.index(dims) + 1) % 3],), True, what)


@pytest.mark.parametrize("dims", RAGGED, ids=gid)
@WHAT
def test_slab_ragged(syn, dims, what):
    """(32, 72, L) and (32, L, 72) on four ranks: nyl = 18 (one side block and two positions) resp. nz_local = 18; the
    18 L resp. L 18 rows of a rank end in a masked x tile wherever that is no multiple of 32"""
    family(syn, dims, 4, (CHAIN_KINDS[(RAGGED.index(dims) + 2) % 3],), True, what)


@pytest.mark.parametrize("dims,P,side", [((100, 196, 72), 4, False), ((140, 252, 48), 3, False), ((32, 16, 128), 8, True),
                                         ((16, 16, 16), 1, False), ((96, 48, 64), 1, True)],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
@WHAT
def test_slab_rank_counts(syn, dims, P, side, what):
    """odd rows per rank (nyl = 49, radix 5 / 7), three ranks (nyl = 84), thin rows (nyl = 2 on eight ranks), and one rank
    exchanging with itself (packed rows are the natural rows)"""
    family(syn, dims, P, (CHAIN_KINDS[(dims[0] // 4) % 3],), side, what)


# ---- every schedule on two grids ------------------------------------------------------------------------------------------
SCHEDULES = {"S1": (1, {}), "S2": (2, {}), "S3": (3, dict(slab_batch=1)), "S4": (3, dict(slab_batch=0, slab_chunks=1)),
             "S5": (3, dict(slab_batch=0, slab_chunks=2)), "S6": (3, dict(slab_batch=0, slab_chunks=4)),
             "S7": (3, dict(slab_pipeline=0)), "S8": (3, dict(slab_batch=1, side_array=0))}
SCHEDULE_GRIDS = [((96, 48, 64), 2), ((32, 72, 100), 4)]
FIRST_SCHEDULE = {}  # (dims, P) -> (schedule, results) of the first schedule that ran on that grid


@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("dims,P", SCHEDULE_GRIDS, ids=lambda v: gid(v) if isinstance(v, tuple) else f"P{v}")
def test_slab_schedules(syn, dims, P, name):
    form, tuning = SCHEDULES[name]
    chunks = chunk_rule(dims, P, tuning.get("slab_chunks", 1))
    if dims == (96, 48, 64):
        assert chunks == tuning.get("slab_chunks", 1)  # 32 planes per rank: two and four chunks of whole x tiles
    chk = check_slab(syn, dims, P, CHAIN_KINDS, side=(name != "S8"), form=form, tuning=tuning, schedule=name, chunks=chunks)
    first, got = FIRST_SCHEDULE.setdefault((dims, P), (name, chk.got))
    if first != name:
        n, of = differing(chk.got, got)
        print(f"SLABBITS {gid(dims)} P={P} {name} against {first}: {n} of {of} elements differ")
        if BITS_BETWEEN_SCHEDULES:
            assert n == 0, (dims, P, name, first, n)


@pytest.mark.parametrize("dims,P", SCHEDULE_GRIDS, ids=lambda v: gid(v) if isinstance(v, tuple) else f"P{v}")
def test_slab_schedule_grids_against_one_context(syn, dims, P):
    """the two grids of test_slab_schedules, with all three chained sequences, against one context"""
    kept = FIRST_SCHEDULE.get((dims, P))
    got = kept[1] if kept else check_slab(syn, dims, P, CHAIN_KINDS, side=True, form=1, schedule="S1").got
    against_one_context(syn, dims, P, CHAIN_KINDS, got)


@pytest.mark.parametrize("name", ["S3", "S5"])
@pytest.mark.parametrize("producer", ["velocity", "absorption"])
def test_slab_abandoned_forward_exchange(syn, producer, name):
    """a chained stage starts the forward exchanges of a consumer that never comes: kw_fused_velocity(CHAIN_U) followed
    by an unchained kw_fused_velocity_gradient on other input, kw_fused_absorption_pressure(CHAIN_P) followed by
    kw_fused_scale_source (drain_ahead); then kw_fused_destroy / kw_fused_create / a stage"""
    dims, P = (96, 48, 64), 2
    form, tuning = SCHEDULES[name]
    t0 = time.monotonic()
    g = SlabGrid(syn, dims, P, form, tuning)
    try:
        chk = Checker((0, 1, 2), nyquist=True)
        for again in (False, True):
            tag = f"{producer} abandoned{' after re-creation' if again else ''}"
            before = len(g.starts())
            if producer == "velocity":
                got, ref, _ = g.velocity(g.noise(), [g.noise() for _ in range(3)], True, CHAIN_U)
                for a in range(3):
                    chk(f"{tag} u{a}", got[a], ref[a])
                ahead = len(g.starts())
                assert all(g.group.in_flight), "no forward exchange was started ahead"
                got, ref = g.velocity_gradient([g.noise() for _ in range(3)])
                for a in range(3):
                    chk(f"{tag} du{a} of other input", got[a], ref[a])
            else:
                p_dev, ref, _ = g.absorption(g.noise(), g.noise(), g.noise(), True, CHAIN_P)
                chk(f"{tag} p", p_dev.read(), ref)
                ahead = len(g.starts())
                assert all(g.group.in_flight), "no forward exchange was started ahead"
                got, ref = g.scale_source(g.noise())
                chk(f"{tag} scaled source", got, ref)
            # the producer did start forward exchanges ahead: the last pieces it logged go forward (slot below the first
            # backward one) and still wait for their consumer
            assert ahead > before and g.starts()[ahead - 1][1] % COMM_SLOTS < 12, g.starts()[ahead - 1]
            assert not any(g.group.in_flight), g.group.in_flight  # ... and the next stage waited for them
            if not again:
                g.recreate()
        got, ref = g.scale_source(g.noise())
        chk("scale source after re-creation", got, ref)
        g.check_readonly()
    finally:
        g.close()
    report(f"{gid(dims)} P={P} {name} {producer} abandoned", chk, t0)


# ---- kw_fused_shift_velocity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,P", [((96, 16, n), 2) for n in RAGGED_LENGTHS] + [((32, 72, 100), 4)],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else f"P{v}")
def test_slab_shift_velocity(syn, dims, P):
    """axes 0, 1 and 2 with the random Hermitian filter and the fp64 reference of test_gpu_shift_lengths.py; x and y lines
    are slab-local, axis 2 sends the real array through the exchange and back (two exchanges of nz_local * nyl * nx floats
    per peer and call)"""
    nx, ny, nz = dims
    rng = np.random.default_rng(7919 * nx + 31 * ny + nz)
    bits = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    g = SlabGrid(syn, dims, P)
    try:
        for axis in (0, 1, 2):
            n, ax = dims[axis], 2 - axis  # array axes are (z, y, x)
            h = random_hermitian_filter(rng, n)
            u = rng.standard_normal((nz, ny, nx)).astype(np.float32)
            full = n * np.fft.ifft(np.fft.fft(u.astype(np.float64), axis=ax) *
                                   h.astype(np.complex128).reshape([-1 if i == ax else 1 for i in range(3)]), axis=ax)
            ref = full.real
            assert np.linalg.norm(ref) > 0.0
            assert np.linalg.norm(full.imag) <= 1e-12 * np.linalg.norm(ref), "the filter is not Hermitian"
            d_h = g.vector(h.view(np.float32))
            d_in = g.field(u)
            d_out = g.field(rng.standard_normal(u.shape).astype(np.float32))
            before = len(g.starts())
            g.dev.call("fused_shift_velocity", axis, d_in.ptr, d_out.ptr, d_h.ptr)
            got = d_out.read()
            assert bits(d_in.read(), u), (dims, axis, "input changed")
            g.dev.call("fused_shift_velocity", axis, d_in.ptr, d_in.ptr, d_h.ptr)  # in place
            assert bits(d_in.read(), got), (dims, axis, "in-place result differs from the out-of-place one")
            assert bits(d_h.read(), h.view(np.float32)), (dims, axis, "filter changed")
            per_peer = g.nzl * g.nyl * nx * 4
            assert g.starts()[before:] == ([(3, ZSHIFT_SLOT, per_peer, 0, per_peer)] * 4 if axis == 2 else []), (dims, axis)
            w, ln, up = metrics(got, ref, (ax,))
            print(f"\nSLAB SHIFT {gid(dims)} P={P} axis {axis}: {w:.2e}/{ln:.2e}/{up:.2e}")
            assert w <= TOL_WHOLE and ln <= TOL_LINE and up <= TOL_UPPER, (dims, axis, w, ln, up)
        assert not any(g.group.in_flight)
    finally:
        g.close()


# ---- the absorption epilogues ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,P,name", [((96, 48, 64), 2, "S1"), ((96, 48, 64), 2, "S3"), ((96, 48, 64), 2, "S5"),
                                         ((32, 72, 100), 4, "S3")], ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_slab_absorption_epilogues(syn, dims, P, name):
    """kw_fused_density(terms = 4, 5, 6), plain and chained, and kw_fused_absorption_pressure_one: the bodies, combinations,
    references and bounds of test_gpu_absorption_lengths.check_grid on a slab grid"""
    form, tuning = SCHEDULES[name]
    t0 = time.monotonic()
    g = SlabGrid(syn, dims, P, form, tuning)
    try:
        rec = Recorder((0, 1, 2), False)
        loose = {}
        for nonlinear, arrays in BOTH:
            tag = f"nl={nonlinear} arrays={int(arrays)}"
            loose[f"stokes p {tag}"] = stokes.density_stage(g, nonlinear, arrays, rec)
            for which in (0, 1):
                errs = one_term.density_stage_terms(g, which, nonlinear, arrays, rec)
                loose[f"one-term which={which} p of both stages {tag}"] = errs["p"]
        for arrays in (False, True):
            for which in (0, 1):
                err, err2, _ = one_term.pressure_stage(g, which, arrays, rec)
                loose[f"two-term entry which={which} arrays={int(arrays)}"] = err2
        g.check_readonly()
        assert not any(g.group.in_flight), g.group.in_flight
    finally:
        g.close()
    report(f"ABSORPTION {gid(dims)} P={P} {name}", rec, t0)
    print(f"SLAB ABSORPTION {gid(dims)} P={P} {name}: loose p {max(loose.values()):.2e}")
    assert max(loose.values()) <= TOL_P, (dims, loose)
