"""Every fused stage entry point (kw_fused_velocity, _initial_velocity, _velocity_gradient, _density,
_absorption_pressure, _scale_source) at every fast-path line length, against the fp64 stage functions of
oracle/kwave_np.py on the same float32 inputs.

Inputs are white noise (every bin carries the same energy), each stage runs once with zero previous state (the output
is then the spectral term alone) and once with random state, and the operators are the generator's times a random real
factor per bin in [0.5, 1.5] that keeps the symmetry the real operators have (r[k] = r[N-k] for the y / z derivative
vectors; kappa, nabla1/2 and sourceKappa symmetric under (kz, ky) -> (-kz, -ky) on the kx = 0 and kx = Nx/2 planes), so
the |k| symmetry of the physical operators no longer hides a transposed or shifted operator read.  Every array the
stage touches sits between 4 KiB guard bands of 0xFF bytes (NaN): a kernel that writes outside an array fails the guard
check, one that reads outside it turns its result into NaN.  Read-only inputs are checked unchanged.

Per output three numbers are checked: the rel-L2 of the whole array, the worst rel-L2 over the lines along each tested
axis, and the rel-L2 of the error restricted to the upper half of that axis's spectrum (|f| >= 1/4).

Tolerances: at most 4x the worst value measured over the whole matrix below on an MI355X, never above 5e-6.  Measured
worst (every stage, variant and chained sequence; the largest in the linear chain's pressure, 864 x 16 x 48 and
896 x 108 x 1):
  whole array 5.5e-7 -> 2.2e-6;  upper half of the spectrum 5.4e-7 -> 2.1e-6;  worst line 2.2e-6 -> 5e-6 (the cap).
Per stage the worst line is 1.0e-6 (velocity), 9.9e-7 (initial velocity), 8.9e-7 (velocity gradient), 1.9e-6 (density),
7.7e-7 (absorption pressure), 8.2e-7 (scale source).  A chained call (KW_FUSED_CHAIN_U / U_IN_SCRATCH / CHAIN_TERMS /
TERMS_IN_SCRATCH / CHAIN_P / P_IN_SCRATCH) gave the unchained call's result bit for bit everywhere: that is asserted.

Grids with the x-Nyquist column kept apart (the side array: every Nx that is a multiple of 32, asserted at set-up from
kw_fused_angular_elems): (96, L, 16) and (96, 16, L) at every length, (32, 72, L) and (32, L, 72) at nine lengths whose 72
line positions end in a partial side block.  There a fourth number is checked per output, the rel-L2 over (z, y) of the
x-Nyquist component sum_x (-1)^x o[z, y, x]: with white-noise inputs it carries 1 / Nx of the energy, so a fault in a few
bins of the side array is diluted about tenfold in the whole-array figure and not at all in this one.  Measured worst on
these grids, under the same rule: whole array 5.6e-7 and upper half 5.5e-7 (96 x 16 x 504), worst line 1.8e-6
(32 x 72 x 240): the three bounds above stay as they are.  x-Nyquist component 4.9e-7 (96 x 504 x 16) -> 1.9e-6.  (With
a linear chain, which the two ragged grids of 1024 no longer run to stay within the time of the mixed grids,
32 x 1024 x 72 gave 5.8e-7, 5.8e-7 and 5.0e-7.)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
from oracle import kwave_np as knp  # noqa: E402
from gpu_buffers import BONA, C2, DT, DT_RHO0_SG, ETA, RHO0, TAU, Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_WHOLE = 2.2e-6
TOL_LINE = 5e-6
TOL_UPPER = 2.1e-6
TOL_NYQUIST = 1.9e-6

CHAIN_U, P_IN_SCRATCH = 1, 2           # kw_fused_velocity flags
U_IN_SCRATCH, CHAIN_TERMS = 1, 2       # kw_fused_density / kw_fused_velocity_gradient flags
TERMS_IN_SCRATCH, CHAIN_P = 1, 2       # kw_fused_absorption_pressure flags

ALPHA_POWER = 1.5


def _lengths():
    import re
    src = open(os.path.join(ROOT, "k-wave-fluid-cuda_amd", "csrc", "kw_fused.hip")).read()
    short = re.search(r"#define KW_FUSED_LENGTHS_SHORT\(X\)(.*?)\n#define", src, re.S).group(1)
    long_ = re.search(r"#define KW_FUSED_LENGTHS_LONG\(X\)(.*?)\n#if", src, re.S).group(1)
    no_tail = re.search(r"constexpr bool has_partial_x_tiles\(int L\)\n\{.*?\n\}\n", src, re.S).group(0)
    listed = [int(x) for x in re.findall(r"X\((\d+)\)", short + long_)]
    return listed, sorted({int(x) for x in re.findall(r"case (\d+):", no_tail)})


LENGTHS, NO_TAIL = _lengths()
AXIS_GRIDS = list(dict.fromkeys([(n, 16, 16) for n in LENGTHS] + [(16, n, 16) for n in LENGTHS] + [(16, 16, n) for n in LENGTHS]))
TWO_D_NY = 108  # no multiple of 16, 20, 24 or 32: every x tile size ends in a masked tile
TWO_D_GRIDS = [(n, TWO_D_NY, 1) for n in LENGTHS if n not in NO_TAIL]
MIXED_GRIDS = [(140, 252, 48), (864, 16, 48), (100, 196, 72)]
# Nx = 96: 48 main bins (three 16-column tiles; two 32-column tiles, the second half valid, at 240 and 400) and the
# x-Nyquist column apart as the side array, handled by one more tile index
SIDE_NX = 96
SIDE_GRIDS = list(dict.fromkeys([(SIDE_NX, n, 16) for n in LENGTHS] + [(SIDE_NX, 16, n) for n in LENGTHS]))
# 72 line positions: four and a half 16-position side blocks, two and a quarter 32-position ones.  The lengths: both with
# 32-column z tiles (240, 400), the shortest, both ends of the 512 split (512, 540), factors 3, 5 and 7, the longest
RAGGED_NX, RAGGED_POSITIONS = 32, 72
RAGGED_LENGTHS = (16, 72, 100, 240, 256, 400, 512, 540, 1024)
RAGGED_SIDE_GRIDS = list(dict.fromkeys([(RAGGED_NX, RAGGED_POSITIONS, n) for n in RAGGED_LENGTHS] +
                                       [(RAGGED_NX, n, RAGGED_POSITIONS) for n in RAGGED_LENGTHS]))


def _g(x):
    return x.ptr if hasattr(x, "ptr") else x


# ---- operators ----------------------------------------------------------------------------------------------------------
def _sym_vec(f):
    """f[k] = f[N-k]"""
    n = f.size
    return 0.5 * (f + f[(-np.arange(n)) % n])


def _sym_planes(f):
    """symmetric under (kz, ky) -> (-kz, -ky) on the kx = 0 and (even Nx) kx = Nx/2 planes"""
    nz, ny, _ = f.shape
    iz, iy = (-np.arange(nz)) % nz, (-np.arange(ny)) % ny
    for kx in (0, f.shape[2] - 1):
        pl = f[:, :, kx]
        f[:, :, kx] = 0.5 * (pl + pl[iz][:, iy])
    return f


def make_operators(syn, rng, nx, ny, nz):
    ops = syn.kspace_operators(nx, ny, nz, 1.0, 1.0, 1.0)
    out = {}
    for name in ("ddx_k_shift_pos_r", "ddx_k_shift_neg_r", "ddy_k_shift_pos", "ddy_k_shift_neg", "ddz_k_shift_pos",
                 "ddz_k_shift_neg"):
        c = knp._c(ops[name])
        f = rng.uniform(0.5, 1.5, c.size)
        if not name.startswith("ddx"):
            f = _sym_vec(f)
        c = (c * f).astype(np.complex64)
        out[name] = np.stack([c.real, c.imag], axis=-1).astype(np.float32)
    gen = knp.kspace_real_operators(nx, ny, nz, 1.0, 1.0, 1.0, 1.0, DT, ALPHA_POWER)
    for name in ("kappa", "source_kappa", "nabla1", "nabla2"):
        out[name] = (gen[name] * _sym_planes(rng.uniform(0.5, 1.5, gen[name].shape))).astype(np.float32)
    return out


# ---- metrics ------------------------------------------------------------------------------------------------------------
def metrics(got, ref, axes):
    """(whole rel-L2, worst line rel-L2, upper-half-spectrum rel-L2) of got against ref, the last two over `axes`."""
    got = got.astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite output"
    err = got - ref
    nref = np.linalg.norm(ref)
    if nref == 0.0:
        assert np.max(np.abs(got)) == 0.0
        return 0.0, 0.0, 0.0
    whole = float(np.linalg.norm(err) / nref)
    line = upper = 0.0
    for a in axes:
        n = ref.shape[a]
        e, r = np.moveaxis(err, a, -1).reshape(-1, n), np.moveaxis(ref, a, -1).reshape(-1, n)
        ln, rn = np.linalg.norm(e, axis=1), np.linalg.norm(r, axis=1)
        line = max(line, float(np.max(ln / np.maximum(rn, 1e-3 * np.sqrt(np.mean(rn ** 2))))))
        hi = np.abs(np.fft.fftfreq(n)) >= 0.25
        E, R = np.fft.fft(e, axis=1)[:, hi], np.fft.fft(r, axis=1)[:, hi]
        upper = max(upper, float(np.linalg.norm(E) / max(np.linalg.norm(R), 1e-30 * nref)))
    return whole, line, upper


def nyquist_error(got, ref):
    """rel-L2 over (z, y) of the x-Nyquist component sum_x (-1)^x o[z, y, x]: what the side array alone carries"""
    sign = 1.0 - 2.0 * (np.arange(ref.shape[2]) % 2)
    g, r = got.astype(np.float64) @ sign, ref @ sign
    nref = np.linalg.norm(r)
    if nref == 0.0:
        assert np.max(np.abs(g)) == 0.0
        return 0.0
    return float(np.linalg.norm(g - r) / nref)


class Checker:
    def __init__(self, axes, nyquist=False):
        self.axes, self.rows, self.nyquist = axes, [], ([] if nyquist else None)

    def __call__(self, label, got, ref):
        self.rows.append((label,) + metrics(got, ref, self.axes))
        if self.nyquist is not None:
            self.nyquist.append((label + " x-Nyquist", nyquist_error(got, ref)))

    def worst(self):
        """(whole, line, upper, x-Nyquist) maxima over the rows compared with fp64"""
        rows = [r[1:] for r in self.rows if not r[0].endswith("vs unchained")]
        return tuple(max(r[i] for r in rows) for i in range(3)) + (max((v for _, v in self.nyquist or []), default=0.0),)

    def chain(self, label, chained, unchained):
        """chained and unchained calls run the same arithmetic: the number of elements that differ in any bit"""
        self.rows.append((label + " vs unchained", float(np.count_nonzero(chained.view(np.uint32) != unchained.view(np.uint32))),
                          0.0, 0.0))

    def failures(self):
        bad = []
        for label, w, ln, up in self.rows:
            if label.endswith("vs unchained"):
                if w != 0.0:
                    bad.append((label, w))
            elif not (w <= TOL_WHOLE and ln <= TOL_LINE and up <= TOL_UPPER):
                bad.append((label, w, ln, up))
        bad += [(label, v) for label, v in self.nyquist or [] if not v <= TOL_NYQUIST]
        return bad


# ---- one grid -----------------------------------------------------------------------------------------------------------
class Grid:
    def __init__(self, syn, dims, plane_kernels=1, seed=0):
        import kwave_amd  # noqa: F401
        self.nx, self.ny, self.nz = nx, ny, nz = dims
        self.shape = (nz, ny, nx)
        self.two_d = nz == 1
        self.rng = np.random.default_rng(seed + 7919 * nx + 31 * ny + nz)
        n = self.open(plane_kernels)
        self.ops = make_operators(syn, self.rng, nx, ny, nz)
        self.padded = {name: self.import_reduced(self.ops[name], n) for name in ("kappa", "source_kappa", "nabla1", "nabla2")}
        self.dd = {k: self.vector(v) for k, v in self.ops.items() if k.startswith("dd")}
        b = lambda v, a: v.reshape([-1 if i == 2 - a else 1 for i in range(3)])  # noqa: E731  (x, y, z) -> [nz][ny][nx]
        # fp64 views of the float32 operators, broadcast over [nz][ny][nx(/2+1)]
        self.k64 = {k: self.ops[k].astype(np.float64) for k in ("kappa", "source_kappa", "nabla1", "nabla2")}
        self.dd_pos = [b(knp._c(self.ops[k]), a) for a, k in enumerate(("ddx_k_shift_pos_r", "ddy_k_shift_pos", "ddz_k_shift_pos"))]
        self.dd_neg = [b(knp._c(self.ops[k]), a) for a, k in enumerate(("ddx_k_shift_neg_r", "ddy_k_shift_neg", "ddz_k_shift_neg"))]
        self.bcast = b
        self.readonly = []

    # the device side of the set-up, which a slab grid (test_gpu_slab_stages.SlabGrid) spreads over its ranks
    def open(self, plane_kernels):
        """creates self.dev with the pipeline ready, sets self.side; returns the floats of one imported reduced array"""
        from kwave_amd import capi
        nx, ny, nz = self.nx, self.ny, self.nz
        self.dev = d = capi.Device()
        set_constants(d, nx, ny, nz)
        t = capi.default_tuning()
        t.plane_kernels = plane_kernels
        d.call("set_tuning", C.addressof(t))
        ok = C.c_int()
        d.call("fused_supported", C.byref(ok))
        assert ok.value == 1, (nx, ny, nz)
        d.call("fused_create")
        n = C.c_size_t()
        # a plane of the pipeline's layout: rows of Nx/2 bins and the x-Nyquist column behind them (the side array), or
        # rows of Nx/2 + 1 bins padded to whole 16-column tiles
        d.call("fused_angular_elems", C.byref(n))
        assert n.value in ((nx // 2 + 1) * ny, (nx // 2 + 1 + 15) // 16 * 16 * ny), ((nx, ny, nz), n.value)
        self.side = n.value == (nx // 2 + 1) * ny and (nx // 2 + 1) % 16 != 0
        d.call("fused_reduced_elems", C.byref(n))
        return n.value

    def import_reduced(self, host, n):
        """a reduced operator [nz][ny][nx/2+1] in the pipeline's layout (n floats)"""
        src = Guarded(self.dev, host)
        dst = Guarded(self.dev, np.full(n, np.nan, dtype=np.float32))
        self.dev.call("fused_import_reduced", dst.ptr, src.ptr)
        return dst

    def vector(self, host):
        """a derivative vector"""
        return Guarded(self.dev, host)

    # inputs
    def noise(self, scale=1.0):
        return (scale * self.rng.standard_normal(self.shape)).astype(np.float32)

    def field(self, host):
        return Guarded(self.dev, host)

    def ro(self, host):
        """a read-only input: checked unchanged at the end"""
        g = Guarded(self.dev, host)
        self.readonly.append((g, np.asarray(host, dtype=np.float32).copy()))
        return g

    def media(self, lo, hi):
        return self.rng.uniform(lo, hi, self.shape).astype(np.float32)

    def pml_vectors(self):
        v = [self.rng.uniform(0.5, 1.0, n).astype(np.float32) for n in (self.nx, self.ny, self.nz)]
        if self.two_d:
            v[2] = np.ones(1, np.float32)
        return v

    def comps(self, arrs):
        """in 2-D the z components are zero, as the solver keeps them"""
        return [np.zeros(self.shape, np.float32) if (self.two_d and a == 2) else x for a, x in enumerate(arrs)]

    def check_readonly(self):
        for g, host in self.readonly:
            assert np.array_equal(g.read().view(np.uint32), host.view(np.uint32)), "read-only input changed"

    def close(self):
        self.dev.close()

    # stages: each runs on the device and returns (outputs, fp64 references)
    def velocity(self, p_h, u_h, dt_arrays, flags=0, p_dev=None):
        pml = self.pml_vectors()
        dts = [self.media(0.5, 1.5) for _ in range(3)] if dt_arrays else [None] * 3
        p = p_dev if p_dev is not None else self.ro(p_h)
        u = [self.field(x) for x in u_h]
        dd = [self.dd[k] for k in ("ddx_k_shift_pos_r", "ddy_k_shift_pos", "ddz_k_shift_pos")]
        self.dev.call("fused_velocity", _g(p), *[x.ptr for x in u], *[self.ro(x).ptr if x is not None else None for x in dts],
                      *[self.ro(x).ptr for x in pml], self.padded["kappa"].ptr, *[x.ptr for x in dd], flags)
        dtr = [x.astype(np.float64) if x is not None else DT_RHO0_SG[a] for a, x in enumerate(dts)]
        ref = knp.stage_velocity(p_h.astype(np.float64), [x.astype(np.float64) for x in u_h], dtr,
                                 [self.bcast(x.astype(np.float64), a) for a, x in enumerate(pml)], self.k64["kappa"], self.dd_pos)
        return [x.read() for x in u], ref, (dts, pml)

    def initial_velocity(self, p_h, dt_arrays):
        dts = [self.media(0.5, 1.5) for _ in range(3)] if dt_arrays else [None] * 3
        u = [self.field(x) for x in self.comps([self.noise() for _ in range(3)])]  # write-only: garbage in (2-D: u_z stays 0)
        dd = [self.dd[k] for k in ("ddx_k_shift_pos_r", "ddy_k_shift_pos", "ddz_k_shift_pos")]
        self.dev.call("fused_initial_velocity", self.ro(p_h).ptr, *[x.ptr for x in u],
                      *[self.ro(x).ptr if x is not None else None for x in dts], self.padded["kappa"].ptr, *[x.ptr for x in dd])
        dtr = [x.astype(np.float64) if x is not None else DT_RHO0_SG[a] for a, x in enumerate(dts)]
        ref = knp.stage_initial_velocity(p_h.astype(np.float64), dtr, self.k64["kappa"], self.dd_pos)
        return [x.read() for x in u], ref

    def velocity_gradient(self, u_h, flags=0):
        du = [self.field(self.noise()) for _ in range(3)]
        dd = [self.dd[k] for k in ("ddx_k_shift_neg_r", "ddy_k_shift_neg", "ddz_k_shift_neg")]
        self.dev.call("fused_velocity_gradient", *[self.ro(x).ptr for x in u_h], *[x.ptr for x in du],
                      self.padded["kappa"].ptr, *[x.ptr for x in dd], flags)
        ref = knp.stage_velocity_gradient([x.astype(np.float64) for x in u_h], self.k64["kappa"], self.dd_neg)
        return [x.read() for x in du], ref

    def density(self, u_h, rho_h, nonlinear, terms, media_arrays, store_du, flags=0):
        """returns ({name: device result}, {name: fp64}), names rho0..2, du0..2, t0..2; with CHAIN_TERMS the t arrays
        the entry point leaves untouched are checked unchanged instead"""
        pml = self.pml_vectors()
        rho0 = self.media(0.8, 1.8) if media_arrays else None
        bona = self.media(0.2, 1.0) if media_arrays else None
        c2 = self.media(1.0, 3.0) if media_arrays else None
        rho = [self.field(x) for x in rho_h]
        du = [self.field(self.noise()) for _ in range(3)] if store_du else [None] * 3
        t_init = [self.noise() for _ in range(3)]
        t = [None] * 3
        if terms in (1, 2):
            t = [self.field(t_init[i]) for i in range(terms + 1)] + [None] * (2 - terms)
        elif terms == 3:
            t = [self.field(t_init[0]), self.ro(c2) if c2 is not None else None, None]
        dd = [self.dd[k] for k in ("ddx_k_shift_neg_r", "ddy_k_shift_neg", "ddz_k_shift_neg")]
        self.dev.call("fused_density", int(nonlinear), *[self.ro(x).ptr for x in u_h], *[x.ptr for x in rho],
                      *[self.ro(x).ptr for x in pml], _g(self.ro(rho0)) if rho0 is not None else None,
                      self.padded["kappa"].ptr, *[x.ptr for x in dd], *[_g(x) for x in du], terms,
                      _g(self.ro(bona)) if bona is not None else None, *[_g(x) for x in t], flags)
        f8 = lambda x, s: x.astype(np.float64) if x is not None else s  # noqa: E731
        ref = knp.stage_density([x.astype(np.float64) for x in u_h], [x.astype(np.float64) for x in rho_h],
                                [self.bcast(x.astype(np.float64), a) for a, x in enumerate(pml)], f8(rho0, RHO0), DT,
                                self.k64["kappa"], self.dd_neg, nonlinear, terms, f8(bona, BONA), f8(c2, C2))
        got, want = {}, {}
        for a in range(3):
            got[f"rho{a}"], want[f"rho{a}"] = rho[a].read(), ref["rho"][a]
            if store_du:
                got[f"du{a}"], want[f"du{a}"] = du[a].read(), ref["du"][a]
        # what the chained form stores of its terms (the rest goes to scratch and the t arrays stay as they were)
        stored = {0: [], 1: [0, 1], 2: [0, 1, 2], 3: [0]}[terms]
        if flags & CHAIN_TERMS:
            stored = {1: [0], 2: [1], 3: [0]}[terms]
        for i in range(3):
            if t[i] is None or (terms == 3 and i == 1):
                continue
            if i in stored:
                got[f"t{i}"], want[f"t{i}"] = t[i].read(), ref["t"][i]
            else:
                assert np.array_equal(t[i].read().view(np.uint32), t_init[i].view(np.uint32)), f"t{i} written under CHAIN_TERMS"
        return got, want, (rho0, bona, c2)

    def absorption(self, first_h, vgt_h, dsum_h, media_arrays, flags=0):
        c2 = self.media(1.0, 3.0) if media_arrays else None
        tau = self.media(0.5, 1.0) if media_arrays else None
        eta = self.media(0.2, 0.6) if media_arrays else None
        p = self.field(self.noise())  # write-only
        ins = [None, None] if flags & TERMS_IN_SCRATCH else [self.ro(vgt_h).ptr, self.ro(dsum_h).ptr]
        self.dev.call("fused_absorption_pressure", p.ptr, *ins, self.ro(first_h).ptr, self.padded["nabla1"].ptr,
                      self.padded["nabla2"].ptr, *[self.ro(x).ptr if x is not None else None for x in (c2, tau, eta)], flags)
        f8 = lambda x, s: x.astype(np.float64) if x is not None else s  # noqa: E731
        ref = knp.stage_absorption_pressure(first_h.astype(np.float64), vgt_h.astype(np.float64), dsum_h.astype(np.float64),
                                            self.k64["nabla1"], self.k64["nabla2"], f8(c2, C2), f8(tau, TAU), f8(eta, ETA))
        return p, ref, (c2, tau, eta)

    def scale_source(self, s_h):
        s = self.field(s_h)
        self.dev.call("fused_scale_source", s.ptr, self.padded["source_kappa"].ptr)
        return s.read(), knp.stage_scale_source(s_h.astype(np.float64), self.k64["source_kappa"])


def run_stages(g, chk):
    """every stage of one grid, unchained, with zero and with random previous state"""
    zero = [np.zeros(g.shape, np.float32) for _ in range(3)]
    p = g.noise()
    for label, u0, dt_arrays in (("velocity/zero u/dt arrays", zero, True), ("velocity/random u/dt scalars", g.comps([g.noise() for _ in range(3)]), False)):
        got, ref, _ = g.velocity(p, u0, dt_arrays)
        for a in range(3):
            chk(f"{label} u{a}", got[a], ref[a])
    for dt_arrays in (True, False):
        got, ref = g.initial_velocity(p, dt_arrays)
        for a in range(3):
            chk(f"initial velocity/dt arrays={dt_arrays} u{a}", got[a], ref[a])
    u = g.comps([g.noise() for _ in range(3)])
    got, ref = g.velocity_gradient(u)
    for a in range(3):
        chk(f"velocity gradient du{a}", got[a], ref[a])
    for nonlinear, terms, arrays, state, store_du in ((False, 0, True, False, True), (True, 0, False, True, False),
                                                      (False, 1, True, True, False), (True, 2, True, True, True),
                                                      (True, 2, False, False, False), (True, 3, True, True, False),
                                                      (False, 3, False, True, False)):
        rho = g.comps([g.noise(0.1) for _ in range(3)]) if state else zero
        got, want, _ = g.density(u, rho, nonlinear, terms, arrays, store_du)
        for k in got:
            chk(f"density/nl={int(nonlinear)} terms={terms} arrays={int(arrays)} state={int(state)} {k}", got[k], want[k])
    for arrays in (True, False):
        first, vgt, dsum = g.noise(), g.noise(), g.noise()
        p_dev, ref, _ = g.absorption(first, vgt, dsum, arrays)
        chk(f"absorption pressure/arrays={int(arrays)} p", p_dev.read(), ref)
    got, ref = g.scale_source(g.noise())
    chk("scale source", got, ref)


def run_chain(g, chk, kind):
    """velocity(CHAIN_U) -> density(U_IN_SCRATCH | CHAIN_TERMS) -> absorption(TERMS_IN_SCRATCH | CHAIN_P) ->
    velocity(P_IN_SCRATCH); kind "nonlinear" (terms 2) / "linear" (terms 1) / "lossless" (terms 3: density chains p).
    The unchained calls come first (they use the same scratch); every chained output is compared with fp64 and with them."""
    nonlinear = kind != "linear"
    terms = {"nonlinear": 2, "linear": 1, "lossless": 3}[kind]
    p0, u0 = g.noise(), g.comps([g.noise() for _ in range(3)])
    rho0_h = g.comps([g.noise(0.1) for _ in range(3)])
    rng_state = g.rng.bit_generator.state

    def sequence(chained):
        g.rng.bit_generator.state = rng_state  # the same media both times
        out = {}
        u1, ref, _ = g.velocity(p0, u0, True, CHAIN_U if chained else 0)
        for a in range(3):
            out[f"u{a}"] = (u1[a], ref[a])
        got, want, _ = g.density(u1, rho0_h, nonlinear, terms, True, False, (U_IN_SCRATCH | CHAIN_TERMS) if chained else 0)
        out.update({k: (got[k], want[k]) for k in got})
        if terms == 3:
            p_h = got["t0"]
            p_dev = g.field(p_h)
        else:
            # fp32 terms as the unchained density wrote them: the chained one left two of them in scratch only
            src = unchained_terms if chained else got
            first = got["t1"] if nonlinear else got["t0"]
            vgt = src["t2"] if nonlinear else src["t1"]
            dsum = src["t0"]
            p_dev, ref, _ = g.absorption(first, vgt, dsum, True, (TERMS_IN_SCRATCH | CHAIN_P) if chained else 0)
            p_h = p_dev.read()
            out["p"] = (p_h, ref)
        u2, ref, _ = g.velocity(p_h, u1, False, P_IN_SCRATCH if chained else 0, p_dev=p_dev if chained else None)
        for a in range(3):
            out[f"u{a} after p"] = (u2[a], ref[a])
        return out, got

    unchained_terms = {}
    plain, got = sequence(False)
    unchained_terms.update({k: v for k, v in got.items() if k.startswith("t")})
    chained, _ = sequence(True)
    for k, (v, ref) in chained.items():
        chk(f"chain {kind} {k}", v, ref)
        chk.chain(f"chain {kind} {k}", v, plain[k][0])


def check_grid(syn, dims, axes, chains, plane_kernels=1, side=False):
    """side: the grid must keep its x-Nyquist column as the side array, and that component is checked on its own"""
    g = Grid(syn, dims, plane_kernels)
    try:
        assert g.side or not side, dims
        chk = Checker(axes, nyquist=side)
        run_stages(g, chk)
        for kind in chains:
            run_chain(g, chk, kind)
        g.check_readonly()
        return chk
    finally:
        g.close()


def _assert_ok(chk, dims):
    print("%s: worst whole %.3e line %.3e upper %.3e x-Nyquist %.3e" % ((dims,) + chk.worst()))
    bad = chk.failures()
    assert not bad, (dims, bad[:8])


CHAIN_KINDS = ("nonlinear", "linear", "lossless")


@pytest.mark.parametrize("dims", AXIS_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_stages_every_length(syn, dims):
    """every length along x, y and z with the other two sides 16; one chained sequence per grid, in turn"""
    if dims == (16, 16, 16):
        _assert_ok(check_grid(syn, dims, (0, 1, 2), CHAIN_KINDS), dims)
        return
    axis = 2 - next(a for a in range(3) if dims[a] != 16)  # array axes are (z, y, x)
    _assert_ok(check_grid(syn, dims, (axis,), (CHAIN_KINDS[AXIS_GRIDS.index(dims) % 3],)), dims)


@pytest.mark.parametrize("dims", TWO_D_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_stages_masked_x_tiles_2d(syn, dims):
    """2-D grids whose Ny rows end in a partial x tile (TAIL kernels)"""
    _assert_ok(check_grid(syn, dims, (1, 2), (CHAIN_KINDS[TWO_D_GRIDS.index(dims) % 3],)), dims)


@pytest.mark.parametrize("dims", SIDE_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_stages_every_length_with_side_array(syn, dims):
    """(96, L, 16) and (96, 16, L): every y- and z-pass kernel at every length with three (at 240 and 400 along z: one
    and a half) main column tiles and the side block of the x-Nyquist column, whose lanes are line positions and whose
    operators k_import_reduced_side laid out per length; one chained sequence per grid, in turn"""
    axes = tuple(2 - a for a in (1, 2) if dims[a] != 16) or (0, 1)  # array axes are (z, y, x)
    _assert_ok(check_grid(syn, dims, axes, (CHAIN_KINDS[SIDE_GRIDS.index(dims) % 3],), side=True), dims)


@pytest.mark.parametrize("dims", RAGGED_SIDE_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_stages_ragged_side_blocks(syn, dims):
    """(32, 72, L) and (32, L, 72): 72 line positions end in a partial side block, in the z-pass (positions are ky) and in
    the y-pass (positions are z): the dead, masked and clamped lanes of tile_coord; one chained sequence per grid, in
    turn, but for the two grids of 1024"""
    chains = () if max(dims) == 1024 else (CHAIN_KINDS[RAGGED_SIDE_GRIDS.index(dims) % 3],)  # 2.4 M points: stages only
    _assert_ok(check_grid(syn, dims, (0, 1, 2), chains, side=True), dims)


def test_lengths_without_tails_refused_in_2d():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    try:
        for n in LENGTHS:
            set_constants(d, n, TWO_D_NY, 1)
            ok = C.c_int()
            d.call("fused_supported", C.byref(ok))
            assert ok.value == (0 if n in NO_TAIL else 1), n
    finally:
        d.close()


@pytest.mark.parametrize("plane", [1, 0])
@pytest.mark.parametrize("n", [32, 64])
def test_stages_whole_plane_kernels(syn, n, plane):
    _assert_ok(check_grid(syn, (n, n, n), (0, 1, 2), CHAIN_KINDS, plane), (n, plane))


@pytest.mark.parametrize("dims", MIXED_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_stages_mixed_grids(syn, dims):
    _assert_ok(check_grid(syn, dims, (0, 1, 2), CHAIN_KINDS), dims)


def test_fused_supported_matches_length_table():
    """kw_fused_supported of (n, 16, 16), (16, n, 16), (16, 16, n) for n = 8..1100 is true exactly for the listed n;
    2-D grids (n, Ny, 1) follow the no-tail rule (Ny rows a multiple of 16 for the ten lengths without masked tiles).
    No kernel runs."""
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    listed = set(LENGTHS)
    d = capi.Device()
    try:
        ok = C.c_int()
        for n in range(8, 1101):
            for dims in ((n, 16, 16), (16, n, 16), (16, 16, n)):
                set_constants(d, *dims)
                d.call("fused_supported", C.byref(ok))
                assert ok.value == (1 if n in listed else 0), dims
        for n in LENGTHS:
            for ny in (16, 48, 72, 108, 112):
                set_constants(d, n, ny, 1)
                d.call("fused_supported", C.byref(ok))
                assert ok.value == (0 if (n in NO_TAIL and ny % 16) else 1), (n, ny)
    finally:
        d.close()
