"""Every entry point of csrc/kw_solver_kernels.hip, and the 1-D FFT wrapper, called on its own against a float64
restatement of its header and the SolverCudaKernels.cu lines it cites.  That includes the kernels without a counterpart in
the reference, restated from include/kwave_hip.h alone: kw_sum_pressure_stokes_{nonlinear,linear} (Stokes absorption),
kw_sum_pressure_terms_one_{nonlinear,linear} and kw_compute_absorbtion_term_one (one-term power law).  The fused
epilogues are compared with the first four bit for bit (tests/test_gpu_absorption_lengths.py); both sides of that
comparison call one __device__ function, so the exact numpy float32 restatements here are what pins that function.

Inputs are white noise with O(1) media, PML vectors in (0, 1] and random complex ddx/ddy/ddz.  Every array sits between
NaN guard bands (gpu_buffers.Guarded); read-only inputs must come back unchanged.

Per-element checks, never rel-L2:
  * exact bits against a numpy float32 restatement in the reference's association order, for the kernels that have no
    product feeding a sum (nothing to contract into an FMA; divisions are correctly rounded, the HIP default that
    test_division_is_correctly_rounded pins in the ISA);
  * otherwise |gpu - fp64| <= (k + 1) * 2^-24 * M element by element, where k is the number of roundings on the longest
    path of the expression (written next to each reference) and M is the same expression in fp64 on absolute values.
A call through pointers offset by one element (4 bytes real, 8 bytes complex), one argument at a time and all together,
must give the aligned call's result bit for bit (V4 -> V1, P2 -> P1).  The one exception is compute_velocity_gradient,
whose P2 and P1 code fuse different products of the complex multiply into an FMA: that pair meets the fp64 bound only.

Grids (nx x ny x nz) and the variants they run:
  32x24x16 V4 / V4 / P2;  28x9x3 V4 / V4 / P1;  30x7x5 V1 / V1 / P2;  33x5x7 V1 / V1 / P1  (row / flat real / k-space)
  36x20x1, 35x13x1 the nz == 1 branches;  260x70x33 many blocks with a ragged last one;
  8x300x240 (non-uniform shift only): 72 000 rows -> chunked launches with a partial last chunk.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
from gpu_buffers import Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ALIGNED_GRIDS = [(32, 24, 16), (28, 9, 3)]
GRIDS = ALIGNED_GRIDS + [(30, 7, 5), (33, 5, 7), (36, 20, 1), (35, 13, 1), (260, 70, 33)]
gid = lambda d: "x".join(map(str, d))  # noqa: E731
WORST = {}  # (family, k) -> worst |gpu - fp64| / (2^-24 M) seen, against its k + 1


@pytest.fixture(scope="module")
def dev():
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    yield d
    if WORST:
        print("\nworst |gpu - fp64| / (2^-24 M) per kernel family (bound k + 1):")
        for (fam, k), r in sorted(WORST.items()):
            print(f"  {fam:34s} k = {k:2d}: {r:6.3f}  (bound {k + 1})")
    d.close()


# ---- arguments and calls -----------------------------------------------------------------------------------------------
class Arg:
    """one pointer argument: host data (None -> NULL), read-only or not, complex (8-byte elements) or real"""

    def __init__(self, name, host, ro=False, cplx=False, dtype=np.float32):
        self.name, self.host, self.ro, self.cplx, self.dtype = name, host, ro, cplx, dtype


def call(dev, entry, items, shift=()):
    """kw_<entry>(ctx, *items) with every Arg in its own guarded buffer; the Args named in `shift` (or all, "all") start
    one element past the aligned interior.  Returns {name: array after the call} of the written arguments."""
    bufs, conv = [], []
    for it in items:
        if not isinstance(it, Arg):
            conv.append(it)
            continue
        if it.host is None:
            conv.append(None)
            continue
        off = 0
        if shift == "all" or it.name in shift:
            off = 8 if it.cplx else np.dtype(it.dtype).itemsize
        g = Guarded(dev, it.host, off, it.dtype)
        bufs.append((g, it))
        conv.append(g.ptr)
    dev.call(entry, *conv)
    out = {}
    for g, it in bufs:
        v = g.read()
        g.free()
        if it.ro:
            assert np.array_equal(v.view(np.uint8), np.ascontiguousarray(it.host, it.dtype).view(np.uint8)), \
                f"{entry}: read-only {it.name} changed"
        else:
            out[it.name] = v
    return out


def pointer_names(items):
    return [it.name for it in items if isinstance(it, Arg) and it.host is not None and it.dtype == np.float32]


def check_exact(label, got, want):
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} elements differ; first at {tuple(i)}: "
                             f"got {got[tuple(i)]!r}, want {want[tuple(i)]!r}")


def check_bound(family, label, got, ref, M, k):
    """|got - ref| <= (k + 1) 2^-24 M element by element"""
    got = got.astype(np.float64)
    err = np.abs(got - ref)
    ok = err <= (k + 1) * U * M
    if not ok.all():
        i = np.argwhere(~ok)[0]
        raise AssertionError(f"{label}: {int((~ok).sum())} of {ok.size} elements outside (k+1) 2^-24 M, k = {k}; first at "
                             f"{tuple(i)}: got {got[tuple(i)]!r}, fp64 {ref[tuple(i)]!r}, M {M[tuple(i)]!r}")
    ratio = float(np.max(np.where(M > 0, err / np.where(M > 0, M, 1.0) / U, 0.0)))
    WORST[(family, k)] = max(WORST.get((family, k), 0.0), ratio)


def check_variants(dev, entry, items, base, names=None, bound=None):
    """the call through misaligned pointers, each argument alone and then all together, equals `base` bit for bit
    (or, where `bound` is given, meets the fp64 bound that bound(outputs) checks)"""
    for sh in [(n,) for n in (names or pointer_names(items))] + ["all"]:
        out = call(dev, entry, items, sh)
        if bound is not None:
            bound(out)
            continue
        for k, v in base.items():
            check_exact(f"{entry} shift={sh} {k} vs aligned", out[k], v)


# ---- grid data -----------------------------------------------------------------------------------------------------------
class G:
    def __init__(self, dev, dims, seed=0):
        self.nx, self.ny, self.nz = dims
        self.dims = dims
        self.shape = (self.nz, self.ny, self.nx)
        self.nxc = self.nx // 2 + 1
        self.cshape = (self.nz, self.ny, self.nxc)
        self.k = set_constants(dev, *dims)
        self.rng = np.random.default_rng(seed + 7919 * self.nx + 31 * self.ny + self.nz)
        self.aligned = dims in ALIGNED_GRIDS

    def c(self, name):
        """a float32 constant of kw_constants, as float64"""
        return float(np.float32(getattr(self.k, name)))

    def noise(self, shape=None):
        return self.rng.standard_normal(shape or self.shape).astype(np.float32)

    def media(self, lo=0.5, hi=1.5, shape=None):
        return self.rng.uniform(lo, hi, shape or self.shape).astype(np.float32)

    def pml(self):
        return [(1.0 - self.rng.uniform(0.0, 1.0, n)).astype(np.float32) for n in (self.nx, self.ny, self.nz)]

    def cnoise(self, shape):
        return self.rng.standard_normal(tuple(shape) + (2,)).astype(np.float32)

    def bcast(self, v, axis):
        """a per-axis vector (x, y, z) broadcast over [nz][ny][nx]"""
        return v.astype(np.float64).reshape([-1 if i == 2 - axis else 1 for i in range(3)])


f8 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
A = np.abs


def cplx(a):
    return f8(a[..., 0]) + 1j * f8(a[..., 1])


def split(z):
    return np.stack([z.real, z.imag], axis=-1)


def cmul_ref(a, b, s=-1.0):
    """cuCmulf on (re, im) pairs in fp64; s = +1 with absolute inputs gives M"""
    return np.stack([a[..., 0] * b[..., 0] + s * a[..., 1] * b[..., 1], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


# ---- real-space row kernels ------------------------------------------------------------------------------------------------
def velocity_ref(g, u, gr, d, pml, s=-1.0):
    """SolverCudaKernels.cu:184-215 / :278-308.  Heterogeneous: (u pml - (fd g) d) pml, k = 4 (fd*g, *d, -, *pml);
    homogeneous: dtRho0Sg fd computed in float, (u pml - div g) pml, k = 4"""
    fd = g.c("fft_divider")
    out = []
    for a in range(3):
        p = g.bcast(pml[a], a)
        if d is None:
            div = (g.c(("dt_rho0_sgx", "dt_rho0_sgy", "dt_rho0_sgz")[a]) * fd)
            ifft = div * f8(gr[a])
        else:
            ifft = fd * f8(gr[a]) * f8(d[a])
        out.append((f8(u[a]) * p + s * ifft) * p)
    return out


@pytest.mark.parametrize("het", [True, False], ids=["het", "homog"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_compute_velocity(dev, dims, het):
    g = G(dev, dims)
    u, gr = [g.noise() for _ in range(3)], [g.noise() for _ in range(3)]
    d = [g.media() for _ in range(3)] if het else None
    pml = g.pml()
    items = [Arg(f"u{a}", u[a]) for a in range(3)] + [Arg(f"g{a}", gr[a], ro=True) for a in range(3)] + \
            [Arg(f"d{a}", d[a] if het else None, ro=True) for a in range(3)] + [Arg(f"pml{a}", pml[a], ro=True) for a in range(3)]
    out = call(dev, "compute_velocity", items)
    ref = velocity_ref(g, u, gr, d, pml)
    M = velocity_ref(g, [A(x) for x in u], [A(x) for x in gr], d, pml, s=1.0)
    for a in range(3):
        check_bound("velocity", f"velocity het={het} u{a}", out[f"u{a}"], ref[a], M[a], 4)
    if g.aligned:
        check_variants(dev, "compute_velocity", items, out, None if het else ["u0", "g1", "pml0"])


def density_ref(g, r, du, pml, rho0, nonlinear, s=-1.0):
    """SolverCudaKernels.cu:1358-1393 nonlinear: sumRhosDt = (2 (rx + ry + rz) + rho0) dt, k = 8
    (+, +, *2, +rho0, *dt, *du, -, *pml); :1470-1497 linear: dtRho0 = dt rho0 (scalar: c.dt_rho0), k = 4"""
    r0 = g.c("rho0") if rho0 is None else f8(rho0)
    if nonlinear:
        coef = (2.0 * (f8(r[0]) + f8(r[1]) + f8(r[2])) + r0) * g.c("dt")
    else:
        coef = g.c("dt_rho0") if rho0 is None else g.c("dt") * r0
    return [g.bcast(pml[a], a) * (g.bcast(pml[a], a) * f8(r[a]) + s * coef * f8(du[a])) for a in range(3)]


@pytest.mark.parametrize("rho0_array", [True, False], ids=["rho0 array", "rho0 scalar"])
@pytest.mark.parametrize("nonlinear", [True, False], ids=["nonlinear", "linear"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_compute_density(dev, dims, nonlinear, rho0_array):
    g = G(dev, dims)
    r, du, pml = [g.noise() for _ in range(3)], [g.noise() for _ in range(3)], g.pml()
    rho0 = g.media() if rho0_array else None
    entry = "compute_density_nonlinear" if nonlinear else "compute_density_linear"
    items = [Arg(f"r{a}", r[a]) for a in range(3)] + [Arg(f"pml{a}", pml[a], ro=True) for a in range(3)] + \
            [Arg(f"du{a}", du[a], ro=True) for a in range(3)] + [Arg("rho0", rho0, ro=True)]
    out = call(dev, entry, items)
    ref = density_ref(g, r, du, pml, rho0, nonlinear)
    M = density_ref(g, [A(x) for x in r], [A(x) for x in du], pml, rho0, nonlinear, s=1.0)
    for a in range(3):
        check_bound(entry, f"{entry} rho0 array={rho0_array} r{a}", out[f"r{a}"], ref[a], M[a], 8 if nonlinear else 4)
    if g.aligned:
        check_variants(dev, entry, items, out, None if (nonlinear and rho0_array) else ["r2", "du0", "rho0" if rho0_array else "pml0"])


# ---- flat real kernels -------------------------------------------------------------------------------------------------
def opt_array(g, flag, lo, hi):
    return g.media(lo, hi) if flag else None


@pytest.mark.parametrize("rho0_array", [True, False], ids=["rho0 array", "rho0 scalar"])
@pytest.mark.parametrize("bona_array", [True, False], ids=["bona array", "bona scalar"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_pressure_terms_nonlinear(dev, dims, bona_array, rho0_array):
    """SolverCudaKernels.cu:1577-1602: densitySum = rx + ry + rz (k = 2); nonlinearTerm = (B/A s s) / (2 rho0) + s (k = 6);
    velGradSum = rho0 (dx + dy + dz) (k = 3).  The outputs are write-only: they start as noise."""
    g = G(dev, dims)
    r, du = [g.noise() for _ in range(3)], [g.noise() for _ in range(3)]
    bona, rho0 = opt_array(g, bona_array, 0.2, 1.0), opt_array(g, rho0_array, 0.8, 1.8)
    items = [Arg("dsum", g.noise()), Arg("nl", g.noise()), Arg("vgs", g.noise())] + \
            [Arg(f"r{a}", r[a], ro=True) for a in range(3)] + [Arg(f"du{a}", du[a], ro=True) for a in range(3)] + \
            [Arg("bona", bona, ro=True), Arg("rho0", rho0, ro=True)]
    out = call(dev, "compute_pressure_terms_nonlinear", items)
    b = g.c("b_on_a") if bona is None else f8(bona)
    r0 = g.c("rho0") if rho0 is None else f8(rho0)
    s = f8(r[0]) + f8(r[1]) + f8(r[2])
    sa = A(f8(r[0])) + A(f8(r[1])) + A(f8(r[2]))
    dsum = f8(du[0]) + f8(du[1]) + f8(du[2])
    dsa = A(f8(du[0])) + A(f8(du[1])) + A(f8(du[2]))
    lab = f"pressure terms nonlinear bona={bona_array} rho0={rho0_array}"
    check_bound("pressure_terms_nonlinear", lab + " densitySum", out["dsum"], s, sa, 2)
    check_bound("pressure_terms_nonlinear", lab + " nonlinearTerm", out["nl"], (b * s * s) / (2.0 * r0) + s,
                (b * sa * sa) / (2.0 * r0) + sa, 6)
    check_bound("pressure_terms_nonlinear", lab + " velGradSum", out["vgs"], r0 * dsum, r0 * dsa, 3)
    if g.aligned:
        check_variants(dev, "compute_pressure_terms_nonlinear", items, out,
                       None if (bona_array and rho0_array) else ["nl", "r1", "du2"])


@pytest.mark.parametrize("rho0_array", [True, False], ids=["rho0 array", "rho0 scalar"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_pressure_terms_linear(dev, dims, rho0_array):
    """SolverCudaKernels.cu:1724-1742, exact: densitySum = (rx + ry) + rz; velGradSum = rho0 ((dx + dy) + dz)"""
    g = G(dev, dims)
    r, du = [g.noise() for _ in range(3)], [g.noise() for _ in range(3)]
    rho0 = opt_array(g, rho0_array, 0.8, 1.8)
    items = [Arg("dsum", g.noise()), Arg("vgs", g.noise())] + [Arg(f"r{a}", r[a], ro=True) for a in range(3)] + \
            [Arg(f"du{a}", du[a], ro=True) for a in range(3)] + [Arg("rho0", rho0, ro=True)]
    out = call(dev, "compute_pressure_terms_linear", items)
    r0 = np.float32(g.k.rho0) if rho0 is None else rho0
    check_exact("pressure terms linear densitySum", out["dsum"], (r[0] + r[1]) + r[2])
    check_exact("pressure terms linear velGradSum", out["vgs"], r0 * ((du[0] + du[1]) + du[2]))
    if g.aligned:
        check_variants(dev, "compute_pressure_terms_linear", items, out, None if rho0_array else ["vgs", "r2"])


@pytest.mark.parametrize("tau_array", [True, False], ids=["tau/eta arrays", "tau/eta scalars"])
@pytest.mark.parametrize("c2_array", [True, False], ids=["c2 array", "c2 scalar"])
@pytest.mark.parametrize("entry", ["sum_pressure_terms_nonlinear", "sum_pressure_terms_linear"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_sum_pressure_terms(dev, dims, entry, c2_array, tau_array):
    """SolverCudaKernels.cu:1865-1879 / :1966-1980: p = c2 (first + fd ((tauTerm tau) - (etaTerm eta))), k = 5"""
    g = G(dev, dims)
    first, tt, et = g.noise(), g.noise(), g.noise()
    c2 = opt_array(g, c2_array, 1.0, 3.0)
    tau, eta = opt_array(g, tau_array, 0.5, 1.0), opt_array(g, tau_array, 0.2, 0.6)
    terms = [Arg("first", first, ro=True), Arg("tau_term", tt, ro=True), Arg("eta_term", et, ro=True)]
    if entry == "sum_pressure_terms_linear":   # (p, tauTerm, etaTerm, densitySum, ...)
        terms = terms[1:] + terms[:1]
    items = [Arg("p", g.noise())] + terms + [Arg("c2", c2, ro=True), Arg("tau", tau, ro=True), Arg("eta", eta, ro=True)]
    out = call(dev, entry, items)
    cc = g.c("c2") if c2 is None else f8(c2)
    ta = g.c("absorb_tau") if tau is None else f8(tau)
    ea = g.c("absorb_eta") if eta is None else f8(eta)
    fd = g.c("fft_divider")
    ref = cc * (f8(first) + fd * (f8(tt) * ta - f8(et) * ea))
    M = cc * (A(f8(first)) + fd * (A(f8(tt)) * ta + A(f8(et)) * ea))
    check_bound("sum_pressure_terms", f"{entry} c2={c2_array} tau={tau_array}", out["p"], ref, M, 5)
    if g.aligned:
        check_variants(dev, entry, items, out, None if (c2_array and tau_array) else ["p", "eta_term"])


@pytest.mark.parametrize("media", range(8), ids=lambda m: f"c2={m & 1} bona={(m >> 1) & 1} rho0={m >> 2}")
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_sum_pressure_nonlinear_lossless(dev, dims, media):
    """SolverCudaKernels.cu:2067-2084: p = c2 (s + (B/A (s s)) / (2 rho0)), s = rx + ry + rz, k = 7"""
    g = G(dev, dims)
    r = [g.noise() for _ in range(3)]
    c2, bona, rho0 = opt_array(g, media & 1, 1.0, 3.0), opt_array(g, media & 2, 0.2, 1.0), opt_array(g, media & 4, 0.8, 1.8)
    items = [Arg("p", g.noise())] + [Arg(f"r{a}", r[a], ro=True) for a in range(3)] + \
            [Arg("c2", c2, ro=True), Arg("bona", bona, ro=True), Arg("rho0", rho0, ro=True)]
    out = call(dev, "sum_pressure_nonlinear_lossless", items)
    cc = g.c("c2") if c2 is None else f8(c2)
    b = g.c("b_on_a") if bona is None else f8(bona)
    r0 = g.c("rho0") if rho0 is None else f8(rho0)
    s = f8(r[0]) + f8(r[1]) + f8(r[2])
    sa = A(f8(r[0])) + A(f8(r[1])) + A(f8(r[2]))
    check_bound("sum_pressure_nonlinear_lossless", f"nonlinear lossless media={media}", out["p"],
                cc * (s + (b * (s * s)) / (2.0 * r0)), cc * (sa + (b * (sa * sa)) / (2.0 * r0)), 7)
    if g.aligned:
        check_variants(dev, "sum_pressure_nonlinear_lossless", items, out, None if media == 7 else ["p", "r0"])


@pytest.mark.parametrize("c2_array", [True, False], ids=["c2 array", "c2 scalar"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_sum_pressure_linear_lossless(dev, dims, c2_array):
    """SolverCudaKernels.cu:2224-2236, exact: p = c2 ((rx + ry) + rz)"""
    g = G(dev, dims)
    r = [g.noise() for _ in range(3)]
    c2 = opt_array(g, c2_array, 1.0, 3.0)
    items = [Arg("p", g.noise())] + [Arg(f"r{a}", r[a], ro=True) for a in range(3)] + [Arg("c2", c2, ro=True)]
    out = call(dev, "sum_pressure_linear_lossless", items)
    cc = np.float32(g.k.c2) if c2 is None else c2
    check_exact("linear lossless p", out["p"], cc * ((r[0] + r[1]) + r[2]))
    if g.aligned:
        check_variants(dev, "sum_pressure_linear_lossless", items, out)


def pick(g, array, name):
    """the float32 operand of an exact restatement: the array, or the scalar of kw_constants that NULL selects"""
    return np.float32(getattr(g.k, name)) if array is None else array


STOKES_MEDIA = (15, 0, 5, 10)  # bits: c2, bona, rho0, tau arrays (all, none, and each argument once on either side)


@pytest.mark.parametrize("media", STOKES_MEDIA, ids=lambda m: f"c2={m & 1} bona={(m >> 1) & 1} rho0={(m >> 2) & 1} tau={m >> 3}")
@pytest.mark.parametrize("nonlinear", [True, False], ids=["nonlinear", "linear"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_sum_pressure_stokes(dev, dims, nonlinear, media):
    """kwave_hip.h (Stokes absorption), exact: every product and sum rounded on its own, in the header's order (the
    shared kw_stokes_pressure switches fma contraction off; the division is correctly rounded, 2 rho0 is exact):
      rhoSum = (rx + ry) + rz;  duSum = (dx + dy) + dz;  absorb = tau (rho0 duSum)
      first = rhoSum  |  (((B/A rhoSum) rhoSum) / (2 rho0)) + rhoSum;  p = c2 (first + absorb)
    The fused density epilogue (terms == 4) is compared with this kernel bit for bit elsewhere; both call one __device__
    function, so this restatement is what pins that function itself."""
    g = G(dev, dims)
    r, du = [g.noise() for _ in range(3)], [g.noise() for _ in range(3)]
    c2, bona = opt_array(g, media & 1, 1.0, 3.0), opt_array(g, nonlinear and media & 2, 0.2, 1.0)
    rho0, tau = opt_array(g, media & 4, 0.8, 1.8), opt_array(g, media & 8, 0.5, 1.0)
    entry = "sum_pressure_stokes_nonlinear" if nonlinear else "sum_pressure_stokes_linear"
    items = [Arg("p", g.noise())] + [Arg(f"r{a}", r[a], ro=True) for a in range(3)] + \
            [Arg(f"du{a}", du[a], ro=True) for a in range(3)] + [Arg("c2", c2, ro=True)] + \
            ([Arg("bona", bona, ro=True)] if nonlinear else []) + [Arg("rho0", rho0, ro=True), Arg("tau", tau, ro=True)]
    out = call(dev, entry, items)
    cc, b, r0, ta = pick(g, c2, "c2"), pick(g, bona, "b_on_a"), pick(g, rho0, "rho0"), pick(g, tau, "absorb_tau")
    rho_sum, du_sum = (r[0] + r[1]) + r[2], (du[0] + du[1]) + du[2]
    absorb = ta * (r0 * du_sum)
    first = (((b * rho_sum) * rho_sum) / (np.float32(2.0) * r0)) + rho_sum if nonlinear else rho_sum
    check_exact(f"{entry} media={media}", out["p"], cc * (first + absorb))
    if g.aligned:
        check_variants(dev, entry, items, out, None if media == 15 else ["p", "r1", "du2"])


@pytest.mark.parametrize("which", [0, 1], ids=["no_dispersion", "no_absorption"])
@pytest.mark.parametrize("coef_array", [True, False], ids=["coef array", "coef scalar"])
@pytest.mark.parametrize("c2_array", [True, False], ids=["c2 array", "c2 scalar"])
@pytest.mark.parametrize("entry", ["sum_pressure_terms_one_nonlinear", "sum_pressure_terms_one_linear"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_sum_pressure_terms_one(dev, dims, entry, c2_array, coef_array, which):
    """kwave_hip.h (one-term power law), exact: p = c2 (first + (fd (term coef))) for which == 0 (coef NULL -> absorb_tau),
    p = c2 (first - (fd (term coef))) for which == 1 (coef NULL -> absorb_eta); no fma contraction (kw_one_term_pressure)"""
    g = G(dev, dims)
    first, term = g.noise(), g.noise()
    c2 = opt_array(g, c2_array, 1.0, 3.0)
    coef = opt_array(g, coef_array, 0.2, 1.0)
    terms = [Arg("first", first, ro=True), Arg("term", term, ro=True)]
    if entry == "sum_pressure_terms_one_linear":   # (p, term, densitySum, ...)
        terms = terms[::-1]
    items = [Arg("p", g.noise())] + terms + [Arg("c2", c2, ro=True), Arg("coef", coef, ro=True), which]
    out = call(dev, entry, items)
    cc, co = pick(g, c2, "c2"), pick(g, coef, "absorb_eta" if which else "absorb_tau")
    scaled = np.float32(g.k.fft_divider) * (term * co)
    check_exact(f"{entry} c2={c2_array} coef={coef_array} which={which}", out["p"],
                cc * (first - scaled) if which else cc * (first + scaled))
    if g.aligned:
        check_variants(dev, entry, items, out, None if (c2_array and coef_array) else ["p", "term"])


@pytest.mark.parametrize("c2_array", [True, False], ids=["c2 array", "c2 scalar"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_add_initial_pressure_source(dev, dims, c2_array):
    """SolverCudaKernels.cu:864-884, exact: p = p0; rho_x = rho_y = p0 / (dim c2), dim = 3 (2 when nz == 1, rho_z = 0)"""
    g = G(dev, dims)
    p0 = g.noise()
    c2 = opt_array(g, c2_array, 1.0, 3.0)
    items = [Arg("p", g.noise()), Arg("r0", g.noise()), Arg("r1", g.noise()), Arg("r2", g.noise()), Arg("p0", p0, ro=True),
             Arg("c2", c2, ro=True)]
    out = call(dev, "add_initial_pressure_source", items)
    two_d = g.nz == 1
    cc = np.float32(g.k.c2) if c2 is None else c2
    rho = p0 / (np.float32(2.0 if two_d else 3.0) * cc)
    check_exact("initial pressure p", out["p"], p0)
    check_exact("initial pressure rho_x", out["r0"], rho)
    check_exact("initial pressure rho_y", out["r1"], rho)
    check_exact("initial pressure rho_z", out["r2"], np.zeros_like(p0) if two_d else rho)
    if g.aligned:
        check_variants(dev, "add_initial_pressure_source", items, out, None if c2_array else ["r2", "p0"])


@pytest.mark.parametrize("het", [True, False], ids=["het", "homog"])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_compute_initial_velocity(dev, dims, het):
    """SolverCudaKernels.cu:949-982, exact: u (d (fd 0.5)) with dt/(rho0 dx) arrays; u ((fd 0.5) dtRho0Sg) without"""
    g = G(dev, dims)
    u = [g.noise() for _ in range(3)]
    d = [g.media() for _ in range(3)] if het else None
    items = [Arg(f"u{a}", u[a]) for a in range(3)] + [Arg(f"d{a}", d[a] if het else None, ro=True) for a in range(3)]
    out = call(dev, "compute_initial_velocity", items)
    half = np.float32(g.k.fft_divider) * np.float32(0.5)
    for a in range(3):
        sg = np.float32(getattr(g.k, ("dt_rho0_sgx", "dt_rho0_sgy", "dt_rho0_sgz")[a]))
        check_exact(f"initial velocity het={het} u{a}", out[f"u{a}"], u[a] * (d[a] * half) if het else u[a] * (half * sg))
    if g.aligned:
        check_variants(dev, "compute_initial_velocity", items, out, None if het else ["u1"])


@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_scaled_sources(dev, dims):
    """SolverCudaKernels.cu:765-770 / :795-807, exact: u += s; rho_x, rho_y (and rho_z in 3-D) += s"""
    g = G(dev, dims)
    s, u, r = g.noise(), g.noise(), [g.noise() for _ in range(3)]
    items = [Arg("u", u), Arg("s", s, ro=True)]
    out = call(dev, "add_velocity_scaled_source", items)
    check_exact("velocity scaled source", out["u"], u + s)
    if g.aligned:
        check_variants(dev, "add_velocity_scaled_source", items, out)
    two_d = g.nz == 1
    items = [Arg("r0", r[0]), Arg("r1", r[1]), Arg("r2", r[2], ro=two_d), Arg("s", s, ro=True)]
    out = call(dev, "add_pressure_scaled_source", items)
    for a in range(2 if two_d else 3):
        check_exact(f"pressure scaled source r{a}", out[f"r{a}"], r[a] + s)
    if g.aligned:
        check_variants(dev, "add_pressure_scaled_source", items, out)


# ---- non-uniform shift -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", GRIDS + [(8, 300, 240)], ids=gid)
def test_velocity_gradient_shift_nonuniform(dev, dims):
    """SolverCudaKernels.cu:1285-1301, exact (one product per element): du_x *= dxudxn[x], du_y *= dyudyn[y], du_z *= dzudzn[z].
    8x300x240 has 72 000 rows: two launches of 218 and 22 z-planes"""
    g = G(dev, dims)
    du, n = [g.noise() for _ in range(3)], [g.media(0.5, 1.5, (m,)) for m in (g.nx, g.ny, g.nz)]
    items = [Arg(f"du{a}", du[a]) for a in range(3)] + [Arg(f"n{a}", n[a], ro=True) for a in range(3)]
    out = call(dev, "compute_velocity_gradient_shift_nonuniform", items)
    for a in range(3):
        check_exact(f"nonuniform shift du{a}", out[f"du{a}"], du[a] * n[a].reshape([-1 if i == 2 - a else 1 for i in range(3)]))


def test_velocity_gradient_shift_nonuniform_rejects_tall_planes(dev):
    """ny > 65535 would need launches with no rows: refused before any launch"""
    from kwave_amd import capi
    set_constants(dev, 1, 70000, 1)
    buf = dev.zeros(70000)
    with pytest.raises(capi.KWaveError, match=r"kw_status 1\].*ny <= 65535"):
        dev.call("compute_velocity_gradient_shift_nonuniform", buf, buf, buf, buf, buf, buf)
    buf.free()


# ---- k-space kernels ---------------------------------------------------------------------------------------------------
def dd_vectors(g):
    return [g.cnoise((m,)) for m in (g.nxc, g.ny, g.nz)]


def kspace_dd(dd):
    """ddx[x], ddy[y], ddz[z] broadcast over [nz][ny][nxc]"""
    return [f8(dd[a]).reshape([-1 if i == 2 - a else 1 for i in range(3)] + [2]) for a in range(3)]


@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_compute_pressure_gradient(dev, dims):
    """SolverCudaKernels.cu:1139-1157: eKappa = X kappa; X, Y, Z = eKappa * ddx[x], ddy[y], ddz[z], k = 3"""
    g = G(dev, dims)
    X, kappa, dd = g.cnoise(g.cshape), g.media(0.0, 1.0, g.cshape), dd_vectors(g)
    items = [Arg("X", X, cplx=True), Arg("Y", g.cnoise(g.cshape), cplx=True), Arg("Z", g.cnoise(g.cshape), cplx=True),
             Arg("kappa", kappa, ro=True)] + [Arg(f"dd{a}", dd[a], ro=True, cplx=True) for a in range(3)]
    out = call(dev, "compute_pressure_gradient", items)
    ek = f8(X) * f8(kappa)[..., None]
    ddb = kspace_dd(dd)
    for a, name in enumerate("XYZ"):
        check_bound("pressure_gradient", f"pressure gradient {name}", out[name], cmul_ref(ek, ddb[a]),
                    cmul_ref(A(ek), A(ddb[a]), 1.0), 3)
    if g.aligned:
        check_variants(dev, "compute_pressure_gradient", items, out, ["X", "Y", "Z", "kappa"])


@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_compute_velocity_gradient(dev, dims):
    """SolverCudaKernels.cu:1210-1239: eKappa = kappa fd; X = (X eKappa) * ddx[x] ..., k = 4"""
    g = G(dev, dims)
    V, kappa, dd = [g.cnoise(g.cshape) for _ in range(3)], g.media(0.0, 1.0, g.cshape), dd_vectors(g)
    items = [Arg(n, V[a], cplx=True) for a, n in enumerate("XYZ")] + [Arg("kappa", kappa, ro=True)] + \
            [Arg(f"dd{a}", dd[a], ro=True, cplx=True) for a in range(3)]
    ek = (f8(kappa) * g.c("fft_divider"))[..., None]
    ddb = kspace_dd(dd)

    def bound(out):
        for a, name in enumerate("XYZ"):
            sc = f8(V[a]) * ek
            check_bound("velocity_gradient", f"velocity gradient {name}", out[name], cmul_ref(sc, ddb[a]),
                        cmul_ref(A(sc), A(ddb[a]), 1.0), 4)
    out = call(dev, "compute_velocity_gradient", items)
    bound(out)
    if g.aligned:
        # P2 and P1 are not bit-identical: the backend fuses a different product of cmul's imaginary part into the
        # v_fma (P1: a.y b.x fused + round(a.x b.y); P2: a.x b.y fused + round(a.y b.x)), so the pair meets the bound only
        check_variants(dev, "compute_velocity_gradient", items, out, ["X", "Y", "Z", "kappa"], bound=bound)


@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_compute_absorbtion_term(dev, dims):
    """SolverCudaKernels.cu:1812-1820, exact: A *= nabla1, B *= nabla2 (both parts)"""
    g = G(dev, dims)
    Ah, Bh, n1, n2 = g.cnoise(g.cshape), g.cnoise(g.cshape), g.media(0.0, 2.0, g.cshape), g.media(0.0, 2.0, g.cshape)
    items = [Arg("A", Ah, cplx=True), Arg("B", Bh, cplx=True), Arg("n1", n1, ro=True), Arg("n2", n2, ro=True)]
    out = call(dev, "compute_absorbtion_term", items)
    check_exact("absorption A", out["A"], Ah * n1[..., None])
    check_exact("absorption B", out["B"], Bh * n2[..., None])
    if g.aligned:
        check_variants(dev, "compute_absorbtion_term", items, out)


@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_compute_absorbtion_term_one(dev, dims):
    """kwave_hip.h (one-term power law), exact: the same for one spectrum, A *= nabla (k_absorbtion_term_one scales both
    parts by the real operator: one product per component, no sum)"""
    g = G(dev, dims)
    Ah, n = g.cnoise(g.cshape), g.media(0.0, 2.0, g.cshape)
    items = [Arg("A", Ah, cplx=True), Arg("n", n, ro=True)]
    out = call(dev, "compute_absorbtion_term_one", items)
    check_exact("absorption term, one spectrum", out["A"], Ah * n[..., None])
    if g.aligned:
        check_variants(dev, "compute_absorbtion_term_one", items, out)


@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_compute_source_gradient(dev, dims):
    """SolverCudaKernels.cu:740-745, exact: S *= (sourceKappa fd)"""
    g = G(dev, dims)
    S, sk = g.cnoise(g.cshape), g.media(0.0, 1.0, g.cshape)
    items = [Arg("S", S, cplx=True), Arg("sk", sk, ro=True)]
    out = call(dev, "compute_source_gradient", items)
    check_exact("source gradient", out["S"], S * (sk * np.float32(g.k.fft_divider))[..., None])
    if g.aligned:
        check_variants(dev, "compute_source_gradient", items, out)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("dims", GRIDS, ids=gid)
def test_compute_velocity_shift(dev, dims, axis):
    """SolverCudaKernels.cu:2617-2689: T = (T * shift[k]) divider_axis on the kw_fft_r2c_1d(axis) layout, k = 3"""
    g = G(dev, dims)
    sh = [g.nx, g.ny, g.nz]
    sh[axis] = sh[axis] // 2 + 1
    T, shift = g.cnoise((sh[2], sh[1], sh[0])), g.cnoise((sh[axis],))
    items = [axis, Arg("T", T, cplx=True), Arg("shift", shift, ro=True, cplx=True)]
    out = call(dev, "compute_velocity_shift", items)
    sb = f8(shift).reshape([-1 if i == 2 - axis else 1 for i in range(3)] + [2])
    div = g.c(("fft_divider_x", "fft_divider_y", "fft_divider_z")[axis])
    check_bound("velocity_shift", f"velocity shift axis {axis}", out["T"], cmul_ref(f8(T), sb) * div,
                cmul_ref(A(f8(T)), A(sb), 1.0) * div, 3)


# ---- sources -------------------------------------------------------------------------------------------------------------
SOURCE_SIZES = (1, 255, 256, 257, 5003)
NT = 9


def source_index(g, n, duplicates):
    """n indices in random order that include the first and the last grid element (n = 1: the last)"""
    N = g.nx * g.ny * g.nz
    if n == 1:
        return np.array([N - 1], np.uint64)
    if duplicates:
        idx = g.rng.integers(1, N - 1, n - 2)
        idx[: n // 4] = idx[n // 4: 2 * (n // 4)]  # a quarter of them twice
    else:
        idx = g.rng.choice(np.arange(1, N - 1), n - 2, replace=False)
    idx = np.concatenate([[0, N - 1], idx])
    return g.rng.permutation(idx).astype(np.uint64)


def source_cases(g, mode, many):
    for n in SOURCE_SIZES:
        if n > g.nx * g.ny * g.nz:
            continue
        for t in (0, NT // 2, NT - 1):
            yield n, t, source_index(g, n, mode == 0 and many == 0)


def scatter_ref(field, idx, v, mode):
    out = field.copy()
    if mode == 0:
        out[idx] = v
    elif mode == 1:
        out[idx] = out[idx] + v  # indices unique
    return out


MODES = [(0, "dirichlet"), (1, "additive no correction"), (2, "additive (k-space)")]


@pytest.mark.parametrize("many", [0, 1])
@pytest.mark.parametrize("mode", MODES, ids=lambda m: m[1])
@pytest.mark.parametrize("dims", [(32, 24, 16), (36, 20, 1)], ids=gid)
def test_add_velocity_source(dev, dims, mode, many):
    """SolverCudaKernels.cu:504-528: u[index[i]] = / += input[many ? t n + i : t]; the k-space corrected mode leaves u"""
    mode = mode[0]
    g = G(dev, dims)
    for n, t, idx in source_cases(g, mode, many):
        set_constants(dev, *dims, velocity_source_size=n, velocity_source_mode=mode, velocity_source_many=many)
        u = g.noise().reshape(-1)
        inp = g.noise((NT * n,) if many else (NT,))
        out = call(dev, "add_velocity_source", [Arg("u", u), Arg("in", inp, ro=True), Arg("idx", idx, ro=True, dtype=np.uint64), t])
        v = inp[t * n: (t + 1) * n] if many else inp[t]
        check_exact(f"velocity source n={n} t={t}", out["u"], scatter_ref(u, idx.astype(np.int64), v, mode))


@pytest.mark.parametrize("many", [0, 1])
@pytest.mark.parametrize("mode", MODES, ids=lambda m: m[1])
@pytest.mark.parametrize("dims", [(32, 24, 16), (36, 20, 1), (35, 13, 1)], ids=gid)
def test_add_pressure_source(dev, dims, mode, many):
    """SolverCudaKernels.cu:570-629: rho_x, rho_y (rho_z in 3-D only) = / += input[many ? t n + i : t]"""
    mode = mode[0]
    g = G(dev, dims)
    two_d = g.nz == 1
    for n, t, idx in source_cases(g, mode, many):
        set_constants(dev, *dims, pressure_source_size=n, pressure_source_mode=mode, pressure_source_many=many)
        r = [g.noise().reshape(-1) for _ in range(3)]
        inp = g.noise((NT * n,) if many else (NT,))
        items = [Arg("r0", r[0]), Arg("r1", r[1]), Arg("r2", r[2], ro=two_d), Arg("in", inp, ro=True),
                 Arg("idx", idx, ro=True, dtype=np.uint64), t]
        out = call(dev, "add_pressure_source", items)
        v = inp[t * n: (t + 1) * n] if many else inp[t]
        for a in range(2 if two_d else 3):
            check_exact(f"pressure source n={n} t={t} r{a}", out[f"r{a}"], scatter_ref(r[a], idx.astype(np.int64), v, mode))


@pytest.mark.parametrize("many", [0, 1])
def test_insert_source_into_scaling_matrix(dev, many):
    """SolverCudaKernels.cu:679-697: scaled[index[i]] = input[many ? t n + i : t]; the rest of the matrix is kept"""
    g = G(dev, (32, 24, 16))
    for n, t, idx in source_cases(g, 0, many):
        sc = g.noise().reshape(-1)
        inp = g.noise((NT * n,) if many else (NT,))
        out = call(dev, "insert_source_into_scaling_matrix",
                    [Arg("s", sc), Arg("in", inp, ro=True), Arg("idx", idx, ro=True, dtype=np.uint64), n, many, t])
        v = inp[t * n: (t + 1) * n] if many else inp[t]
        check_exact(f"insert source n={n} t={t}", out["s"], scatter_ref(sc, idx.astype(np.int64), v, 0))


def test_add_transducer_source(dev):
    """SolverCudaKernels.cu:463-471: ux[index[i]] += input[delay[i] + t]; the largest delay reaches the series' end"""
    g = G(dev, (32, 24, 16))
    L = 40
    for n, t, idx in source_cases(g, 1, 1):
        set_constants(dev, 32, 24, 16, velocity_source_size=n)
        delay = g.rng.integers(0, L - NT + 1, n).astype(np.uint64)
        delay[g.rng.integers(0, n)] = L - NT  # delay + (NT - 1) == L - 1
        ux, inp = g.noise().reshape(-1), g.noise((L,))
        out = call(dev, "add_transducer_source", [Arg("ux", ux), Arg("idx", idx, ro=True, dtype=np.uint64),
                                                  Arg("in", inp, ro=True), Arg("delay", delay, ro=True, dtype=np.uint64), t])
        want = ux.copy()
        want[idx.astype(np.int64)] = ux[idx.astype(np.int64)] + inp[(delay + np.uint64(t)).astype(np.int64)]
        check_exact(f"transducer source n={n} t={t}", out["ux"], want)


# ---- 1-D FFT wrapper ---------------------------------------------------------------------------------------------------
FFT_GRIDS = [((13, 11, 7), 0), ((13, 11, 7), 1), ((13, 11, 7), 2), ((980, 5, 3), 0), ((5, 980, 3), 1), ((5, 3, 980), 2)]


@pytest.mark.parametrize("dims,axis", FFT_GRIDS, ids=[f"{gid(d)}-axis{a}" for d, a in FFT_GRIDS])
def test_fft_1d(dev, dims, axis):
    """kw_fft_r2c_1d / kw_fft_c2r_1d along `axis` against numpy.fft in fp64: [z][y][x] with the transformed axis shortened
    to n/2 + 1; c2r unnormalised.  Per element |gpu - fp64| <= (k + 1) 2^-24 M, M = sum of |terms| of the DFT sum,
    k = 6 ceil(log2 n): a few roundings per butterfly stage"""
    g = G(dev, dims)
    n = dims[axis]
    ax = 2 - axis
    t0 = time.perf_counter()
    dev.call("fft_create_plans_1d", axis)
    plan_s = time.perf_counter() - t0
    print(f"\nrocFFT 1-D plans for {gid(dims)} axis {axis}: {plan_s:.2f} s")
    k = 6 * int(np.ceil(np.log2(n)))
    x = g.noise()
    sh = list(g.shape)
    sh[ax] = n // 2 + 1
    out = call(dev, "fft_r2c_1d", [axis, Arg("x", x, ro=True), Arg("X", np.zeros(sh + [2], np.float32), cplx=True)])
    ref = np.fft.rfft(f8(x), axis=ax)
    M = np.sum(A(f8(x)), axis=ax, keepdims=True) * np.ones(sh)
    check_bound("fft_1d", f"r2c axis {axis}", out["X"], split(ref), M[..., None], k)
    # c2r of a Hermitian half spectrum (imaginary parts of the self-conjugate bins zero)
    Xh = g.cnoise(sh)
    idx = [slice(None)] * 3
    selfconj = [0] + ([n // 2] if n % 2 == 0 else [])
    for b in selfconj:
        idx[ax] = b
        Xh[tuple(idx) + (1,)] = 0.0
    out = call(dev, "fft_c2r_1d", [axis, Arg("X", Xh, cplx=True), Arg("x", g.noise())])
    ref = np.fft.irfft(cplx(Xh), n=n, axis=ax) * n
    w = np.full(n // 2 + 1, 2.0)
    w[selfconj] = 1.0
    wb = w.reshape([-1 if i == ax else 1 for i in range(3)])
    M = np.sum(wb * (A(f8(Xh[..., 0])) + A(f8(Xh[..., 1]))), axis=ax, keepdims=True) * np.ones(g.shape)
    check_bound("fft_1d", f"c2r axis {axis}", out["x"], ref, M, k)
    dev.call("fft_destroy_plans")


# ---- ISA facts the exact checks rely on ----------------------------------------------------------------------------------
def device_asm(src):
    """gfx950 assembly of one csrc file, compiled as build.py compiles it"""
    import subprocess
    import tempfile
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    csrc = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([os.path.join(rocm, "bin", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize",
                        "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        os.path.join(csrc, src), "-o", out], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return open(out).read()


def kernel_bodies(asm, name):
    """{symbol: instructions} of every instantiation of kernel `name`"""
    import re
    bodies = {}
    for m in re.finditer(r"^(_Z\w*" + name + r"\w*):", asm, re.M):
        body = asm[m.end():]
        bodies[m.group(1)] = body[:body.find("s_endpgm")]
    assert bodies, name
    return bodies


def test_division_is_correctly_rounded_and_denormals_kept():
    """The exact checks of divisions (initial pressure source, kw_divide) need IEEE division, and the 40-bit codec test
    needs float32 denormals: clang's HIP defaults (-fhip-fp32-correctly-rounded-divide-sqrt, no denormal flush), which
    build.py does not override.  Pinned in the ISA: a / b is the v_div_scale / v_div_fmas / v_div_fixup sequence, not a
    bare v_rcp_f32, and every kernel of both files runs with float32 denormals on (float_denorm_mode_32 = 3)."""
    src = open(os.path.join(ROOT, "k-wave-fluid-cuda_amd", "build.py")).read()
    for flag in ("fast-math", "no-hip-fp32-correctly-rounded", "unsafe-math", "approx-func", "denormal", "ftz"):
        assert flag not in src, flag
    for f, kernels in (("kw_solver_kernels.hip", ("k_add_initial_pressure_source",)), ("kw_sampling_kernels.hip", ("k_divide",))):
        asm = device_asm(f)
        for kern in kernels:
            for sym, body in kernel_bodies(asm, kern).items():
                for ins in ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32"):
                    assert ins in body, (sym, ins)
        modes = [line.split()[-1] for line in asm.splitlines() if ".amdhsa_float_denorm_mode_32" in line]
        assert modes and set(modes) == {"3"}, (f, sorted(set(modes)))
