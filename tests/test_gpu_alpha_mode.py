"""One-term power-law absorption on the GPU: absorbing_flag = 3 (no_dispersion, eta = 0) and 4 (no_absorption, tau = 0).

Yardstick: the unchanged fp64 oracle (oracle/kwave_np.py NumpySim) built on the flag-1 problem with sim.eta (or sim.tau)
multiplied by zero before stepping: stage_absorption_pressure then computes exactly the mode (tests/test_alpha_mode_host.py
holds that premise on the CPU).  Tolerance: relative L2 <= 1e-5 on p, u and rho, the project's TOL.

FAR = 1e-3: at 32^3, 40 steps, alpha_power = 1.5 the four runs (mode, other mode, full power law, lossless) lie 4e-3 ... 1.6e-2
from one another, so every parity test also asserts that the GPU result is >= FAR from the three others: a swapped
operator, a dropped term or a silent run of flag 1 cannot pass.

Bits: the x-inverse epilogue of kw_fused_absorption_pressure_one, chained or not, whole-plane or three-launch form, and
kw_sum_pressure_terms_one_* all evaluate kw_one_term_pressure without fma contraction: asserted bit-identical.
"""
import concurrent.futures
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_l2

sys.path.insert(0, ROOT)
from oracle import kwave_np as knp  # noqa: E402
from gpu_buffers import BONA, C2, DT, ETA, RHO0, TAU, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-5
FAR = 1e-3
FIELDS = ("p", "ux", "uy", "uz", "rhox", "rhoy", "rhoz")
MODES = ("no_dispersion", "no_absorption")
ZEROED = {"no_dispersion": ("eta",), "no_absorption": ("tau",), "full": (), "lossless": ("tau", "eta")}
_REFS = {}  # the four fp64 runs of a problem, computed once and shared by both modes' tests


def gpu(pr, **kw):
    import kwave_amd  # noqa: F401
    from kwave_amd.solver import HostSolver
    return HostSolver(pr, **kw)


def references(syn, key, pr, steps):
    """{run: fields} for the mode runs, the full power law and the lossless run of the flag-1 twin of pr (the four
    NumpySim runs side by side: numpy's FFT releases the interpreter lock)"""
    if key not in _REFS:
        def one(zeroed):
            sim = knp.NumpySim(syn.alpha_mode_as_power_law(pr))
            for name in zeroed:
                setattr(sim, name, getattr(sim, name) * 0)
            for _ in range(steps):
                sim.step()
            return {"p": sim.p, "ux": sim.u[0], "uy": sim.u[1], "uz": sim.u[2], "rhox": sim.rho[0], "rhoy": sim.rho[1],
                    "rhoz": sim.rho[2]}
        with concurrent.futures.ThreadPoolExecutor(4) as pool:
            _REFS[key] = dict(zip(ZEROED, pool.map(one, ZEROED.values())))
    return _REFS[key]


def check(pr, refs, mode, steps, label, **kw):
    g = gpu(pr, **kw)
    g.run(steps)
    got = {f: g.field(f) for f in FIELDS}
    g.close()
    want, errs = refs[mode], {}
    for f in FIELDS:
        if np.abs(want[f]).max() == 0.0:  # (2-D: u_z, rho_z)
            assert not got[f].any(), f
        else:
            errs[f] = rel_l2(got[f], want[f])
    far = {run: rel_l2(got["p"], refs[run]["p"]) for run in ZEROED if run != mode}
    print(f"{label} {mode}: {errs} far {far}")
    assert max(errs.values()) <= TOL, (label, errs)
    assert min(far.values()) >= FAR, (label, far)


# ---- 1: media -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("heterogeneous", [False, True])
@pytest.mark.parametrize("nonlinear", [False, True])
def test_media_p0_32(syn, heterogeneous, nonlinear, mode):
    pr = syn.make_problem(32, heterogeneous=heterogeneous, nonlinear=nonlinear, absorbing=True, alpha_mode=mode, source="p0")
    refs = references(syn, ("media", heterogeneous, nonlinear), pr, 40)
    for fused in (True, False):
        check(pr, refs, mode, 40, f"het={heterogeneous} nonlinear={nonlinear} fused={fused}", fused_kernels=fused)


# ---- 2: sources -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("source,smode", [("p_source", 0), ("p_source", 1), ("p_source", 2), ("u_source", 1)])
def test_time_varying_sources(syn, source, smode, mode):
    """nt_src = 25 of 40 steps: with a pressure source the fused run takes the element-wise terms kernel and the unchained
    one-term stage while the source is on, and the chained path afterwards"""
    pr = syn.make_problem(32, heterogeneous=True, nonlinear=True, absorbing=True, alpha_mode=mode, source=source,
                          source_mode=smode, source_many=1, nt=40, nt_src=25, pml_size=4)
    refs = references(syn, ("src", source, smode), pr, 40)
    for fused in (True, False):
        check(pr, refs, mode, 40, f"{source} mode {smode} fused={fused}", fused_kernels=fused)


# ---- 3: every kernel form -------------------------------------------------------------------------------------------------
# (one mode per grid, alternating, to keep this file near 25 s: the kernels of both modes are one instantiation, told
# apart by a runtime selector, and every other test of this file runs both modes)
@pytest.mark.parametrize("dims,mode", [
    ((512, 16, 16), MODES[0]), ((16, 512, 16), MODES[1]), ((16, 16, 512), MODES[0]),  # long x lines; 2 x 256 y and z lines
    ((448, 16, 16), MODES[1]),                    # radix-7, long-line code object
    ((400, 16, 16), MODES[0]),                    # mixed radix (25 x 16), short-line code object
    ((100, 16, 108), MODES[1]),                   # masked tails: 1728 rows do not fill whole x tiles
    ((64, 64, 64), MODES[0]), ((32, 32, 48), MODES[1]),  # whole-plane kernels
])
def test_kernel_forms(syn, dims, mode):
    nx, ny, nz = dims
    pr = syn.make_problem(nx, ny, nz, heterogeneous=True, nonlinear=True, absorbing=True, alpha_mode=mode, source="p0", pml_size=4)
    check(pr, references(syn, ("forms", dims), pr, 24), mode, 24, str(dims), fused_kernels=True)


# ---- 4: 2-D and non-uniform grids -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_2d_grid(syn, mode):
    pr = syn.as_2d_file(syn.make_problem(64, 48, 1, heterogeneous=True, nonlinear=True, absorbing=True, alpha_mode=mode,
                                         source="p0", nt=40, pml_size=6, sensor="random"))
    refs = references(syn, "2d", pr, 40)
    for fused in (True, False):
        check(pr, refs, mode, 40, f"2-D fused={fused}", fused_kernels=fused)


@pytest.mark.parametrize("mode", MODES)
def test_nonuniform_grid(syn, mode):
    """non-uniform grid on the fused passes: gradients as arrays, scaled, the element-wise terms, the unchained stage"""
    pr = syn.make_problem(32, heterogeneous=True, nonlinear=True, absorbing=True, alpha_mode=mode, source="p0", pml_size=4,
                          nonuniform=True)
    refs = references(syn, "nonuniform", pr, 40)
    for fused in (True, False):
        check(pr, refs, mode, 40, f"non-uniform fused={fused}", fused_kernels=fused)


# ---- 5: stage level -------------------------------------------------------------------------------------------------------
STAGE_GRIDS = [((32, 32, 16), 1), ((32, 32, 16), 0), ((64, 64, 16), 1), ((256, 16, 16), 1), ((100, 16, 108), 1)]


def density_and_pressure_stages(g, which, nonlinear, arrays):
    """kw_fused_density(terms = 5 | 6) followed by kw_fused_absorption_pressure_one, plain and chained, on white noise
    that the Grid g (test_gpu_stages.Grid) draws next (a fresh Grid of the same dims draws the same for every
    `plane_kernels`); returns its host inputs and, per flags, what the two calls wrote.  The plain call also stores
    the three gradients."""
    from test_gpu_stages import CHAIN_TERMS, TERMS_IN_SCRATCH
    d = g.dev
    u_h = g.comps([g.noise() for _ in range(3)])
    rho_h = g.comps([g.noise() for _ in range(3)])
    pml = g.pml_vectors()
    med = {k: (g.media(lo, hi) if arrays else None) for k, (lo, hi) in
           dict(rho0=(0.8, 1.8), bona=(0.2, 1.0), c2=(1.0, 3.0), coef=(0.5, 1.0)).items()}
    dev = {k: (g.ro(v) if v is not None else None) for k, v in med.items()}
    ptr = lambda x: x.ptr if x is not None else None  # noqa: E731
    dd = [g.dd[k] for k in ("ddx_k_shift_neg_r", "ddy_k_shift_neg", "ddz_k_shift_neg")]
    pml_d = [g.ro(x) for x in pml]
    u_d = [g.ro(x) for x in u_h]
    t_init = [g.noise() for _ in range(3)]
    i_first = 1 if nonlinear else 0
    i_term = 0 if which else (2 if nonlinear else 1)
    nabla = g.padded["nabla2" if which else "nabla1"]
    out = {}
    for flags in (0, CHAIN_TERMS):
        rho = [g.field(x) for x in rho_h]
        t = [g.field(x) for x in t_init]
        du = [g.field(g.noise()) for _ in range(3)] if flags == 0 else [None] * 3
        d.call("fused_density", nonlinear, *[x.ptr for x in u_d], *[x.ptr for x in rho], *[x.ptr for x in pml_d], ptr(dev["rho0"]),
               g.padded["kappa"].ptr, *[x.ptr for x in dd], *[ptr(x) for x in du], 5 + which, ptr(dev["bona"]),
               *[x.ptr for x in t], flags)
        p = g.field(g.noise())
        d.call("fused_absorption_pressure_one", p.ptr, None if flags else t[i_term].ptr, t[i_first].ptr, nabla.ptr, ptr(dev["c2"]),
               ptr(dev["coef"]), which, TERMS_IN_SCRATCH if flags else 0)
        out[flags] = dict(rho=[x.read() for x in rho], t=[x.read() for x in t], p=p.read(),
                          du=[x.read() for x in du if x is not None])
    return dict(u=u_h, rho=rho_h, pml=pml, med=med, t_init=t_init, i_first=i_first, i_term=i_term), out


def density_stage_terms(g, which, nonlinear, arrays, rec=None):
    """the body of test_density_stage_terms on the Grid g: asserts every bit identity and returns {quantity: rel-L2
    against fp64}; rec(label, got, fp64), when given, is handed each stored quantity, and p also against the fp64 stage
    function applied to the float32 `first` and term that the plain call stored (one stage's rounding, not two)"""
    from test_gpu_stages import CHAIN_TERMS
    inp, out = density_and_pressure_stages(g, which, nonlinear, arrays)
    u_h, rho_h, pml, med, t_init, i_first, i_term = (inp[k] for k in ("u", "rho", "pml", "med", "t_init", "i_first", "i_term"))
    bits = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    for a in range(3):
        assert bits(out[0]["rho"][a], out[CHAIN_TERMS]["rho"][a]), f"rho{a}: chained differs from plain"
    assert bits(out[0]["t"][i_first], out[CHAIN_TERMS]["t"][i_first]), "first: chained differs from plain"
    assert bits(out[0]["p"], out[CHAIN_TERMS]["p"]), "p from the chained spectrum differs from p from the stored term"
    for i in range(3):  # what each form must leave alone
        if i not in (i_first, i_term):
            assert bits(out[0]["t"][i], t_init[i]), f"t{i} written by the plain call"
        if i != i_first:
            assert bits(out[CHAIN_TERMS]["t"][i], t_init[i]), f"t{i} written under CHAIN_TERMS"
    f8 = lambda x, s: x.astype(np.float64) if x is not None else s  # noqa: E731
    ref = knp.stage_density([x.astype(np.float64) for x in u_h], [x.astype(np.float64) for x in rho_h],
                            [g.bcast(x.astype(np.float64), a) for a, x in enumerate(pml)], f8(med["rho0"], RHO0), DT,
                            g.k64["kappa"], g.dd_neg, bool(nonlinear), 2 if nonlinear else 1, f8(med["bona"], BONA))
    S, first, vgt = (ref["t"][0], ref["t"][1], ref["t"][2]) if nonlinear else (ref["t"][0], ref["t"][0], ref["t"][1])
    errs = {f"rho{a}": rel_l2(out[0]["rho"][a], ref["rho"][a]) for a in range(3) if np.abs(ref["rho"][a]).max() > 0}
    errs["first"] = rel_l2(out[0]["t"][i_first], first)
    errs["term"] = rel_l2(out[0]["t"][i_term], S if which else vgt)
    zero = 0.0 * g.k64["nabla1"]
    coef = f8(med["coef"], ETA if which else TAU)
    want = knp.stage_absorption_pressure(first, vgt, S, zero if which else g.k64["nabla1"], g.k64["nabla2"] if which else zero,
                                         f8(med["c2"], C2), 0.0 if which else coef, coef if which else 0.0)
    errs["p"] = rel_l2(out[0]["p"], want)
    if rec is not None:
        for a in range(3):
            rec(f"one-term rho{a}", out[0]["rho"][a], ref["rho"][a])
            rec(f"one-term du{a}", out[0]["du"][a], ref["du"][a])
        rec("one-term first", out[0]["t"][i_first], first)
        rec("one-term term", out[0]["t"][i_term], S if which else vgt)
        stored = [out[0]["t"][i].astype(np.float64) for i in (i_first, i_term)]
        rec("one-term p from the stored term", out[0]["p"], knp.stage_absorption_pressure(
            stored[0], stored[1], stored[1], zero if which else g.k64["nabla1"], g.k64["nabla2"] if which else zero,
            f8(med["c2"], C2), 0.0 if which else coef, coef if which else 0.0))
    return errs


@pytest.mark.parametrize("dims,plane", STAGE_GRIDS)
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("nonlinear", [1, 0])
@pytest.mark.parametrize("arrays", [True, False])
def test_density_stage_terms(syn, dims, plane, which, nonlinear, arrays):
    """kw_fused_density(terms = 5 | 6) on white noise between guard bands: densities, `first` and the one term against
    the fp64 stage function; the chained call stores `first` alone (same bits) and leaves the other t arrays untouched;
    its spectrum, consumed by kw_fused_absorption_pressure_one(TERMS_IN_SCRATCH), gives the bits of the unchained stage."""
    from test_gpu_stages import Grid
    g = Grid(syn, dims, plane_kernels=plane)
    try:
        errs = density_stage_terms(g, which, nonlinear, arrays)
        print(f"{dims} plane={plane} which={which} nonlinear={nonlinear} arrays={arrays}: {errs}")
        assert max(errs.values()) <= TOL, errs
        g.check_readonly()
    finally:
        g.close()


def pressure_stage(g, which, arrays, rec=None):
    """the body of test_pressure_stage_bits_and_fp64 on the Grid g: asserts every bit identity and returns (rel-L2(p),
    rel-L2(p of the two-term entry point), whether those two agree in every bit); rec(label, got, fp64), when given, is
    handed p"""
    from test_gpu_stages import CHAIN_P, P_IN_SCRATCH
    d = g.dev
    dims = (g.nx, g.ny, g.nz)
    first_h, term_h = g.noise(), g.noise()
    c2 = g.media(1.0, 3.0) if arrays else None
    coef = g.media(0.5, 1.0) if arrays else None
    ptr = lambda x: x.ptr if x is not None else None  # noqa: E731
    first_d, term_d = g.ro(first_h), g.ro(term_h)
    c2_d, coef_d = (g.ro(c2), g.ro(coef)) if arrays else (None, None)
    nabla = g.padded["nabla2" if which else "nabla1"]
    bits = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    ps = {}
    for flags in (0, CHAIN_P):
        p = g.field(g.noise())
        d.call("fused_absorption_pressure_one", p.ptr, term_d.ptr, first_d.ptr, nabla.ptr, ptr(c2_d), ptr(coef_d), which, flags)
        ps[flags] = p
    p_plain = ps[0].read()
    assert bits(p_plain, ps[CHAIN_P].read()), "chained p differs from plain p"
    # the consumer of the chained spectrum (still in scratch: nothing ran since the chained call)
    dd_pos = [g.dd[k] for k in ("ddx_k_shift_pos_r", "ddy_k_shift_pos", "ddz_k_shift_pos")]
    pml_d = [g.ro(x) for x in g.pml_vectors()]
    u0 = g.comps([g.noise() for _ in range(3)])
    vel = {}
    for flags in (P_IN_SCRATCH, 0):
        uu = [g.field(x) for x in u0]
        d.call("fused_velocity", ps[CHAIN_P].ptr, *[x.ptr for x in uu], None, None, None, *[x.ptr for x in pml_d],
               g.padded["kappa"].ptr, *[x.ptr for x in dd_pos], flags)
        vel[flags] = [x.read() for x in uu]
    for a in range(3):
        assert bits(vel[0][a], vel[P_IN_SCRATCH][a]), f"u{a} from the chained spectrum"
    # the stage's inverse-transformed term itself: fft_divider = 1, first = 0, c2 = coef = 1 make p = 1 * (0 + 1 * (term * 1))
    ones, zeros = g.ro(np.ones(g.shape, np.float32)), g.ro(np.zeros(g.shape, np.float32))
    raw = g.field(g.noise())
    set_constants(d, *dims, fft_divider=1.0)
    d.call("fused_absorption_pressure_one", raw.ptr, term_d.ptr, zeros.ptr, nabla.ptr, ones.ptr, ones.ptr, 0, 0)
    d.sync()
    set_constants(d, *dims)
    q = g.field(g.noise())
    d.call("sum_pressure_terms_one_linear", q.ptr, raw.ptr, first_d.ptr, ptr(c2_d), ptr(coef_d), which)
    assert bits(q.read(), p_plain), "element-wise kernel differs from the epilogue"
    q2 = g.field(g.noise())
    d.call("sum_pressure_terms_one_nonlinear", q2.ptr, first_d.ptr, raw.ptr, ptr(c2_d), ptr(coef_d), which)
    assert bits(q2.read(), p_plain), "nonlinear element-wise entry differs from the epilogue"
    # fp64
    f8 = lambda x, s: x.astype(np.float64) if x is not None else s  # noqa: E731
    zero = 0.0 * g.k64["nabla1"]
    co = f8(coef, ETA if which else TAU)
    want = knp.stage_absorption_pressure(first_h.astype(np.float64), term_h.astype(np.float64), term_h.astype(np.float64),
                                         zero if which else g.k64["nabla1"], g.k64["nabla2"] if which else zero, f8(c2, C2),
                                         0.0 if which else co, co if which else 0.0)
    err = rel_l2(p_plain, want)
    # the two-term entry point with the other coefficient an array of zeros (arrays for both, as it requires)
    co_arr = g.ro(coef if arrays else np.full(g.shape, ETA if which else TAU, np.float32))
    p2 = g.field(g.noise())
    tau_eta = (zeros.ptr, co_arr.ptr) if which else (co_arr.ptr, zeros.ptr)
    d.call("fused_absorption_pressure", p2.ptr, term_d.ptr, term_d.ptr, first_d.ptr, g.padded["nabla1"].ptr,
           g.padded["nabla2"].ptr, ptr(c2_d), *tau_eta, 0)
    p2_h = p2.read()
    err2 = rel_l2(p2_h, want)
    if rec is not None:
        rec("one-term pressure stage p", p_plain, want)
    return err, err2, bits(p2_h, p_plain)


@pytest.mark.parametrize("dims,plane", STAGE_GRIDS)
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("arrays", [True, False])
def test_pressure_stage_bits_and_fp64(syn, dims, plane, which, arrays):
    """kw_fused_absorption_pressure_one on white noise: p against the fp64 stage function; the chained call gives the
    same p and a spectrum from which kw_fused_velocity(P_IN_SCRATCH) computes the bits it computes from p; the
    element-wise kernel fed the stage's own inverse-transformed term gives the same bits; the two-term entry point with
    a zero coefficient array holds the fp64 bound too (its bits are compared and printed, not gated)."""
    from test_gpu_stages import Grid
    g = Grid(syn, dims, plane_kernels=plane)
    try:
        err, err2, same = pressure_stage(g, which, arrays)
        print(f"{dims} plane={plane} which={which} arrays={arrays}: rel-L2(p) = {err:.3e}, two-term entry {err2:.3e}, "
              f"two-term bits equal: {same}")
        assert err <= TOL and err2 <= TOL
        g.check_readonly()
    finally:
        g.close()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("nonlinear,arrays", [(1, True), (0, False)])
def test_stage_whole_plane_form_gives_the_bits_of_the_three_launch_form(syn, which, nonlinear, arrays):
    """(32,32,16) with plane_kernels 1 and 0 on the same inputs: the density epilogue (terms 5 | 6) and the one-term
    pressure sum, plain and chained, write the same bits in their whole-plane and their three-launch forms"""
    outs = {}
    from test_gpu_stages import Grid
    for plane in (1, 0):
        g = Grid(syn, (32, 32, 16), plane_kernels=plane)
        try:
            _, outs[plane] = density_and_pressure_stages(g, which, nonlinear, arrays)
        finally:
            g.close()
    for flags, res in outs[1].items():
        other = outs[0][flags]
        assert np.abs(res["p"]).max() > 0
        assert np.array_equal(res["p"].view(np.uint32), other["p"].view(np.uint32)), ("p", flags)
        for name in ("rho", "t", "du"):
            for a in range(len(res[name])):
                assert np.array_equal(res[name][a].view(np.uint32), other[name][a].view(np.uint32)), (name, a, flags)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", [(32, 32, 32), (64, 64, 16)])
def test_whole_plane_kernels_give_the_bits_of_the_three_launch_form(syn, dims, mode):
    nx, ny, nz = dims
    for source, smode in (("p0", 0), ("p_source", 1)):
        pr = syn.make_problem(nx, ny, nz, heterogeneous=True, nonlinear=True, absorbing=True, alpha_mode=mode, source=source,
                              source_mode=smode, source_many=1 if source != "p0" else 0, nt=16,
                              nt_src=None if source == "p0" else 6, pml_size=4, sensor="random")
        out = {}
        for plane in (1, 0):
            g = gpu(pr, p_raw=1, p_max=1, tuning={"plane_kernels": plane})
            g.run(12)
            g.finish()
            out[plane] = {f: g.field(f) for f in FIELDS}
            out[plane]["series"] = g.stream("p")
            g.close()
        for f, v in out[1].items():
            assert np.abs(v).max() > 0 and np.array_equal(v, out[0][f]), (f, source)


# ---- 6: the work is really gone -------------------------------------------------------------------------------------------
def test_one_stage_one_operator_one_coefficient(syn):
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    absent = {"no_dispersion": ("nabla2", "eta"), "no_absorption": ("nabla1", "tau"), None: ()}
    present = {"no_dispersion": ("nabla1", "tau"), "no_absorption": ("nabla2", "eta"), None: ("nabla1", "nabla2", "tau", "eta")}
    for mode in (*MODES, None):
        pr = syn.make_problem(32, heterogeneous=True, nonlinear=True, absorbing=True, alpha_mode=mode, source="p0", pml_size=4)
        g = gpu(pr, fused_kernels=True)
        g.run(2)
        capi.check(capi.load().kw_profile_enable(g.ctx, 1))
        g.run(6)
        seen = capi.profile_collect(g.ctx)
        capi.check(capi.load().kw_profile_enable(g.ctx, 0))
        for name in absent[mode]:
            with pytest.raises(capi.KWaveError):
                g.field(name)
        for name in present[mode]:
            assert g.field(name).size, name
        g.close()
        assert seen["fused_density"][0] == 6 and seen["fused_velocity"][0] == 6
        if mode is None:  # the power-law path is untouched
            assert seen["fused_absorption_pressure"][0] == 6 and "fused_absorption_pressure_one" not in seen, seen
            assert seen["k_zfused_absorb[2]"][0] == 6
        else:
            assert "fused_absorption_pressure" not in seen and seen["fused_absorption_pressure_one"][0] == 6, seen
            assert "k_zfused_absorb[2]" not in seen and seen["k_zfused_absorb[1]"][0] == 6, seen
            assert not any(k.startswith("sum_pressure") or k.startswith("compute_pressure_terms") for k in seen), seen
    # homogeneous: the coefficient in use is the scalar of the constants, the other one is 0.0, no array at all
    for mode, used, unused in (("no_dispersion", "tau", "eta"), ("no_absorption", "eta", "tau")):
        pr = syn.make_problem(32, heterogeneous=False, nonlinear=False, absorbing=True, alpha_mode=mode, source="p0", pml_size=4)
        g = gpu(pr)
        g.run(1)
        for name in ("tau", "eta"):
            with pytest.raises(capi.KWaveError):
                g.field(name)
        ref = knp.NumpySim(syn.alpha_mode_as_power_law(pr))
        assert g.scalar("absorb_" + used) == pytest.approx(float(getattr(ref, used)), rel=1e-5)
        assert g.scalar("absorb_" + unused) == 0.0
        g.close()


# ---- 7: validation --------------------------------------------------------------------------------------------------------
def test_flags_above_four_are_refused(syn):
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    pr = syn.make_problem(16, heterogeneous=False, nonlinear=False, absorbing=True, source="p0", pml_size=4)
    pr["absorbing_flag"] = np.array([[[5]]], dtype=np.uint64)
    with pytest.raises(capi.KWaveError, match="absorbing_flag"):
        gpu(pr)


def test_entry_points_reject_bad_arguments(syn):
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    set_constants(d, 32, 16, 16)
    a = [d.zeros((16, 16, 32)) for _ in range(7)]
    L, INVALID = d.L, 1
    ok = [x.ptr for x in a]
    assert L.kw_sum_pressure_terms_one_nonlinear(d.ctx, None, ok[1], ok[2], None, None, 0) == INVALID
    assert L.kw_sum_pressure_terms_one_linear(d.ctx, ok[0], None, ok[2], None, None, 1) == INVALID
    assert L.kw_sum_pressure_terms_one_linear(d.ctx, ok[0], ok[1], ok[2], None, None, 2) == INVALID  # no such mode
    assert L.kw_sum_pressure_terms_one_linear(d.ctx, ok[0], ok[1], ok[2], None, None, 1) == 0
    assert L.kw_compute_absorbtion_term_one(d.ctx, None, ok[1]) == INVALID
    assert L.kw_compute_absorbtion_term_one(d.ctx, ok[0], None) == INVALID
    d.call("fused_create")
    n = C.c_size_t()
    d.call("fused_reduced_elems", C.byref(n))
    kappa = d.zeros(n.value)
    dd = [d.zeros(2 * k) for k in (17, 16, 16)]
    pml = [d.zeros(k) for k in (32, 16, 16)]
    u = [d.zeros((16, 16, 32)) for _ in range(3)]

    def density(nonlinear, terms, t, flags=0):
        return L.kw_fused_density(d.ctx, nonlinear, *[x.ptr for x in u], *ok[:3], *[x.ptr for x in pml], None, kappa.ptr,
                                  *[x.ptr for x in dd], None, None, None, terms, None, *t, flags)
    assert density(1, 7, ok[3:6]) == INVALID                  # terms > 6
    assert density(1, 5, (ok[3], None, ok[5])) == INVALID     # nonlinear: `first` goes to t1
    assert density(1, 5, (None, ok[4], None)) == INVALID      # plain no_dispersion: the term goes to t2
    assert density(0, 6, (None, None, None)) == INVALID       # linear: `first` goes to t0
    assert density(1, 5, (None, ok[4], None), 2) == 0         # chained (KW_FUSED_CHAIN_TERMS): `first` alone
    assert density(0, 6, (ok[3], None, None)) == 0

    def pressure(p, term, first, nabla, which, flags):
        return L.kw_fused_absorption_pressure_one(d.ctx, p, term, first, nabla, None, None, which, flags)
    assert pressure(None, ok[1], ok[2], kappa.ptr, 0, 0) == INVALID
    assert pressure(ok[0], None, ok[2], kappa.ptr, 0, 0) == INVALID   # no term and none in scratch
    assert pressure(ok[0], ok[1], None, kappa.ptr, 0, 0) == INVALID
    assert pressure(ok[0], ok[1], ok[2], None, 0, 0) == INVALID
    assert pressure(ok[0], ok[1], ok[2], kappa.ptr, 2, 0) == INVALID  # no such mode
    assert pressure(ok[0], ok[1], ok[2], kappa.ptr, 0, 4) == INVALID  # no such flag
    assert pressure(ok[0], ok[1], ok[2], kappa.ptr, 1, 0) == 0
    d.sync()
    d.close()


# ---- 8: slabs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,mode", [(2, "no_dispersion"), (4, "no_absorption")])
def test_slab_ranks_match_the_single_rank_run(syn, tmp_path, world, mode):
    dims, steps = (32, 32, 32), 16
    out = str(tmp_path / f"alpha_mode_{world}.npz")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(29810 + world), os.path.join(HERE, "alpha_mode_dist_worker.py"), "--dims", *map(str, dims),
           "--steps", str(steps), "--mode", mode, "--out", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout[-4000:]
    res = np.load(out)
    # a chained absorbing step has 13 transposes (3 velocity, 6 density, 4 absorption); with one term the absorption
    # stage has 2, which leaves 11.  Every transpose is the same number of exchange callbacks on a given rank layout.
    per_step, per_step_full = res["exchanges_per_step"]
    print(f"world {world} {mode}: {per_step} callbacks per step, full power law {per_step_full}")
    assert per_step_full > 0 and per_step_full % 13 == 0
    assert per_step == 11 * (per_step_full // 13)
    pr = syn.make_problem(*dims, heterogeneous=True, nonlinear=True, absorbing=True, alpha_mode=mode, source="p_source",
                          source_mode=1, source_many=1, nt=steps, nt_src=8, pml_size=4, sensor="random")
    g = gpu(pr, p_raw=1)
    g.run(steps)
    g.finish()
    for f in ("p", "ux", "uz", "rhoy"):
        assert rel_l2(res[f], g.field(f)) <= TOL, f
    assert rel_l2(res["series"], g.stream("p")) <= TOL
    g.close()
    refs = references(syn, ("slab",), pr, steps)
    assert rel_l2(res["p"], refs[mode]["p"]) <= TOL
    assert min(rel_l2(res["p"], refs[run]["p"]) for run in ZEROED if run != mode) >= FAR


# ---- 9: restart and the command line --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("source,split", [("p0", 1), ("p_source", 5)])
def test_restart_is_bit_identical(syn, source, split, mode):
    nt = 16
    streams = dict(p_raw=1, p_max=1, u_raw=1)
    pr = syn.make_problem(32, 16, 32, heterogeneous=True, nonlinear=True, absorbing=True, alpha_mode=mode, nt=nt, pml_size=4,
                          sensor="random", source=source, source_many=1 if source != "p0" else 0,
                          nt_src=None if source == "p0" else 9)
    ref = gpu(pr, **streams)
    ref.run(nt)
    ref.finish()
    a = gpu(pr, **streams)
    a.run(split)
    state = a.checkpoint_state()
    a.close()
    b = gpu(pr, **streams)
    b.restore_state(state)
    b.run(nt - split)
    b.finish()
    for f in FIELDS:
        assert np.array_equal(b.field(f), ref.field(f)), f
    for s in ("p", "p_max", "ux"):
        assert np.array_equal(b.stream(s), ref.stream(s)), s
    b.close()
    ref.close()


@pytest.mark.parametrize("mode,flag", [("no_dispersion", "3"), ("no_absorption", "4")])
def test_command_line_output_file_carries_the_flag(syn, tmp_path, mode, flag):
    import kwave_amd  # noqa: F401
    import h5dump_util
    from kwave_amd import capi, h5io
    if not (os.path.exists(h5io.H5_LIB_PATH) and h5dump_util.available()):
        pytest.skip("HDF5 component or h5dump not available")
    pr = syn.make_problem(32, heterogeneous=True, nonlinear=True, absorbing=True, alpha_mode=mode, source="p0", nt=12, pml_size=4)
    path_in, path_out = str(tmp_path / "in.h5"), str(tmp_path / "out.h5")
    h5io.write_input_file(pr, path_in)
    exe = os.path.join(capi.PKG, "lib", "kspaceFirstOrder-HIP")
    r = subprocess.run([exe, "-i", path_in, "-o", path_out, "--p_raw", "--p_final"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    for name, value in (("absorbing_flag", flag), ("alpha_power", "1.5")):
        dump = subprocess.run([h5dump_util.H5DUMP, "-d", "/" + name, path_out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True, timeout=60)
        assert dump.returncode == 0, dump.stdout
        data = dump.stdout.split("DATA {", 1)[1]
        assert data.split(":", 1)[1].split()[0].rstrip(",") == value, (name, dump.stdout)
    mem = gpu(pr, p_raw=1)
    mem.run(12)
    mem.finish()
    assert np.array_equal(h5io.read_dataset(path_out, "p_final"), mem.field("p"))
    mem.close()
