"""Stokes absorption (absorbing_flag = 2, alpha_power = 2) on the GPU.

Yardstick: the unchanged fp64 oracle (oracle/kwave_np.py NumpySim) run as the power law with absorbing_flag = 1 and
alpha_power = 2, which is the Stokes equation of state (tests/test_stokes_host.py holds that premise to 1e-10 on the
CPU).  Tolerance: relative L2 <= 1e-5 on p, u and rho, the project's TOL (the fp32 C oracle sits at 6.6e-7 from NumpySim
at 40 steps).  A lossless run of the same problems is >= 1e-3 away, so a dropped tau term cannot pass.

Bits: the fused density epilogue (terms == 4), chained or not, whole-plane or three-launch form, and the element-wise
kernel on the stored gradients all evaluate kw_stokes_pressure without fma contraction: asserted bit-identical.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_l2

sys.path.insert(0, ROOT)
from oracle import kwave_np as knp  # noqa: E402
from gpu_buffers import BONA, C2, DT, RHO0, TAU, Guarded, set_constants  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-5
FAR = 1e-3  # what a lossless run differs by at 40 steps (measured on the CPU: 2.9e-3 p0, 1.3e-2 p-source)
FIELDS = ("p", "ux", "uy", "uz", "rhox", "rhoy", "rhoz")


def gpu(pr, **kw):
    import kwave_amd  # noqa: F401
    from kwave_amd.solver import HostSolver
    return HostSolver(pr, **kw)


def numpy_fields(sim):
    return {"p": sim.p, "ux": sim.u[0], "uy": sim.u[1], "uz": sim.u[2], "rhox": sim.rho[0], "rhoy": sim.rho[1],
            "rhoz": sim.rho[2]}


def reference(syn, pr, steps, lossless=False):
    """NumpySim of the power law at alpha_power = 2 (absorbing_flag = 1); lossless: the same problem with flag 0"""
    ref = syn.stokes_as_power_law(pr)
    if lossless:
        ref["absorbing_flag"] = np.array([[[0]]], dtype=np.uint64)
    sim = knp.NumpySim(ref)
    for _ in range(steps):
        sim.step()
    return numpy_fields(sim)


def errors(pr, want, steps, **kw):
    g = gpu(pr, **kw)
    g.run(steps)
    got = {f: g.field(f) for f in FIELDS}
    g.close()
    errs = {}
    for f in FIELDS:
        if np.abs(want[f]).max() == 0.0:  # (2-D: u_z, rho_z)
            assert not got[f].any(), f
        else:
            errs[f] = rel_l2(got[f], want[f])
    return errs, got


# ---- 1 + 2: parity with the oracle, and distance from the lossless run ------------------------------------------------
@pytest.mark.parametrize("heterogeneous", [False, True])
@pytest.mark.parametrize("nonlinear", [False, True])
def test_media_p0_32(syn, heterogeneous, nonlinear):
    pr = syn.make_problem(32, heterogeneous=heterogeneous, nonlinear=nonlinear, absorbing=True, stokes=True, source="p0")
    want, far = reference(syn, pr, 40), reference(syn, pr, 40, lossless=True)
    assert rel_l2(far["p"], want["p"]) >= FAR
    for fused in (True, False):
        errs, got = errors(pr, want, 40, fused_kernels=fused)
        print(f"het={heterogeneous} nonlinear={nonlinear} fused={fused}: {errs}")
        assert max(errs.values()) <= TOL, (fused, errs)
        assert rel_l2(got["p"], far["p"]) >= FAR, fused


@pytest.mark.parametrize("source,mode", [("p_source", 0), ("p_source", 1), ("p_source", 2), ("u_source", 1)])
def test_time_varying_sources(syn, source, mode):
    """nt_src = 25 of 40 steps: with a pressure source the fused run takes the element-wise kernel on stored gradients
    while the source is on, and the chained density epilogue afterwards"""
    pr = syn.make_problem(32, heterogeneous=True, nonlinear=True, absorbing=True, stokes=True, source=source, source_mode=mode,
                          source_many=1, nt=40, nt_src=25, pml_size=4)
    want, far = reference(syn, pr, 40), reference(syn, pr, 40, lossless=True)
    assert rel_l2(far["p"], want["p"]) >= FAR
    for fused in (True, False):
        errs, got = errors(pr, want, 40, fused_kernels=fused)
        print(f"{source} mode {mode} fused={fused}: {errs}")
        assert max(errs.values()) <= TOL, (fused, errs)
        assert rel_l2(got["p"], far["p"]) >= FAR, fused


# ---- 3: every kernel form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [
    (512, 16, 16), (16, 512, 16), (16, 16, 512),  # long x lines (8 lines per tile); 2 x 256 y and z lines
    (448, 16, 16),                                # radix-7, long-line code object
    (400, 16, 16),                                # mixed radix (25 x 16), short-line code object
    (100, 16, 108),                               # masked tails: 1728 rows do not fill whole x tiles
    (64, 64, 64), (32, 32, 48),                   # whole-plane kernels
])
def test_kernel_forms(syn, dims):
    nx, ny, nz = dims
    pr = syn.make_problem(nx, ny, nz, heterogeneous=True, nonlinear=True, absorbing=True, stokes=True, source="p0", pml_size=4)
    steps = 24
    want = reference(syn, pr, steps)
    errs, _ = errors(pr, want, steps, fused_kernels=True)
    print(f"{dims}: {errs}")
    assert max(errs.values()) <= TOL, errs


def test_2d_grid(syn):
    pr = syn.as_2d_file(syn.make_problem(64, 48, 1, heterogeneous=True, nonlinear=True, absorbing=True, stokes=True, source="p0",
                                         nt=40, pml_size=6, sensor="random"))
    want = reference(syn, pr, 40)
    for fused in (True, False):
        errs, _ = errors(pr, want, 40, fused_kernels=fused)
        print(f"2-D fused={fused}: {errs}")
        assert max(errs.values()) <= TOL, (fused, errs)


def test_nonuniform_grid(syn):
    """non-uniform grid on the fused passes: gradients as arrays, scaled, then the element-wise kernels"""
    pr = syn.make_problem(32, heterogeneous=True, nonlinear=True, absorbing=True, stokes=True, source="p0", pml_size=4,
                          nonuniform=True)
    want = reference(syn, pr, 40)
    for fused in (True, False):
        errs, _ = errors(pr, want, 40, fused_kernels=fused)
        print(f"non-uniform fused={fused}: {errs}")
        assert max(errs.values()) <= TOL, (fused, errs)


# ---- 4: the absorption stage is gone ------------------------------------------------------------------------------------
def test_no_absorption_stage_and_no_absorption_operators(syn):
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    seen = {}
    for stokes in (True, False):
        pr = syn.make_problem(32, heterogeneous=True, nonlinear=True, absorbing=True, stokes=stokes, source="p0", pml_size=4)
        g = gpu(pr, fused_kernels=True)
        g.run(2)
        capi.check(capi.load().kw_profile_enable(g.ctx, 1))
        g.run(6)
        seen[stokes] = capi.profile_collect(g.ctx)
        capi.check(capi.load().kw_profile_enable(g.ctx, 0))
        if stokes:
            for name in ("nabla1", "nabla2", "eta"):
                with pytest.raises(capi.KWaveError):
                    g.field(name)
            assert g.field("tau").shape == (32, 32, 32)  # heterogeneous: tau is an array; nothing else of the power law
        else:
            assert g.field("nabla1").size and g.field("eta").size
        g.close()
    assert "fused_absorption_pressure" not in seen[True], seen[True]
    assert seen[True]["fused_density"][0] == 6 and seen[True]["fused_velocity"][0] == 6
    assert not any(k.startswith("sum_pressure") or k.startswith("compute_pressure_terms") for k in seen[True]), seen[True]
    assert seen[False]["fused_absorption_pressure"][0] == 6  # the power-law path is untouched
    # homogeneous: tau is the scalar of the constants, no array at all
    pr = syn.make_problem(32, heterogeneous=False, nonlinear=False, absorbing=True, stokes=True, source="p0", pml_size=4)
    g = gpu(pr)
    g.run(1)
    with pytest.raises(capi.KWaveError):
        g.field("tau")
    ref = knp.NumpySim(syn.stokes_as_power_law(pr))
    assert g.scalar("absorb_tau") == pytest.approx(float(ref.tau), rel=1e-6) and g.scalar("absorb_eta") == 0.0
    g.close()


# ---- 5: validation ------------------------------------------------------------------------------------------------------
def test_flag_two_needs_alpha_power_two(syn):
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    pr = syn.make_problem(16, heterogeneous=False, nonlinear=False, absorbing=True, stokes=True, source="p0", pml_size=4)
    pr["alpha_power"] = np.array([[[1.5]]], dtype=np.float32)
    with pytest.raises(capi.KWaveError, match="alpha_power"):
        gpu(pr)
    pr["alpha_power"] = np.array([[[1.0]]], dtype=np.float32)
    with pytest.raises(capi.KWaveError, match="must not equal to 1.0"):
        gpu(pr)


def test_entry_points_reject_bad_arguments(syn):
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    d = capi.Device()
    set_constants(d, 32, 16, 16)
    a = [d.zeros((16, 16, 32)) for _ in range(7)]
    L, INVALID = d.L, 1
    ok = [x.ptr for x in a]
    assert L.kw_sum_pressure_stokes_nonlinear(d.ctx, None, *ok[1:], None, None, None, None) == INVALID
    assert L.kw_sum_pressure_stokes_linear(d.ctx, None, *ok[1:], None, None, None) == INVALID
    assert L.kw_sum_pressure_stokes_linear(d.ctx, *ok[:6], None, None, None, None) == INVALID  # a gradient missing
    assert L.kw_sum_pressure_stokes_nonlinear(d.ctx, *ok, None, None, None, None) == 0
    d.call("fused_create")
    n = C.c_size_t()
    d.call("fused_reduced_elems", C.byref(n))
    kappa = d.zeros(n.value)
    dd = [d.zeros(2 * k) for k in (17, 16, 16)]
    pml = [d.zeros(k) for k in (32, 16, 16)]
    u = [d.zeros((16, 16, 32)) for _ in range(3)]

    def density(terms, t0):
        return L.kw_fused_density(d.ctx, 1, *[x.ptr for x in u], *ok[:3], *[x.ptr for x in pml], None, kappa.ptr,
                                  *[x.ptr for x in dd], None, None, None, terms, None, t0, None, None, 0)
    assert density(4, None) == INVALID   # terms == 4 without its output
    assert density(5, ok[3]) == INVALID  # terms > 4
    assert density(4, ok[3]) == 0
    d.sync()
    d.close()


# ---- 6: bits --------------------------------------------------------------------------------------------------------------
def density_stage(g, nonlinear, arrays, rec=None):
    """the body of test_density_stage_bits_and_fp64 on the Grid g (test_gpu_stages.Grid): asserts every bit identity and
    returns rel-L2(p) against fp64; rec(label, got, fp64), when given, is handed the stored densities and gradients"""
    from test_gpu_stages import CHAIN_TERMS, P_IN_SCRATCH
    d = g.dev
    u_h = g.comps([g.noise() for _ in range(3)])
    rho_h = g.comps([g.noise() for _ in range(3)])
    pml = g.pml_vectors()
    med = {k: (g.media(lo, hi) if arrays else None) for k, (lo, hi) in
           dict(rho0=(0.8, 1.8), bona=(0.2, 1.0), c2=(1.0, 3.0), tau=(0.5, 1.0)).items()}
    dev = {k: (g.ro(v) if v is not None else None) for k, v in med.items()}
    ptr = lambda x: x.ptr if x is not None else None  # noqa: E731
    dd = [g.dd[k] for k in ("ddx_k_shift_neg_r", "ddy_k_shift_neg", "ddz_k_shift_neg")]
    pml_d = [g.ro(x) for x in pml]
    u_d = [g.ro(x) for x in u_h]
    out = {}
    for flags in (0, CHAIN_TERMS):
        rho = [g.field(x) for x in rho_h]
        du = [g.field(g.noise()) for _ in range(3)] if flags == 0 else [None] * 3
        p = g.field(g.noise())
        d.call("fused_density", nonlinear, *[x.ptr for x in u_d], *[x.ptr for x in rho], *[x.ptr for x in pml_d], ptr(dev["rho0"]),
               g.padded["kappa"].ptr, *[x.ptr for x in dd], *[ptr(x) for x in du], 4, ptr(dev["bona"]), p.ptr, ptr(dev["c2"]),
               ptr(dev["tau"]), flags)
        out[flags] = dict(p=p.read(), rho=[x.read() for x in rho], p_dev=p, rho_dev=rho, du_dev=du)
    assert np.array_equal(out[0]["p"].view(np.uint32), out[CHAIN_TERMS]["p"].view(np.uint32)), "chained p differs from plain p"
    for a in range(3):
        assert np.array_equal(out[0]["rho"][a].view(np.uint32), out[CHAIN_TERMS]["rho"][a].view(np.uint32))
    # the consumer of the chained spectrum (the spectrum is still in scratch: nothing ran since the chained call)
    dd_pos = [g.dd[k] for k in ("ddx_k_shift_pos_r", "ddy_k_shift_pos", "ddz_k_shift_pos")]
    u0 = g.comps([g.noise() for _ in range(3)])
    vel = {}
    for flags in (P_IN_SCRATCH, 0):
        uu = [g.field(x) for x in u0]
        d.call("fused_velocity", out[CHAIN_TERMS]["p_dev"].ptr, *[x.ptr for x in uu], None, None, None, *[x.ptr for x in pml_d],
               g.padded["kappa"].ptr, *[x.ptr for x in dd_pos], flags)
        vel[flags] = [x.read() for x in uu]
    for a in range(3):
        assert np.array_equal(vel[0][a].view(np.uint32), vel[P_IN_SCRATCH][a].view(np.uint32)), f"u{a} from the chained spectrum"
    # element-wise kernel on what the plain call stored
    q = g.field(g.noise())
    args = [q.ptr, *[x.ptr for x in out[0]["rho_dev"]], *[x.ptr for x in out[0]["du_dev"]], ptr(dev["c2"])]
    if nonlinear:
        d.call("sum_pressure_stokes_nonlinear", *args, ptr(dev["bona"]), ptr(dev["rho0"]), ptr(dev["tau"]))
    else:
        d.call("sum_pressure_stokes_linear", *args, ptr(dev["rho0"]), ptr(dev["tau"]))
    assert np.array_equal(q.read().view(np.uint32), out[0]["p"].view(np.uint32)), "element-wise kernel differs from the epilogue"
    du_plain = [x.read() for x in out[0]["du_dev"]]
    for a in range(3):  # inputs of the element-wise kernel, and the p that kw_fused_velocity read
        assert np.array_equal(out[0]["rho_dev"][a].read().view(np.uint32), out[0]["rho"][a].view(np.uint32)), f"rho{a} changed"
    assert np.array_equal(out[CHAIN_TERMS]["p_dev"].read().view(np.uint32), out[0]["p"].view(np.uint32)), "p changed"
    # fp64
    f8 = lambda x, s: x.astype(np.float64) if x is not None else s  # noqa: E731
    ref = knp.stage_density([x.astype(np.float64) for x in u_h], [x.astype(np.float64) for x in rho_h],
                            [g.bcast(x.astype(np.float64), a) for a, x in enumerate(pml)], f8(med["rho0"], RHO0), DT,
                            g.k64["kappa"], g.dd_neg, bool(nonlinear), 2 if nonlinear else 1, f8(med["bona"], BONA))
    S, first, vgt = (ref["t"][0], ref["t"][1], ref["t"][2]) if nonlinear else (ref["t"][0], ref["t"][0], ref["t"][1])
    ones = np.ones((g.nz, g.ny, g.nx // 2 + 1))
    want = knp.stage_absorption_pressure(first, vgt, S, ones, 0.0 * ones, f8(med["c2"], C2), f8(med["tau"], TAU), 0.0)
    if rec is not None:  # what the plain call stored, quantity by quantity
        for a in range(3):
            rec(f"stokes rho{a}", out[0]["rho"][a], ref["rho"][a])
            rec(f"stokes du{a}", du_plain[a], ref["du"][a])
    return rel_l2(out[0]["p"], want)


@pytest.mark.parametrize("dims,plane", [((32, 32, 16), 1), ((32, 32, 16), 0), ((64, 64, 16), 1), ((256, 16, 16), 1),
                                        ((100, 16, 108), 1), ((512, 16, 16), 1), ((48, 32, 1), 1)])
@pytest.mark.parametrize("nonlinear,arrays", [(1, True), (0, False)])
def test_density_stage_bits_and_fp64(syn, dims, plane, nonlinear, arrays):
    """kw_fused_density(terms = 4) on white-noise inputs between guard bands: plain and chained give the same p, which
    is also what kw_sum_pressure_stokes_* computes from the densities and gradients the plain call stored (the path of a
    step with an active pressure source); p against the fp64 stage functions of the oracle.  The chained spectrum is
    consumed by kw_fused_velocity(KW_FUSED_P_IN_SCRATCH), which must give the bits of the call that reads p."""
    from test_gpu_stages import Grid
    g = Grid(syn, dims, plane_kernels=plane)
    try:
        err = density_stage(g, nonlinear, arrays)
        print(f"{dims} plane={plane} nonlinear={nonlinear} arrays={arrays}: rel-L2(p) = {err:.3e}")
        assert err <= TOL
        g.check_readonly()
    finally:
        g.close()


@pytest.mark.parametrize("dims", [(32, 32, 32), (64, 64, 16)])
def test_whole_plane_kernels_give_the_bits_of_the_three_launch_form(syn, dims):
    nx, ny, nz = dims
    for source, mode in (("p0", 0), ("p_source", 1)):
        pr = syn.make_problem(nx, ny, nz, heterogeneous=True, nonlinear=True, absorbing=True, stokes=True, source=source,
                              source_mode=mode, source_many=1 if source != "p0" else 0, nt=16, nt_src=None if source == "p0" else 6,
                              pml_size=4, sensor="random")
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


# ---- 7: around it -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
def test_slab_ranks_match_the_single_rank_run(syn, tmp_path, world):
    dims, steps = (32, 32, 32), 16
    out = str(tmp_path / f"stokes_{world}.npz")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(29790 + world), os.path.join(HERE, "stokes_dist_worker.py"), "--dims", *map(str, dims),
           "--steps", str(steps), "--out", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout[-4000:]
    res = np.load(out)
    pr = syn.make_problem(*dims, heterogeneous=True, nonlinear=True, absorbing=True, stokes=True, source="p_source",
                          source_mode=1, source_many=1, nt=steps, nt_src=8, pml_size=4, sensor="random")
    assert int(res["exchanges"][0]) > 0
    g = gpu(pr, p_raw=1)
    g.run(steps)
    g.finish()
    for f in ("p", "ux", "uz", "rhoy"):
        assert rel_l2(res[f], g.field(f)) <= TOL, f
    assert rel_l2(res["series"], g.stream("p")) <= TOL
    g.close()
    want = reference(syn, pr, steps)
    assert rel_l2(res["p"], want["p"]) <= TOL


@pytest.mark.parametrize("source,split", [("p0", 1), ("p_source", 5)])
def test_restart_is_bit_identical(syn, source, split):
    nt = 16
    streams = dict(p_raw=1, p_max=1, u_raw=1)
    pr = syn.make_problem(32, 16, 32, heterogeneous=True, nonlinear=True, absorbing=True, stokes=True, nt=nt, pml_size=4,
                          sensor="random", source=source, source_many=1 if source != "p0" else 0, nt_src=None if source == "p0" else 9)
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


def test_command_line_output_file_carries_the_flag(syn, tmp_path):
    import kwave_amd  # noqa: F401
    import h5dump_util
    from kwave_amd import capi, h5io
    if not (os.path.exists(h5io.H5_LIB_PATH) and h5dump_util.available()):
        pytest.skip("HDF5 component or h5dump not available")
    pr = syn.make_problem(32, heterogeneous=True, nonlinear=True, absorbing=True, stokes=True, source="p0", nt=12, pml_size=4)
    path_in, path_out = str(tmp_path / "in.h5"), str(tmp_path / "out.h5")
    h5io.write_input_file(pr, path_in)
    exe = os.path.join(capi.PKG, "lib", "kspaceFirstOrder-HIP")
    r = subprocess.run([exe, "-i", path_in, "-o", path_out, "--p_raw", "--p_final"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    for name, value in (("absorbing_flag", "2"), ("alpha_power", "2")):
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
