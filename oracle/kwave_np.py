"""Independent fp64 NumPy restatement of the per-step algorithm.

TEST INFRASTRUCTURE ONLY.  Its purpose is to bound the error of the fp32 C oracle
(oracle/kwave_oracle.c) — test K4 of SURVEY.md §8c — and to provide the closed-form K1 check.
It follows the same reference lines as the C oracle (KSpaceSolver/KSpaceFirstOrderSolver.cpp:864-943,
2087-2396, 2404-2703; KSpaceSolver/SolverCudaKernels.cu per kernel) but is written against
numpy.fft.rfftn/irfftn in float64, with whole-array expressions, so an indexing or ordering slip in one
restatement does not repeat in the other.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np


def _sc(a) -> float:
    return float(np.asarray(a).reshape(-1)[0])


def _c(pairs: np.ndarray) -> np.ndarray:
    p = np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
    return p[:, 0] + 1j * p[:, 1]


def complete_2d(pr: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A 2-D problem (Nz == 1) as the degenerate 3-D one both restatements run: the z datasets a 2-D input file does not
    have, with the values that make the 3-D formulas reduce to the reference's SD::k2D ones (zero z-gradient operators,
    unit z-PML and z-shift, rho0_sgz = rho0_sgx; u_z and rho_z then stay zero)."""
    if int(_sc(pr["Nz"])) != 1:
        return pr
    out = dict(pr)
    zero_c = np.zeros((1, 1, 2), dtype=np.float32)
    one = np.ones((1, 1, 1), dtype=np.float32)
    out.setdefault("ddz_k_shift_pos", zero_c)
    out.setdefault("ddz_k_shift_neg", zero_c)
    out.setdefault("z_shift_neg_r", np.array([[[1.0, 0.0]]], dtype=np.float32))
    out.setdefault("pml_z", one)
    out.setdefault("pml_z_sgz", one)
    out.setdefault("rho0_sgz", pr["rho0_sgx"])
    out.setdefault("dz", pr["dx"])  # never used: the only z bin is 0 (the reference sets 1/dz^2 = 0 in 2-D)
    return out


def kspace_real_operators(nx, ny, nz, dx, dy, dz, c_ref, dt, alpha_power=None) -> Dict[str, np.ndarray]:
    """The reduced real k-space operators [nz][ny][nx/2+1] (KSpaceFirstOrderSolver.cpp:2404-2643): kappa, sourceKappa
    and, given alpha_power, nabla1 / nabla2 (0 at k = 0)."""
    fx = 0.5 - np.abs(0.5 - np.arange(nx // 2 + 1) / nx)
    fy = 0.5 - np.abs(0.5 - np.arange(ny) / ny)
    fz = 0.5 - np.abs(0.5 - np.arange(nz) / nz)
    kk = np.sqrt((fz ** 2 / dz ** 2).reshape(-1, 1, 1) + (fy ** 2 / dy ** 2).reshape(1, -1, 1)
                 + (fx ** 2 / dx ** 2).reshape(1, 1, -1))
    arg = c_ref * dt * math.pi * kk
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["kappa"] = np.where(arg == 0.0, 1.0, np.sin(arg) / arg)
    out["source_kappa"] = np.cos(arg)
    if alpha_power is not None:
        k2pi = 2.0 * math.pi * kk
        with np.errstate(divide="ignore"):
            n1 = np.power(k2pi, alpha_power - 2.0)
            n2 = np.power(k2pi, alpha_power - 1.0)
        n1[np.isinf(n1)] = 0.0
        n2[np.isinf(n2)] = 0.0
        out["nabla1"], out["nabla2"] = n1, n2
    return out


def fft_r2c(a: np.ndarray) -> np.ndarray:
    """Forward R2C transform of a [nz][ny][nx] real array: [nz][ny][nx/2+1] complex."""
    return np.fft.rfftn(a, axes=(0, 1, 2))


def fft_c2r(c: np.ndarray, shape) -> np.ndarray:
    """Unnormalised inverse (cuFFT C2R): the 1/N lives in the consumers."""
    return np.fft.irfftn(c, s=tuple(shape), axes=(0, 1, 2)) * float(np.prod(shape))


# ---- the stages of one step, as pure float64 functions: one per fused entry point of include/kwave_hip.h -------------
# Arguments broadcast against [nz][ny][nx]: fields are arrays of that shape; media are arrays or scalars; the derivative
# operators are complex vectors shaped (1, 1, nx/2+1), (1, ny, 1), (nz, 1, 1); kappa / nabla / sourceKappa are real
# [nz][ny][nx/2+1].  Each returns new arrays and changes none of its arguments.

def stage_velocity(p, u, dtrho, pml_sg, kappa, dd_pos):
    """A1-A4 (kw_fused_velocity): u_i <- pml_sg_i (pml_sg_i u_i - dt/rho0_sg_i Fi(dd_i+ kappa F(p)) / N)."""
    shape = np.shape(p)
    d = 1.0 / float(np.prod(shape))
    e = fft_r2c(p) * kappa
    return [(u[a] * pml_sg[a] - d * fft_c2r(e * dd_pos[a], shape) * dtrho[a]) * pml_sg[a] for a in range(3)]


def stage_initial_velocity(p, dtrho, kappa, dd_pos):
    """A12 second half (kw_fused_initial_velocity): u_i = dt/rho0_sg_i Fi(dd_i+ kappa F(p)) / (2 N)."""
    shape = np.shape(p)
    d = 1.0 / float(np.prod(shape))
    e = fft_r2c(p) * kappa
    return [fft_c2r(e * dd_pos[a], shape) * dtrho[a] * d * 0.5 for a in range(3)]


def stage_velocity_gradient(u, kappa, dd_neg, dudn=None):
    """A6-A8 (kw_fused_velocity_gradient): du_i = Fi(dd_i- kappa F(u_i)) / N, times dudn_i on a non-uniform grid
    (SolverCudaKernels.cu:1285-1301; the fused entry point leaves that scaling to the caller)."""
    shape = np.shape(u[0])
    kd = kappa / float(np.prod(shape))
    du = [fft_c2r(fft_r2c(u[a]) * kd * dd_neg[a], shape) for a in range(3)]
    if dudn is not None:
        du = [du[a] * dudn[a] for a in range(3)]
    return du


def density_update(rho, du, pml, rho0, dt, nonlinear):
    """A9: rho_i <- pml_i (pml_i rho_i - s du_i), s = dt (2 sum(rho) + rho0) nonlinear, dt rho0 linear."""
    s = (2.0 * (rho[0] + rho[1] + rho[2]) + rho0) * dt if nonlinear else dt * rho0
    return [pml[a] * (pml[a] * rho[a] - s * du[a]) for a in range(3)]


def pressure_terms(rho, du, rho0, bona, nonlinear):
    """computePressureTerms{Linear,Nonlinear}: (density sum S, first term of the pressure sum, rho0 sum(du)); the first
    term is S linear, S + BonA S^2 / (2 rho0) nonlinear."""
    S = rho[0] + rho[1] + rho[2]
    first = (bona * S * S / (2.0 * rho0) + S) if nonlinear else S
    return S, first, rho0 * (du[0] + du[1] + du[2])


def equation_of_state(rho, c2, rho0, bona, nonlinear):
    """A11 lossless (sumPressure{Nonlinear,Linear}Lossless): p = c2 (S + BonA S^2 / (2 rho0)) | c2 S."""
    S = rho[0] + rho[1] + rho[2]
    return c2 * (S + bona * S * S / (2.0 * rho0)) if nonlinear else c2 * S


def stage_density(u, rho, pml, rho0, dt, kappa, dd_neg, nonlinear, terms=0, bona=0.0, c2=None):
    """A6-A9 and the pressure terms of A11 (kw_fused_density).  Returns {"du", "rho", "t"}: "t" is what the entry point
    writes to t0..t2 — terms 1: [sum rho, rho0 sum du]; 2: [sum rho, nonlinear term, rho0 sum du]; 3: [p] (lossless
    equation of state; c2 an input)."""
    du = stage_velocity_gradient(u, kappa, dd_neg)
    rho_n = density_update(rho, du, pml, rho0, dt, nonlinear)
    t = []
    if terms in (1, 2):
        S, first, vgt = pressure_terms(rho_n, du, rho0, bona, terms == 2)
        t = [S, vgt] if terms == 1 else [S, first, vgt]
    elif terms == 3:
        t = [equation_of_state(rho_n, c2, rho0, bona, nonlinear)]
    return {"du": du, "rho": rho_n, "t": t}


def stage_absorption_pressure(first, vel_grad_term, density_sum, nabla1, nabla2, c2, tau, eta):
    """A11 absorbing, after the terms (kw_fused_absorption_pressure):
    p = c2 (first + (tau Fi(nabla1 F(rho0 sum du)) - eta Fi(nabla2 F(sum rho))) / N)."""
    shape = np.shape(density_sum)
    d = 1.0 / float(np.prod(shape))
    tau_term = fft_c2r(fft_r2c(vel_grad_term) * nabla1, shape)
    eta_term = fft_c2r(fft_r2c(density_sum) * nabla2, shape)
    return c2 * (first + d * (tau_term * tau - eta_term * eta))


def stage_scale_source(s, source_kappa):
    """FFT part of scaleSource (kw_fused_scale_source): Fi(sourceKappa F(s)) / N."""
    shape = np.shape(s)
    return fft_c2r(fft_r2c(s) * source_kappa, shape) / float(np.prod(shape))


class NumpySim:
    def __init__(self, pr: Dict[str, np.ndarray]):
        pr = complete_2d(pr)
        self.pr = pr
        nx, ny, nz = (int(_sc(pr[k])) for k in ("Nx", "Ny", "Nz"))
        self.nx, self.ny, self.nz = nx, ny, nz
        self.shape = (nz, ny, nx)
        self.N = nx * ny * nz
        self.dt = _sc(pr["dt"])
        self.nonlinear = int(_sc(pr["nonlinear_flag"]))
        self.absorbing = int(_sc(pr["absorbing_flag"]))
        f8 = lambda k: np.asarray(pr[k], dtype=np.float64)
        self.c0 = f8("c0") if pr["c0"].size > 1 else _sc(pr["c0"])
        self.rho0 = f8("rho0") if pr["rho0"].size > 1 else _sc(pr["rho0"])
        self.dtrho = [self.dt / (f8(k) if pr[k].size > 1 else _sc(pr[k])) for k in ("rho0_sgx", "rho0_sgy", "rho0_sgz")]
        self.bona = (f8("BonA") if pr["BonA"].size > 1 else _sc(pr["BonA"])) if "BonA" in pr else 0.0
        # non-uniform grid (MatrixContainer.cpp:301-329): dt/rho0_sg carries the staggered-grid derivative scaling
        # (KSpaceFirstOrderSolver.cpp:2650-2685 / SolverCudaKernels.cu:372-410), the velocity gradient the regular one
        self.nonuniform = int(_sc(pr.get("nonuniform_grid_flag", 0)))
        self.dudn = None
        if self.nonuniform:
            sg = [f8("dxudxn_sgx").reshape(1, 1, -1), f8("dyudyn_sgy").reshape(1, -1, 1), f8("dzudzn_sgz").reshape(-1, 1, 1)]
            self.dtrho = [self.dtrho[a] * sg[a] for a in range(3)]
            self.dudn = [f8("dxudxn").reshape(1, 1, -1), f8("dyudyn").reshape(1, -1, 1), f8("dzudzn").reshape(-1, 1, 1)]
        # operators, broadcast shapes
        self.ddx_pos = _c(pr["ddx_k_shift_pos_r"]).reshape(1, 1, -1)
        self.ddy_pos = _c(pr["ddy_k_shift_pos"]).reshape(1, -1, 1)
        self.ddz_pos = _c(pr["ddz_k_shift_pos"]).reshape(-1, 1, 1)
        self.ddx_neg = _c(pr["ddx_k_shift_neg_r"]).reshape(1, 1, -1)
        self.ddy_neg = _c(pr["ddy_k_shift_neg"]).reshape(1, -1, 1)
        self.ddz_neg = _c(pr["ddz_k_shift_neg"]).reshape(-1, 1, 1)
        self.pml = [f8("pml_x").reshape(1, 1, -1), f8("pml_y").reshape(1, -1, 1), f8("pml_z").reshape(-1, 1, 1)]
        self.pml_sg = [f8("pml_x_sgx").reshape(1, 1, -1), f8("pml_y_sgy").reshape(1, -1, 1),
                       f8("pml_z_sgz").reshape(-1, 1, 1)]
        # generators (KSpaceFirstOrderSolver.cpp:2404-2643)
        dx, dy, dz, c_ref = (_sc(pr[k]) for k in ("dx", "dy", "dz", "c_ref"))
        gen = kspace_real_operators(nx, ny, nz, dx, dy, dz, c_ref, self.dt,
                                    _sc(pr["alpha_power"]) if self.absorbing else None)
        self.kappa, self.source_kappa = gen["kappa"], gen["source_kappa"]
        if self.absorbing:
            y = _sc(pr["alpha_power"])
            self.nabla1, self.nabla2 = gen["nabla1"], gen["nabla2"]
            a_np = 100.0 * (1.0e-6 / (2.0 * math.pi)) ** y / (20.0 * math.log10(math.e))
            alpha = f8("alpha_coeff") if pr["alpha_coeff"].size > 1 else _sc(pr["alpha_coeff"])
            a2 = 2.0 * a_np * alpha
            self.tau = -a2 * np.power(self.c0, y - 1.0)
            self.eta = a2 * np.power(self.c0, y) * math.tan(math.pi * y / 2.0)
        self.c2 = self.c0 * self.c0
        z = lambda: np.zeros(self.shape)
        self.p = z()
        self.u = [z(), z(), z()]
        self.rho = [z(), z(), z()]
        self.du = [z(), z(), z()]
        self.t = 0

    # helpers
    def F(self, a):
        return fft_r2c(a)

    def Fi(self, c):
        return fft_c2r(c, self.shape)

    def _src_values(self, inp, n, many):
        inp = np.asarray(inp, dtype=np.float64).reshape(-1)
        return inp[self.t * n:(self.t + 1) * n] if many else np.full(n, inp[self.t])

    def _scaled(self, inp, idx, many):
        T = np.zeros(self.N)
        T[idx] = self._src_values(inp, idx.size, many)
        return stage_scale_source(T.reshape(self.shape), self.source_kappa)

    def step(self):
        pr = self.pr
        dd_pos = (self.ddx_pos, self.ddy_pos, self.ddz_pos)
        # A1-A4
        self.u = stage_velocity(self.p, self.u, self.dtrho, self.pml_sg, self.kappa, dd_pos)
        # A5
        names = ("ux", "uy", "uz")
        if any(int(_sc(pr.get(f"{nm}_source_flag", 0))) for nm in names) or int(_sc(pr.get("transducer_source_flag", 0))):
            idx = np.asarray(pr["u_source_index"], dtype=np.int64).reshape(-1) - 1
            mode = int(_sc(pr["u_source_mode"]))
            many = int(_sc(pr["u_source_many"]))
            for a, nm in enumerate(names):
                if int(_sc(pr.get(f"{nm}_source_flag", 0))) > self.t:
                    flat = self.u[a].reshape(-1)
                    if mode == 2:
                        self.u[a] = self.u[a] + self._scaled(pr[f"{nm}_source_input"], idx, many)
                    else:
                        v = self._src_values(pr[f"{nm}_source_input"], idx.size, many)
                        if mode == 0:
                            flat[idx] = v
                        else:
                            np.add.at(flat, idx, v)
            if int(_sc(pr.get("transducer_source_flag", 0))) > self.t:
                dm = np.asarray(pr["delay_mask"], dtype=np.int64).reshape(-1) - 1
                sig = np.asarray(pr["transducer_source_input"], dtype=np.float64).reshape(-1)
                np.add.at(self.u[0].reshape(-1), idx, sig[dm + self.t])
        # A6-A8
        self.du = stage_velocity_gradient(self.u, self.kappa, (self.ddx_neg, self.ddy_neg, self.ddz_neg), self.dudn)
        # A9
        self.rho = density_update(self.rho, self.du, self.pml, self.rho0, self.dt, self.nonlinear)
        # A10
        if int(_sc(pr.get("p_source_flag", 0))) > self.t:
            idx = np.asarray(pr["p_source_index"], dtype=np.int64).reshape(-1) - 1
            mode = int(_sc(pr["p_source_mode"]))
            many = int(_sc(pr["p_source_many"]))
            ndim = 2 if self.nz == 1 else 3  # SD::k2D: rho_x, rho_y only
            if mode == 2:
                sc = self._scaled(pr["p_source_input"], idx, many)
                self.rho = [r + sc if a < ndim else r for a, r in enumerate(self.rho)]
            else:
                v = self._src_values(pr["p_source_input"], idx.size, many)
                for a in range(ndim):
                    flat = self.rho[a].reshape(-1)
                    if mode == 0:
                        flat[idx] = v
                    else:
                        np.add.at(flat, idx, v)
        # A11
        if not self.absorbing:
            self.p = equation_of_state(self.rho, self.c2, self.rho0, self.bona, self.nonlinear)
        else:
            S, first, vgt = pressure_terms(self.rho, self.du, self.rho0, self.bona, self.nonlinear)
            self.p = stage_absorption_pressure(first, vgt, S, self.nabla1, self.nabla2, self.c2, self.tau, self.eta)
        # A12
        if self.t == 0 and int(_sc(pr.get("p0_source_flag", 0))) == 1:
            p0 = np.asarray(pr["p0_source_input"], dtype=np.float64)
            self.p = p0.copy()
            ndim = 2 if self.nz == 1 else 3  # SolverCudaKernels.cu:873-876 dimScalingFactor
            self.rho = [p0 / (ndim * self.c2) if a < ndim else np.zeros_like(p0) for a in range(3)]
            self.u = stage_initial_velocity(self.p, self.dtrho, self.kappa, dd_pos)
        self.t += 1


def closed_form_pressure(pr: Dict[str, np.ndarray], n_steps: int) -> np.ndarray:
    """K1: homogeneous lossless linear medium, c0 == c_ref, PML == 1, p0 source only.

    p(n dt) = Fi{ cos(c |k| n dt) F{p0} } / N exactly for the k-space corrected scheme, where |k| is
    the wavenumber magnitude used by kappa (KSpaceFirstOrderSolver.cpp:2404-2452).
    Sample index n corresponds to the field after step n (storeSensorData follows the update, :930).
    """
    nx, ny, nz = (int(_sc(pr[k])) for k in ("Nx", "Ny", "Nz"))
    dx, dy, dz = (_sc(pr[k]) for k in ("dx", "dy", "dz"))
    c, dt = _sc(pr["c0"]), _sc(pr["dt"])
    fx = 0.5 - np.abs(0.5 - np.arange(nx // 2 + 1) / nx)
    fy = 0.5 - np.abs(0.5 - np.arange(ny) / ny)
    fz = 0.5 - np.abs(0.5 - np.arange(nz) / nz)
    k = 2.0 * math.pi * np.sqrt((fz ** 2 / dz ** 2).reshape(-1, 1, 1) + (fy ** 2 / dy ** 2).reshape(1, -1, 1)
                                + (fx ** 2 / dx ** 2).reshape(1, 1, -1))
    p0 = np.asarray(pr["p0_source_input"], dtype=np.float64)
    spec = np.fft.rfftn(p0, axes=(0, 1, 2)) * np.cos(c * k * n_steps * dt)
    return np.fft.irfftn(spec, s=(nz, ny, nx), axes=(0, 1, 2))


def absorbing_mode_recurrence(pr: Dict[str, np.ndarray], n_steps: int):
    """K8: homogeneous *absorbing* linear medium (scalar c0, rho0, alpha_coeff), PML == 1 (periodic box), p0 source only.

    Every operator of the step is then diagonal in k-space, so the whole scheme closes per Fourier mode on three
    scalars — p^, R^ = sum_i rho_i^ and S^ = sum_i ddk_i^- kappa u_i^ — independently of any FFT code, field kernel or
    generator loop of the restatements:
        S <- S + (dt/rho0) kappa^2 |k|^2 p          (A2-A4 then A6-A7: sum_i ddk_i^+ ddk_i^- = -|k|^2 by construction)
        R <- R - dt rho0 S                           (A9, linear)
        p <- c^2 ( R (1 - eta nabla2) + tau nabla1 rho0 S )          (A11 absorbing linear, SolverCudaKernels.cu:1978)
    starting after step 0 from  p = p0^, R = p0^/c^2, S = -(dt / 2 rho0) kappa^2 |k|^2 p0^   (A12: u = +dt/(2 rho0) grad p0).
    kappa = sinc(c_ref dt |k| / 2), nabla1 = |k|^(y-2), nabla2 = |k|^(y-1) (0 at k = 0), tau = -2 a c0^(y-1),
    eta = 2 a c0^y tan(pi y / 2), a = alpha_coeff * 100 (1e-6 / 2 pi)^y / (20 log10 e)  (KSpaceFirstOrderSolver.cpp:2514-2643).
    Returns (p, ux) in fp64 after step n_steps; ux from u_x^ <- u_x^ - (dt/rho0) ddx^+ kappa p^ alongside.
    """
    nx, ny, nz = (int(_sc(pr[k])) for k in ("Nx", "Ny", "Nz"))
    dx, dy, dz = (_sc(pr[k]) for k in ("dx", "dy", "dz"))
    c0, rho0, dt, c_ref = _sc(pr["c0"]), _sc(pr["rho0"]), _sc(pr["dt"]), _sc(pr["c_ref"])
    y, alpha = _sc(pr["alpha_power"]), _sc(pr["alpha_coeff"])
    kx = 2.0 * math.pi * np.fft.rfftfreq(nx, dx)
    ky = 2.0 * math.pi * np.fft.fftfreq(ny, dy)
    kz = 2.0 * math.pi * np.fft.fftfreq(nz, dz)
    k2 = (kz ** 2).reshape(-1, 1, 1) + (ky ** 2).reshape(1, -1, 1) + (kx ** 2).reshape(1, 1, -1)
    k = np.sqrt(k2)
    kappa = np.sinc(c_ref * dt * k / 2.0 / math.pi)  # np.sinc(x) = sin(pi x) / (pi x)
    with np.errstate(divide="ignore"):
        nabla1 = np.where(k > 0, k ** (y - 2.0), 0.0)
    nabla2 = np.where(k > 0, k ** (y - 1.0), 0.0)
    a_np = alpha * 100.0 * (1.0e-6 / (2.0 * math.pi)) ** y / (20.0 * math.log10(math.e))
    tau = -2.0 * a_np * c0 ** (y - 1.0)
    eta = 2.0 * a_np * c0 ** y * math.tan(math.pi * y / 2.0)
    ddx_pos = (1j * kx * np.exp(1j * kx * dx / 2.0)).reshape(1, 1, -1)
    p0 = np.fft.rfftn(np.asarray(pr["p0_source_input"], dtype=np.float64), axes=(0, 1, 2))
    g = (dt / rho0) * kappa ** 2 * k2
    p, R, S = p0.copy(), p0 / c0 ** 2, -0.5 * g * p0
    ux = 0.5 * (dt / rho0) * ddx_pos * kappa * p0
    for _ in range(n_steps):
        ux = ux - (dt / rho0) * ddx_pos * kappa * p
        S = S + g * p
        R = R - dt * rho0 * S
        p = c0 ** 2 * (R * (1.0 - eta * nabla2) + tau * nabla1 * rho0 * S)
    back = lambda a: np.fft.irfftn(a, s=(nz, ny, nx), axes=(0, 1, 2))
    return back(p), back(ux)
