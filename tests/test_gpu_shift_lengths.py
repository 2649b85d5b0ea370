"""kw_fused_shift_velocity (k_xshift<LEN, TAIL> along x, k_zfused<LEN, Z_SHIFT> along y and z) at every fast-path line
length, against fp64 numpy on the same float32 data.

Filter: a random Hermitian vector instead of the physical half-cell shift — H[k] random complex with modulus in
[0.5, 1.5] for 0 < k < N/2, H[N-k] = conj(H[k]), H[0] and H[N/2] real — so that a read of a neighbouring or mirrored bin
cannot hide behind a smooth unit-modulus filter.  Input: white noise between guard bands (gpu_buffers.Guarded); the output
buffer starts as other noise.  Reference: N * ifft(fft(in, axis) * H, axis).real in float64 (the kernel's inverse is
unnormalised and the 1/N is folded into H, see kwave_hip.h); its imaginary part is asserted negligible, which checks the
construction of H.  test_gpu_kernels.test_fused_shift_velocity_matches_oracle stays as the test with the physical filter.

Checks per grid and axis: test_gpu_stages.metrics along the tested axis (whole array, worst line, upper half of the
spectrum) within TOL_WHOLE, TOL_LINE and TOL_UPPER of test_gpu_stages.py — a one-axis transform pair of the same line
kernels has fewer roundings than the three-axis stages those numbers were measured on; the in-place call gives the
out-of-place bits; the input of the out-of-place call is unchanged; guard bands intact.

Grids: (n,16,16) / (16,n,16) / (16,16,n) for the axis along n; (n,108,1) for axes 0 and 1 (what the host calls in 2-D);
(64,100,108) and the three mixed grids for all axes.  The masked kernel k_xshift<LEN, true> runs when Ny*Nz is no multiple
of the 2*nl_x(Nx) = 16, 20, 24 or 32 rows of an x tile:
  * 108 rows (2-D) leave a partial tile for all four tile heights;
  * the 256 rows of (n,16,16) are 16 mod 20 and 16 mod 24: a full launch plus a masked one for the 20- and 24-row classes;
  * the 10800 rows of (64,100,108) are 16 mod 32: the same for the 32-row class;
  * in 3-D Ny*Nz is always a multiple of 16 (every length is a multiple of 4), so the 16-row class has no masked case there.

These tests were not run on a GPU when they were written: no measured worst values are recorded here yet.  Each test
prints (whole array / worst line / upper half) per axis on a line that starts with SHIFT; the first run on an MI355X should
put the largest of them here, next to the tolerances 2.2e-6 / 5e-6 / 2.1e-6.
"""
import numpy as np
import pytest

from gpu_buffers import Guarded, set_constants
from test_gpu_stages import AXIS_GRIDS, MIXED_GRIDS, TOL_LINE, TOL_UPPER, TOL_WHOLE, TWO_D_GRIDS, metrics

pytestmark = pytest.mark.gpu

gid = lambda d: "x".join(map(str, d))  # noqa: E731


def random_hermitian_filter(rng, n):
    h = np.zeros(n, np.complex128)
    k = np.arange(1, (n + 1) // 2)
    h[k] = rng.uniform(0.5, 1.5, k.size) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, k.size))
    h = h.astype(np.complex64)
    h[n - k] = np.conj(h[k])
    h[0] = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
    if n % 2 == 0:
        h[n // 2] = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
    return h


def check_shift(dims, axes):
    import kwave_amd  # noqa: F401
    from kwave_amd import capi
    nx, ny, nz = dims
    rng = np.random.default_rng(7919 * nx + 31 * ny + nz)
    d = capi.Device()
    try:
        set_constants(d, nx, ny, nz)
        d.call("fused_create")
        bits = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
        for axis in axes:
            n, ax = dims[axis], 2 - axis  # array axes are (z, y, x)
            h = random_hermitian_filter(rng, n)
            u = rng.standard_normal((nz, ny, nx)).astype(np.float32)
            full = n * np.fft.ifft(np.fft.fft(u.astype(np.float64), axis=ax) *
                                   h.astype(np.complex128).reshape([-1 if i == ax else 1 for i in range(3)]), axis=ax)
            ref = full.real
            assert np.linalg.norm(ref) > 0.0
            assert np.linalg.norm(full.imag) <= 1e-12 * np.linalg.norm(ref), "the filter is not Hermitian"
            d_h = Guarded(d, h.view(np.float32))
            d_in = Guarded(d, u)
            d_out = Guarded(d, rng.standard_normal(u.shape).astype(np.float32))
            d.call("fused_shift_velocity", axis, d_in.ptr, d_out.ptr, d_h.ptr)
            got = d_out.read()
            assert bits(d_in.read(), u), (dims, axis, "input changed")
            d.call("fused_shift_velocity", axis, d_in.ptr, d_in.ptr, d_h.ptr)  # in place
            assert bits(d_in.read(), got), (dims, axis, "in-place result differs from the out-of-place one")
            assert bits(d_h.read(), h.view(np.float32)), (dims, axis, "filter changed")
            w, ln, up = metrics(got, ref, (ax,))
            print(f"\nSHIFT {gid(dims)} axis {axis}: {w:.2e}/{ln:.2e}/{up:.2e}")
            assert w <= TOL_WHOLE and ln <= TOL_LINE and up <= TOL_UPPER, (dims, axis, w, ln, up)
    finally:
        d.close()


@pytest.mark.parametrize("dims", AXIS_GRIDS, ids=gid)
def test_shift_every_length(dims):
    axes = (0, 1, 2) if dims == (16, 16, 16) else (next(a for a in range(3) if dims[a] != 16),)
    check_shift(dims, axes)


@pytest.mark.parametrize("dims", TWO_D_GRIDS, ids=gid)
def test_shift_masked_x_tiles_2d(dims):
    check_shift(dims, (0, 1))


@pytest.mark.parametrize("dims", [(64, 100, 108)] + MIXED_GRIDS, ids=gid)
def test_shift_mixed_grids(dims):
    check_shift(dims, (0, 1, 2))
