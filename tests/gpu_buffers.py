"""Device buffers and constants shared by the kernel-level GPU tests (a plain module, imported by name from tests/).

Guarded: a device array between GUARD-byte bands of 0xFF bytes (NaN as float32).  A kernel that writes outside the
array fails the guard check on read(); one that reads outside it turns its result into NaN.  `offset` moves the
array's start by that many bytes past the 256-byte aligned interior, to hand a kernel a misaligned pointer.

run / check_exact / check_bound: one entry-point call through guarded buffers, a byte-for-byte comparison and the
per-element bound |gpu - fp64| <= (k + 1) 2^-24 M of the kernel-level tests (k roundings on the longest path, M the same
sums on absolute values); WORST keeps the worst ratio seen per (family, k) for the modules' end-of-run report.
"""
import numpy as np

GUARD = 4096
U = 2.0 ** -24
WORST = {}  # (family, k) -> worst |gpu - fp64| / (2^-24 M) seen, against its k + 1

# scalar media of the Constants (arbitrary, O(1)); the operators are generated with dx = dy = dz = 1, c_ref = 1
DT, RHO0, C2, BONA, TAU, ETA = 0.7, 1.3, 2.1, 0.6, 0.8, 0.45
DT_RHO0_SG = (0.9, 1.1, 0.75)


def set_constants(dev, nx, ny, nz, nz_global=None, **extra):
    """kw_set_constants for an nx x ny x nz grid with the scalar media above; `extra` sets further fields (sources).
    nz_global: the context is one Z-slab of nz planes out of nz_global, whose transforms span the global grid"""
    from kwave_amd import capi
    nzg = nz if nz_global is None else nz_global
    k = capi.Constants()
    k.nx, k.ny, k.nz, k.n_elements = nx, ny, nz, nx * ny * nz
    k.nx_complex, k.ny_complex, k.nz_complex = nx // 2 + 1, ny, nz
    k.n_elements_complex = (nx // 2 + 1) * ny * nz
    k.fft_divider = 1.0 / (nx * ny * nzg)
    k.fft_divider_x, k.fft_divider_y, k.fft_divider_z = 1.0 / nx, 1.0 / ny, 1.0 / nzg
    k.dt, k.dt_by_2, k.c2, k.rho0, k.dt_rho0 = DT, DT / 2, C2, RHO0, DT * RHO0
    k.dt_rho0_sgx, k.dt_rho0_sgy, k.dt_rho0_sgz = DT_RHO0_SG
    k.b_on_a, k.absorb_tau, k.absorb_eta = BONA, TAU, ETA
    for name, v in extra.items():
        setattr(k, name, v)
    dev.set_constants(k)
    return k


class Guarded:
    """A device array between GUARD-byte bands of 0xFF bytes; .ptr is the 256-byte aligned interior plus `offset`."""

    def __init__(self, dev, host, offset=0, dtype=np.float32):
        host = np.ascontiguousarray(host, dtype=dtype)
        self.dev, self.shape, self.dtype, self.n, self.offset = dev, host.shape, host.dtype, host.nbytes, offset
        self.total = GUARD + (offset + self.n + 255) // 256 * 256 + GUARD
        self.buf = dev.empty(self.total, np.uint8)
        self.buf.fill_bytes(0xFF)
        self.ptr = self.buf.ptr + GUARD + offset
        self.write(host)

    def write(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.nbytes == self.n
        from kwave_amd import capi
        capi.check(self.dev.L.kw_memcpy_h2d(self.dev.ctx, self.ptr, host.ctypes.data, self.n))

    def read(self):
        raw = self.buf.download()
        lo, hi = raw[:GUARD + self.offset], raw[GUARD + self.offset + self.n:]
        assert np.all(lo == 0xFF) and np.all(hi == 0xFF), "guard band overwritten"
        return raw[GUARD + self.offset:GUARD + self.offset + self.n].view(self.dtype).reshape(self.shape).copy()

    def free(self):
        self.buf.free()


def run(dev, entry, items):
    """kw_<entry>(ctx, *args): (name, host array, read-only[, byte offset]) tuples go through guarded buffers (None ->
    NULL), the rest as they are; returns {name: array after the call} of the written buffers"""
    bufs, conv = [], []
    for it in items:
        if isinstance(it, tuple):
            name, h, ro = it[:3]
            if h is None:
                conv.append(None)
                continue
            g = Guarded(dev, h, it[3] if len(it) > 3 else 0, h.dtype)
            bufs.append((name, g, h, ro))
            conv.append(g.ptr)
        else:
            conv.append(it)
    dev.call(entry, *conv)
    out = {}
    for name, g, h, ro in bufs:
        v = g.read()
        g.free()
        if ro:
            assert np.array_equal(v.view(np.uint8), h.view(np.uint8)), f"{entry}: read-only {name} changed"
        else:
            out[name] = v
    return out


def check_bound(family, label, got, ref, M, k):
    got = got.astype(np.float64)
    err = np.abs(got - ref)
    ok = err <= (k + 1) * U * M
    if not ok.all():
        i = np.argwhere(~ok)[0]
        raise AssertionError(f"{label}: {int((~ok).sum())} of {ok.size} elements outside (k+1) 2^-24 M, k = {k}; first at "
                             f"{tuple(i)}: got {got[tuple(i)]!r}, fp64 {ref[tuple(i)]!r}, M {M[tuple(i)]!r}")
    ratio = float(np.max(np.where(M > 0, err / np.where(M > 0, M, 1.0) / U, 0.0)))
    WORST[(family, k)] = max(WORST.get((family, k), 0.0), ratio)


def check_exact(label, got, want):
    bad = got.view(np.uint8) != np.ascontiguousarray(want).view(np.uint8)
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} bytes differ; first at {tuple(i)}")


def report_worst(prefixes):
    """print the worst ratios of the families that start with one of `prefixes`"""
    rows = [(fam, k, r) for (fam, k), r in sorted(WORST.items()) if fam.startswith(tuple(prefixes))]
    if rows:
        print("\nworst |gpu - fp64| / (2^-24 M) per kernel (bound k + 1):")
        for fam, k, r in rows:
            print(f"  {fam:34s} k = {k:2d}: {r:6.3f}  (bound {k + 1})")
