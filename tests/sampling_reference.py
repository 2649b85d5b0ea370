"""The reduce operators of the sampling kernels restated in plain NumPy (a plain module, imported by name from tests/):
the reference of tests/test_gpu_raw_samplers.py, of the solver-level sampling pin in tests/test_gpu_solver.py and of
the oracle's special-value test in tests/test_oracle_kat.py.

The definition is the reference's (OutputStreamsCudaKernels.cu:83-126): buf = v, buf += v * v contracted into one FMA,
buf = max(buf, v), buf = min(buf, v), where max / min on floats are CUDA's fmaxf / fminf:
  * a NaN operand yields the other operand, two NaNs yield NaN;
  * zeros of unlike sign yield +0 for max and -0 for min;
  * otherwise the larger / smaller value.
Results are compared as bit patterns; where the reference result is NaN any NaN is accepted (the payload is not part of
the definition)."""
import numpy as np

F32, F64 = np.float32, np.float64
OP_NONE, OP_RMS, OP_MAX, OP_MIN = 0, 1, 2, 3
FLT_MAX = np.finfo(F32).max
FLT_MIN = F32(2.0 ** -126)
DEN_MIN = F32(2.0 ** -149)
DEN_MAX = np.array([0x007FFFFF], np.uint32).view(F32)[0]
# the values the host gives a fresh stream buffer (BaseOutputStream.cpp:271-367)
INIT = {OP_NONE: F32(0.0), OP_RMS: F32(0.0), OP_MAX: -FLT_MAX, OP_MIN: FLT_MAX}

_POS = np.array([0.0, DEN_MIN, DEN_MAX, FLT_MIN, 1.0, FLT_MAX, np.inf], F32)
SPECIAL = np.concatenate([_POS, -_POS, np.array([np.nan], F32)])
SPECIAL_NO_NAN = SPECIAL[:-1]  # for RMS inputs: every square is finite in exact arithmetic, or exactly inf


def special_field(rng, shape, values=SPECIAL):
    """every element drawn from `values`; each value appears when the field has room for all of them"""
    size = int(np.prod(shape))
    out = values[rng.integers(0, values.size, size)]
    if size >= values.size:
        out[rng.permutation(size)[:values.size]] = values
    return out.reshape(shape).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def max_ref(b, v):
    b, v = np.asarray(b, F32), np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        out = np.where(b > v, b, v)                                              # the larger value
        out = np.where((b == 0) & (v == 0), (bits(b) & bits(v)).view(F32), out)  # +0 unless both are -0
    out = np.where(np.isnan(v), b, out)                                          # NaN operand: the other one
    return np.where(np.isnan(b), v, out).astype(F32)                             # (two NaNs: NaN)


def min_ref(b, v):
    b, v = np.asarray(b, F32), np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        out = np.where(b < v, b, v)
        out = np.where((b == 0) & (v == 0), (bits(b) | bits(v)).view(F32), out)  # -0 unless both are +0
    out = np.where(np.isnan(v), b, out)
    return np.where(np.isnan(b), v, out).astype(F32)


def _finite64(x):
    """float32 -> float64 with +-inf replaced by +-2^128, the value the overflow threshold is measured against"""
    x64 = np.asarray(x).astype(F64)
    return np.where(np.isinf(x64), np.copysign(F64(2.0 ** 128), x64), x64)


def fma_sq_ref(b, v):
    """fl32(v * v + b), rounded once: v * v is exact in float64 (48 bits), an error-free TwoSum adds b (s + e is the
    exact sum), and s is rounded to float32 to nearest even — unless s lies exactly half-way between two float32
    neighbours (the overflow threshold included) and e is not zero: then the sign of e says on which side the exact sum
    lies.  Every other s rounds as the exact sum does, because the float32 mid-points are float64 numbers."""
    b, v = np.asarray(b, F32), np.asarray(v, F32)
    with np.errstate(all="ignore"):
        b64, p = b.astype(F64), v.astype(F64) * v.astype(F64)
        s = p + b64
        bb = s - p
        e = (p - (s - bb)) + (b64 - bb)
        r = s.astype(F32)
        d = s - _finite64(r)
        other = np.nextafter(r, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32))
        tie = np.isfinite(s) & (d != 0) & (d == (_finite64(other) - _finite64(r)) / 2)
        beyond = tie & (e != 0) & (np.sign(e) == np.sign(d))
        return np.where(beyond, other, r).astype(F32)


def reduce_ref(op, b, v):
    if op == OP_NONE:
        return np.array(v, F32)
    return {OP_RMS: fma_sq_ref, OP_MAX: max_ref, OP_MIN: min_ref}[op](b, v)


def post_rms_ref(buf, scale):
    """sqrtf(buf * scale): the product is rounded to float32, so it has at most 24 significant bits; the float64 square
    root of such an argument rounded to float32 is the correctly rounded float32 square root (double rounding cannot
    occur: a root of a 24-bit number that is not itself a 24-bit number lies further than 2^-53 relative from every
    float32 mid-point)."""
    with np.errstate(all="ignore"):
        prod = (np.asarray(buf, F32) * F32(scale)).astype(F32)
        return np.sqrt(prod.astype(F64)).astype(F32)


def check_bits(label, got, want):
    """bit for bit; where the reference is NaN, any NaN"""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} elements differ; first at {i}: got {got[i]!r} "
                             f"(0x{bits(got)[i]:08x}), want {want[i]!r} (0x{bits(want)[i]:08x})")
