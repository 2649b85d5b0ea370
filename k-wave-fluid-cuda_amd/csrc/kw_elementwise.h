// kw_elementwise.h — what the element-wise kernels of the operator files share (kw_cw.hip, kw_angular.hip,
// kw_angular_time.hip, kw_plane_recon.hip, kw_thermal.hip; kw_solver_kernels.hip takes aligned16): the launch shape —
// 256 threads, at most CU count x 8 blocks striding over the work — the alignment tests that select the 16-byte kernels,
// two constants, the preamble of the kw_*_mix entry points, and under hipcc the folded bin index, kx^2 + ky^2 of a bin, the
// body of the rocFFT twins that multiply by an H, the fixed-point phase word and the embedding kernel of the two operators
// that work on a record [t][y][x].
#ifndef KW_ELEMENTWISE_H
#define KW_ELEMENTWISE_H
#include <cstdint>

#include "kw_internal.h"

constexpr int kBlocksPerCu = 8; // grid cap: CU count x 8 blocks of 256 threads (the samplers' cap)

// CU count x 8 blocks at the most, shrunk to the work: `work` = threads wanted
inline unsigned capped_grid(const kw_ctx* ctx, uint64_t work)
{
  uint64_t       g   = (work + 255) / 256;
  const uint64_t cap = static_cast<uint64_t>(ctx->cu_count) * kBlocksPerCu;
  if (g > cap) g = cap;
  if (g == 0) g = 1;
  return static_cast<unsigned>(g);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kLog2e = 1.4426950408889634073599246810019;

// What every kw_*_mix entry point (the rocFFT twins of the operator passes) begins with: the context, the profile label,
// the bins of the half-spectrum [nz][ny][nx / 2 + 1] (a context without constants has no bins: nothing to do), and the
// pointers.  Declares the constants under the name `c` and the bin count under the name `n` that the caller gives.
#define KW_MIX_ENTRY(ctx, label, c, n, out_spec, spec, op)                                                             \
  KW_CHECK_CTX(ctx);                                                                                                   \
  KW_PROF(ctx, label);                                                                                                 \
  const kw_constants& c = (ctx)->c;                                                                                    \
  const uint64_t n = (ctx)->have_consts ? static_cast<uint64_t>(c.nx / 2 + 1) * c.ny * c.nz : 0;                       \
  if (n == 0) return KW_OK;                                                                                            \
  KW_REQUIRE(out_spec && spec && op && out_spec != spec)

#ifdef __HIPCC__
// bin i of an n-point transform folded onto 0 ... n/2: |k| in units of the bin spacing (the sign does not matter)
__device__ __forceinline__ uint32_t kw_folded(uint32_t i, uint32_t n) { return i <= n / 2 ? i : n - i; }

// kx^2 + ky^2 of column ix (0 ... Ex/2) and row iy, float64
__device__ __forceinline__ double kw_kr2(double dkx, double dky, uint32_t ex, uint32_t ey, uint32_t ix, uint32_t iy)
{
#pragma clang fp contract(off)
  const double kx = dkx * static_cast<double>(kw_folded(ix, ex));
  const double ky = dky * static_cast<double>(kw_folded(iy, ey));
  return (kx * kx) + (ky * ky);
}

// a bin times its H, real or complex; no contraction
__device__ __forceinline__ float2 kw_times(const float2& x, float h) { return make_float2(h * x.x, h * x.y); }
__device__ __forceinline__ float2 kw_times(const float2& x, float hr, float hi)
{
#pragma clang fp contract(off)
  return make_float2((hr * x.x) - (hi * x.y), (hr * x.y) + (hi * x.x));
}
__device__ __forceinline__ float2 kw_times(const float2& x, const float2& h) { return kw_times(x, h.x, h.y); }

// The body of the rocFFT twin of a multiply pass: out[e] = spec[e] h(gl, kr2, m) on the natural half-spectrum
// [n2][g.ey][g.ex / 2 + 1], out of place, grid-stride; bin e is column ix, row iy, bin m along the third axis.  The
// constants g (a struct with dkx, dky, ex, ey) are staged in LDS for the called H (see time_h); gl is that copy.
template<class G, class F>
__device__ __forceinline__ void half_spectrum_mix(float2* __restrict__ out, const float2* __restrict__ spec, const G& g,
                                                  uint32_t n2, F h)
{
  __shared__ G gsh;
  if (threadIdx.x == 0) gsh = g;
  __syncthreads();
  const auto     gl  = (const __attribute__((address_space(3))) G*)&gsh;
  const uint32_t nxc = g.ex / 2 + 1;
  const uint64_t n   = static_cast<uint64_t>(nxc) * g.ey * n2;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t ix = static_cast<uint32_t>(e % nxc);
    const uint64_t r  = e / nxc;
    const uint32_t iy = static_cast<uint32_t>(r % g.ey), m = static_cast<uint32_t>(r / g.ey);
    const auto hv = h(gl, kw_kr2(g.dkx, g.dky, g.ex, g.ey, ix, iy), m);
    out[e] = kw_times(spec[e], hv);
  }
}

// fixed-point turns: round(frac(turns) 2^32) as a wrapping 32-bit word (negative turns are covered by floor)
__device__ __forceinline__ uint32_t kw_phase_word(double turns)
{
  const double w = rint((turns - floor(turns)) * 4294967296.0);
  return static_cast<uint32_t>(static_cast<uint64_t>(w) & 0xFFFFFFFFull);
}

struct kw_record_dims { uint32_t ex, ey, lt, nx, ny, nt; };

namespace {
// vol [lt][ey][ex] <- src [nt][ny][nx] in the corner, zero elsewhere; Mirror: mirrored in time as well (rows t and lt - t
// take src[t]; lt >= 2 nt - 1: no row is claimed twice).  V = 4: 16-byte accesses (ex, nx multiples of 4)
template<int V, bool Mirror>
__global__ __launch_bounds__(256) void k_record_embed(float* __restrict__ vol, const float* __restrict__ src, kw_record_dims d)
{
  const uint32_t exv = d.ex / V;
  const uint64_t n   = static_cast<uint64_t>(exv) * d.ey * d.lt;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t ix = static_cast<uint32_t>(e % exv) * V;
    const uint64_t r  = e / exv;
    const uint32_t iy = static_cast<uint32_t>(r % d.ey), t = static_cast<uint32_t>(r / d.ey);
    const uint32_t ts = (!Mirror || t < d.nt) ? t : d.lt - t; // the source row: t itself, or its mirror image
    const bool inside = ix < d.nx && iy < d.ny && ts < d.nt;
    const uint64_t s  = (static_cast<uint64_t>(ts) * d.ny + iy) * d.nx + ix;
    if constexpr (V == 4)
    {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (inside) v = *reinterpret_cast<const float4*>(src + s);
      *reinterpret_cast<float4*>(vol + e * 4) = v;
    }
    else vol[e] = inside ? src[s] : 0.f;
  }
}
} // namespace
#endif // __HIPCC__
#endif
