// kw_recon_device.h — the per-bin arithmetic of the k-space reconstructions, shared by the plane reconstruction
// (kw_plane_recon.hip: k_zfused_recon, k_plane_recon_mix) and the batched line reconstruction (kw_line_recon.hip:
// k_yfused_line_recon, k_line_recon_mix), and the crop kernel of both.  kwave_hip.h "k-space plane reconstruction"
// documents the definition and the order of the arithmetic; the two operators differ in rho2 alone.
#ifndef KW_RECON_DEVICE_H
#define KW_RECON_DEVICE_H
#include "kw_elementwise.h"

#ifdef __HIPCC__
namespace {

// w(rho2, m') * scale: sqrt(m'^2 - rho2) / m' on the propagating side, 1 at the origin, 0 elsewhere.  float64 up to the
// square root, float32 from there; no contraction.  Real calls, not inlined, as time_h (kw_angular_time.hip): unrolled
// over the R2 bins of a thread the float64 square roots would be scheduled side by side and cost the z-pass its registers.
__device__ __attribute__((noinline)) float recon_w(double rho2, uint32_t mp, float scale)
{
#pragma clang fp contract(off)
  const double md = static_cast<double>(mp);
  const double d  = (md * md) - rho2;
  if (mp == 0) return rho2 == 0.0 ? scale : 0.f;
  if (d < 0.0) return 0.f;
  return (static_cast<float>(sqrt(d)) / static_cast<float>(mp)) * scale;
}

// the gather position f = sqrt(m'^2 + rho2) of bin m', float64
__device__ __attribute__((noinline)) double recon_f(double rho2, uint32_t mp)
{
#pragma clang fp contract(off)
  const double md = static_cast<double>(mp);
  return sqrt((md * md) + rho2);
}

__device__ __forceinline__ float2 recon_scale(const float2& x, float w)
{
#pragma clang fp contract(off)
  return make_float2(w * x.x, w * x.y);
}

// G from the two neighbours T0 = T[i0], T1 = T[min(i0 + 1, M)] and a = f - i0
__device__ __forceinline__ float2 recon_pick(const float2& t0, const float2& t1, float a, bool nearest)
{
#pragma clang fp contract(off)
  if (nearest) return a < 0.5f ? t0 : t1;
  return make_float2((a * (t1.x - t0.x)) + t0.x, (a * (t1.y - t0.y)) + t0.y);
}

__device__ __forceinline__ float recon_clamp(float x, bool positivity) { return (positivity && !(x > 0.f)) ? 0.f : x; }

// out [nt][ny][nx] <- the corner of vol [lt][ey][ex] (nt = the planes), clamped at 0 on request.  The line reconstruction
// reads it as out [frames][depth][Ny] <- vol [frames][Lt][Ey]: (ex, ey, lt) = (Ey, Lt, F), (nx, ny, nt) = (Ny, depth, F).
template<int V> __global__ __launch_bounds__(256) void k_recon_crop(float* __restrict__ out, const float* __restrict__ vol, kw_record_dims d,
                                                                    int positivity)
{
  const uint32_t nxv = d.nx / V;
  const uint64_t n   = static_cast<uint64_t>(nxv) * d.ny * d.nt;
  const bool     pos = positivity != 0;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t ix = static_cast<uint32_t>(e % nxv) * V;
    const uint64_t r  = e / nxv;
    const uint32_t iy = static_cast<uint32_t>(r % d.ny), t = static_cast<uint32_t>(r / d.ny);
    const uint64_t s  = (static_cast<uint64_t>(t) * d.ey + iy) * d.ex + ix;
    if constexpr (V == 4)
    {
      float4 q = *reinterpret_cast<const float4*>(vol + s);
      q.x = recon_clamp(q.x, pos); q.y = recon_clamp(q.y, pos); q.z = recon_clamp(q.z, pos); q.w = recon_clamp(q.w, pos);
      *reinterpret_cast<float4*>(out + e * 4) = q;
    }
    else out[e] = recon_clamp(vol[s], pos);
  }
}

} // namespace
#endif // __HIPCC__
#endif
