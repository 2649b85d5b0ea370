// kw_recon_device.h — what the k-space reconstructions share: the plane reconstruction (kw_plane_recon.hip:
// k_zfused_recon, k_plane_recon_mix) and the batched line reconstruction (kw_line_recon.hip: k_yfused_line_recon,
// k_line_recon_mix).  The per-bin arithmetic, the argument struct of the fused kernels, the gather of the rocFFT twins
// (recon_gather) and the crop kernel.  kwave_hip.h "k-space plane reconstruction" documents the
// definition and the order of the arithmetic; the two operators differ in rho2 and in the direction of their lines alone.
#ifndef KW_RECON_DEVICE_H
#define KW_RECON_DEVICE_H
#include "kw_elementwise.h"
#include "kw_fused.hip"

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

// the argument of the two fused passes (k_zfused_recon, k_yfused_line_recon): weight and gather along the line, formed per bin
struct ZReconArgs
{
  float2*  s;             // scratch array 0, in place (rows [t][ky][P], side array at side_off; line pass: [frame][t][P])
  PassGeo  geo;
  double   dkx, dky, dk2; // 2 pi / (Ex dx), 2 pi / (Ey dy), (2 pi / (Lt dt c0))^2; line pass: dkx of the sensor axis, no dky
  float    scale;         // 2 / (Ex Ey Lt); line pass: 2 / (Ey Lt)
  uint32_t ex, ny;        // Ex (the bin counts along x), rows of a plane
  uint32_t nearest;
};

// The gather of the rocFFT twins: G of bin m' of a line in memory whose bin i is line[i * stride]; M = Lt / 2
__device__ __forceinline__ float2 recon_gather(const float2* __restrict__ line, uint64_t stride, double rho2, uint32_t mp,
                                               uint32_t M, float scale, bool nearest)
{
  const double f = recon_f(rho2, mp);
  float2 res = make_float2(0.f, 0.f);
  if (f <= static_cast<double>(M))
  {
    const uint32_t i0 = static_cast<uint32_t>(f);
    const uint32_t i1 = i0 + 1u <= M ? i0 + 1u : M;
    const float    al = static_cast<float>(f - static_cast<double>(i0));
    const float2   t0 = recon_scale(line[static_cast<uint64_t>(i0) * stride], recon_w(rho2, i0, scale));
    const float2   t1 = recon_scale(line[static_cast<uint64_t>(i1) * stride], recon_w(rho2, i1, scale));
    res = recon_pick(t0, t1, al, nearest);
  }
  return res;
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
