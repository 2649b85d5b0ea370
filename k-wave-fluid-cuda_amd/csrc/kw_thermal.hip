// kw_thermal.hip — element-wise kernels of the Pennes bioheat solver (DESIGN.md "Bioheat"): the explicit temperature
// update with the CEM43 thermal dose and the running maximum in one pass, and the dose increment alone.
//
//   T     <- T + dt * ( diff_scale * a * (d0 [+ d1 + d2]) - P * (T - T_a) + heat_on * a * Q )
//   cem43 += (dt / 60) * R^(43 - T)  on the updated T:  R = 0.5 at T >= 43, 0.25 at 37 <= T < 43, nothing below 37
//   T_max <- max(T_max, T)
//
// The FFT stages that produce d0..d2 are the existing ones (kw_fused_scale_source / kw_fused_initial_velocity /
// kw_fused_velocity_gradient, or their rocFFT twins), driven with thermal operators by host/ThermalSolver.cpp.
//
// House style of kw_solver_kernels.hip: 256 threads, 16 B per lane over the body, the n % 4 tail element by element; the
// grid is capped at CU count x 8 blocks and strides over the rest.  Which of a / P / T_a are arrays, whether Q and T_max
// exist and how many divergence arrays there are is a compile-time mask: no pointer is tested per element.
// Both kernels are bandwidth-bound (up to 13 array passes of 4 B per point against ~15 flops): R^(43 - T) is one exp2f.
#include <utility>

#include "kw_elementwise.h"

namespace {

enum : int
{
  M_FLUX = 1,  // three divergence arrays (flux form); otherwise d0 alone (Laplacian form)
  M_A    = 2,  // a is an array
  M_P    = 4,  // P is an array
  M_TA   = 8,  // T_a is an array
  M_Q    = 16, // heat source present and on
  M_TMAX = 32, // running maximum kept
  M_ALL  = 64
};

struct ThermalArgs
{
  float*       T;
  float*       cem43;
  float*       tmax;
  const float* d0;
  const float* d1;
  const float* d2;
  const float* a;
  const float* P;
  const float* Ta;
  const float* Q;
  float        diff_scale, a_s, P_s, Ta_s, dt, dt60;
  uint64_t     n;
};

// (dt / 60) * R^(43 - T) as exp2f(s * (T - 43)), s = 1 (R = 0.5) or 2 (R = 0.25); 0 below 37
__device__ __forceinline__ float dose_increment(float T, float dt60)
{
  if (!(T >= 37.0f)) return 0.0f;
  const float x = T - 43.0f;
  return dt60 * exp2f(T >= 43.0f ? x : 2.0f * x);
}

// one point; the association order is fixed (tests/test_gpu_thermal.py derives its bound from it):
//   s = (d0 + d1) + d2;  r = (diff_scale * a) * s;  r = fma(-P, T - T_a, r);  r = fma(a, Q, r);  T = fma(dt, r, T)
template<int MASK>
__device__ __forceinline__ float update_point(float T, float d0, float d1, float d2, float a, float P, float Ta, float Q,
                                              float diff_scale, float dt)
{
  float s = d0;
  if (MASK & M_FLUX) s = (d0 + d1) + d2;
  float r = (diff_scale * a) * s;
  r       = __fmaf_rn(-P, T - Ta, r);
  if (MASK & M_Q) r = __fmaf_rn(a, Q, r);
  return __fmaf_rn(dt, r, T);
}

template<int V> struct TV;
template<> struct TV<4>
{
  using T = float4;
  static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void store(float* p, const T& v) { *reinterpret_cast<float4*>(p) = v; }
  static __device__ __forceinline__ T splat(float s) { return make_float4(s, s, s, s); }
};
template<> struct TV<1>
{
  using T = float;
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, const T& v) { *p = v; }
  static __device__ __forceinline__ T splat(float s) { return s; }
};
__device__ __forceinline__ float get(const float& v, int) { return v; }
__device__ __forceinline__ float get(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ void  put(float& v, int, float s) { v = s; }
__device__ __forceinline__ void  put(float4& v, int k, float s)
{
  if (k == 0) v.x = s; else if (k == 1) v.y = s; else if (k == 2) v.z = s; else v.w = s;
}

// V values at element offset i
template<int V, int MASK> __device__ __forceinline__ void update_group(const ThermalArgs& g, uint64_t i)
{
  using VT = typename TV<V>::T;
  VT       vT  = TV<V>::load(g.T + i);
  VT       vc  = TV<V>::load(g.cem43 + i);
  const VT vd0 = TV<V>::load(g.d0 + i);
  const VT vd1 = (MASK & M_FLUX) ? TV<V>::load(g.d1 + i) : TV<V>::splat(0.0f);
  const VT vd2 = (MASK & M_FLUX) ? TV<V>::load(g.d2 + i) : TV<V>::splat(0.0f);
  const VT va  = (MASK & M_A) ? TV<V>::load(g.a + i) : TV<V>::splat(g.a_s);
  const VT vP  = (MASK & M_P) ? TV<V>::load(g.P + i) : TV<V>::splat(g.P_s);
  const VT vTa = (MASK & M_TA) ? TV<V>::load(g.Ta + i) : TV<V>::splat(g.Ta_s);
  const VT vQ  = (MASK & M_Q) ? TV<V>::load(g.Q + i) : TV<V>::splat(0.0f);
  VT       vm  = (MASK & M_TMAX) ? TV<V>::load(g.tmax + i) : TV<V>::splat(0.0f);
#pragma unroll
  for (int k = 0; k < V; k++)
  {
    const float t = update_point<MASK>(get(vT, k), get(vd0, k), get(vd1, k), get(vd2, k), get(va, k), get(vP, k), get(vTa, k),
                                       get(vQ, k), g.diff_scale, g.dt);
    put(vT, k, t);
    put(vc, k, get(vc, k) + dose_increment(t, g.dt60));
    if (MASK & M_TMAX) put(vm, k, fmaxf(get(vm, k), t));
  }
  TV<V>::store(g.T + i, vT);
  TV<V>::store(g.cem43 + i, vc);
  if (MASK & M_TMAX) TV<V>::store(g.tmax + i, vm);
}

template<int V, int MASK> __global__ __launch_bounds__(256) void k_thermal_update(ThermalArgs g)
{
  const uint64_t tid    = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  const uint64_t groups = g.n / V;
  for (uint64_t q = tid; q < groups; q += stride) update_group<V, MASK>(g, q * V);
  if (V > 1)
  { // the n % V tail, element by element
    const uint64_t i = groups * V + tid;
    if (i < g.n) update_group<1, MASK>(g, i);
  }
}

template<int V> __global__ __launch_bounds__(256) void k_thermal_dose(float* __restrict__ cem43, const float* __restrict__ T,
                                                                       float dt60, uint64_t n)
{
  using VT = typename TV<V>::T;
  const uint64_t tid    = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  const uint64_t groups = n / V;
  for (uint64_t q = tid; q < groups; q += stride)
  {
    const VT vT = TV<V>::load(T + q * V);
    VT       vc = TV<V>::load(cem43 + q * V);
#pragma unroll
    for (int k = 0; k < V; k++) put(vc, k, get(vc, k) + dose_increment(get(vT, k), dt60));
    TV<V>::store(cem43 + q * V, vc);
  }
  if (V > 1)
  {
    const uint64_t i = groups * V + tid;
    if (i < n) cem43[i] += dose_increment(T[i], dt60);
  }
}

using UpdateKernel = void (*)(ThermalArgs);
template<int V, int... M> UpdateKernel update_kernel(int mask, std::integer_sequence<int, M...>)
{
  static const UpdateKernel table[] = { k_thermal_update<V, M>... };
  return table[mask];
}

} // namespace

extern "C" {

kw_status kw_thermal_update(kw_ctx* ctx, float* T, float* cem43, float* T_max, const float* d0, const float* d1,
                            const float* d2, float diff_scale, const float* a, float a_s, const float* P, float P_s,
                            const float* T_a, float T_a_s, const float* Q, float dt, int heat_on, uint64_t n)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "thermal_update");
  if (n == 0) return KW_OK;
  KW_REQUIRE(T && cem43 && d0);
  KW_REQUIRE((d1 == nullptr) == (d2 == nullptr));
  int mask = 0;
  if (d1 != nullptr) mask |= M_FLUX;
  if (a != nullptr) mask |= M_A;
  if (P != nullptr) mask |= M_P;
  if (T_a != nullptr) mask |= M_TA;
  if (Q != nullptr && heat_on != 0) mask |= M_Q;
  if (T_max != nullptr) mask |= M_TMAX;
  ThermalArgs g{ T, cem43, T_max, d0, d1, d2, a, P, T_a, (mask & M_Q) ? Q : nullptr, diff_scale, a_s, P_s, T_a_s, dt, dt / 60.0f, n };
  const bool v4 = aligned16(T) && aligned16(cem43) && aligned16(T_max) && aligned16(d0) && aligned16(d1) && aligned16(d2) &&
                  aligned16(a) && aligned16(P) && aligned16(T_a) && aligned16(g.Q);
  const uint64_t     work = v4 ? n / 4 : n; // (a grid has at least one block: the threads of the tail are always there)
  const UpdateKernel k    = v4 ? update_kernel<4>(mask, std::make_integer_sequence<int, M_ALL>())
                               : update_kernel<1>(mask, std::make_integer_sequence<int, M_ALL>());
  hipLaunchKernelGGL(k, dim3(capped_grid(ctx, work)), dim3(256), 0, ctx->stream, g);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_thermal_dose(kw_ctx* ctx, float* cem43, const float* T, float dt, uint64_t n)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "thermal_dose");
  if (n == 0) return KW_OK;
  KW_REQUIRE(cem43 && T);
  const float dt60 = dt / 60.0f;
  if (aligned16(cem43) && aligned16(T))
    hipLaunchKernelGGL((k_thermal_dose<4>), dim3(capped_grid(ctx, n / 4)), dim3(256), 0, ctx->stream, cem43, T,
                       dt60, n);
  else
    hipLaunchKernelGGL((k_thermal_dose<1>), dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream, cem43, T, dt60, n);
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
