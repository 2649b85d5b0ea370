// kw_cw.hip — device code of the CW field propagator (DESIGN.md "CW field propagator"): the steady-state pressure of a
// continuous-wave source in a homogeneous lossless medium, evaluated as the exact k-space solution of the driven wave
// equation at one late time T — one forward and one inverse 3-D FFT of a complex field with a complex multiply between.
//
//   kw_cw_operator     G(|k|) exp(-i w T) / (Ex Ey Ez) on the reduced grid, evaluated in float64, rounded once
//   k_zfused_pair      the z-pass of kw_fused_cw_pair (kw_fused_main.hip): both real-transform spectra forward along z,
//                      the 2x2 mix with (Gr, Gi) in registers, both inverses — this file's code object holds its kernels
//   kw_cw_mix          the same mix element-wise on two kw_fft_r2c_3d spectra (rocFFT path, and the fused stage's twin)
//   kw_cw_embed        zero-filled expanded pair with the source in its [0, N) corner
//   kw_cw_extract      the corner cropped back: Re P, Im P, |P|, arg P, q |P|^2
//
// The field is complex but the pipeline is R2C / C2R: with S = Sr + i Si and G = Gr + i Gi (G depends on |k| only, so
// F{Sr} and F{Si} are mixed bin by bin)
//   Pr^ = Gr Sr^ - Gi Si^        Pi^ = Gi Sr^ + Gr Si^
// are Hermitian half-spectra again, and two C2R transforms give Re P and Im P.
#include "kw_elementwise.h"
#include "kw_fused.hip"

namespace {

// =====================================================================================================================
// z-fused pair: tile (ky = blockIdx.y, kx tile = blockIdx.x) of the two spectra a.in[0] (Sr^) and a.in[1] (Si^), the
// operators a.op[0] = Gr and a.op[1] = Gi in the imported run layout (load_op_run).  The body spells the line-tile steps
// of kw_fused.hip out, as k_zfused does (see "line-tile steps" there for why and for the exchange-buffer discipline);
// its own are the second array and the 2x2 mix:
//   forward 0   write columns | barrier | read rows            (array 1's lines requested before the barrier: in flight
//   barrier                                                      during array 0's transform, as in Z_ABSORB)
//   forward 1   write columns | barrier | read rows   -> mix in registers
//   inverse 0   write rows (each thread the row it has just read: no barrier) | barrier | read columns -> store
//   barrier     (the next inverse writes rows while others may still read their columns: Z_PGRAD's second output)
//   inverse 1   write rows | barrier | read columns -> store
// No occupancy hint: two spectra and two operator runs are held at once, the budget of one wave per SIMD is there to be
// used by the 20- to 32-point lines (tools/kernel_resources.py; DESIGN.md has the table).
// =====================================================================================================================
template<int L> __global__ __launch_bounds__((Geo<L, nl_z(L)>::THREADS)) void k_zfused_pair(ZArgs a)
{
  using G = Geo<L, nl_z(L)>;
  constexpr int R1 = G::R1, R2 = G::R2;
  constexpr bool WA = G::WA;
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  load_twiddles<L>(twl, a.tw);
  const int       c     = threadIdx.x % G::NL;
  const int       j     = threadIdx.x / G::NL;
  const TileCoord tc    = tile_coord<G::NL>(a.nxc, a.P, a.side_off, gridDim.y, c);
  if (tc.dead) return;
  const uint32_t ky     = tc.pos;
  const bool     valid  = tc.valid;
  const uint32_t zstr   = a.ny * tc.pitch;
  const uint32_t base   = ky * tc.pitch + (tc.side ? 0u : tc.kx) + tc.off;
  const uint32_t basel  = ky * tc.pitch + tc.col + tc.off;
  constexpr int  OPV    = op_vec(R2);
  const uint32_t opbase = tc.side ? a.op_side_off + (((ky / NLMAX) * (R2 / OPV) * R1 + j) * NLMAX + ky % NLMAX) * OPV
                                  : (((ky * (a.Pop / NLMAX) + tc.col / NLMAX) * (R2 / OPV) * R1 + j) * NLMAX + tc.col % NLMAX) * OPV;
  const float2* __restrict__ in0 = a.in[0];
  const float2* __restrict__ in1 = a.in[1];

  float2 v[R1];
  if (ACTW(R2, j))
  {
    const uint32_t lb = (basel + static_cast<uint32_t>(j) * zstr) * static_cast<uint32_t>(sizeof(float2));
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++) v[n1] = ld_uni<WA>(in0, static_cast<uint64_t>(n1 * R2) * zstr, lb);
  }
  // the operator values of the bins this thread holds after the forward transforms (kz = j + R1*k2)
  float gr[R2], gi[R2];
  if (ACTW(R1, j))
  {
    load_op_run<R2, R1>(gr, a.op[0], opbase);
    load_op_run<R2, R1>(gi, a.op[1], opbase);
  }
  lds_barrier(); // twiddle table visible (the loads above stay in flight across it)

  if (ACTW(R2, j))
  {
    step_a<L, kFwd>(v, j, twl);
#pragma unroll
    for (int k1 = 0; k1 < R1; k1++) lds[k1 * G::SF + j * G::NL + c] = v[k1];
    // the second array's lines: in flight during the first array's transform
    uint32_t lb = basel + static_cast<uint32_t>(j) * zstr;
    asm volatile("" : "+v"(lb));
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++)
      v[n1] = ld_uni<WA>(in1, static_cast<uint64_t>(n1 * R2) * zstr, lb * static_cast<uint32_t>(sizeof(float2)));
  }
  lds_barrier();
  float2 X[R2], Y[R2];
  if (ACTW(R1, j))
  {
#pragma unroll
    for (int n2 = 0; n2 < R2; n2++) X[n2] = lds[j * G::SF + n2 * G::NL + c];
    Dft<R2, kFwd>::run(X);
  }
  lds_barrier(); // every row has been read before the second forward transform overwrites the columns
  if (ACTW(R2, j))
  {
    step_a<L, kFwd>(v, j, twl);
#pragma unroll
    for (int k1 = 0; k1 < R1; k1++) lds[k1 * G::SF + j * G::NL + c] = v[k1];
  }
  lds_barrier();
  if (ACTW(R1, j))
  {
#pragma unroll
    for (int n2 = 0; n2 < R2; n2++) Y[n2] = lds[j * G::SF + n2 * G::NL + c];
    Dft<R2, kFwd>::run(Y);
    //   Pr^ = Gr Sr^ - Gi Si^     Pi^ = Gi Sr^ + Gr Si^     (G carries exp(-i w T) and the 1/N of the transform pair)
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++)
    {
      const float2 x = X[k2], y = Y[k2];
      X[k2] = make_float2(gr[k2] * x.x - gi[k2] * y.x, gr[k2] * x.y - gi[k2] * y.y);
      Y[k2] = make_float2(gi[k2] * x.x + gr[k2] * y.x, gi[k2] * x.y + gr[k2] * y.y);
    }
  }

  float2 r[R1];
  inverse_from_regs<L, false, G::NL>(X, r, lds, c, j, twl);
  if (ACTW(R2, j) && valid)
  {
    float2* __restrict__ out = a.out[0];
    uint32_t ob = base + static_cast<uint32_t>(j) * zstr;
    asm volatile("" : "+v"(ob));
#pragma unroll
    for (int q2 = 0; q2 < R1; q2++) st_uni<WA>(out, static_cast<uint64_t>(R2 * q2) * zstr, ob * static_cast<uint32_t>(sizeof(float2)), r[q2]);
  }
  lds_barrier();
  inverse_from_regs<L, false, G::NL>(Y, r, lds, c, j, twl);
  if (ACTW(R2, j) && valid)
  {
    float2* __restrict__ out = a.out[1];
    uint32_t ob = base + static_cast<uint32_t>(j) * zstr;
    asm volatile("" : "+v"(ob));
#pragma unroll
    for (int q2 = 0; q2 < R1; q2++) st_uni<WA>(out, static_cast<uint64_t>(R2 * q2) * zstr, ob * static_cast<uint32_t>(sizeof(float2)), r[q2]);
  }
}

// The same on lines of 512 = 2 x 256 (k_zfused_split's steps; the operators are imported in ITS run layout whenever
// kw_tuning::split512 is on, so this is the form that goes with them).  Eight 256-point exchanges per tile — two forward
// halves per array, two inverse halves per output — each writing exactly the cells its thread read in the one before
// (column / row / column / row ...): the only barriers are the ones inside them.
template<int L> __global__ __launch_bounds__(Geo<L / 2>::THREADS) void k_zfused_pair_split(ZArgs a)
{
  constexpr int H = L / 2;
  using G = Geo<H>;
  constexpr int R1 = G::R1, R2 = G::R2;
  static_assert(R1 == R2 && G::TPL == R1 && H == R1 * R2, "split lines are built on the balanced 256-point transform");
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  __shared__ float2 tw2[H];
  load_twiddles_split<L>(twl, tw2, a.tw);
  const LineTile t      = line_tile<G>(a.nxc, a.P, a.side_off, a.ny, 1u);
  if (t.tc.dead) return;
  const int      c      = t.c, j = t.j;
  const uint32_t opbase = op_run_base<2 * R2, R1>(t, a.Pop, a.op_side_off); // run: bins 2*(j + R1*k2) + h at run index 2*k2 + h

  float2 Xa[R2], Xb[R2], Ya[R2], Yb[R2]; // after the forward transforms: bins 2*(j + R1*k2) and 2*(j + R1*k2) + 1
  {
    float2 va[R1], vb[R1], ua[R1], ub[R1];
    load_split_halves<L>(va, vb, a.in[0], t);
    load_split_halves<L>(ua, ub, a.in[1], t); // the second array's lines: in flight during the first array's transforms
    lds_barrier(); // twiddle tables visible
    split_butterfly<L>(va, vb, j, tw2);
    line_fft<H, kFwd>(va, Xa, lds, c, j, twl);
    line_fft<H, kFwd, true>(vb, Xb, lds, c, j, twl);
    split_butterfly<L>(ua, ub, j, tw2);
    line_fft<H, kFwd>(ua, Ya, lds, c, j, twl);       // after a read by columns: writes columns
    line_fft<H, kFwd, true>(ub, Yb, lds, c, j, twl); // after a read by rows: writes rows
  }
  {
    float gr[2 * R2], gi[2 * R2];
    load_op_run<2 * R2, R1>(gr, a.op[0], opbase);
    load_op_run<2 * R2, R1>(gi, a.op[1], opbase);
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++)
    {
      const float ra = gr[2 * k2], ia = gi[2 * k2], rb = gr[2 * k2 + 1], ib = gi[2 * k2 + 1];
      const float2 xa = Xa[k2], ya = Ya[k2], xb = Xb[k2], yb = Yb[k2];
      Xa[k2] = make_float2(ra * xa.x - ia * ya.x, ra * xa.y - ia * ya.y);
      Ya[k2] = make_float2(ia * xa.x + ra * ya.x, ia * xa.y + ra * ya.y);
      Xb[k2] = make_float2(rb * xb.x - ib * yb.x, rb * xb.y - ib * yb.y);
      Yb[k2] = make_float2(ib * xb.x + rb * yb.x, ib * xb.y + rb * yb.y);
    }
  }
#pragma unroll 1
  for (int o = 0; o < 2; o++)
  {
    float2 ra[R1], rb[R1];
    {
      float2 w[R2];
#pragma unroll
      for (int k2 = 0; k2 < R2; k2++) w[k2] = o ? Ya[k2] : Xa[k2];
      inverse_from_regs<H, true>(w, ra, lds, c, j, twl); // after a read by columns: write columns
#pragma unroll
      for (int k2 = 0; k2 < R2; k2++) w[k2] = o ? Yb[k2] : Xb[k2];
      inverse_from_regs<H>(w, rb, lds, c, j, twl);       // after a read by rows: write rows
    }
    store_split_halves<L>(a.out[o], t, ra, rb, tw2);
  }
}

// =====================================================================================================================
// element-wise kernels: 256 threads, at most CU count x 8 blocks striding over the work (kw_elementwise.h)
// =====================================================================================================================
// G(a) exp(-i w T) * divider for a = c0 |k| in the regular form (kwave_hip.h), all in float64:
//   G = i [ sin(a T)/a - T exp(i (a + w) T/2) sinc((a - w) T/2) ] / (a + w)
// sinc(0) = 1 and sin(a T)/a -> T at a = 0 are the functions' own values there, not treated bins: the form is regular at
// the resonance a = w and at a = 0.
__global__ __launch_bounds__(256) void k_cw_operator(float* __restrict__ g_re, float* __restrict__ g_im, uint32_t nxc,
                                                     uint32_t ny, uint32_t nz, double c0, double w, double T, double dkx,
                                                     double dky, double dkz, double divider)
{
  const uint64_t n = static_cast<uint64_t>(nxc) * ny * nz;
  double swT, cwT;
  sincos(w * T, &swT, &cwT);
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t ix = static_cast<uint32_t>(e % nxc);
    const uint64_t r  = e / nxc;
    const uint32_t iy = static_cast<uint32_t>(r % ny), iz = static_cast<uint32_t>(r / ny);
    const double kx = dkx * static_cast<double>(ix);
    const double ky = dky * static_cast<double>(kw_folded(iy, ny)); // |k| only: the sign of a bin does not matter
    const double kz = dkz * static_cast<double>(kw_folded(iz, nz));
    const double a  = c0 * sqrt(kx * kx + ky * ky + kz * kz);
    const double s1 = (a == 0.0) ? T : sin(a * T) / a;
    const double x  = 0.5 * (a - w) * T;
    const double sc = (x == 0.0) ? 1.0 : sin(x) / x;
    double st, ct;
    sincos(0.5 * (a + w) * T, &st, &ct);
    const double Gr = (T * sc * st) / (a + w);
    const double Gi = (s1 - T * sc * ct) / (a + w);
    g_re[e] = static_cast<float>((Gr * cwT + Gi * swT) * divider);
    g_im[e] = static_cast<float>((Gi * cwT - Gr * swT) * divider);
  }
}

// the 2x2 mix on two interleaved complex spectra, in place; association order (kwave_hip.h), no contraction into fma:
//   re' = (gr * re) - (gi * im),   im' = (gi * re) + (gr * im)     for the real and the imaginary component of a bin alike
__device__ __forceinline__ void mix_bin(float2& x, float2& y, float gr, float gi)
{
#pragma clang fp contract(off)
  const float2 p = make_float2((gr * x.x) - (gi * y.x), (gr * x.y) - (gi * y.y));
  const float2 q = make_float2((gi * x.x) + (gr * y.x), (gi * x.y) + (gr * y.y));
  x = p;
  y = q;
}

template<int V> __global__ __launch_bounds__(256) void k_cw_mix(float2* __restrict__ sre, float2* __restrict__ sim,
                                                               const float* __restrict__ gre, const float* __restrict__ gim,
                                                               uint64_t n)
{
  const uint64_t tid    = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  const uint64_t groups = n / V;
  for (uint64_t q = tid; q < groups; q += stride)
  {
    if constexpr (V == 2)
    { // two bins per lane: 16 bytes of each spectrum, 8 of each operator
      float4 x = *reinterpret_cast<const float4*>(sre + 2 * q), y = *reinterpret_cast<const float4*>(sim + 2 * q);
      const float2 r = *reinterpret_cast<const float2*>(gre + 2 * q), i = *reinterpret_cast<const float2*>(gim + 2 * q);
      float2 x0 = make_float2(x.x, x.y), y0 = make_float2(y.x, y.y), x1 = make_float2(x.z, x.w), y1 = make_float2(y.z, y.w);
      mix_bin(x0, y0, r.x, i.x);
      mix_bin(x1, y1, r.y, i.y);
      *reinterpret_cast<float4*>(sre + 2 * q) = make_float4(x0.x, x0.y, x1.x, x1.y);
      *reinterpret_cast<float4*>(sim + 2 * q) = make_float4(y0.x, y0.y, y1.x, y1.y);
    }
    else
    {
      float2 x = sre[q], y = sim[q];
      mix_bin(x, y, gre[q], gim[q]);
      sre[q] = x;
      sim[q] = y;
    }
  }
  if (V > 1)
  { // the n % V tail
    const uint64_t e = groups * V + tid;
    if (e < n)
    {
      float2 x = sre[e], y = sim[e];
      mix_bin(x, y, gre[e], gim[e]);
      sre[e] = x;
      sim[e] = y;
    }
  }
}

struct CwDims
{
  uint32_t ex, ey, ez; // expanded grid
  uint32_t nx, ny, nz; // domain: its [0, nx) x [0, ny) x [0, nz) corner
};

template<int V> struct CV;
template<> struct CV<4>
{
  using T = float4;
  static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void store(float* p, const T& v) { *reinterpret_cast<float4*>(p) = v; }
};
template<> struct CV<1>
{
  using T = float;
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, const T& v) { *p = v; }
};
__device__ __forceinline__ float get(const float& v, int) { return v; }
__device__ __forceinline__ float get(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ void  put(float& v, int, float s) { v = s; }
__device__ __forceinline__ void  put(float4& v, int k, float s)
{
  if (k == 0) v.x = s; else if (k == 1) v.y = s; else if (k == 2) v.z = s; else v.w = s;
}

// expanded pair <- 0 outside the corner, the source inside it.  PARTS: a = Sr, b = Si; otherwise a = A, b = phi and
// S = A (cos phi + i sin phi).  SCALED: times the complex source scale (sr + i si) in the order
//   re = (Sr * sr) - (Si * si),  im = (Sr * si) + (Si * sr)   (no contraction); without it the values are stored as they are.
// One group of V consecutive x of the EXPANDED grid per lane and iteration (V = 4 needs ex and nx multiples of 4).
template<int V, bool PARTS, bool SCALED>
__global__ __launch_bounds__(256) void k_cw_embed(float* __restrict__ ere, float* __restrict__ eim, const float* __restrict__ a,
                                                  const float* __restrict__ b, float sr, float si, CwDims d)
{
  using VT = typename CV<V>::T;
  const uint32_t gx     = d.ex / V;
  const uint64_t groups = static_cast<uint64_t>(gx) * d.ey * d.ez;
  for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < groups;
       q += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t x = static_cast<uint32_t>(q % gx) * V;
    const uint64_t r = q / gx;
    const uint32_t y = static_cast<uint32_t>(r % d.ey), z = static_cast<uint32_t>(r / d.ey);
    VT vr{}, vi{};
    if (x < d.nx && y < d.ny && z < d.nz)
    {
      const uint64_t s  = (static_cast<uint64_t>(z) * d.ny + y) * d.nx + x;
      const VT       va = CV<V>::load(a + s), vb = CV<V>::load(b + s);
#pragma unroll
      for (int k = 0; k < V; k++)
      {
#pragma clang fp contract(off)
        float re = get(va, k), im = get(vb, k);
        if (!PARTS)
        {
          float sn, cs;
          sincosf(im, &sn, &cs);
          im = re * sn;
          re = re * cs;
        }
        if (SCALED)
        {
          const float t = (re * sr) - (im * si);
          im            = (re * si) + (im * sr);
          re            = t;
        }
        put(vr, k, re);
        put(vi, k, im);
      }
    }
    const uint64_t e = (static_cast<uint64_t>(z) * d.ey + y) * d.ex + x;
    CV<V>::store(ere + e, vr);
    CV<V>::store(eim + e, vi);
  }
}

struct CwExtractArgs
{
  const float* ere;
  const float* eim;
  float*       re;
  float*       im;
  float*       amp;
  float*       phase;
  float*       Q;
  const float* q;   // per point, or NULL with q_s
  float        q_s;
  CwDims       d;
};

// the corner cropped back to the domain; every output optional.  |P| = sqrtf((re * re) + (im * im)), Q = q * ((re * re) +
// (im * im)) without contraction; the phase is atan2 evaluated in float64 and rounded once (a float32 atan2 of 1-2 ulp is
// up to 2^-21 rad off near +-pi).
template<int V> __global__ __launch_bounds__(256) void k_cw_extract(CwExtractArgs g)
{
  using VT = typename CV<V>::T;
  const CwDims&  d      = g.d;
  const uint32_t gx     = d.nx / V;
  const uint64_t groups = static_cast<uint64_t>(gx) * d.ny * d.nz;
  for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < groups;
       p += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t x = static_cast<uint32_t>(p % gx) * V;
    const uint64_t r = p / gx;
    const uint32_t y = static_cast<uint32_t>(r % d.ny), z = static_cast<uint32_t>(r / d.ny);
    const uint64_t e = (static_cast<uint64_t>(z) * d.ey + y) * d.ex + x;
    const uint64_t s = (static_cast<uint64_t>(z) * d.ny + y) * d.nx + x;
    const VT vr = CV<V>::load(g.ere + e), vi = CV<V>::load(g.eim + e);
    if (g.re != nullptr) CV<V>::store(g.re + s, vr);
    if (g.im != nullptr) CV<V>::store(g.im + s, vi);
    if (g.amp != nullptr || g.Q != nullptr)
    {
      VT vq{}, va{}, vQ{};
      if (g.Q != nullptr && g.q != nullptr) vq = CV<V>::load(g.q + s);
#pragma unroll
      for (int k = 0; k < V; k++)
      {
#pragma clang fp contract(off)
        const float re = get(vr, k), im = get(vi, k);
        const float m2 = (re * re) + (im * im);
        put(va, k, sqrtf(m2));
        put(vQ, k, (g.q != nullptr ? get(vq, k) : g.q_s) * m2);
      }
      if (g.amp != nullptr) CV<V>::store(g.amp + s, va);
      if (g.Q != nullptr) CV<V>::store(g.Q + s, vQ);
    }
    if (g.phase != nullptr)
    {
      VT vp{};
#pragma unroll
      for (int k = 0; k < V; k++)
        put(vp, k, static_cast<float>(atan2(static_cast<double>(get(vi, k)), static_cast<double>(get(vr, k)))));
      CV<V>::store(g.phase + s, vp);
    }
  }
}

} // namespace

namespace kwfused {

// the z-pass of kw_fused_cw_pair: a.in / a.out [0..1] and a.op[0..1] are set by the caller, the geometry here
kw_status zfused_pair(kw_ctx* ctx, ZArgs a)
{
  const auto& f = ctx->fused;
  KW_PROF(ctx, "k_zfused_pair");
  a.tw          = f.tw[2];
  a.divider     = 1.0f; // the operators carry the 1/N
  a.nxc         = f.nxm;
  a.side_off    = f.side_off;
  a.op_side_off = f.side_off;
  a.P           = f.P;
  a.Pop         = f.P;
  a.ny          = f.nyl;
  a.nz          = f.nz_global;
  a.narr        = 2;
  if (f.nz_global == 512 && f.split512)
  {
    LAUNCH((k_zfused_pair_split<512>), z_pass_grid(ctx, NLMAX), dim3(Geo<256>::THREADS), a);
    return KW_OK;
  }
  return KW_LAUNCH_ZPASS((k_zfused_pair<LEN>), f.nz_global, z_pass_grid(ctx, nl_z(f.nz_global)), a);
}

} // namespace kwfused

extern "C" {

kw_status kw_cw_operator(kw_ctx* ctx, float* g_re, float* g_im, double c0, double w, double T, double dkx, double dky,
                         double dkz)
{
  KW_CHECK_CONSTS(ctx);
  KW_PROF(ctx, "cw_operator");
  KW_REQUIRE(g_re && g_im);
  KW_REQUIRE(c0 > 0.0 && w > 0.0 && T > 0.0 && dkx > 0.0 && dky > 0.0 && dkz > 0.0);
  const kw_constants& c = ctx->c;
  const uint64_t n = static_cast<uint64_t>(c.nx_complex) * c.ny * c.nz;
  const double divider = 1.0 / (static_cast<double>(c.nx) * static_cast<double>(c.ny) * static_cast<double>(c.nz));
  hipLaunchKernelGGL(k_cw_operator, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream, g_re, g_im, c.nx_complex, c.ny,
                     c.nz, c0, w, T, dkx, dky, dkz, divider);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_cw_mix(kw_ctx* ctx, float* spec_re, float* spec_im, const float* g_re, const float* g_im, uint64_t n_bins)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "cw_mix");
  if (n_bins == 0) return KW_OK;
  KW_REQUIRE(spec_re && spec_im && g_re && g_im);
  float2* sre = reinterpret_cast<float2*>(spec_re);
  float2* sim = reinterpret_cast<float2*>(spec_im);
  if (aligned16(spec_re) && aligned16(spec_im) && aligned8(g_re) && aligned8(g_im))
    hipLaunchKernelGGL((k_cw_mix<2>), dim3(capped_grid(ctx, n_bins / 2)), dim3(256), 0, ctx->stream, sre, sim, g_re, g_im, n_bins);
  else
    hipLaunchKernelGGL((k_cw_mix<1>), dim3(capped_grid(ctx, n_bins)), dim3(256), 0, ctx->stream, sre, sim, g_re, g_im, n_bins);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_cw_embed(kw_ctx* ctx, float* ex_re, float* ex_im, const float* a, const float* b, int parts, float scale_re,
                      float scale_im, uint32_t ex, uint32_t ey, uint32_t ez, uint32_t nx, uint32_t ny, uint32_t nz)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "cw_embed");
  const uint64_t n = static_cast<uint64_t>(ex) * ey * ez;
  if (n == 0) return KW_OK;
  KW_REQUIRE(nx <= ex && ny <= ey && nz <= ez);
  KW_REQUIRE(ex_re && ex_im);
  const uint64_t nd = static_cast<uint64_t>(nx) * ny * nz;
  KW_REQUIRE(nd == 0 || (a && b));
  const CwDims d{ ex, ey, ez, nx, ny, nz };
  const bool scaled = !(scale_re == 1.0f && scale_im == 0.0f);
  const bool v4 = ex % 4 == 0 && nx % 4 == 0 && aligned16(ex_re) && aligned16(ex_im) && aligned16(a) && aligned16(b);
  const dim3 grid(capped_grid(ctx, v4 ? n / 4 : n));
#define EMBED(V, P, S) hipLaunchKernelGGL((k_cw_embed<V, P, S>), grid, dim3(256), 0, ctx->stream, ex_re, ex_im, a, b, scale_re, scale_im, d)
#define EMBED_V(V)                                                                                                     \
  do {                                                                                                                 \
    if (parts != 0) { if (scaled) EMBED(V, true, true); else EMBED(V, true, false); }                                  \
    else            { if (scaled) EMBED(V, false, true); else EMBED(V, false, false); }                                \
  } while (0)
  if (v4) EMBED_V(4); else EMBED_V(1);
#undef EMBED_V
#undef EMBED
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_cw_extract(kw_ctx* ctx, const float* ex_re, const float* ex_im, uint32_t ex, uint32_t ey, uint32_t ez, uint32_t nx,
                        uint32_t ny, uint32_t nz, float* out_re, float* out_im, float* out_amp, float* out_phase, float* out_q,
                        const float* q, float q_scalar)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "cw_extract");
  const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
  if (n == 0) return KW_OK;
  KW_REQUIRE(nx <= ex && ny <= ey && nz <= ez);
  KW_REQUIRE(ex_re && ex_im);
  CwExtractArgs g{ ex_re, ex_im, out_re, out_im, out_amp, out_phase, out_q, (out_q != nullptr) ? q : nullptr, q_scalar,
                   CwDims{ ex, ey, ez, nx, ny, nz } };
  const bool v4 = ex % 4 == 0 && nx % 4 == 0 && aligned16(ex_re) && aligned16(ex_im) && aligned16(out_re) && aligned16(out_im) &&
                  aligned16(out_amp) && aligned16(out_phase) && aligned16(out_q) && aligned16(g.q);
  if (v4) hipLaunchKernelGGL((k_cw_extract<4>), dim3(capped_grid(ctx, n / 4)), dim3(256), 0, ctx->stream, g);
  else hipLaunchKernelGGL((k_cw_extract<1>), dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream, g);
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
