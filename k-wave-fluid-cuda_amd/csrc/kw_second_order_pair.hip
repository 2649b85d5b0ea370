// kw_second_order_pair.hip — the exact k-space propagator with both initial conditions (DESIGN.md "Exact k-space
// propagator", "dp0/dt"): p(0) = p0 and dp/dt(0) = dp0dt, each embedded and transformed once into a kept spectrum of its
// own (kw_fused_second_order_forward / kw_fused_second_order_frames_forward, or the rocFFT transforms), and per output time
//   p^(t) = Hc(|k|; t) P0 + Hs(|k|; t) V0
// with Hc the H of kw_second_order.hip and Hs its companion (lossless sin(c0 |k| t) / (c0 |k|)).  Both operators depend on
// every bin index, so the two spectra cannot be folded before the transform along the line: one pass carries both forward,
// mixes them in registers and runs ONE inverse.  A code object of its own: kw_second_order.hip's kernels are what they
// were, and a propagator without dp0dt launches exactly those.
//
//   second_h_pair                  (Hc, Hs) of one bin, one sincosf for both: shared by the fused passes and the twins
//   k_zfused_second_order_pair     the z-pass of kw_fused_second_order_time_pair: lines of both kept spectra forward along
//                                  z, Hc X + Hs Y in registers, one inverse along z into scratch array 0
//   k_yfused_second_order_pair     the same along y on a frames context (kw_fused_second_order_frames_time_pair)
//   kw_second_order_mix_pair       the same mix on the natural half-spectra of kw_fft_r2c_3d (rocFFT path, and the twin)
//   kw_second_order_frames_mix_pair   ... of kw_fft_r2c_frames
// Hs is real and depends on |k| only, as Hc: the mixed half-spectrum stays Hermitian.
#include "kw_elementwise.h"
#include "kw_fused.hip"
#include "kw_second_order_op.h" // SecondH (with c0 and t for Hs), time_constants, valid_op

namespace {

// (Hc, Hs)(|k|; t) * divider of bin m along z (kwave_hip.h "Exact k-space propagator", "dp0/dt"): second_h's float64
// expressions in its order up to the phase word, ONE sincosf of the word's angle for both operators, and for Hs the
// reciprocal of w = c0 k (lossless) or (c0 k) r (absorbing) formed in float64 and rounded once; no contraction.
// A real call with its constants in LDS, for second_h's reasons (kw_second_order.hip).
typedef const __attribute__((address_space(3))) SecondH* SecondHLds;
__device__ __attribute__((noinline)) float2 second_h_pair(SecondHLds g, double kr2, uint32_t m)
{
#pragma clang fp contract(off)
  const double kz = g->dkz * static_cast<double>(kw_folded(m, g->ez));
  const double k2 = kr2 + (kz * kz);
  const float  divider = g->divider;
  if (k2 == 0.0) return make_float2(divider, static_cast<float>(g->t) * divider);
  const double k  = sqrt(k2);
  const double ct = g->ct;
  const double ck = g->c0 * k;
  float sn, cs;
  if (g->absorbing == 0)
  {
    const uint32_t word = kw_phase_word((k * ct) / kTwoPi);
    const float    ang  = static_cast<float>(static_cast<int32_t>(word)) * 1.4629180792671596e-9f;
    sincosf(ang, &sn, &cs);
    return make_float2(cs * divider, (sn * static_cast<float>(1.0 / ck)) * divider);
  }
  const uint32_t pw   = g->power;
  const double   s    = pw == kPowStokes ? k : (pw == kPowHalf ? sqrt(k) : pow(k, g->ym1));
  const double   gg   = g->ac * s;
  const double   B    = (1.0 - (g->twoT * gg)) - (gg * gg);
  const double   r    = sqrt(B);
  const uint32_t word = kw_phase_word(((k * r) * ct) / kTwoPi);
  const float    ang  = static_cast<float>(static_cast<int32_t>(word)) * 1.4629180792671596e-9f;
  sincosf(ang, &sn, &cs);
  const float E = exp2f(-static_cast<float>(((k * gg) * ct) * kLog2e));
  const float q = static_cast<float>(gg / r);
  const double w = ck * r;
  return make_float2((E * (cs + (q * sn))) * divider, ((E * sn) * static_cast<float>(1.0 / w)) * divider);
}

// X <- Hc X + Hs Y on the R2 bins m = j + R1 k2 of a row thread; no contraction
template<int R1, int R2>
__device__ __forceinline__ void mix_rows(float2 (&X)[R2], const float2 (&Y)[R2], SecondHLds gl, double kr2, int j)
{
#pragma clang fp contract(off)
#pragma unroll
  for (int k2 = 0; k2 < R2; k2++)
  {
    const float2 h = second_h_pair(gl, kr2, static_cast<uint32_t>(j + R1 * k2));
    const float2 x = X[k2], y = Y[k2];
    X[k2] = make_float2((h.x * x.x) + (h.y * y.x), (h.x * x.y) + (h.y * y.y));
  }
}

struct ZSecondPairArgs
{
  const float2* in_p;  // the kept (kx, ky, z) half-spectrum of p0, scratch layout (rows [z][ky][P], side array at side_off)
  const float2* in_v;  // that of dp0dt
  float2*       out;   // scratch array 0
  PassGeo       geo;
  SecondH       g;
};

// =====================================================================================================================
// The body of both pair passes on the line-tile steps (kw_fused.hip), k_zfused_second_order's with k_zfused_pair's
// schedule of two forwards in one block (kw_cw.hip):
//   load P | barrier (twiddles, gsh) | fwd_cols P, V's lines requested (in flight during P's transform) | barrier |
//   fwd_rows P -> X | barrier (every row read before V's columns overwrite the buffer) | fwd_cols V | barrier |
//   fwd_rows V -> Y, X <- Hc X + Hs Y | inverse_from_regs -> store
// The inverse's row writes follow the same threads' row reads, so no barrier stands between the second forward and the
// inverse (exchange-buffer discipline).  Nothing is read from memory for the operators, neither kept array is written.
// FRAMES: the tile and kr2 of k_yfused_second_order, otherwise those of k_zfused_second_order.
// =====================================================================================================================
template<int L, bool FRAMES> __device__ __forceinline__ void second_order_pair_body(const ZSecondPairArgs& a)
{
  using G = Geo<L, nl_z(L)>;
  constexpr int R1 = G::R1, R2 = G::R2;
  __shared__ float2  lds[G::LDSB];
  __shared__ float2  twl[G::TWN];
  __shared__ SecondH gsh;
  load_twiddles<L>(twl, a.geo.tw);
  const LineTile t = FRAMES ? line_tile<G>(a.geo.nxc, a.geo.P, a.geo.side_off, 1u, a.g.ey)
                            : line_tile<G>(a.geo.nxc, a.geo.P, a.geo.side_off, a.g.ey, 1u);
  if (t.tc.dead) return;
  const int      c = t.c, j = t.j;
  if (threadIdx.x == 0) gsh = a.g; // (published by the barrier that publishes the twiddle table)

  float2 v[R1];
  if (ACTW(R2, j)) load_lines<G>(v, a.in_p, t);
  lds_barrier(); // twiddle table visible (the loads above stay in flight across it)

  if (ACTW(R2, j))
  {
    fwd_cols<L, kFwd, G::NL>(v, lds, c, j, twl);
    load_lines<G>(v, a.in_v, t); // the second spectrum's lines: in flight during the first one's transform
  }
  lds_barrier();
  float2 X[R2], Y[R2];
  if (ACTW(R1, j)) fwd_rows<L, kFwd, G::NL>(X, lds, c, j);
  lds_barrier(); // every row has been read before the second forward transform overwrites the columns
  if (ACTW(R2, j)) fwd_cols<L, kFwd, G::NL>(v, lds, c, j, twl);
  lds_barrier();
  if (ACTW(R1, j))
  {
    fwd_rows<L, kFwd, G::NL>(Y, lds, c, j);
    const SecondHLds gl = (SecondHLds)&gsh;
    // the true column: the side array holds bin Ex/2 = a.geo.nxc; pad lanes (never stored) take the last main column
    const uint32_t col = t.tc.side ? a.geo.nxc : t.tc.col;
    const double kr2 = FRAMES ? frame_kr2(a.g.dkx, a.g.ex, col) : kw_kr2(a.g.dkx, a.g.dky, a.g.ex, a.g.ey, col, t.pos);
    mix_rows<R1, R2>(X, Y, gl, kr2, j);
  }

  float2 r[R1];
  inverse_from_regs<L, false, G::NL>(X, r, lds, c, j, twl);
  store_lines<G>(a.out, t, r);
}

// z-pass: tile (ky = blockIdx.y, kx tile = blockIdx.x; the side array's blocks as in tile_coord), as k_zfused_second_order
template<int L> __global__ __launch_bounds__((Geo<L, nl_z(L)>::THREADS)) void k_zfused_second_order_pair(ZSecondPairArgs a)
{
  second_order_pair_body<L, false>(a);
}

// the pass along y of a frames context: tile (frame = blockIdx.y, kx tile = blockIdx.x), the side array's blocks at NL
// frames each and those past the last frame returning, as k_yfused_second_order (its 2^29 limit as well)
template<int L> __global__ __launch_bounds__((Geo<L, nl_z(L)>::THREADS)) void k_yfused_second_order_pair(ZSecondPairArgs a)
{
  second_order_pair_body<L, true>(a);
}

// The body of the rocFFT twins: out[e] = Hc spec_p[e] + Hs spec_v[e] on the natural half-spectra [n2][g.ey][g.ex / 2 + 1],
// out of place, grid-stride (half_spectrum_mix with two inputs); FRAMES: every frame the same operators, the bin
// "along z" is 0 (k_second_order_frames_mix)
template<bool FRAMES>
__device__ __forceinline__ void half_spectrum_mix_pair(float2* __restrict__ out, const float2* __restrict__ spec_p,
                                                       const float2* __restrict__ spec_v, const SecondH& g, uint32_t n2)
{
#pragma clang fp contract(off)
  __shared__ SecondH gsh;
  if (threadIdx.x == 0) gsh = g;
  __syncthreads();
  const SecondHLds gl  = (SecondHLds)&gsh;
  const uint32_t   nxc = g.ex / 2 + 1;
  const uint64_t   n   = static_cast<uint64_t>(nxc) * g.ey * n2;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t ix = static_cast<uint32_t>(e % nxc);
    const uint64_t r  = e / nxc;
    const uint32_t iy = static_cast<uint32_t>(r % g.ey), m = static_cast<uint32_t>(r / g.ey);
    const float2 h = second_h_pair(gl, kw_kr2(g.dkx, g.dky, g.ex, g.ey, ix, iy), FRAMES ? 0u : m);
    const float2 x = spec_p[e], y = spec_v[e];
    out[e] = make_float2((h.x * x.x) + (h.y * y.x), (h.x * x.y) + (h.y * y.y));
  }
}

__global__ __launch_bounds__(256) void k_second_order_mix_pair(float2* __restrict__ out, const float2* __restrict__ spec_p,
                                                               const float2* __restrict__ spec_v, SecondH g)
{
  half_spectrum_mix_pair<false>(out, spec_p, spec_v, g, g.ez);
}

__global__ __launch_bounds__(256) void k_second_order_frames_mix_pair(float2* __restrict__ out, const float2* __restrict__ spec_p,
                                                                      const float2* __restrict__ spec_v, SecondH g, uint32_t frames)
{
  half_spectrum_mix_pair<true>(out, spec_p, spec_v, g, frames);
}

} // namespace

namespace kwfused {

// the z-pass of kw_fused_second_order_time_pair: lines of both kept spectra to `out`, Hc and Hs of the time `op`
kw_status zfused_second_order_pair(kw_ctx* ctx, const float2* in_p, const float2* in_v, float2* out, const kw_second_order_op* op)
{
  const kw_constants& c = ctx->c;
  KW_PROF(ctx, "k_zfused_second_order_pair");
  ZSecondPairArgs a{};
  a.in_p = in_p; a.in_v = in_v; a.out = out;
  a.geo = pass_geo(ctx, 2);
  a.g   = time_constants(c, op, static_cast<float>(1.0 / (static_cast<double>(c.nx) * c.ny * c.nz)));
  return KW_LAUNCH_ZPASS((k_zfused_second_order_pair<LEN>), c.nz, z_pass_grid(ctx, nl_z(c.nz)), a);
}

// the pass along y of kw_fused_second_order_frames_time_pair: yfused_second_order's launch with both kept spectra
kw_status yfused_second_order_pair(kw_ctx* ctx, const float2* in_p, const float2* in_v, float2* out, const kw_second_order_op* op)
{
  const auto& f = ctx->fused;
  const kw_constants& c = ctx->c;
  KW_PROF(ctx, "k_yfused_second_order_pair");
  ZSecondPairArgs a{};
  a.in_p = in_p; a.in_v = in_v; a.out = out;
  a.geo = pass_geo(ctx, 1);
  a.g   = time_constants(c, op, static_cast<float>(1.0 / (static_cast<double>(c.nx) * c.ny)), true);
  // the tiles of a row, one more tile index for the side array's blocks, by the frames
  const dim3 grid(z_tiles(f.P, c.ny) + (f.side_off != 0 ? 1u : 0u), c.nz, 1);
  return KW_LAUNCH_ZPASS((k_yfused_second_order_pair<LEN>), c.ny, grid, a);
}

} // namespace kwfused

extern "C" {

kw_status kw_second_order_mix_pair(kw_ctx* ctx, float* out_spec, const float* spec_p, const float* spec_v,
                                   const kw_second_order_op* op, float divider)
{
  KW_MIX_ENTRY(ctx, "second_order_mix_pair", c, n, out_spec, spec_p, op);
  KW_REQUIRE(spec_v && out_spec != spec_v);
  KW_REQUIRE(valid_op(op));
  const SecondH g = time_constants(c, op, divider);
  hipLaunchKernelGGL(k_second_order_mix_pair, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<float2*>(out_spec), reinterpret_cast<const float2*>(spec_p),
                     reinterpret_cast<const float2*>(spec_v), g);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_second_order_frames_mix_pair(kw_ctx* ctx, float* out_spec, const float* spec_p, const float* spec_v,
                                          const kw_second_order_op* op, float divider)
{
  KW_MIX_ENTRY(ctx, "second_order_frames_mix_pair", c, n, out_spec, spec_p, op);
  KW_REQUIRE(spec_v && out_spec != spec_v);
  KW_REQUIRE(valid_op(op, true));
  const SecondH g = time_constants(c, op, divider, true);
  hipLaunchKernelGGL(k_second_order_frames_mix_pair, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<float2*>(out_spec), reinterpret_cast<const float2*>(spec_p),
                     reinterpret_cast<const float2*>(spec_v), g, c.nz);
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
