// kw_second_order.hip — device code of the exact k-space propagator (DESIGN.md "Exact k-space propagator"): an initial
// pressure p0[z][y][x] in a homogeneous medium, lossless or power-law absorbing, carried to any time t by
//   p(., ., .; t) = irfftn( rfftn(p0 embedded in Ez x Ey x Ex) H(|k|; t) )
// The forward half runs once (kw_fused_second_order_forward keeps the (kx, ky, z) half-spectrum), and every output time costs
// one z-pass that forms H in registers, one y-inverse and one x-inverse.
//
//   second_h               H of one bin (kwave_hip.h documents the order): shared by the fused kernel and the twin
//   k_zfused_second_order  the z-pass of kw_fused_second_order_time (kw_fused_main.hip): lines of the kept spectrum forward
//                          along z, times H, inverse along z into scratch array 0 — k_zfused_time's shape with a real H of
//                          all three bin indices, no operator array and no table in memory
//   kw_second_order_mix    the same H on the natural [Ez][Ey][Ex/2 + 1] spectrum of kw_fft_r2c_3d (rocFFT path, and the twin)
// The batched 2-D form (DESIGN.md "Exact k-space propagator on frames"): F planes p0[f][y][x] on a frames context
// (kw_fused_set_frames) (nx, ny, nz) = (Ex, Ey, F), no transform along z, the bin along y where the 3-D operator has kz:
//   k_yfused_second_order        the one pass between the x passes of kw_fused_second_order_frames_time: lines of the kept
//                                (kx, y, frame) spectrum forward along y, times H, inverse along y into scratch array 0
//   kw_second_order_frames_mix   the same H on the natural [F][Ey][Ex/2 + 1] spectra of kw_fft_r2c_frames
// H is real and depends on |k| only, so the half-spectrum stays Hermitian.  Embedding, crop, sensor records and the
// aggregates over the output times use kw_angular_time_embed, kw_plane_recon_crop and the samplers.
#include "kw_elementwise.h"
#include "kw_fused.hip"
#include "kw_second_order_op.h" // SecondH, time_constants, valid_op: shared with kw_second_order_line.hip

namespace {

// H(|k|; t) * divider of bin m along z (kwave_hip.h "Exact k-space propagator"): float64 up to the phase word and the
// exponent of the decay, float32 from there; no contraction.
// A real call, not inlined, as time_h (kw_angular_time.hip): unrolled over the R2 bins of a thread the two float64 square
// roots, the float64 power and the sincosf would multiply the z-pass's registers; called, the kernel keeps the registers
// of k_zfused's multiply plus the callee's.  The constants are read from LDS (the caller's copy): a by-value or
// by-reference struct would go through scratch memory on every call.
typedef const __attribute__((address_space(3))) SecondH* SecondHLds;
__device__ __attribute__((noinline)) float second_h(SecondHLds g, double kr2, uint32_t m)
{
#pragma clang fp contract(off)
  const double kz = g->dkz * static_cast<double>(kw_folded(m, g->ez));
  const double k2 = kr2 + (kz * kz);
  const float  divider = g->divider;
  if (k2 == 0.0) return divider;
  const double k  = sqrt(k2);
  const double ct = g->ct;
  if (g->absorbing == 0)
  {
    const uint32_t word = kw_phase_word((k * ct) / kTwoPi);
    const float    ang  = static_cast<float>(static_cast<int32_t>(word)) * 1.4629180792671596e-9f;
    return cosf(ang) * divider;
  }
  const uint32_t pw   = g->power;
  const double   s    = pw == kPowStokes ? k : (pw == kPowHalf ? sqrt(k) : pow(k, g->ym1));
  const double   gg   = g->ac * s;
  const double   B    = (1.0 - (g->twoT * gg)) - (gg * gg);
  const double   r    = sqrt(B);
  const uint32_t word = kw_phase_word(((k * r) * ct) / kTwoPi);
  const float    ang  = static_cast<float>(static_cast<int32_t>(word)) * 1.4629180792671596e-9f;
  float sn, cs;
  sincosf(ang, &sn, &cs);
  const float E = exp2f(-static_cast<float>(((k * gg) * ct) * kLog2e));
  const float q = static_cast<float>(gg / r);
  return (E * (cs + (q * sn))) * divider;
}

// =====================================================================================================================
// z-pass of the propagator: tile (ky = blockIdx.y, kx tile = blockIdx.x; the side array's blocks as in tile_coord) of the
// kept spectrum, on the line-tile steps (kw_fused.hip), in k_zfused_time's order.  Its own:
//   - the lines are read from a.in (the kept spectrum) and written to a.out (scratch array 0): a.in survives for the next
//     output time
//   - after the forward transform row thread (c, j) holds the bins m = j + R1 k2 along z; it forms H(kx of its column, ky,
//     m) there and scales both parts.  Nothing is read from memory for it.  second_h is called, not inlined (see there);
//     its constants are staged in LDS once per block.
//   load | barrier (twiddles, gsh) | fwd_cols | barrier | fwd_rows -> H | inverse_from_regs -> store
// =====================================================================================================================
struct ZSecondArgs
{
  const float2* in;   // the kept (kx, ky, z) half-spectrum, scratch layout (rows [z][ky][P], side array at side_off)
  float2*       out;  // scratch array 0
  PassGeo       geo;
  SecondH       g;
};

template<int L> __global__ __launch_bounds__((Geo<L, nl_z(L)>::THREADS)) void k_zfused_second_order(ZSecondArgs a)
{
  using G = Geo<L, nl_z(L)>;
  constexpr int R1 = G::R1, R2 = G::R2;
  __shared__ float2  lds[G::LDSB];
  __shared__ float2  twl[G::TWN];
  __shared__ SecondH gsh;
  load_twiddles<L>(twl, a.geo.tw);
  const LineTile t = line_tile<G>(a.geo.nxc, a.geo.P, a.geo.side_off, a.g.ey, 1u);
  if (t.tc.dead) return;
  const int      c = t.c, j = t.j;
  if (threadIdx.x == 0) gsh = a.g; // (published by the barrier that publishes the twiddle table)

  float2 v[R1];
  if (ACTW(R2, j)) load_lines<G>(v, a.in, t);
  lds_barrier(); // twiddle table visible (the loads above stay in flight across it)

  if (ACTW(R2, j)) fwd_cols<L, kFwd, G::NL>(v, lds, c, j, twl);
  lds_barrier();
  float2 X[R2];
  if (ACTW(R1, j))
  {
    fwd_rows<L, kFwd, G::NL>(X, lds, c, j);
    const SecondHLds gl = (SecondHLds)&gsh;
    // the true column: the side array holds bin Ex/2 = a.geo.nxc; pad lanes (never stored) take the last main column
    const double kr2 = kw_kr2(a.g.dkx, a.g.dky, a.g.ex, a.g.ey, t.tc.side ? a.geo.nxc : t.tc.col, t.pos);
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++)
    {
      const float h = second_h(gl, kr2, static_cast<uint32_t>(j + R1 * k2));
      X[k2] = make_float2(h * X[k2].x, h * X[k2].y);
    }
  }

  float2 r[R1];
  inverse_from_regs<L, false, G::NL>(X, r, lds, c, j, twl);
  store_lines<G>(a.out, t, r);
}

// =====================================================================================================================
// The pass along y of the batched 2-D propagator: tile (frame = blockIdx.y, kx tile = blockIdx.x) of the kept spectrum of
// a frames context, on the line-tile steps with k_yfused_line_recon's geometry — lines along the pipeline's y,
// (lmul, bmul) = (1, ny); the blocks of the x-Nyquist side array [F][Ey] (blockIdx.x = gridDim.x - 1) take the column Ex/2
// at NL frames each, lane c <-> frame NL * blockIdx.y + c, and those past the last frame return — in
// k_zfused_second_order's order.  Its own:
//   - a.in (the kept spectrum) is read, a.out (scratch array 0) written: a.in survives for the next output time
//   - row thread (c, j) holds the bins m = j + R1 k2 along y; the bin along the line takes the place of the z bin in
//     second_h (a.g.dkz, a.g.ez = 2 pi / (Ey dy), Ey: frame_constants) and kr2 = (kx*kx) of the thread's true column.
//     Nothing is read from memory for H; second_h is called, its constants staged in LDS once per block.
// The lanes' 32-bit byte offsets hold the frame's offset, so the array ends below 2^29 elements (kw_fused_supported).
//   load | barrier (twiddles, gsh) | fwd_cols | barrier | fwd_rows -> H | inverse_from_regs -> store
// =====================================================================================================================
template<int L> __global__ __launch_bounds__((Geo<L, nl_z(L)>::THREADS)) void k_yfused_second_order(ZSecondArgs a)
{
  using G = Geo<L, nl_z(L)>;
  constexpr int R1 = G::R1, R2 = G::R2;
  __shared__ float2  lds[G::LDSB];
  __shared__ float2  twl[G::TWN];
  __shared__ SecondH gsh;
  load_twiddles<L>(twl, a.geo.tw);
  const LineTile t = line_tile<G>(a.geo.nxc, a.geo.P, a.geo.side_off, 1u, a.g.ey);
  if (t.tc.dead) return;
  const int      c = t.c, j = t.j;
  if (threadIdx.x == 0) gsh = a.g; // (published by the barrier that publishes the twiddle table)

  float2 v[R1];
  if (ACTW(R2, j)) load_lines<G>(v, a.in, t);
  lds_barrier(); // twiddle table visible (the loads above stay in flight across it)

  if (ACTW(R2, j)) fwd_cols<L, kFwd, G::NL>(v, lds, c, j, twl);
  lds_barrier();
  float2 X[R2];
  if (ACTW(R1, j))
  {
    fwd_rows<L, kFwd, G::NL>(X, lds, c, j);
    const SecondHLds gl = (SecondHLds)&gsh;
    // the true column: the side array holds bin Ex/2 = a.geo.nxc; pad lanes (never stored) take the last main column
    const double kr2 = frame_kr2(a.g.dkx, a.g.ex, t.tc.side ? a.geo.nxc : t.tc.col);
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++)
    {
      const float h = second_h(gl, kr2, static_cast<uint32_t>(j + R1 * k2));
      X[k2] = make_float2(h * X[k2].x, h * X[k2].y);
    }
  }

  float2 r[R1];
  inverse_from_regs<L, false, G::NL>(X, r, lds, c, j, twl);
  store_lines<G>(a.out, t, r);
}

// the rocFFT twin: out[e] = spec[e] H on the natural [ez][ey][ex/2 + 1] half-spectrum, out of place
__global__ __launch_bounds__(256) void k_second_order_mix(float2* __restrict__ out, const float2* __restrict__ spec, SecondH g)
{
  half_spectrum_mix(out, spec, g, g.ez, [](SecondHLds gl, double kr2, uint32_t m) { return second_h(gl, kr2, m); });
}

// the twin of the batched 2-D form: the natural [F][ey][ex/2 + 1] spectra, every frame the same H.  half_spectrum_mix forms
// kr2 = (kx*kx) + (ky*ky) of the bin; the bin "along z" is 0, so second_h adds 0 to it: k2 is the fused pass's
// (kx*kx) + (ky*ky) to the bit (ky from the same dky and Ey: frame_constants)
__global__ __launch_bounds__(256) void k_second_order_frames_mix(float2* __restrict__ out, const float2* __restrict__ spec, SecondH g,
                                                                 uint32_t frames)
{
  half_spectrum_mix(out, spec, g, frames, [](SecondHLds gl, double kr2, uint32_t) { return second_h(gl, kr2, 0u); });
}

} // namespace

namespace kwfused {

// the z-pass of kw_fused_second_order_time: lines of `in` (the kept spectrum) to `out`, H of the time `op`
kw_status zfused_second_order(kw_ctx* ctx, const float2* in, float2* out, const kw_second_order_op* op)
{
  const kw_constants& c = ctx->c;
  KW_PROF(ctx, "k_zfused_second_order");
  ZSecondArgs a{};
  a.in = in; a.out = out;
  a.geo = pass_geo(ctx, 2);
  a.g   = time_constants(c, op, static_cast<float>(1.0 / (static_cast<double>(c.nx) * c.ny * c.nz)));
  return KW_LAUNCH_ZPASS((k_zfused_second_order<LEN>), c.nz, z_pass_grid(ctx, nl_z(c.nz)), a);
}

// the pass along y of kw_fused_second_order_frames_time: lines of `in` (the kept spectrum of the frames) to `out`
kw_status yfused_second_order(kw_ctx* ctx, const float2* in, float2* out, const kw_second_order_op* op)
{
  const auto& f = ctx->fused;
  const kw_constants& c = ctx->c;
  KW_PROF(ctx, "k_yfused_second_order");
  ZSecondArgs a{};
  a.in = in; a.out = out;
  a.geo = pass_geo(ctx, 1);
  a.g   = time_constants(c, op, static_cast<float>(1.0 / (static_cast<double>(c.nx) * c.ny)), true);
  // the tiles of a row, one more tile index for the side array's blocks, by the frames
  const dim3 grid(z_tiles(f.P, c.ny) + (f.side_off != 0 ? 1u : 0u), c.nz, 1);
  return KW_LAUNCH_ZPASS((k_yfused_second_order<LEN>), c.ny, grid, a);
}

} // namespace kwfused

extern "C" {

kw_status kw_second_order_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_second_order_op* op, float divider)
{
  KW_MIX_ENTRY(ctx, "second_order_mix", c, n, out_spec, spec, op);
  KW_REQUIRE(valid_op(op));
  const SecondH g = time_constants(c, op, divider);
  hipLaunchKernelGGL(k_second_order_mix, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<float2*>(out_spec), reinterpret_cast<const float2*>(spec), g);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_second_order_frames_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_second_order_op* op, float divider)
{
  KW_MIX_ENTRY(ctx, "second_order_frames_mix", c, n, out_spec, spec, op);
  KW_REQUIRE(valid_op(op, true));
  const SecondH g = time_constants(c, op, divider, true);
  hipLaunchKernelGGL(k_second_order_frames_mix, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<float2*>(out_spec), reinterpret_cast<const float2*>(spec), g, c.nz);
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
