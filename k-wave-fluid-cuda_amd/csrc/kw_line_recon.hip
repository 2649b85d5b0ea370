// kw_line_recon.hip — device code of the batched k-space line reconstruction (DESIGN.md "k-space line reconstruction"): F
// frames p[t][y] of a linear array, each embedded mirrored in time in a plane [Lt][Ey], to F images
//   p0 = 2 irfft2(G),   G[m] = interpolation of T = S w at f = sqrt(m'^2 + rho2) along the temporal axis of S = fft2(v)
// — the plane reconstruction's definition with one lateral axis (kwave_hip.h documents both), rho2 = ky^2 / dk^2.  The
// volume is [F][Lt][Ey] on a frames context (kw_fused_set_frames): the sensor axis where the pipeline has x, t on y, the
// frame on z with no transform along it.  The per-bin arithmetic is the plane kernels' (kw_recon_device.h).
//
//   k_yfused_line_recon  the one pass between the x passes of kw_fused_line_recon (kw_fused_main.hip): lines of scratch
//                        array 0 along t (the pipeline's y), tile position = the frame; k_zfused_recon's body
//   kw_line_recon_mix    the same on the natural [F][Lt][Ey/2 + 1] spectra of kw_fft_r2c_frames (rocFFT path, and the twin)
//   kw_line_recon_embed / _crop   the mirrored embedding of the frames; the first rows of every image, clamped on request
#include "kw_recon_device.h"

namespace {

// ky^2 / dk^2 of column i (0 ... Ey/2), float64
__device__ __forceinline__ double line_rho2(double dks, double dk2, uint32_t ey, uint32_t i)
{
#pragma clang fp contract(off)
  const double k = dks * static_cast<double>(kw_folded(i, ey));
  return (k * k) / dk2;
}

// =====================================================================================================================
// The pass along t: tile (frame = blockIdx.y, column tile = blockIdx.x) of scratch array 0, in place, on the line-tile
// steps with lines along the pipeline's y: (lmul, bmul) = (1, ny).  The blocks of the x-Nyquist side array [F][Lt]
// (blockIdx.x = gridDim.x - 1) take the column Ey/2 at NL frames each, lane c <-> frame NL * blockIdx.y + c; those past the
// last frame return.  rho2 depends on the column alone.  Barrier order and buffer discipline are k_zfused_recon's
// (kw_plane_recon.hip): T goes back into the cells the thread read last itself, a barrier, the gather of T[i0], T[i1] of
// the thread's own column (bins m' <= M only), a barrier, the inverse.  No LDS beyond Geo::LDSB, nothing read from memory
// but the lines.  The body is k_zfused_recon's but for the line_tile strides and rho2: a change there is a change here.
// The lanes' 32-bit byte offsets hold the frame's offset, so the array ends below 2^29 elements (kw_fused_supported).
//   load | barrier (twiddles) | fwd_cols | barrier | fwd_rows -> T | barrier | gather | barrier | inverse_from_regs -> store
// =====================================================================================================================
template<int L> __global__ __launch_bounds__((Geo<L, nl_z(L)>::THREADS)) void k_yfused_line_recon(ZReconArgs a)
{
  using G = Geo<L, nl_z(L)>;
  constexpr int R1 = G::R1, R2 = G::R2;
  constexpr uint32_t M = L / 2;
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  load_twiddles<L>(twl, a.geo.tw);
  const LineTile t      = line_tile<G>(a.geo.nxc, a.geo.P, a.geo.side_off, 1u, a.ny);
  if (t.tc.dead) return;
  const int      c      = t.c, j = t.j;

  float2 v[R1];
  if (ACTW(R2, j)) load_lines<G>(v, a.s, t);
  lds_barrier(); // twiddle table visible (the loads above stay in flight across it)

  if (ACTW(R2, j)) fwd_cols<L, kFwd, G::NL>(v, lds, c, j, twl);
  lds_barrier();
  float2 X[R2];
  // the true column: the side array holds bin Ey/2 = a.geo.nxc; pad lanes (never stored) take the last main column
  const double rho2 = line_rho2(a.dkx, a.dk2, a.ex, t.tc.side ? a.geo.nxc : t.tc.col);
  if (ACTW(R1, j))
  {
    fwd_rows<L, kFwd, G::NL>(X, lds, c, j);
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++)
    {
      const uint32_t m  = static_cast<uint32_t>(j + R1 * k2);
      const uint32_t mp = m <= M ? m : static_cast<uint32_t>(L) - m;
      lds[j * G::SF + k2 * G::NL + c] = recon_scale(X[k2], recon_w(rho2, mp, a.scale));
    }
  }
  lds_barrier(); // T of the whole line is in the buffer
  if (ACTW(R1, j))
  {
    const bool nearest = a.nearest != 0;
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++)
    {
      const uint32_t m  = static_cast<uint32_t>(j + R1 * k2);
      const uint32_t mp = m <= M ? m : static_cast<uint32_t>(L) - m;
      const double   f  = recon_f(rho2, mp);
      const bool     in = f <= static_cast<double>(M);
      // (f > M: the indices are clamped into the line and the value dropped)
      const uint32_t i0 = in ? static_cast<uint32_t>(f) : M;
      const uint32_t i1 = i0 + 1u <= M ? i0 + 1u : M;
      const float    al = static_cast<float>(f - static_cast<double>(i0));
      const float2   t0 = lds[(i0 % R1) * G::SF + (i0 / R1) * G::NL + c];
      const float2   t1 = lds[(i1 % R1) * G::SF + (i1 / R1) * G::NL + c];
      const float2   g  = recon_pick(t0, t1, al, nearest);
      X[k2] = in ? g : make_float2(0.f, 0.f);
    }
  }
  lds_barrier(); // every gather is done before the inverse overwrites the buffer

  float2 r[R1];
  inverse_from_regs<L, false, G::NL>(X, r, lds, c, j, twl);
  store_lines<G>(a.s, t, r);
}

struct LineMix
{
  double   dks, dk2;
  float    scale;
  uint32_t ey, lt, frames;
  uint32_t nearest;
};

// the rocFFT twin: out[m] = G[m] of the line (column iy, frame) of the natural [F][lt][ey/2 + 1] half-spectra, out of place
__global__ __launch_bounds__(256) void k_line_recon_mix(float2* __restrict__ out, const float2* __restrict__ spec, LineMix g)
{
  const uint32_t nyc = g.ey / 2 + 1;
  const uint64_t pl  = static_cast<uint64_t>(nyc) * g.lt;
  const uint64_t n   = pl * g.frames;
  const uint32_t M   = g.lt / 2;
  const bool nearest = g.nearest != 0;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t iy = static_cast<uint32_t>(e % nyc);
    const uint64_t r  = e / nyc;
    const uint32_t m  = static_cast<uint32_t>(r % g.lt);
    const uint32_t mp = m <= M ? m : g.lt - m;
    const double rho2 = line_rho2(g.dks, g.dk2, g.ey, iy);
    out[e] = recon_gather(spec + (e - static_cast<uint64_t>(m) * nyc), nyc, rho2, mp, M, g.scale, nearest); // from bin 0 of the line
  }
}

struct kw_frame_dims { uint32_t ey, lt, frames, ny, nt; };

// vol [frames][lt][ey] <- src [frames][nt][ny] in the corner of every plane, mirrored in time (rows t and lt - t take
// src[t]; lt >= 2 nt - 1: no row is claimed twice), zero elsewhere.  V = 4: 16-byte accesses (ey, ny multiples of 4)
template<int V> __global__ __launch_bounds__(256) void k_line_embed(float* __restrict__ vol, const float* __restrict__ src, kw_frame_dims d)
{
  const uint32_t eyv = d.ey / V;
  const uint64_t n   = static_cast<uint64_t>(eyv) * d.lt * d.frames;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t iy = static_cast<uint32_t>(e % eyv) * V;
    const uint64_t r  = e / eyv;
    const uint32_t t  = static_cast<uint32_t>(r % d.lt), fr = static_cast<uint32_t>(r / d.lt);
    const uint32_t ts = t < d.nt ? t : d.lt - t; // the source row: t itself, or its mirror image
    const bool inside = iy < d.ny && ts < d.nt;
    const uint64_t s  = (static_cast<uint64_t>(fr) * d.nt + ts) * d.ny + iy;
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

namespace kwfused {

// the pass along t of kw_fused_line_recon: the lines of `s` in place
kw_status yfused_line_recon(kw_ctx* ctx, float2* s, const kw_plane_recon_op* op)
{
  const auto& f = ctx->fused;
  const kw_constants& c = ctx->c;
  KW_PROF(ctx, "k_yfused_line_recon");
  const double dk = kTwoPi / (static_cast<double>(c.ny) * op->dt * op->c0);
  ZReconArgs a{};
  a.s   = s;
  a.geo = pass_geo(ctx, 1);
  a.dkx = kTwoPi / (static_cast<double>(c.nx) * op->dx);
  a.dk2 = dk * dk;
  a.scale    = static_cast<float>(2.0 / (static_cast<double>(c.nx) * c.ny));
  a.ex       = c.nx;
  a.ny       = c.ny;
  a.nearest  = op->interp == 1 ? 1u : 0u;
  // the tiles of a row, one more tile index for the side array's blocks, by the frames
  const dim3 grid(z_tiles(f.P, c.ny) + (f.side_off != 0 ? 1u : 0u), c.nz, 1);
  return KW_LAUNCH_ZPASS((k_yfused_line_recon<LEN>), c.ny, grid, a);
}

} // namespace kwfused

extern "C" {

kw_status kw_line_recon_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_plane_recon_op* op, float scale)
{
  KW_MIX_ENTRY(ctx, "line_recon_mix", c, n, out_spec, spec, op);
  KW_REQUIRE(op->dx > 0.0 && op->dt > 0.0 && op->c0 > 0.0 && (op->interp == 0 || op->interp == 1));
  const double dk = kTwoPi / (static_cast<double>(c.ny) * op->dt * op->c0);
  LineMix g{};
  g.dks = kTwoPi / (static_cast<double>(c.nx) * op->dx);
  g.dk2 = dk * dk;
  g.scale = scale;
  g.ey = c.nx; g.lt = c.ny; g.frames = c.nz;
  g.nearest = op->interp == 1 ? 1u : 0u;
  hipLaunchKernelGGL(k_line_recon_mix, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<float2*>(out_spec), reinterpret_cast<const float2*>(spec), g);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_line_recon_embed(kw_ctx* ctx, float* vol, const float* src, uint32_t ey, uint32_t lt, uint32_t frames, uint32_t ny,
                              uint32_t nt)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "line_recon_embed");
  const uint64_t n = static_cast<uint64_t>(ey) * lt * frames;
  if (n == 0) return KW_OK;
  KW_REQUIRE(ny <= ey && (nt == 0 || 2ull * nt - 1ull <= lt));
  KW_REQUIRE(vol != nullptr);
  const uint64_t nd = static_cast<uint64_t>(ny) * nt * frames;
  KW_REQUIRE(nd == 0 || src != nullptr);
  const kw_frame_dims d{ ey, lt, frames, nd == 0 ? 0u : ny, nd == 0 ? 0u : nt };
  const bool v4 = ey % 4 == 0 && ny % 4 == 0 && aligned16(vol) && aligned16(src);
  if (v4) hipLaunchKernelGGL(k_line_embed<4>, dim3(capped_grid(ctx, n / 4)), dim3(256), 0, ctx->stream, vol, src, d);
  else hipLaunchKernelGGL(k_line_embed<1>, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream, vol, src, d);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_line_recon_crop(kw_ctx* ctx, float* out, const float* vol, uint32_t ey, uint32_t lt, uint32_t frames, uint32_t ny,
                             uint32_t depth, int32_t positivity)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "line_recon_crop");
  const uint64_t n = static_cast<uint64_t>(ny) * depth * frames;
  if (n == 0) return KW_OK;
  KW_REQUIRE(ny <= ey && depth <= lt);
  KW_REQUIRE(out != nullptr && vol != nullptr);
  const kw_record_dims d{ ey, lt, frames, ny, depth, frames };
  const bool v4 = ey % 4 == 0 && ny % 4 == 0 && aligned16(out) && aligned16(vol);
  if (v4) hipLaunchKernelGGL(k_recon_crop<4>, dim3(capped_grid(ctx, n / 4)), dim3(256), 0, ctx->stream, out, vol, d, positivity);
  else hipLaunchKernelGGL(k_recon_crop<1>, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream, out, vol, d, positivity);
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
