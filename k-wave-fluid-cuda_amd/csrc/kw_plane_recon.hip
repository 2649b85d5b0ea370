// kw_plane_recon.hip — device code of the k-space plane reconstruction (DESIGN.md "k-space plane reconstruction"): the
// record p[t][y][x] of a planar sensor, embedded mirrored in time in a volume [Lt][Ey][Ex], to the initial pressure
//   p0 = 2 irfftn(G),   G[m] = interpolation of T = S w at f = sqrt(m'^2 + rho2) along the temporal axis of S = fftn(v)
// (kwave_hip.h documents the definition and the order of the arithmetic).  The re-gridding from w to kz moves data between
// the bins of one (kx, ky) line — the line the z-pass of the fused pipeline holds in LDS.
//
//   recon_w / recon_f    weight and gather position of one bin: shared by the fused kernel and the twin, and with the
//                        line reconstruction (kw_recon_device.h, with recon_scale, recon_pick, the twins' recon_gather
//                        and the crop kernel)
//   k_zfused_recon       the z-pass of kw_fused_plane_recon (kw_fused_main.hip): lines of scratch array 0 forward along t,
//                        T written back into the exchange buffer, the gather from LDS, inverse along t, in place — no
//                        operator array and no index table in memory
//   kw_plane_recon_mix   the same on the natural [Lt][Ey][Ex/2 + 1] spectrum of kw_fft_r2c_3d (rocFFT path, and the twin)
//   kw_plane_recon_embed / _crop   the mirrored embedding of the record; the first planes of the domain crop, clamped on request
#include "kw_recon_device.h"

namespace {

// (kx^2 + ky^2) / dk^2 of column ix (0 ... Ex/2) and row iy, float64
__device__ __forceinline__ double recon_rho2(double dkx, double dky, double dk2, uint32_t ex, uint32_t ey, uint32_t ix, uint32_t iy)
{
#pragma clang fp contract(off)
  return kw_kr2(dkx, dky, ex, ey, ix, iy) / dk2;
}

// =====================================================================================================================
// z-pass of the reconstruction: tile (ky = blockIdx.y, kx tile = blockIdx.x; the side array's blocks as in tile_coord) of
// scratch array 0, in place, on the line-tile steps (kw_fused.hip).  Its own: between the forward and the inverse
// transform, where row thread (c, j) holds the bins m = j + R1 k2 of column c:
//   1. it writes T[m] = w X[m] back into row j of the exchange buffer, at the cell of bin m
//      (lds[(m % R1) SF + (m / R1) NL + c]) — the cells it read last itself, so no barrier is needed before the write
//   2. a barrier
//   3. it gathers T[i0] and T[min(i0 + 1, M)] of its own column for each of its bins and forms G; only cells of bins
//      m' <= M are read (the cells of the upper half are written and never looked at: T[m'] is the lower half's)
//   4. a second barrier, before inverse_from_regs overwrites the buffer
// No LDS beyond Geo::LDSB, nothing read from memory but the lines.
// k_yfused_line_recon (kw_line_recon.hip) is this body with lines along y and rho2 of the column alone: a change to the
// weight, the gather or the barrier order here is a change there as well.
//   load | barrier (twiddles) | fwd_cols | barrier | fwd_rows -> 1. | barrier | 3. | barrier | inverse_from_regs -> store
// =====================================================================================================================
template<int L> __global__ __launch_bounds__((Geo<L, nl_z(L)>::THREADS)) void k_zfused_recon(ZReconArgs a)
{
  using G = Geo<L, nl_z(L)>;
  constexpr int R1 = G::R1, R2 = G::R2;
  constexpr uint32_t M = L / 2;
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  load_twiddles<L>(twl, a.geo.tw);
  const LineTile t      = line_tile<G>(a.geo.nxc, a.geo.P, a.geo.side_off, a.ny, 1u);
  if (t.tc.dead) return;
  const int      c      = t.c, j = t.j;

  float2 v[R1];
  if (ACTW(R2, j)) load_lines<G>(v, a.s, t);
  lds_barrier(); // twiddle table visible (the loads above stay in flight across it)

  if (ACTW(R2, j)) fwd_cols<L, kFwd, G::NL>(v, lds, c, j, twl);
  lds_barrier();
  float2 X[R2];
  // the true column: the side array holds bin Ex/2 = a.geo.nxc; pad lanes (never stored) take the last main column
  const double rho2 = recon_rho2(a.dkx, a.dky, a.dk2, a.ex, a.ny, t.tc.side ? a.geo.nxc : t.tc.col, t.pos);
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

struct ReconMix
{
  double   dkx, dky, dk2;
  float    scale;
  uint32_t ex, ey, lt;
  uint32_t nearest;
};

// the rocFFT twin: out[m] = G[m] of the line (ix, iy) of the natural [lt][ey][ex/2 + 1] half-spectrum, out of place
__global__ __launch_bounds__(256) void k_plane_recon_mix(float2* __restrict__ out, const float2* __restrict__ spec, ReconMix g)
{
  const uint32_t nxc = g.ex / 2 + 1;
  const uint64_t pl  = static_cast<uint64_t>(nxc) * g.ey;
  const uint64_t n   = pl * g.lt;
  const uint32_t M   = g.lt / 2;
  const bool nearest = g.nearest != 0;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t ix = static_cast<uint32_t>(e % nxc);
    const uint64_t r  = e / nxc;
    const uint32_t iy = static_cast<uint32_t>(r % g.ey), m = static_cast<uint32_t>(r / g.ey);
    const uint32_t mp = m <= M ? m : g.lt - m;
    const double rho2 = recon_rho2(g.dkx, g.dky, g.dk2, g.ex, g.ey, ix, iy);
    out[e] = recon_gather(spec + (e - static_cast<uint64_t>(m) * pl), pl, rho2, mp, M, g.scale, nearest);
  }
}

bool op_ok(const kw_plane_recon_op* op)
{
  return op->dx > 0.0 && op->dy > 0.0 && op->dt > 0.0 && op->c0 > 0.0 && (op->interp == 0 || op->interp == 1);
}

} // namespace

namespace kwfused {

// the z-pass of kw_fused_plane_recon: the lines of `s` in place
kw_status zfused_recon(kw_ctx* ctx, float2* s, const kw_plane_recon_op* op)
{
  const kw_constants& c = ctx->c;
  KW_PROF(ctx, "k_zfused_recon");
  const double dk = kTwoPi / (static_cast<double>(c.nz) * op->dt * op->c0);
  ZReconArgs a{};
  a.s   = s;
  a.geo = pass_geo(ctx, 2);
  a.dkx = kTwoPi / (static_cast<double>(c.nx) * op->dx);
  a.dky = kTwoPi / (static_cast<double>(c.ny) * op->dy);
  a.dk2 = dk * dk;
  a.scale    = static_cast<float>(2.0 / (static_cast<double>(c.nx) * c.ny * c.nz));
  a.ex       = c.nx;
  a.ny       = c.ny;
  a.nearest  = op->interp == 1 ? 1u : 0u;
  return KW_LAUNCH_ZPASS((k_zfused_recon<LEN>), c.nz, z_pass_grid(ctx, nl_z(c.nz)), a);
}

} // namespace kwfused

extern "C" {

kw_status kw_plane_recon_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_plane_recon_op* op, float scale)
{
  KW_MIX_ENTRY(ctx, "plane_recon_mix", c, n, out_spec, spec, op);
  KW_REQUIRE(op_ok(op));
  const double dk = kTwoPi / (static_cast<double>(c.nz) * op->dt * op->c0);
  ReconMix g{};
  g.dkx = kTwoPi / (static_cast<double>(c.nx) * op->dx);
  g.dky = kTwoPi / (static_cast<double>(c.ny) * op->dy);
  g.dk2 = dk * dk;
  g.scale = scale;
  g.ex = c.nx; g.ey = c.ny; g.lt = c.nz;
  g.nearest = op->interp == 1 ? 1u : 0u;
  hipLaunchKernelGGL(k_plane_recon_mix, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<float2*>(out_spec), reinterpret_cast<const float2*>(spec), g);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_plane_recon_embed(kw_ctx* ctx, float* vol, const float* src, uint32_t ex, uint32_t ey, uint32_t lt, uint32_t nx,
                               uint32_t ny, uint32_t nt)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "plane_recon_embed");
  const uint64_t n = static_cast<uint64_t>(ex) * ey * lt;
  if (n == 0) return KW_OK;
  KW_REQUIRE(nx <= ex && ny <= ey && (nt == 0 || 2ull * nt - 1ull <= lt));
  KW_REQUIRE(vol != nullptr);
  const uint64_t nd = static_cast<uint64_t>(nx) * ny * nt;
  KW_REQUIRE(nd == 0 || src != nullptr);
  const kw_record_dims d{ ex, ey, lt, nx, ny, nd == 0 ? 0u : nt };
  const bool v4 = ex % 4 == 0 && nx % 4 == 0 && aligned16(vol) && aligned16(src);
  if (v4) hipLaunchKernelGGL((k_record_embed<4, true>), dim3(capped_grid(ctx, n / 4)), dim3(256), 0, ctx->stream, vol, src, d);
  else hipLaunchKernelGGL((k_record_embed<1, true>), dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream, vol, src, d);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_plane_recon_crop(kw_ctx* ctx, float* out, const float* vol, uint32_t ex, uint32_t ey, uint32_t lt, uint32_t nx,
                              uint32_t ny, uint32_t planes, int32_t positivity)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "plane_recon_crop");
  const uint64_t n = static_cast<uint64_t>(nx) * ny * planes;
  if (n == 0) return KW_OK;
  KW_REQUIRE(nx <= ex && ny <= ey && planes <= lt);
  KW_REQUIRE(out != nullptr && vol != nullptr);
  const kw_record_dims d{ ex, ey, lt, nx, ny, planes };
  const bool v4 = ex % 4 == 0 && nx % 4 == 0 && aligned16(out) && aligned16(vol);
  if (v4) hipLaunchKernelGGL(k_recon_crop<4>, dim3(capped_grid(ctx, n / 4)), dim3(256), 0, ctx->stream, out, vol, d, positivity);
  else hipLaunchKernelGGL(k_recon_crop<1>, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream, out, vol, d, positivity);
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
