// kw_second_order_plane.hip — the plane-sensor record of the 3-D exact k-space propagator (DESIGN.md "Plane-sensor record
// of the propagator"): what the plane z = r dz of the volume records at many output times, with no inverse along z and no
// 3-D round trip per time.  On the grid (nx, ny, nz) = (Ex, Ey, Ez) of kw_set_constants:
//   p(x, y, z_r; t) = irfft2_xy[ G(kx, ky; t) ],   kx = 0 ... Ex/2, ky = 0 ... Ey - 1
//   G(kx, ky; t)    = sum over m = 0 ... Ez/2 of H(kx, ky, m; t) Q(kx, ky, m)                 H real
//   Q(kx, ky, m)    = q(kx, ky, m) + q(kx, ky, Ez - m)   (0 and, Ez even, Ez/2 pair with themselves: q(kx, ky, m) alone)
//   q(kx, ky, kz)   = rfftn(p0 embedded)(kx, ky, kz) exp(+2 pi i kz r / Ez) / (Ex Ey Ez)      no dependence on time
// H depends on kz through min(kz, Ez - kz) only, hence the fold; and on ky through min(ky, Ey - ky) only, so the columns
// (kx, ky) and (kx, Ey - ky) share every H.
//
//   k_plane_prepare  Q [Ey][Ex/2 + 1][Ez/2 + 1] <- the natural [Ez][Ey][Ex/2 + 1] spectrum of kw_fft_r2c_3d: the plane's
//                    phase, the divider, the fold, and the transposition that puts the folded bin in the fastest position
//                    (32 x 32 tiles through LDS: both sides of the copy are contiguous)
//   k_plane_record   G [n_times][Ey][Ex/2 + 1] <- Q: a block owns KX consecutive kx columns, one ky pair (ky, Ey - ky) and
//                    256 times (a thread each); it walks the folded bins in chunks of 64 whose 2 KX Q columns sit in LDS
//                    next to the bins' time-independent factors (KX x 64, one per thread of the block: a prologue per
//                    chunk, no table in memory); per bin a thread forms KX values of H for its time and feeds each to the
//                    two columns of the pair from LDS broadcasts.
// The inverse over the record is a batched 2-D C2R over the n_times planes of G (kw_fft_c2r_frames on a context
// (Ex, Ey, n_times)).  An accumulator takes its bins in ascending m by one fmaf each, whatever the tile, the other times of
// the call or their number: a record's bits do not depend on them.
#include "kw_elementwise.h"
#include "kw_second_order_op.h"

namespace {

constexpr int kPlaneTimes = 256; // threads of a record block: one output time each
constexpr int kPlaneKx    = 4;   // kx columns of a record block; its chunks hold kPlaneTimes / kPlaneKx = 64 folded bins
constexpr int kPlaneTile  = 32;  // the transposition's tile

struct PlaneArgs
{
  const float2* q;      // [ey][nxc][mf]
  float2*       g;      // [n_times][ey][nxc]
  const double* times;  // [n_times], seconds
  double        c0;
  SecondH       h;      // (ct and divider are not read)
  uint32_t      nxc, ey, mf, n_times;
};

// grid (kx tiles, ky pairs 0 ... Ey/2, time tiles)
template<int KX> __global__ __launch_bounds__(kPlaneTimes) void k_plane_record(PlaneArgs a)
{
  constexpr int kPlaneChunk = kPlaneTimes / KX; // folded bins per LDS slab: one bin of the chunk's prologue per thread
  static_assert(KX * kPlaneChunk == kPlaneTimes, "KX divides the block");
  __shared__ float2  qs[2][KX][kPlaneChunk];
  __shared__ LineBin bins[KX][kPlaneChunk];
  const uint32_t kx0 = blockIdx.x * KX, ky = blockIdx.y, ky2 = a.ey - ky;
  const bool     pair = ky != 0 && ky2 != ky; // rows 0 and (Ey even) Ey/2 stand alone
  const uint32_t cols = a.nxc - kx0 < KX ? a.nxc - kx0 : KX; // live columns of the tile
  const uint32_t t  = blockIdx.z * kPlaneTimes + threadIdx.x;
  const bool     live = t < a.n_times;
  const double   ct = live ? a.c0 * a.times[t] : 0.0;
  const bool     absorbing = a.h.absorbing != 0;
  // the thread's bin of the prologue: column pc, bin pm of the chunk; kr2 as the z-pass hands it to second_h
  const uint32_t pc = threadIdx.x / kPlaneChunk, pm = threadIdx.x % kPlaneChunk;
  const double   kr2 = kw_kr2(a.h.dkx, a.h.dky, a.h.ex, a.h.ey, kx0 + pc, ky);

  float ar[2][KX], ai[2][KX];
#pragma unroll
  for (int c = 0; c < KX; c++) ar[0][c] = ai[0][c] = ar[1][c] = ai[1][c] = 0.f;

  for (uint32_t m0 = 0; m0 < a.mf; m0 += kPlaneChunk)
  {
    const uint32_t n = a.mf - m0 < kPlaneChunk ? a.mf - m0 : kPlaneChunk;
    __syncthreads(); // the chunk before has been read
#pragma unroll
    for (int s = 0; s < 2; s++) // the row ky, then its partner: KX columns of mf bins each, contiguous in Q
    {
      const uint64_t row = static_cast<uint64_t>(s == 0 ? ky : ky2) * a.nxc + kx0;
      const bool     in  = pc < cols && pm < n && (s == 0 || pair);
      qs[s][pc][pm] = in ? a.q[(row + pc) * a.mf + (m0 + pm)] : make_float2(0.f, 0.f);
    }
    if (pc < cols && pm < n) bins[pc][pm] = line_bin(a.h, kr2, m0 + pm);
    __syncthreads();
    if (!live) continue; // a wave past the last time has staged its share of the chunk and skips the sums
    for (uint32_t mm = 0; mm < n; mm++)
    {
#pragma unroll
      for (int c = 0; c < KX; c++)
      {
        if (c >= static_cast<int>(cols)) break;
        const LineBin& b = bins[c][mm];
        const float    h = line_h(b.kr, b.kg, b.q, b.zero, ct, absorbing);
        const float2   v = qs[0][c][mm], w = qs[1][c][mm];
        ar[0][c] = fmaf(h, v.x, ar[0][c]);
        ai[0][c] = fmaf(h, v.y, ai[0][c]);
        ar[1][c] = fmaf(h, w.x, ar[1][c]);
        ai[1][c] = fmaf(h, w.y, ai[1][c]);
      }
    }
  }
  if (!live) return;
  const uint64_t plane = static_cast<uint64_t>(t) * a.ey;
#pragma unroll
  for (int c = 0; c < KX; c++)
  {
    if (c >= static_cast<int>(cols)) break;
    a.g[(plane + ky) * a.nxc + kx0 + c] = make_float2(ar[0][c], ai[0][c]);
    if (pair) a.g[(plane + ky2) * a.nxc + kx0 + c] = make_float2(ar[1][c], ai[1][c]);
  }
}

struct PlanePrepareArgs
{
  const float2* spec;  // [ez][ey][nxc]
  float2*       q;     // [ey][nxc][mf]
  uint32_t      nxc, ey, ez, mf, plane;
  float         divider;
};

// block (32, 8); grid (kx tiles, bin tiles, ky): the bins (kx0 ... kx0 + 31, ky, m0 ... m0 + 31)
__global__ __launch_bounds__(kPlaneTile * 8) void k_plane_prepare(PlanePrepareArgs a)
{
  __shared__ float2 tile[kPlaneTile][kPlaneTile + 1];
  __shared__ float2 phase[2][kPlaneTile]; // of the tile's bins m and of their partners Ez - m
  const uint32_t ky = blockIdx.z, kx0 = blockIdx.x * kPlaneTile, m0 = blockIdx.y * kPlaneTile;
  if (threadIdx.y < 2 && m0 + threadIdx.x < a.mf)
    phase[threadIdx.y][threadIdx.x] = row_phase(threadIdx.y == 0 ? m0 + threadIdx.x : a.ez - (m0 + threadIdx.x), a.plane, a.ez);
  __syncthreads();
  for (uint32_t j = threadIdx.y; j < kPlaneTile; j += 8)
  {
    const uint32_t m = m0 + j, kx = kx0 + threadIdx.x;
    if (m >= a.mf || kx >= a.nxc) continue;
    const uint32_t m2 = a.ez - m;
    float2 v = kw_times(kw_times(a.spec[(static_cast<uint64_t>(m) * a.ey + ky) * a.nxc + kx], phase[0][j]), a.divider);
    if (m != 0 && m2 != m) // bins 0 and (Ez even) Ez/2 pair with themselves: taken once
    {
      const float2 w = kw_times(kw_times(a.spec[(static_cast<uint64_t>(m2) * a.ey + ky) * a.nxc + kx], phase[1][j]), a.divider);
      v = make_float2(v.x + w.x, v.y + w.y);
    }
    tile[j][threadIdx.x] = v;
  }
  __syncthreads();
  for (uint32_t j = threadIdx.y; j < kPlaneTile; j += 8)
  {
    const uint32_t kx = kx0 + j, m = m0 + threadIdx.x;
    if (m >= a.mf || kx >= a.nxc) continue;
    a.q[(static_cast<uint64_t>(ky) * a.nxc + kx) * a.mf + m] = tile[threadIdx.x][j];
  }
}

} // namespace

extern "C" {

kw_status kw_second_order_plane_elems(kw_ctx* ctx, size_t* out_elems)
{
  KW_CHECK_CONSTS(ctx);
  KW_REQUIRE(out_elems != nullptr);
  const kw_constants& c = ctx->c;
  *out_elems = static_cast<size_t>(c.ny) * (c.nx / 2 + 1) * (c.nz / 2 + 1);
  return KW_OK;
}

kw_status kw_second_order_plane_prepare(kw_ctx* ctx, float* q, const float* spec, uint32_t plane)
{
  KW_CHECK_CONSTS(ctx);
  KW_PROF(ctx, "second_order_plane_prepare");
  const kw_constants& c = ctx->c;
  KW_REQUIRE(q && spec && q != spec);
  KW_REQUIRE(plane < c.nz);
  PlanePrepareArgs a{};
  a.spec = reinterpret_cast<const float2*>(spec);
  a.q    = reinterpret_cast<float2*>(q);
  a.nxc = c.nx / 2 + 1; a.ey = c.ny; a.ez = c.nz; a.mf = c.nz / 2 + 1; a.plane = plane;
  a.divider = static_cast<float>(1.0 / (static_cast<double>(c.nx) * c.ny * c.nz));
  const dim3 grid((a.nxc + kPlaneTile - 1) / kPlaneTile, (a.mf + kPlaneTile - 1) / kPlaneTile, a.ey);
  KW_REQUIRE(grid.y <= 65535u && grid.z <= 65535u); // block indices
  hipLaunchKernelGGL(k_plane_prepare, grid, dim3(kPlaneTile, 8), 0, ctx->stream, a);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_second_order_plane_record(kw_ctx* ctx, float* g, const float* q, const kw_second_order_op* op, const double* times,
                                       uint32_t n_times)
{
  KW_CHECK_CONSTS(ctx);
  KW_PROF(ctx, "second_order_plane_record");
  const kw_constants& c = ctx->c;
  KW_REQUIRE(g && q && op && times && g != q);
  KW_REQUIRE(n_times >= 1 && (n_times + kPlaneTimes - 1) / kPlaneTimes <= 65535u && c.ny / 2 + 1 <= 65535u); // block indices
  kw_second_order_op o = *op;
  o.t = 0.0; // not looked at: the times come from the array
  KW_REQUIRE(valid_op(&o));
  PlaneArgs a{};
  a.q = reinterpret_cast<const float2*>(q);
  a.g = reinterpret_cast<float2*>(g);
  a.times = times;
  a.c0 = o.c0;
  a.h  = time_constants(c, &o, 1.0f);
  a.nxc = c.nx / 2 + 1; a.ey = c.ny; a.mf = c.nz / 2 + 1; a.n_times = n_times;
  const dim3 grid((a.nxc + kPlaneKx - 1) / kPlaneKx, a.ey / 2 + 1, (n_times + kPlaneTimes - 1) / kPlaneTimes);
  hipLaunchKernelGGL(k_plane_record<kPlaneKx>, grid, dim3(kPlaneTimes), 0, ctx->stream, a);
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
