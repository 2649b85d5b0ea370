// kw_second_order_line.hip — the line-sensor record of the batched 2-D exact k-space propagator (DESIGN.md "Line-sensor
// record of the propagator on frames"): what the row y = r dy of every frame records at many output times, with no
// y-inverse and no x-inverse over the plane.  On the grid (nx, ny, nz) = (Ex, Ey, F) of kw_set_constants:
//   p_f(x, y_r; t) = irfft_x[ G_f(kx; t) ],   kx = 0 ... Ex/2
//   G_f(kx; t)     = sum over m = 0 ... Ey/2 of H(kx, m; t) Q_f(kx, m)                       H real, the same for every frame
//   Q_f(kx, m)     = q_f(kx, m) + q_f(kx, Ey - m)   (0 and, Ey even, Ey/2 pair with themselves: q_f(kx, m) alone)
//   q_f(kx, ky)    = rfft2(p0_f embedded)(kx, ky) exp(+2 pi i ky r / Ey) / (Ex Ey)           no dependence on time
// H depends on ky through min(ky, Ey - ky) only, hence the fold.
//
//   k_line_prepare   Q [Ex/2 + 1][Ey/2 + 1][F] <- the natural [F][Ey][Ex/2 + 1] spectra of kw_fft_r2c_frames: the row's phase,
//                    the divider, the fold, and the transposition that puts the frame in the fastest position (32 x 32 tiles
//                    through LDS: both sides of the copy are contiguous)
//   k_line_record    G [F][n_times][Ex/2 + 1] <- Q: a block owns one kx column, 256 times (a thread each) and a tile of FT
//                    frames; it walks the folded bins in chunks of 64 whose Q[m][f] slab sits in LDS next to the bins'
//                    time-independent factors (formed by the chunk's first threads, a prologue per chunk: no table in
//                    memory); per bin a thread forms H of its time once and feeds 2 FT accumulators from LDS broadcasts.
// The x-inverse is a batched 1-D C2R over the F n_times rows of G (kw_fft_c2r_frames on a context (Ex, 1, F n_times)).
// An accumulator takes its bins in ascending m by one fmaf each, whatever the frame tile, the other times of the call or
// their number: a record's bits do not depend on them.
#include "kw_elementwise.h"
#include "kw_second_order_op.h"

namespace {

constexpr int kLineTimes = 256; // threads of a record block: one output time each
constexpr int kLineChunk = 64;  // folded bins per LDS slab
constexpr int kLineTile  = 32;  // the transposition's tile

struct LineArgs
{
  const float2* q;      // [nxc][mf][frames]
  float2*       g;      // [frames][n_times][nxc]
  const double* times;  // [n_times], seconds
  double        c0;
  SecondH       h;      // (ct and divider are not read)
  uint32_t      nxc, mf, frames, n_times;
};

template<int FT> __global__ __launch_bounds__(kLineTimes) void k_line_record(LineArgs a)
{
  __shared__ float2  qs[kLineChunk * FT];
  __shared__ LineBin bins[kLineChunk];
  const uint32_t kx = blockIdx.x, f0 = blockIdx.z * FT;
  const uint32_t t  = blockIdx.y * kLineTimes + threadIdx.x;
  const bool     live = t < a.n_times;
  const double   ct = live ? a.c0 * a.times[t] : 0.0;
  const bool     absorbing = a.h.absorbing != 0;
  const double   kr2 = frame_kr2(a.h.dkx, a.h.ex, kx);

  float ar[FT], ai[FT];
#pragma unroll
  for (int f = 0; f < FT; f++) ar[f] = ai[f] = 0.f;

  for (uint32_t m0 = 0; m0 < a.mf; m0 += kLineChunk)
  {
    const uint32_t n = a.mf - m0 < kLineChunk ? a.mf - m0 : kLineChunk;
    __syncthreads(); // the chunk before has been read
    for (uint32_t i = threadIdx.x; i < n * FT; i += kLineTimes)
    {
      const uint32_t mm = i / FT, f = f0 + i % FT;
      const uint64_t e  = (static_cast<uint64_t>(kx) * a.mf + (m0 + mm)) * a.frames + f;
      qs[i] = f < a.frames ? a.q[e] : make_float2(0.f, 0.f);
    }
    if (threadIdx.x < n) bins[threadIdx.x] = line_bin(a.h, kr2, m0 + threadIdx.x);
    __syncthreads();
    for (uint32_t mm = 0; mm < n; mm++)
    {
      const LineBin& b = bins[mm];
      const float    h = line_h(b.kr, b.kg, b.q, b.zero, ct, absorbing);
#pragma unroll
      for (int f = 0; f < FT; f++)
      {
        const float2 v = qs[mm * FT + f];
        ar[f] = fmaf(h, v.x, ar[f]);
        ai[f] = fmaf(h, v.y, ai[f]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int f = 0; f < FT; f++)
    if (f0 + f < a.frames)
      a.g[(static_cast<uint64_t>(f0 + f) * a.n_times + t) * a.nxc + kx] = make_float2(ar[f], ai[f]);
}

struct PrepareArgs
{
  const float2* spec;  // [frames][ey][nxc]
  float2*       q;     // [nxc][mf][frames]
  uint32_t      nxc, ey, mf, frames, row;
  float         divider;
};

// block (32, 8); grid (kx tiles, frame tiles, mf): the bins (kx0 ... kx0 + 31, m) of the frames f0 ... f0 + 31
__global__ __launch_bounds__(kLineTile * 8) void k_line_prepare(PrepareArgs a)
{
  __shared__ float2 tile[kLineTile][kLineTile + 1];
  const uint32_t m = blockIdx.z, kx0 = blockIdx.x * kLineTile, f0 = blockIdx.y * kLineTile;
  const uint32_t m2 = a.ey - m;
  const bool     pair = m != 0 && m2 != m; // bins 0 and (Ey even) Ey/2 pair with themselves: taken once
  const float2   p1 = row_phase(m, a.row, a.ey);
  const float2   p2 = pair ? row_phase(m2, a.row, a.ey) : make_float2(0.f, 0.f);
  for (uint32_t j = threadIdx.y; j < kLineTile; j += 8)
  {
    const uint32_t f = f0 + j, kx = kx0 + threadIdx.x;
    if (f >= a.frames || kx >= a.nxc) continue;
    const uint64_t plane = static_cast<uint64_t>(f) * a.ey;
    float2 v = kw_times(kw_times(a.spec[(plane + m) * a.nxc + kx], p1), a.divider);
    if (pair)
    {
      const float2 w = kw_times(kw_times(a.spec[(plane + m2) * a.nxc + kx], p2), a.divider);
      v = make_float2(v.x + w.x, v.y + w.y);
    }
    tile[j][threadIdx.x] = v;
  }
  __syncthreads();
  for (uint32_t j = threadIdx.y; j < kLineTile; j += 8)
  {
    const uint32_t kx = kx0 + j, f = f0 + threadIdx.x;
    if (f >= a.frames || kx >= a.nxc) continue;
    a.q[(static_cast<uint64_t>(kx) * a.mf + m) * a.frames + f] = tile[threadIdx.x][j];
  }
}

template<int FT> void launch_record(kw_ctx* ctx, const LineArgs& a)
{
  const dim3 grid(a.nxc, (a.n_times + kLineTimes - 1) / kLineTimes, (a.frames + FT - 1) / FT);
  hipLaunchKernelGGL(k_line_record<FT>, grid, dim3(kLineTimes), 0, ctx->stream, a);
}

} // namespace

extern "C" {

kw_status kw_second_order_line_elems(kw_ctx* ctx, size_t* out_elems)
{
  KW_CHECK_CONSTS(ctx);
  KW_REQUIRE(out_elems != nullptr);
  const kw_constants& c = ctx->c;
  *out_elems = static_cast<size_t>(c.nx / 2 + 1) * (c.ny / 2 + 1) * c.nz;
  return KW_OK;
}

kw_status kw_second_order_line_prepare(kw_ctx* ctx, float* q, const float* spec, uint32_t row)
{
  KW_CHECK_CONSTS(ctx);
  KW_PROF(ctx, "second_order_line_prepare");
  const kw_constants& c = ctx->c;
  KW_REQUIRE(q && spec && q != spec);
  KW_REQUIRE(row < c.ny);
  KW_REQUIRE(c.ny / 2 + 1 <= 65535u && (c.nz + kLineTile - 1) / kLineTile <= 65535u); // block indices
  PrepareArgs a{};
  a.spec = reinterpret_cast<const float2*>(spec);
  a.q    = reinterpret_cast<float2*>(q);
  a.nxc = c.nx / 2 + 1; a.ey = c.ny; a.mf = c.ny / 2 + 1; a.frames = c.nz; a.row = row;
  a.divider = static_cast<float>(1.0 / (static_cast<double>(c.nx) * c.ny));
  const dim3 grid((a.nxc + kLineTile - 1) / kLineTile, (a.frames + kLineTile - 1) / kLineTile, a.mf);
  hipLaunchKernelGGL(k_line_prepare, grid, dim3(kLineTile, 8), 0, ctx->stream, a);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_second_order_line_record(kw_ctx* ctx, float* g, const float* q, const kw_second_order_op* op, const double* times,
                                      uint32_t n_times)
{
  KW_CHECK_CONSTS(ctx);
  KW_PROF(ctx, "second_order_line_record");
  const kw_constants& c = ctx->c;
  KW_REQUIRE(g && q && op && times && g != q);
  KW_REQUIRE(n_times >= 1 && (n_times + kLineTimes - 1) / kLineTimes <= 65535u);
  kw_second_order_op o = *op;
  o.t = 0.0; // not looked at: the times come from the array
  KW_REQUIRE(valid_op(&o, true));
  LineArgs a{};
  a.q = reinterpret_cast<const float2*>(q);
  a.g = reinterpret_cast<float2*>(g);
  a.times = times;
  a.c0 = o.c0;
  a.h  = time_constants(c, &o, 1.0f, true);
  a.nxc = c.nx / 2 + 1; a.mf = c.ny / 2 + 1; a.frames = c.nz; a.n_times = n_times;
  // the frame tile: the smallest that holds the batch, 64 frames at the most (then the tiles share a column's H)
  if (c.nz == 1) launch_record<1>(ctx, a);
  else if (c.nz <= 4) launch_record<4>(ctx, a);
  else if (c.nz <= 16) launch_record<16>(ctx, a);
  else launch_record<64>(ctx, a);
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
