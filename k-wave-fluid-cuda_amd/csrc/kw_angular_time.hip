// kw_angular_time.hip — device code of the time-domain angular-spectrum projector (DESIGN.md "Time-domain angular-spectrum
// projector"): a real pressure record p0[t][y][x] on a plane is carried to a parallel plane at distance z by
//   p(., ., .; z) = irfftn( rfftn(p0 embedded in Lt x Ey x Ex) H(kx, ky, m; z) )
// The record is a 3-D real array with the time axis where the pipeline has z: the forward half runs once
// (kw_fused_angular_time_forward keeps the (kx, ky, t) half-spectrum), and every plane costs one z-pass that forms H in
// registers, one y-inverse and one x-inverse.
//
//   time_h               H of one bin (kwave_hip.h documents the order): shared by the fused kernel and the twin
//   k_zfused_time        the z-pass of kw_fused_angular_time_plane (kw_fused_main.hip): lines of the kept spectrum forward
//                        along t, times H, inverse along t into scratch array 0 — k_zfused's Z_SOURCE shape, out of place,
//                        with no operator array and no table in memory
//   kw_angular_time_mix  the same H on the natural [Lt][Ey][Ex/2 + 1] spectrum of kw_fft_r2c_3d (rocFFT path, and the twin)
//   kw_angular_time_embed / _reduce   the record into the corner of the zero-filled volume; max_t, min_t and the series
//                        of the domain crop
// One real array is enough: H(-w) = conj H(w) and H depends on kx^2 + ky^2 only, so the half-spectrum stays Hermitian.
#include "kw_elementwise.h"
#include "kw_fused.hip"

namespace {

// what H needs besides the bin: the constants of one plane, float64 on the host
struct TimeH
{
  const double* ak;           // Lt/2 + 1 values alpha(m') k(m') log2(e), or NULL
  double        dkx, dky, dk; // 2 pi / (Ex dx), 2 pi / (Ey dy), 2 pi / (Lt dt c0)
  double        z, cfac;      // plane distance; D^2/2 / (D^2/2 + z^2)
  float         zl2e, divider; // float(z log2(e)); 1 / (Ex Ey Lt), or the twin's
  uint32_t      ex, ey, lt;
  uint32_t      restriction, retarded;
};

// H(kr2, m) * divider (kwave_hip.h "time-domain angular-spectrum projector"): float64 up to the phase word and the
// restriction test, float32 from there; no contraction.
// A real call, not inlined: unrolled over the R2 bins of a thread the float64 square root and the sincosf cost the z-pass
// 222 registers at 256-point lines and spill from 400 on; called, the kernel keeps the registers of k_zfused's multiply
// plus the callee's.  The plane's constants are read from LDS (the caller's copy): a by-value or by-reference struct
// would go through scratch memory on every call.
typedef const __attribute__((address_space(3))) TimeH* TimeHLds;
__device__ __attribute__((noinline)) float2 time_h(TimeHLds g, double kr2, uint32_t m)
{
#pragma clang fp contract(off)
  const uint32_t lt   = g->lt;
  const double   z    = g->z;
  const double*  ak   = g->ak;
  const uint32_t mp   = m <= lt / 2 ? m : lt - m;
  const double   k    = g->dk * static_cast<double>(mp);
  const double   k2   = k * k;
  const double   q    = sqrt(fabs(k2 - kr2));
  const bool     prop = kr2 < k2, evan = kr2 > k2;
  const double   qp   = evan ? 0.0 : q;
  const double   t    = (qp - (g->retarded ? k : 0.0)) * z / kTwoPi;
  const uint32_t word = kw_phase_word(t);
  const float    ang  = static_cast<float>(static_cast<int32_t>(word)) * 1.4629180792671596e-9f;
  float sn, cs;
  sincosf(ang, &sn, &cs);
  const float  q32 = static_cast<float>(q);
  const double akm = (ak != nullptr) ? ak[mp] : 0.0;
  float b = 0.f;
  if (prop) { if (ak != nullptr) b = static_cast<float>(akm * z) / q32; }
  else if (evan) b = q32 * g->zl2e;
  float mag = exp2f(-b) * g->divider;
  if (mp == 0 || 2u * mp == lt) mag = 0.f;                    // the temporal mean and the Nyquist bin
  if (!prop && !evan && akm > 0.0) mag = 0.f;                 // the circle, absorbing
  if (g->restriction && kr2 > k2 * g->cfac) mag = 0.f;        // angular restriction
  const float hr = mag * cs;
  float       hi = -(mag * sn);
  if (m > lt / 2) hi = -hi;
  return make_float2(hr, hi);
}

// =====================================================================================================================
// z-pass of the projector: tile (ky = blockIdx.y, kx tile = blockIdx.x; the side array's blocks as in tile_coord) of the
// kept spectrum, on the line-tile steps (kw_fused.hip).  Its own:
//   - the lines are read from a.in (the kept spectrum) and written to a.out (scratch array 0): a.in survives for the next
//     plane
//   - after the forward transform row thread (c, j) holds the bins m = j + R1 k2; it forms H(kx of its column, ky, m)
//     there and multiplies.  Nothing but the Lt/2 + 1 values of a.g.ak is read for it.  time_h is called, not inlined (see
//     there); its constants and a.g.ak are staged in LDS once per block, and the staged copy points at the staged values.
//   load | barrier (twiddles, aks, gsh) | fwd_cols | barrier | fwd_rows -> H | inverse_from_regs -> store
// =====================================================================================================================
struct ZTimeArgs
{
  const float2* in;   // the kept (kx, ky, t) half-spectrum, scratch layout (rows [t][ky][P], side array at side_off)
  float2*       out;  // scratch array 0
  PassGeo       geo;
  TimeH         g;
};

template<int L> __global__ __launch_bounds__((Geo<L, nl_z(L)>::THREADS)) void k_zfused_time(ZTimeArgs a)
{
  using G = Geo<L, nl_z(L)>;
  constexpr int R1 = G::R1, R2 = G::R2;
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  __shared__ double aks[L / 2 + 1]; // a.g.ak, read once per block instead of once per bin
  __shared__ TimeH  gsh;
  load_twiddles<L>(twl, a.geo.tw);
  const LineTile t      = line_tile<G>(a.geo.nxc, a.geo.P, a.geo.side_off, a.g.ey, 1u);
  if (t.tc.dead) return;
  const int      c      = t.c, j = t.j;
  if (a.g.ak != nullptr)
    for (int e = threadIdx.x; e < L / 2 + 1; e += blockDim.x) aks[e] = a.g.ak[e];
  if (threadIdx.x == 0)
  {
    TimeH g = a.g;
    g.ak = (a.g.ak != nullptr) ? aks : nullptr;
    gsh = g;
  } // (both published by the barrier that publishes the twiddle table)

  float2 v[R1];
  if (ACTW(R2, j)) load_lines<G>(v, a.in, t);
  lds_barrier(); // twiddle table visible (the loads above stay in flight across it)

  if (ACTW(R2, j)) fwd_cols<L, kFwd, G::NL>(v, lds, c, j, twl);
  lds_barrier();
  float2 X[R2];
  if (ACTW(R1, j))
  {
    fwd_rows<L, kFwd, G::NL>(X, lds, c, j);
    const TimeHLds gl = (TimeHLds)&gsh;
    // the true column: the side array holds bin Ex/2 = a.geo.nxc; pad lanes (never stored) take the last main column
    const double kr2 = kw_kr2(a.g.dkx, a.g.dky, a.g.ex, a.g.ey, t.tc.side ? a.geo.nxc : t.tc.col, t.pos);
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++)
    {
      const float2 h = time_h(gl, kr2, static_cast<uint32_t>(j + R1 * k2));
      X[k2] = kw_times(X[k2], h.x, h.y);
    }
  }

  float2 r[R1];
  inverse_from_regs<L, false, G::NL>(X, r, lds, c, j, twl);
  store_lines<G>(a.out, t, r);
}

// the rocFFT twin: out[e] = spec[e] H on the natural [lt][ey][ex/2 + 1] half-spectrum, out of place
__global__ __launch_bounds__(256) void k_angular_time_mix(float2* __restrict__ out, const float2* __restrict__ spec, TimeH g)
{
  half_spectrum_mix(out, spec, g, g.lt, [](TimeHLds gl, double kr2, uint32_t m) { return time_h(gl, kr2, m); });
}

// max_t / min_t and the series of the domain crop.  A block takes a tile of TP * V consecutive points (y, x) of the
// domain and splits the record along t over its 256 / TP thread rows: a small plane with a long record still fills the
// machine.  The rows' partial extrema meet in LDS; max and min are exact and order-free, so the result is deterministic
// without atomics.  Tiles are walked grid-stride.
template<int V, int TP> __global__ __launch_bounds__(256) void k_time_reduce(const float* __restrict__ vol, float* __restrict__ p_max,
                                                                             float* __restrict__ p_min,
                                                                             float* __restrict__ series, kw_record_dims d)
{
  constexpr int TS = 256 / TP;
  __shared__ float smax[TS][TP * V];
  __shared__ float smin[TS][TP * V];
  const uint32_t px = threadIdx.x % TP, ts = threadIdx.x / TP;
  const uint64_t npts  = static_cast<uint64_t>(d.nx) * d.ny;
  const uint64_t tiles = (npts + TP * V - 1) / (TP * V);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
  {
    const uint64_t p  = (tile * TP + px) * V; // first point of this thread (V = 4: nx % 4 == 0, the four share a row)
    const bool     on = p < npts;
    float mx[V], mn[V];
#pragma unroll
    for (int i = 0; i < V; i++) { mx[i] = -INFINITY; mn[i] = INFINITY; }
    if (on)
    {
      const uint32_t iy = static_cast<uint32_t>(p / d.nx), ix = static_cast<uint32_t>(p % d.nx);
      for (uint32_t t = ts; t < d.nt; t += TS)
      {
        const uint64_t s = (static_cast<uint64_t>(t) * d.ey + iy) * d.ex + ix;
        float x[V];
        if constexpr (V == 4)
        {
          const float4 q = *reinterpret_cast<const float4*>(vol + s);
          x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
          if (series != nullptr) *reinterpret_cast<float4*>(series + static_cast<uint64_t>(t) * npts + p) = q;
        }
        else
        {
          x[0] = vol[s];
          if (series != nullptr) series[static_cast<uint64_t>(t) * npts + p] = x[0];
        }
#pragma unroll
        for (int i = 0; i < V; i++) { mx[i] = fmaxf(mx[i], x[i]); mn[i] = fminf(mn[i], x[i]); }
      }
    }
#pragma unroll
    for (int i = 0; i < V; i++) { smax[ts][px * V + i] = mx[i]; smin[ts][px * V + i] = mn[i]; }
    __syncthreads();
    if (ts == 0 && on)
    {
#pragma unroll
      for (int i = 0; i < V; i++)
      {
        float a = mx[i], b = mn[i];
        for (int r = 1; r < TS; r++) { a = fmaxf(a, smax[r][px * V + i]); b = fminf(b, smin[r][px * V + i]); }
        if (p_max != nullptr) p_max[p + i] = a;
        if (p_min != nullptr) p_min[p + i] = b;
      }
    }
    __syncthreads(); // the next tile's partial extrema overwrite the buffers
  }
}

// the constants of one plane on the grid (Ex, Ey, Lt) = (c.nx, c.ny, c.nz), float64 on the host
TimeH plane_constants(const kw_constants& c, const kw_angular_time_op* op, float divider)
{
  TimeH g{};
  g.ak  = op->ak;
  g.dkx = kTwoPi / (static_cast<double>(c.nx) * op->dx);
  g.dky = kTwoPi / (static_cast<double>(c.ny) * op->dy);
  g.dk  = kTwoPi / (static_cast<double>(c.nz) * op->dt * op->c0);
  g.z   = op->z;
  const double dmin = fmin(static_cast<double>(c.nx - 1) * op->dx, static_cast<double>(c.ny - 1) * op->dy);
  const double hd2  = 0.5 * (dmin * dmin);
  g.cfac = hd2 / (hd2 + (op->z * op->z));
  g.zl2e = static_cast<float>(op->z * kLog2e);
  g.divider = divider;
  g.ex = c.nx; g.ey = c.ny; g.lt = c.nz;
  g.restriction = op->restriction != 0 ? 1u : 0u;
  g.retarded    = op->retarded != 0 ? 1u : 0u;
  return g;
}

} // namespace

namespace kwfused {

// the z-pass of kw_fused_angular_time_plane: lines of `in` (the kept spectrum) to `out`, H of the plane `op`
kw_status zfused_time(kw_ctx* ctx, const float2* in, float2* out, const kw_angular_time_op* op)
{
  const kw_constants& c = ctx->c;
  KW_PROF(ctx, "k_zfused_time");
  ZTimeArgs a{};
  a.in = in; a.out = out;
  a.geo = pass_geo(ctx, 2);
  a.g   = plane_constants(c, op, static_cast<float>(1.0 / (static_cast<double>(c.nx) * c.ny * c.nz)));
  return KW_LAUNCH_ZPASS((k_zfused_time<LEN>), c.nz, z_pass_grid(ctx, nl_z(c.nz)), a);
}

} // namespace kwfused

extern "C" {

kw_status kw_angular_time_mix(kw_ctx* ctx, float* out_spec, const float* spec, const kw_angular_time_op* op, float divider)
{
  KW_MIX_ENTRY(ctx, "angular_time_mix", c, n, out_spec, spec, op);
  KW_REQUIRE(c.nx % 2 == 0 && c.nz % 2 == 0);
  KW_REQUIRE(op->dx > 0.0 && op->dy > 0.0 && op->dt > 0.0 && op->c0 > 0.0 && op->z >= 0.0);
  const TimeH g = plane_constants(c, op, divider);
  hipLaunchKernelGGL(k_angular_time_mix, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<float2*>(out_spec), reinterpret_cast<const float2*>(spec), g);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_angular_time_embed(kw_ctx* ctx, float* vol, const float* src, uint32_t ex, uint32_t ey, uint32_t lt, uint32_t nx,
                                uint32_t ny, uint32_t nt)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "angular_time_embed");
  const uint64_t n = static_cast<uint64_t>(ex) * ey * lt;
  if (n == 0) return KW_OK;
  KW_REQUIRE(nx <= ex && ny <= ey && nt <= lt);
  KW_REQUIRE(vol != nullptr);
  const uint64_t nd = static_cast<uint64_t>(nx) * ny * nt;
  KW_REQUIRE(nd == 0 || src != nullptr);
  const kw_record_dims d{ ex, ey, lt, nx, ny, nd == 0 ? 0u : nt };
  const bool v4 = ex % 4 == 0 && nx % 4 == 0 && aligned16(vol) && aligned16(src);
  if (v4) hipLaunchKernelGGL((k_record_embed<4, false>), dim3(capped_grid(ctx, n / 4)), dim3(256), 0, ctx->stream, vol, src, d);
  else hipLaunchKernelGGL((k_record_embed<1, false>), dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream, vol, src, d);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_angular_time_reduce(kw_ctx* ctx, const float* vol, uint32_t ex, uint32_t ey, uint32_t lt, uint32_t nx, uint32_t ny,
                                 uint32_t nt, float* p_max, float* p_min, float* series)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "angular_time_reduce");
  const uint64_t npts = static_cast<uint64_t>(nx) * ny;
  if (npts * nt == 0) return KW_OK;
  if (p_max == nullptr && p_min == nullptr && series == nullptr) return KW_OK;
  KW_REQUIRE(nx <= ex && ny <= ey && nt <= lt);
  KW_REQUIRE(vol != nullptr);
  const kw_record_dims d{ ex, ey, lt, nx, ny, nt };
  const bool v4 = ex % 4 == 0 && nx % 4 == 0 && aligned16(vol) && aligned16(p_max) && aligned16(p_min) && aligned16(series);
  if (v4)
  {
    const uint64_t tiles = (npts + 15) / 16;
    hipLaunchKernelGGL((k_time_reduce<4, 4>), dim3(capped_grid(ctx, tiles * 256)), dim3(256), 0, ctx->stream, vol, p_max, p_min,
                       series, d);
  }
  else
  {
    const uint64_t tiles = (npts + 15) / 16;
    hipLaunchKernelGGL((k_time_reduce<1, 16>), dim3(capped_grid(ctx, tiles * 256)), dim3(256), 0, ctx->stream, vol, p_max, p_min,
                       series, d);
  }
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
