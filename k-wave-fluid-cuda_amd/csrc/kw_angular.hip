// kw_angular.hip — device code of the angular-spectrum CW projector (DESIGN.md "Angular-spectrum projector"): a complex
// pressure plane P0 is carried to the planes z_j = z0 + j dz of a homogeneous, possibly absorbing medium by
//   P(., ., z_j) = ifft2( fft2(P0) H(kx, ky, z_j) )
// The plane is transformed once; every output plane costs a multiply by H and one inverse 2-D transform.  No transform
// runs along z and nothing is expanded along z.
//
//   kw_angular_operator   the five per-bin tables that give H on every plane, evaluated in float64, rounded once; and
//                         their copy in the fused pipeline's plane layout (rows of P bins + the x-Nyquist side array)
//   k_yinv_angular        the y-inverse of kw_fused_angular_planes (kw_fused_main.hip): tile (kx tile, plane) forms H of
//                         its plane from the table lines, mixes the two source spectra and transforms both along y
//   kw_angular_mix        the same H and mix on plain [ky][Ex/2 + 1] spectra for a chunk of planes (rocFFT path, and the
//                         fused stage's twin)
//
// H per bin and plane j, from the tables (a0, a1, b0, b1, alive):
//   phase   a0 + j a1 in wrapping 32-bit arithmetic, in units of 2^-32 turns: exact, whatever j (a float32 product q z_j
//           is 3e-4 rad off at plane 1000); as a signed word it is the reduced argument of ONE sincosf
//   modulus exp2(-(b0 + j b1)) / (Ex Ey): absorption along the oblique path, or the evanescent decay
//   alive   j < alive, else H = 0 (angular restriction: the cut-off kc(z) falls monotonically with z)
// The field is complex but the pipeline is R2C / C2R, and H depends on kx^2 + ky^2 only: the 2x2 mix of kw_cw.hip
//   Pr^ = Hr Sr^ - Hi Si^        Pi^ = Hi Sr^ + Hr Si^
// gives Hermitian half-spectra again.
#include "kw_elementwise.h"
#include "kw_fused.hip"

namespace {

struct AngOpArgs
{
  uint32_t* tab; // 5 tables of nxc * ey words each: a0, a1, b0 (float bits), b1 (float bits), alive
  uint32_t  nxc, ex, ey, nz, restrict_on;
  double    dkx, dky, k, alpha, z0, dz, half_d2; // half_d2 = D^2 / 2
};

__global__ __launch_bounds__(256) void k_angular_operator(AngOpArgs g)
{
  const uint64_t n = static_cast<uint64_t>(g.nxc) * g.ey;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
#pragma clang fp contract(off)
    const uint32_t ix = static_cast<uint32_t>(e % g.nxc), iy = static_cast<uint32_t>(e / g.nxc);
    const double kx  = g.dkx * static_cast<double>(kw_folded(ix, g.ex));
    const double ky  = g.dky * static_cast<double>(kw_folded(iy, g.ey));
    const double kr2 = (kx * kx) + (ky * ky);
    const double k2  = g.k * g.k;
    const double q   = sqrt(fabs(k2 - kr2));
    uint32_t a0 = 0, a1 = 0;
    double   b0 = 0.0, b1 = 0.0;
    if (kr2 < k2)
    {
      a0 = kw_phase_word(q * g.z0 / kTwoPi); // the turns of q z
      a1 = kw_phase_word(q * g.dz / kTwoPi);
      b0 = (g.alpha * g.z0 * g.k / q) * kLog2e;
      b1 = (g.alpha * g.dz * g.k / q) * kLog2e;
    }
    else if (kr2 > k2)
    {
      b0 = (q * g.z0) * kLog2e;
      b1 = (q * g.dz) * kLog2e;
    }
    uint32_t alive = g.nz;
    if (g.restrict_on)
    { // leading planes with kr <= kc(z_j): kc falls with z, so the first plane beyond the cut-off is found by bisection
      const double kr = sqrt(kr2);
      uint32_t lo = 0, hi = g.nz; // planes < lo are alive, planes >= hi are not
      while (lo < hi)
      {
        const uint32_t m  = lo + (hi - lo) / 2;
        const double   z  = g.z0 + static_cast<double>(m) * g.dz;
        const double   kc = g.k * sqrt(g.half_d2 / (g.half_d2 + (z * z)));
        if (kr <= kc) lo = m + 1; else hi = m;
      }
      alive = lo;
    }
    if (kr2 == k2 && g.alpha > 0.0) alive = 0;
    g.tab[e]         = a0;
    g.tab[n + e]     = a1;
    g.tab[2 * n + e] = __float_as_uint(static_cast<float>(b0));
    g.tab[3 * n + e] = __float_as_uint(static_cast<float>(b1));
    g.tab[4 * n + e] = alive;
  }
}

// the tables in the plane layout of the fused pipeline's scratch arrays: per table pe = P * ey (+ ey) words,
//   main  dst[ky * P + kx]  (kx < nxm; pad columns 0)      side  dst[P * ey + ky] = column nxc - 1   (when side != 0)
__global__ __launch_bounds__(256) void k_angular_import(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src,
                                                        uint32_t nxc, uint32_t nxm, uint32_t P, uint32_t ey, uint32_t side,
                                                        uint32_t pe)
{
  const uint64_t n = 5ull * pe;
  const uint64_t nr = static_cast<uint64_t>(nxc) * ey;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t t = static_cast<uint32_t>(e / pe), r = static_cast<uint32_t>(e % pe);
    uint32_t v = 0;
    if (r < P * ey)
    {
      const uint32_t ky = r / P, kx = r % P;
      if (kx < nxm) v = src[t * nr + static_cast<uint64_t>(ky) * nxc + kx];
    }
    else if (side) v = src[t * nr + static_cast<uint64_t>(r - P * ey) * nxc + (nxc - 1u)];
    dst[e] = v;
  }
}

// H of one bin on plane j (kwave_hip.h "angular-spectrum projector"): every step in float32, no contraction
//   angle = float(int32(a0 + j a1)) * (2 pi 2^-32)       one rounding in the conversion, one in the product: <= 2e-7 rad
//   m     = exp2f(-(b0 + (float(j) * b1))) * divider     0 where j >= alive
//   Hr = m * cos(angle),  Hi = -(m * sin(angle))
__device__ __forceinline__ void angular_h(uint32_t a0, uint32_t a1, float b0, float b1, uint32_t alive, uint32_t j,
                                          float divider, float& hr, float& hi)
{
#pragma clang fp contract(off)
  const uint32_t ph  = a0 + j * a1;
  const float    ang = static_cast<float>(static_cast<int32_t>(ph)) * 1.4629180792671596e-9f;
  float sn, cs;
  sincosf(ang, &sn, &cs);
  float m = exp2f(-(b0 + (static_cast<float>(j) * b1))) * divider;
  if (j >= alive) m = 0.f;
  hr = m * cs;
  hi = -(m * sn);
}

// the 2x2 mix of kw_cw_mix, out of place: association order (kwave_hip.h), no contraction into fma
__device__ __forceinline__ void mix_bin(const float2& x, const float2& y, float hr, float hi, float2& p, float2& q)
{
#pragma clang fp contract(off)
  p = make_float2((hr * x.x) - (hi * y.x), (hr * x.y) - (hi * y.y));
  q = make_float2((hi * x.x) + (hr * y.x), (hi * x.y) + (hr * y.y));
}

// =====================================================================================================================
// y-inverse of the projector: tile (kx tile = blockIdx.x, plane = blockIdx.y of the chunk).  A y-pass whose body spells
// the line-tile steps of kw_fused.hip out (see "line-tile steps" there for why); its own:
//   - the input lines are the SOURCE's 2-D spectra a.in[0] (Sr^) and a.in[1] (Si^): the same lines for every plane, no z
//     in the address (side blocks: every lane reads the one side column, whatever its plane)
//   - before the transform each bin is multiplied: the five table lines are read at the very addresses of the spectrum
//     lines, H of plane a.j0 + z is formed and the pair is mixed in registers
//   - both inverse transforms run back to back over the one exchange buffer, into a.out[0] and a.out[1] at plane z
// =====================================================================================================================
template<int L> __global__ __launch_bounds__(Geo<L>::THREADS) void k_yinv_angular(AngArgs a)
{
  using G = Geo<L>;
  constexpr int R1 = G::R1, R2 = G::R2;
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  load_twiddles<L>(twl, a.tw);
  const int       c  = threadIdx.x % G::NL;
  const int       j  = threadIdx.x / G::NL;
  const TileCoord tc = tile_coord<G::NL>(a.nxc, a.P, a.side_off, gridDim.y, c);
  if (tc.dead) return;
  const uint32_t kx    = tc.side ? 0u : tc.kx;
  const bool     valid = tc.valid;
  const uint32_t z     = tc.pos;
  const uint32_t Pe    = tc.pitch;
  const uint32_t soff2 = tc.side ? a.side_off2 : 0u; // the side column of a 2-D plane array
  const uint32_t plane = a.j0 + z;

  float2 vr[R1], vi[R1];
  if (ACTW(R2, j))
  {
    const float2* __restrict__ in0 = a.in[0];
    const float2* __restrict__ in1 = a.in[1];
    const uint32_t* __restrict__ tab = a.tab;
    uint32_t b = static_cast<uint32_t>(j) * Pe + tc.col + soff2;
    asm volatile("" : "+v"(b));
    const uint32_t step = R2 * Pe;
    float2 xr[R1], xi[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++) xr[n1] = ld_uni(in0, static_cast<uint64_t>(n1) * step, b * static_cast<uint32_t>(sizeof(float2)));
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++) xi[n1] = ld_uni(in1, static_cast<uint64_t>(n1) * step, b * static_cast<uint32_t>(sizeof(float2)));
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++)
    {
      const uint32_t e = b + static_cast<uint32_t>(n1) * step;
      float hr, hi;
      angular_h(tab[e], tab[a.tab_elems + e], __uint_as_float(tab[2u * a.tab_elems + e]),
                __uint_as_float(tab[3u * a.tab_elems + e]), tab[4u * a.tab_elems + e], plane, a.divider, hr, hi);
      mix_bin(xr[n1], xi[n1], hr, hi, vr[n1], vi[n1]);
    }
  }
  lds_barrier(); // twiddle table visible
#pragma unroll
  for (int o = 0; o < 2; o++)
  {
    if (ACTW(R2, j))
    {
      float2 (&v)[R1] = o ? vi : vr;
      step_a<L, kInv>(v, j, twl);
#pragma unroll
      for (int k1 = 0; k1 < R1; k1++) lds[k1 * G::SF + j * G::NL + c] = v[k1];
    }
    lds_barrier();
    if (ACTW(R1, j))
    {
      float2 w[R2];
#pragma unroll
      for (int n2 = 0; n2 < R2; n2++) w[n2] = lds[j * G::SF + n2 * G::NL + c];
      Dft<R2, kInv>::run(w);
      if (valid)
      {
        float2* __restrict__ Sout = a.out[o];
        uint32_t b = (z * a.ny + static_cast<uint32_t>(j)) * Pe + kx + tc.off;
        asm volatile("" : "+v"(b));
        const uint32_t step = R1 * Pe;
#pragma unroll
        for (int k2 = 0; k2 < R2; k2++) st_uni(Sout, static_cast<uint64_t>(k2) * step, b * static_cast<uint32_t>(sizeof(float2)), w[k2]);
      }
    }
    if (o == 0) lds_barrier(); // exchange buffer reused by the second transform
  }
}

// the rocFFT twin: planes j0 ... j0 + nplanes - 1 of the mixed pair from the source's [ey][nxc] spectra and the tables in
// their natural order; out_re / out_im are [nplanes][ey][nxc]
__global__ __launch_bounds__(256) void k_angular_mix(float2* __restrict__ out_re, float2* __restrict__ out_im,
                                                     const float2* __restrict__ sre, const float2* __restrict__ sim,
                                                     const uint32_t* __restrict__ tab, uint32_t nr, uint32_t nplanes,
                                                     uint32_t j0, float divider)
{
  const uint64_t n = static_cast<uint64_t>(nr) * nplanes;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const uint32_t bin = static_cast<uint32_t>(e % nr), z = static_cast<uint32_t>(e / nr);
    float hr, hi;
    angular_h(tab[bin], tab[nr + bin], __uint_as_float(tab[2u * nr + bin]), __uint_as_float(tab[3u * nr + bin]),
              tab[4u * nr + bin], j0 + z, divider, hr, hi);
    float2 p, q;
    mix_bin(sre[bin], sim[bin], hr, hi, p, q);
    out_re[e] = p;
    out_im[e] = q;
  }
}

} // namespace

namespace kwfused {

// the y-inverse of kw_fused_angular_planes: a.in / a.out / a.tab / a.j0 are set by the caller, the geometry here
kw_status yinv_angular(kw_ctx* ctx, AngArgs a)
{
  const auto& f = ctx->fused;
  const kw_constants& c = ctx->c;
  KW_PROF(ctx, "k_yinv_angular");
  a.tw        = f.tw[1];
  a.nxc       = f.nxm;
  a.P         = f.P;
  a.ny        = c.ny;
  a.side_off  = f.side_off;
  a.side_off2 = f.P * c.ny;
  a.tab_elems = f.P * c.ny + (f.side_off != 0 ? c.ny : 0u);
  a.divider   = static_cast<float>(1.0 / (static_cast<double>(c.nx) * static_cast<double>(c.ny)));
  const uint32_t side_tile = (f.side_off != 0) ? 1u : 0u;
  const dim3 grid(f.P / nl_yz(c.ny) + side_tile, c.nz, 1);
#define M(LEN) LAUNCH((k_yinv_angular<LEN>), grid, dim3(Geo<LEN>::THREADS), a)
  KW_LEN_SWITCH(c.ny, M)
#undef M
  return KW_OK;
}

} // namespace kwfused

extern "C" {

kw_status kw_angular_operator(kw_ctx* ctx, uint32_t* tables, uint32_t* imported, double dx, double dy, double k, double alpha,
                              double z0, double dz, uint32_t n_planes, int restriction)
{
  KW_CHECK_CONSTS(ctx);
  KW_PROF(ctx, "angular_operator");
  KW_REQUIRE(tables != nullptr);
  KW_REQUIRE(dx > 0.0 && dy > 0.0 && k > 0.0 && alpha >= 0.0 && z0 >= 0.0 && dz > 0.0);
  KW_REQUIRE(n_planes >= 1 && n_planes <= 4096);
  const kw_constants& c = ctx->c;
  KW_REQUIRE(c.nx % 2 == 0 && c.nx_complex == c.nx / 2 + 1);
  AngOpArgs g{};
  g.tab = tables;
  g.nxc = c.nx_complex; g.ex = c.nx; g.ey = c.ny; g.nz = n_planes;
  g.restrict_on = restriction != 0 ? 1u : 0u;
  g.dkx = kTwoPi / (static_cast<double>(c.nx) * dx);
  g.dky = kTwoPi / (static_cast<double>(c.ny) * dy);
  g.k = k; g.alpha = alpha; g.z0 = z0; g.dz = dz;
  const double dmin = fmin(static_cast<double>(c.nx - 1) * dx, static_cast<double>(c.ny - 1) * dy);
  g.half_d2 = 0.5 * (dmin * dmin);
  const uint64_t n = static_cast<uint64_t>(c.nx_complex) * c.ny;
  hipLaunchKernelGGL(k_angular_operator, dim3(capped_grid(ctx, n)), dim3(256), 0, ctx->stream, g);
  KW_LAUNCH_CHECK();
  if (imported != nullptr)
  {
    const auto& f = ctx->fused;
    if (!f.ready) { kw_set_error("kw_angular_operator: kw_fused_create has not been called (imported tables)"); return KW_ERR_STATE; }
    const uint32_t side = (f.side_off != 0) ? 1u : 0u;
    const uint32_t pe   = f.P * c.ny + (side ? c.ny : 0u);
    hipLaunchKernelGGL(k_angular_import, dim3(capped_grid(ctx, 5ull * pe)), dim3(256), 0, ctx->stream, imported, tables,
                       c.nx_complex, f.nxm, f.P, c.ny, side, pe);
    KW_LAUNCH_CHECK();
  }
  return KW_OK;
}

kw_status kw_angular_mix(kw_ctx* ctx, float* out_re, float* out_im, const float* spec_re, const float* spec_im,
                         const uint32_t* tables, uint32_t n_bins, uint32_t n_planes, uint32_t j0, float divider)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "angular_mix");
  if (n_bins == 0 || n_planes == 0) return KW_OK;
  KW_REQUIRE(out_re && out_im && spec_re && spec_im && tables && out_re != out_im);
  KW_REQUIRE(static_cast<uint64_t>(j0) + n_planes <= (1ull << 31));
  hipLaunchKernelGGL(k_angular_mix, dim3(capped_grid(ctx, static_cast<uint64_t>(n_bins) * n_planes)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<float2*>(out_re), reinterpret_cast<float2*>(out_im), reinterpret_cast<const float2*>(spec_re),
                     reinterpret_cast<const float2*>(spec_im), tables, n_bins, n_planes, j0, divider);
  KW_LAUNCH_CHECK();
  return KW_OK;
}
}
