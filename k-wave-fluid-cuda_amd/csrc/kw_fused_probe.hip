// kw_fused_probe.hip — tuning probes of the fused pipeline (kw_fused_probe, tools/probe_passes.py): the memory pattern of
// a line pass without its arithmetic.  The probes that run the pipeline's own kernels are in kw_fused_main.hip.
#include "kw_fused.hip"

namespace {

__global__ void k_probe_copy4(float4* __restrict__ p, size_t n4)
{
  for (size_t e = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n4; e += static_cast<size_t>(gridDim.x) * blockDim.x)
  {
    float4 v = p[e];
    v.x += 1.f;
    p[e] = v;
  }
}
// LEVEL 0: tile loads + tile stores only; 1: plus the LDS exchange (no DFTs)
template<int L, int LEVEL> __global__ __launch_bounds__(Geo<L>::THREADS) void k_probe_tile(PassArgs a)
{
  using G = Geo<L>;
  constexpr int R1 = G::R1, R2 = G::R2;
  __shared__ float2 lds[G::LDSB];
  const int      c   = threadIdx.x % G::NL;
  const int      j   = threadIdx.x / G::NL;
  const uint32_t kx  = blockIdx.x * G::NL + c;
  const uint32_t kxl = min(kx, a.nxc - 1u);
  const uint32_t z   = blockIdx.y;
  float2* __restrict__ S = a.out[blockIdx.z];
  float2 v[R1], w[R2];
  const uint32_t b = (z * a.ain.zmul + j * a.ain.estride) * a.P;
#pragma unroll
  for (int n1 = 0; n1 < R1; n1++) v[n1] = S[b + kxl + n1 * (R2 * a.ain.estride * a.P)];
  if (LEVEL >= 1)
  {
#pragma unroll
    for (int k1 = 0; k1 < R1; k1++) lds[k1 * G::SF + j * G::NL + c] = v[k1];
    lds_barrier();
#pragma unroll
    for (int n2 = 0; n2 < R2; n2++) w[n2] = lds[j * G::SF + n2 * G::NL + c];
  }
  else
  {
#pragma unroll
    for (int n2 = 0; n2 < R2; n2++) w[n2] = make_float2(v[n2 % R1].x + 1.f, v[n2 % R1].y);
  }
  if (kx < a.nxc)
  {
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++) S[b + kx + k2 * (R1 * a.ain.estride * a.P)] = w[k2];
  }
}

// tile loads + stores with 256-B row segments (two complex = one float4 per lane, 16 lanes per row, 32 columns per tile)
template<int L> __global__ __launch_bounds__(256) void k_probe_tile_wide(PassArgs a)
{
  constexpr int R = 16;                    // rows per thread
  const int      c   = threadIdx.x % 16;   // float4 column within the 32-column tile
  const int      j   = threadIdx.x / 16;
  const uint32_t kx  = blockIdx.x * 32 + 2 * c;
  const uint32_t kxl = min(kx, (a.P - 2u));
  const uint32_t z   = blockIdx.y;
  float4* __restrict__ S = reinterpret_cast<float4*>(a.out[0]);
  const uint32_t b = ((z * a.ain.zmul + j * a.ain.estride) * a.P + kxl) / 2;
  const uint32_t step = (R * a.ain.estride * a.P) / 2;
  float4 v[R];
#pragma unroll
  for (int n1 = 0; n1 < R; n1++) v[n1] = S[b + n1 * step];
  if (kx < a.nxc)
  {
#pragma unroll
    for (int n1 = 0; n1 < R; n1++) { v[n1].x += 1.f; S[b + n1 * step] = v[n1]; }
  }
}

// tile loads + stores of lines of 16*R elements, 256 threads, VEC complex per lane (16 lanes per row: 128-B or 256-B
// row segments); XCD: blocks that follow each other in the logical tile order run on the same XCD (same L2 / TLB)
template<int R, int VEC, bool XCD> __global__ __launch_bounds__(256) void k_probe_tile_rt(PassArgs a)
{
  typedef float vf __attribute__((ext_vector_type(2 * VEC)));
  uint32_t bx = blockIdx.x, by = blockIdx.y;
  if (XCD)
  {
    const uint32_t nb = gridDim.x * gridDim.y, b = by * gridDim.x + bx;
    const uint32_t l = (b % 8u) * (nb / 8u) + b / 8u; // nb % 8 == 0 checked by the host
    bx = l % gridDim.x;
    by = l / gridDim.x;
  }
  const int      c   = threadIdx.x % 16;
  const int      j   = threadIdx.x / 16;
  const uint32_t kx  = bx * (16 * VEC) + VEC * c;
  const uint32_t kxl = min(kx, a.P - VEC);
  vf* __restrict__ S = reinterpret_cast<vf*>(a.out[0]);
  const uint32_t b0   = ((by * a.ain.zmul + j * a.ain.estride) * a.P + kxl) / VEC;
  const uint32_t step = (16 * a.ain.estride * a.P) / VEC;
  vf v[R];
#pragma unroll
  for (int n1 = 0; n1 < R; n1++) v[n1] = S[b0 + n1 * step];
  if (kx < a.nxc)
  {
#pragma unroll
    for (int n1 = 0; n1 < R; n1++) { v[n1].x += 1.f; S[b0 + n1 * step] = v[n1]; }
  }
}

// memory pattern of k_xinv<velocity, chain> without its arithmetic: per block 32 spectrum rows in, 32 rows of two real
// arrays in (float4), one real array out, 32 spectrum rows out
template<int L> __global__ __launch_bounds__(GeoX<L>::THREADS) void k_probe_xinv(XinvArgs a)
{
  using G = GeoX<L>;
  constexpr int HALF = L / 2 + 1, Q4 = L / 4, NQ = (2 * G::NL * Q4) / G::THREADS;
  const uint32_t comp = blockIdx.y;
  const uint32_t tile_row0 = blockIdx.x * G::NL * 2;
  const float2* __restrict__ src = a.in[comp];
  float2 acc = make_float2(0.f, 0.f);
  for (int e = threadIdx.x; e < G::NL * HALF; e += G::THREADS)
  {
    const int cc = e / HALF, k = e - cc * HALF;
    const uint32_t r = tile_row0 + 2 * cc;
    const float2 A = src[r * a.P + k], B = src[(r + 1) * a.P + k];
    acc.x += A.x + B.x; acc.y += A.y + B.y;
  }
  float4 keep[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++)
  {
    const uint32_t i = blockIdx.x * (2 * G::NL * L) + 4u * (threadIdx.x + q * G::THREADS);
    const float4 u = ld4(a.out[comp] + i), d = ld4(a.m0[comp] + i);
    keep[q] = make_float4(u.x + d.x + acc.x, u.y + d.y, u.z + d.z, u.w + d.w + acc.y);
    st4(a.out[comp] + i, keep[q]);
  }
  float2* __restrict__ dst = a.fout[comp];
  for (int e = threadIdx.x; e < G::NL * HALF; e += G::THREADS)
  {
    const int cc = e / HALF, k = e - cc * HALF;
    const uint32_t r = tile_row0 + 2 * cc;
    dst[r * a.P + k]       = make_float2(keep[0].x, acc.y);
    dst[(r + 1) * a.P + k] = make_float2(keep[NQ - 1].y, acc.x);
  }
}

} // namespace

// kw_fused_probe with `which` one of 10-16, 20-23, 30-37 (kw_fused_main.hip has checked the pipeline and the single rank)
kw_status kwfused::probe_patterns(kw_ctx* ctx, int which, const float* op)
{
  auto& f = ctx->fused;
  const kw_constants& c = ctx->c;
  if (which == 10)
  {
    const size_t n4 = static_cast<size_t>(f.P) * c.ny * c.nz / 2;
    LAUNCH(k_probe_copy4, dim3(256 * 16), dim3(256), reinterpret_cast<float4*>(f.s[0]), n4);
    return KW_OK;
  }
  if (which >= 11 && which <= 14)
  { // 11/12: y-line tiles, 13/14: z-line tiles; odd: loads + stores only, even: plus the LDS exchange
    KW_REQUIRE(c.nz == c.ny && Fac<256>::R1 == Fac<256>::R2);
    PassArgs a{};
    a.out[0] = f.s[0];
    a.nxc = f.nxm;
    a.P   = f.P;
    a.ain = (which <= 12) ? RowAddr{0u, 0u, 0u, c.ny, 1u} : RowAddr{0u, 0u, 0u, 1u, c.ny};
    const dim3 grid(f.P / nl_yz(c.ny), c.nz, 1);
#define M(LEN)                                                                                                         \
  if (which & 1) LAUNCH((k_probe_tile<LEN, 0>), grid, dim3(Geo<LEN>::THREADS), a);                                    \
  else LAUNCH((k_probe_tile<LEN, 1>), grid, dim3(Geo<LEN>::THREADS), a)
    KW_LEN_SWITCH(c.ny, M)
#undef M
    return KW_OK;
  }
  if (which == 15 || which == 16)
  { // 15: y-line tiles, 16: z-line tiles, 32 columns wide
    KW_REQUIRE(c.nz == c.ny && c.ny == 256);
    PassArgs a{};
    a.out[0] = f.s[0];
    a.nxc = f.nxm;
    a.P   = f.P;
    a.ain = (which == 15) ? RowAddr{0u, 0u, 0u, c.ny, 1u} : RowAddr{0u, 0u, 0u, 1u, c.ny};
    LAUNCH((k_probe_tile_wide<256>), dim3((f.P + 31) / 32, c.nz, 1), dim3(256), a);
    return KW_OK;
  }
  if (which >= 30 && which <= 37)
  { // bit 0: z-lines instead of y-lines; bit 1: 256-B segments; bit 2: XCD-grouped tile order.  Lines of 256 or 512.
    KW_REQUIRE(c.nz == c.ny && (c.ny == 256 || c.ny == 512));
    const int w = which - 30;
    PassArgs a{};
    a.out[0] = f.s[0];
    a.nxc = f.nxm;
    a.P   = f.P;
    a.ain = (w & 1) ? RowAddr{0u, 0u, 0u, 1u, c.ny} : RowAddr{0u, 0u, 0u, c.ny, 1u};
    const int  vec = (w & 2) ? 2 : 1;
    const dim3 grid((f.P + 16 * vec - 1) / (16 * vec), c.nz, 1);
    KW_REQUIRE(!(w & 4) || (grid.x * grid.y) % 8 == 0);
#define PR(R, V, X) LAUNCH((k_probe_tile_rt<R, V, X>), grid, dim3(256), a)
    if (c.ny == 256)
    {
      if (w == 0 || w == 1) PR(16, 1, false); else if (w == 2 || w == 3) PR(16, 2, false);
      else if (w == 4 || w == 5) PR(16, 1, true); else PR(16, 2, true);
    }
    else
    {
      if (w == 0 || w == 1) PR(32, 1, false); else if (w == 2 || w == 3) PR(32, 2, false);
      else if (w == 4 || w == 5) PR(32, 1, true); else PR(32, 2, true);
    }
#undef PR
    return KW_OK;
  }
  if (which >= 20 && which <= 23)
  { // op doubles as the real arrays: needs 6 * (N + pad) floats (u x3, dt/rho0 x3); 21..23 stagger the arrays by a pad
    KW_REQUIRE(op != nullptr && c.nx == 256);
    XinvArgs a{};
    float* base = const_cast<float*>(op);
    static const size_t pads[4] = { 0, 1024, 17408, 263168 };
    const size_t N = static_cast<size_t>(c.nx) * c.ny * c.nz + pads[which - 20];
    for (int i = 0; i < 3; i++) { a.in[i] = f.s[i]; a.fout[i] = f.s[i]; a.out[i] = base + i * N; a.m0[i] = base + (3 + i) * N; }
    a.P = f.P;
    LAUNCH((k_probe_xinv<256>), dim3(c.ny * c.nz / (2 * nl_x(c.nx)), 3, 1), dim3(GeoX<256>::THREADS), a);
    return KW_OK;
  }
  kw_set_error("kw_fused_probe: unknown probe %d", which);
  return KW_ERR_INVALID;
}
