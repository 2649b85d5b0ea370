// kw_fused_main.hip — the fused pipeline's host side (schedule, C-ABI) and the code object of its y-, z-, x-forward,
// x-shift and import kernels.  The kernels themselves and the pipeline's other code objects: kw_fused.hip.
#include "kw_fused.hip"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

// import of a reduced real operator into the layout the z-pass reads (see load_op_run):
// dst[ky][kx tile][q][j][c][V] <- src[kz][ky][nxc], kz = j + r1*(q*V + r)  (split lines: 2j + h + 2*r1*k2, run index 2*k2 + h)
// (rows = nyl local ky, nzg planes: the transposed operators of slab mode have the same form)
// nxc: columns of the source rows; nxm <= nxc: columns that go into the row tiles (nxc - 1 when the x-Nyquist column is
// kept apart: k_import_reduced_side stores that one)
// One block per (ky, kx tile): the 16 x nzg values of the tile are gathered as 64-B row pieces (16 kx of one kz) into
// LDS and leave as the tile's contiguous run in destination order.  (Set-up only.  In a rocprof table the first launch of
// this kernel is charged ~58 ms — it is the first dispatch out of this file's code object; the others take ~56 us.)
__global__ __launch_bounds__(256) void k_import_reduced(float* __restrict__ dst, const float* __restrict__ src, uint32_t nxc,
                                                        uint32_t nxm, uint32_t P, uint32_t nyl, uint32_t nzg, uint32_t r1,
                                                        uint32_t vec, uint32_t split)
{
  __shared__ float tile[NLMAX * 1024];
  const uint32_t nt = P / NLMAX, t = blockIdx.x % nt, ky = blockIdx.x / nt;
  const uint32_t n = NLMAX * nzg;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
  {
    const uint32_t kz = i / NLMAX, kx = t * NLMAX + i % NLMAX;
    tile[i] = (kx < nxm) ? src[(static_cast<size_t>(kz) * nyl + ky) * nxc + kx] : 0.f;
  }
  __syncthreads();
  float* __restrict__ out = dst + static_cast<size_t>(blockIdx.x) * n;
  for (uint32_t p = threadIdx.x; p < n; p += blockDim.x)
  {
    uint32_t r = p;
    const uint32_t v  = r % vec; r /= vec;
    const uint32_t c  = r % NLMAX; r /= NLMAX;
    const uint32_t j  = r % r1;
    const uint32_t q  = r / r1;
    const uint32_t ri = q * vec + v; // position in the thread's run
    const uint32_t kz = split ? 2u * j + (ri & 1u) + 2u * r1 * (ri >> 1) : j + r1 * ri;
    out[p] = tile[kz * NLMAX + c];
  }
}
// the side column (kx = nxc - 1) in the same per-thread run layout, its 16-wide tiles running over ky:
// dst[ky tile][q][j][c][V] <- src[kz][ky = 16 * tile + c][nxc - 1]
__global__ void k_import_reduced_side(float* __restrict__ dst, const float* __restrict__ src, uint32_t nxc, uint32_t nyl,
                                      uint32_t nzg, size_t total, uint32_t r1, uint32_t vec, uint32_t split)
{
  const uint32_t nq = nzg / (r1 * vec);
  for (size_t e = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total;
       e += static_cast<size_t>(gridDim.x) * blockDim.x)
  {
    size_t         r  = e;
    const uint32_t r4 = static_cast<uint32_t>(r % vec); r /= vec;
    const uint32_t c  = static_cast<uint32_t>(r % NLMAX); r /= NLMAX;
    const uint32_t j  = static_cast<uint32_t>(r % r1); r /= r1;
    const uint32_t q  = static_cast<uint32_t>(r % nq); r /= nq;
    const uint32_t ky = static_cast<uint32_t>(r) * NLMAX + c;
    const uint32_t ri = q * vec + r4;
    const uint32_t kz = split ? 2u * j + (ri & 1u) + 2u * r1 * (ri >> 1) : j + r1 * ri;
    dst[e] = (ky < nyl) ? src[(static_cast<size_t>(kz) * nyl + ky) * nxc + (nxc - 1u)] : 0.f;
  }
}

#define KW_FRAMES_MAX 65535u /* frames of a frames context: the frame is blockIdx.y of the pass along t */

bool supported_len(uint32_t n)
{
#define X(LEN) if (n == LEN) return true;
  KW_FUSED_LENGTHS(X)
#undef X
  return false;
}

#define KW_FUSED_READY(ctx)                                                                                            \
  do {                                                                                                                 \
    KW_CHECK_CONSTS(ctx);                                                                                              \
    if (!(ctx)->fused.ready) { kw_set_error("%s: kw_fused_create has not been called", __func__); return KW_ERR_STATE; } \
    if ((ctx)->fused.frames)                                                                                           \
    {                                                                                                                  \
      kw_set_error("%s: not on a context in frames mode (kw_fused_set_frames): its stages are kw_fused_line_recon and kw_fused_second_order_frames_*", __func__); \
      return KW_ERR_INVALID;                                                                                           \
    }                                                                                                                  \
  } while (0)

#define KW_TRY(call) KW_TRY_STATUS(call)

// nzc: planes 0 ... nzc - 1 only (0: the whole array)
kw_status launch_xfwd(kw_ctx* ctx, int narr, const float* const* in, float2* const* out, uint32_t nzc = 0)
{
  const kw_constants& c = ctx->c;
  static const char* const names[3] = { "k_xfwd[1]", "k_xfwd[2]", "k_xfwd[3]" };
  KW_PROF(ctx, names[narr - 1]);
  XfwdArgs a{};
  for (int i = 0; i < narr; i++) { a.in[i] = in[i]; a.out[i] = out[i]; }
  a.tw = ctx->fused.tw[0];
  a.nx = c.nx;
  a.P  = ctx->fused.P;
  a.side_off = ctx->fused.side_off;
  a.nrows = c.ny * (nzc ? nzc : c.nz);
  const uint32_t rows_per_tile = 2u * static_cast<uint32_t>(nl_x(c.nx)), full = a.nrows / rows_per_tile;
  if (full > 0)
  {
    const dim3 grid(full, narr, 1);
#define M(LEN) LAUNCH((k_xfwd<LEN, false>), grid, dim3(GeoX<LEN>::THREADS), a)
    KW_LEN_SWITCH(c.nx, M)
#undef M
  }
  if (a.nrows % rows_per_tile != 0)
  { // the partial last tile, masked
    a.tile0 = full;
    const dim3 grid(1, narr, 1);
#define M(LEN) if constexpr (!has_partial_x_tiles(LEN)) KW_NO_TAIL(LEN) else LAUNCH((k_xfwd<LEN, true>), grid, dim3(GeoX<LEN>::THREADS), a)
    KW_LEN_SWITCH(c.nx, M)
#undef M
  }
  return KW_OK;
}

// y-pass.  pack_out / pack_in select the packed (per-peer-chunk) row layout on that side; with one rank both layouts
// coincide and the pass may run in place.
// mul: optional per-array factor (see PassArgs).  ordered: the arrays must be taken in list order by one block (a later
// one overwrites, in place, the input of an earlier one) — true for the pressure-gradient pair below.
kw_status launch_ypass(kw_ctx* ctx, int dir, int narr, float2* const* in, float2* const* out, bool pack_in, bool pack_out,
                       uint32_t z0 = 0, uint32_t nzc = 0, const float2* const* mul = nullptr, bool ordered = false)
{
  const kw_constants& c = ctx->c;
  const auto& f = ctx->fused;
  if (ordered && narr > 1 && c.ny == 512 && f.split512)
  { // one array per block in these kernels: order by launch instead
    KW_TRY(launch_ypass(ctx, dir, 1, in, out, pack_in, pack_out, z0, nzc, mul, false));
    return launch_ypass(ctx, dir, narr - 1, in + 1, out + 1, pack_in, pack_out, z0, nzc, mul ? mul + 1 : nullptr, true);
  }
  static const char* const names[3][3] = { { "k_ypass_fwd[1]", "k_ypass_fwd[2]", "k_ypass_fwd[3]" },
                                           { "k_ypass_inv[1]", "k_ypass_inv[2]", "k_ypass_inv[3]" },
                                           { "k_ypass_inv_pgrad[1]", "k_ypass_inv_pgrad[2]", "k_ypass_inv_pgrad[3]" } };
  KW_PROF(ctx, names[dir < 0 ? 0 : (mul != nullptr ? 2 : 1)][narr - 1]);
  PassArgs a{};
  for (int i = 0; i < narr; i++) { a.in[i] = in[i]; a.out[i] = out[i]; a.mul[i] = mul ? mul[i] : nullptr; }
  a.tw  = f.tw[1];
  a.nxc = f.nxm;
  a.P   = f.P;
  a.PX  = f.PX;
  a.side_off = f.side_off; // (packed sides: the side array travels as per-peer chunks [nz local][nyl] behind the row chunks)
  const uint32_t side_tile = (a.side_off != 0) ? 1u : 0u; // one more tile index: the blocks of the x-Nyquist side array
  const RowAddr natural{0u, 0u, 0u, c.ny, 1u};
  const RowAddr packed{(1u << 20) / f.nyl + 1u, f.nyl, c.nz * f.nyl, f.nyl, 1u};
  a.ain  = pack_in ? packed : natural;
  a.aout = pack_out ? packed : natural;
  a.narr = narr; // each block walks the arrays of the launch (the next one's lines requested before the current transform)
  { // ... unless the launch would not even fill the chip twice (small grids): then one array per block — three times the
    // blocks, a third of each block's life — is worth more than the prefetch (128^3: y-passes of three arrays 15 -> 13 us,
    // step +3 %).  Not for `ordered` lists (in-place hazards).
    const uint32_t blocks = (f.P / nl_yz(c.ny) + side_tile) * (nzc ? nzc : c.nz);
    if (!ordered && narr > 1 && blocks < 8u * static_cast<uint32_t>(ctx->cu_count)) a.narr = 1;
  }
  a.z0   = z0;
  if (c.ny == 512 && f.split512)
  { // 2 x 256 lines: 16-column tiles, one array per block
    a.narr = 1;
    const dim3 g(f.P / NLMAX + side_tile, nzc ? nzc : c.nz, narr), b(Geo<256>::THREADS);
    if (dir < 0) { if (pack_out) LAUNCH((k_ypass_split<512, kFwd, false, true>), g, b, a);
                   else LAUNCH((k_ypass_split<512, kFwd, false, false>), g, b, a); }
    else         { if (pack_in) LAUNCH((k_ypass_split<512, kInv, true, false>), g, b, a);
                   else LAUNCH((k_ypass_split<512, kInv, false, false>), g, b, a); }
    return KW_OK;
  }
  const dim3 grid(f.P / nl_yz(c.ny) + side_tile, nzc ? nzc : c.nz, narr / a.narr);
  // forward: natural in, natural or packed out; inverse: natural or packed in, natural out
#define M(LEN)                                                                                                         \
  if (dir < 0) { if (pack_out) LAUNCH((k_ypass<LEN, kFwd, false, true>), grid, dim3(Geo<LEN>::THREADS), a);           \
                 else LAUNCH((k_ypass<LEN, kFwd, false, false>), grid, dim3(Geo<LEN>::THREADS), a); }                  \
  else         { if (pack_in) LAUNCH((k_ypass<LEN, kInv, true, false>), grid, dim3(Geo<LEN>::THREADS), a);            \
                 else LAUNCH((k_ypass<LEN, kInv, false, false>), grid, dim3(Geo<LEN>::THREADS), a); }
  KW_LEN_SWITCH(c.ny, M)
#undef M
  return KW_OK;
}

// z-fused on the (possibly transposed) spectra: lines of nz_global elements, nyl local rows, stride nyl*P
template<int MODE> kw_status launch_zfused(kw_ctx* ctx, int narr, ZArgs a)
{
  const kw_constants& c = ctx->c;
  const auto& f = ctx->fused;
  static const char* const names[4][3] = { { "k_zfused_pgrad", "k_zfused_pgrad", "k_zfused_pgrad" },
                                           { "k_zfused_vgrad[1]", "k_zfused_vgrad[2]", "k_zfused_vgrad[3]" },
                                           { "k_zfused_absorb[1]", "k_zfused_absorb[2]", "k_zfused_absorb[3]" },
                                           { "k_zfused_source", "k_zfused_source", "k_zfused_source" } };
  KW_PROF(ctx, names[MODE][narr - 1]);
  if (f.pipelined)
  { // the transposed spectra live in r[] (callers name the arrays by their s[] slots)
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
      {
        if (a.in[i] == f.s[j]) a.in[i] = f.r[j];
        if (a.out[i] == f.s[j]) a.out[i] = f.r[j];
      }
  }
  a.tw      = f.tw[2];
  a.divider = c.fft_divider;
  a.nxc     = f.nxm;
  // 2-D (Nz == 1): the "z" pass runs along y — the y-derivative is the one along the line, there is no third array
  a.axis_of[0] = 0; a.axis_of[1] = f.two_d ? 2u : 1u; a.axis_of[2] = 2;
  if (f.two_d) a.dd[2] = a.dd[1]; // ... whose derivative vector is ddy
  a.side_off    = f.side_off;
  a.op_side_off = f.side_off; // the imported operators hold the side column's values behind the P * ny * nz of the row tiles
  a.P       = f.slab ? f.PX : f.P; // slab mode: the z-pass works on the exchanged rows in place
  a.Pop     = f.P;
  a.ny      = f.nyl;
  a.nz      = f.nz_global;
  a.ky0     = f.rank * f.nyl;
  a.narr    = narr;
  if (f.nz_global == 512 && f.split512)
  { // 2 x 256 lines: one array per block
    LAUNCH((k_zfused_split<512, MODE>), z_pass_grid(ctx, NLMAX, narr), dim3(Geo<256>::THREADS), a);
    return KW_OK;
  }
  // smallest grids (fewer blocks than two per CU): one array per block instead of the arrays back to back (64^3: z-fused
  // kernels 10.6 -> 8.8 us, step +4 %; at 128^3, 640 blocks, the in-block walk with its prefetch is still the faster form)
  dim3 grid = z_pass_grid(ctx, nl_z(f.nz_global));
  if ((MODE == Z_VGRAD || MODE == Z_ABSORB) && narr > 1 && grid.x * grid.y < 2u * static_cast<uint32_t>(ctx->cu_count))
  {
    grid.z = static_cast<uint32_t>(narr);
    a.narr = 1;
  }
  return KW_LAUNCH_ZPASS((k_zfused<LEN, MODE>), f.nz_global, grid, a);
}

// the full tiles go to the code object that holds this epilogue's kernels for rows of this length, the partial last tile
// of the grid (if any; only ever in the last chunk: chunks are whole tiles otherwise) to the one that holds their masked
// forms
template<int EPI, bool CHAIN = false, int TERMS = 0>
kw_status launch_xinv(kw_ctx* ctx, int ncomp, XinvArgs a, uint32_t z0 = 0, uint32_t nzc = 0, bool plane = false)
{
  const kw_constants& c = ctx->c;
  static const char* const names[6][2] = { { "k_xinv_store", "k_xinv_store" }, { "k_xinv_velocity", "k_xinv_velocity_chain" },
                                           { "k_xinv_initvel", "k_xinv_initvel" }, { "k_xinv_density", "k_xinv_density_chain" },
                                           { "k_xinv_psum", "k_xinv_psum_chain" }, { "k_xinv_psum_one", "k_xinv_psum_one_chain" } };
  KW_PROF(ctx, names[EPI][CHAIN ? 1 : 0]);
  a.tw = ctx->fused.tw[0];
  a.c  = c;
  a.P  = ctx->fused.P;
  a.side_off = ctx->fused.side_off;
  a.nrows = c.ny * c.nz;
  if (plane) // one block per z-plane; the kernel does the plane's y transforms as well
    return EPI == EPI_PSUM1   ? xinv_psum_one_plane(CHAIN ? 1 : 0, ctx, ncomp, a, z0, nzc ? nzc : c.nz)
           : EPI != EPI_DENSITY ? xinv_other_plane(EPI, CHAIN ? 1 : 0, ctx, ncomp, a, z0, nzc ? nzc : c.nz)
           : TERMS == 5       ? xinv_density_oneterm_plane(CHAIN ? 1 : 0, ctx, ncomp, a, z0, nzc ? nzc : c.nz)
           : TERMS == 4       ? xinv_density_stokes_plane(CHAIN ? 1 : 0, ctx, ncomp, a, z0, nzc ? nzc : c.nz)
                              : xinv_density_plane(CHAIN ? 1 : 0, TERMS, ctx, ncomp, a, z0, nzc ? nzc : c.nz);
  const uint32_t rows_per_tile = 2u * static_cast<uint32_t>(nl_x(c.nx));
  const uint32_t rows = c.ny * (nzc ? nzc : c.nz), full = rows / rows_per_tile;
  const uint32_t tile0 = z0 * c.ny / rows_per_tile; // chunked launches start on tile boundaries (plane_local_tail)
  const bool long_lines = c.nx >= KW_LONG_LINES;
  if (full > 0)
  {
    if (EPI == EPI_PSUM1) KW_TRY(xinv_psum_one(CHAIN ? 1 : 0, ctx, ncomp, a, tile0, full));
    else if (EPI != EPI_DENSITY) KW_TRY(xinv_other(EPI, CHAIN ? 1 : 0, ctx, ncomp, a, tile0, full));
    else if (TERMS == 5) KW_TRY((long_lines ? xinv_density_oneterm_long : xinv_density_oneterm_short)(CHAIN ? 1 : 0, ctx, ncomp, a, tile0, full));
    else if (TERMS == 4) KW_TRY((long_lines ? xinv_density_stokes_long : xinv_density_stokes_short)(CHAIN ? 1 : 0, ctx, ncomp, a, tile0, full));
    else if (CHAIN) KW_TRY((long_lines ? xinv_density_chain_long : xinv_density_chain_short)(TERMS, ctx, ncomp, a, tile0, full));
    else KW_TRY((long_lines ? xinv_density_plain_long : xinv_density_plain_short)(TERMS, ctx, ncomp, a, tile0, full));
  }
  if (rows % rows_per_tile != 0)
  {
    if (EPI == EPI_PSUM1) KW_TRY(xinv_psum_one_tail(CHAIN ? 1 : 0, ctx, ncomp, a, tile0 + full, 1));
    else if (EPI != EPI_DENSITY) KW_TRY(xinv_other_tail(EPI, CHAIN ? 1 : 0, ctx, ncomp, a, tile0 + full, 1));
    else if (TERMS == 5) KW_TRY(xinv_density_oneterm_tail(CHAIN ? 1 : 0, ctx, ncomp, a, tile0 + full, 1));
    else if (TERMS == 4) KW_TRY(xinv_density_stokes_tail(CHAIN ? 1 : 0, ctx, ncomp, a, tile0 + full, 1));
    else KW_TRY((CHAIN ? xinv_density_chain_tail : xinv_density_plain_tail)(TERMS, ctx, ncomp, a, tile0 + full, 1));
  }
  return KW_OK;
}

// split-phase exchange of scratch array `slot`: start is ordered after the work enqueued so far; wait orders later
// work after its completion.  Without asynchronous callbacks, start is the blocking exchange and wait a no-op.
kw_status xstart_bytes(kw_ctx* ctx, int slot, void* send, void* recv, size_t bytes_per_peer)
{
  const auto& f = ctx->fused;
  if (f.exchange_piece != nullptr)
  {
    const int rc = f.exchange_piece(f.exchange_user, send, recv, bytes_per_peer, 0, bytes_per_peer, slot);
    if (rc != 0) { kw_set_error("slab exchange: the caller's piece callback failed (status %d)", rc); return KW_ERR_COMM; }
    return KW_OK;
  }
  if (f.exchange_start == nullptr && f.exchange == nullptr) return kw_comm_exchange_start(ctx, slot, send, recv, bytes_per_peer);
  const int rc = (f.exchange_start != nullptr) ? f.exchange_start(f.exchange_user, send, recv, bytes_per_peer, slot)
                                               : f.exchange(f.exchange_user, send, recv, bytes_per_peer);
  if (rc != 0) { kw_set_error("slab exchange: the caller's exchange callback failed (status %d)", rc); return KW_ERR_COMM; }
  return KW_OK;
}
kw_status xwait_one(kw_ctx* ctx, int slot);
kw_status xstart(kw_ctx* ctx, int slot, float2* send, float2* recv)
{ // one spectral scratch array: nz local planes x nyl rows per peer, and the same of the x-Nyquist side array behind them
  const auto& f = ctx->fused;
  const size_t rows = static_cast<size_t>(ctx->c.nz) * f.nyl;
  if (f.side_off == 0) return xstart_bytes(ctx, slot, send, recv, rows * f.PX * sizeof(float2));
  if (f.exchange_start == nullptr && f.exchange == nullptr) // the library's exchange: both pieces in one RCCL group
    return kw_comm_exchange_start2(ctx, slot, send, recv, rows * f.PX * sizeof(float2), send + f.side_off, recv + f.side_off,
                                   rows * sizeof(float2));
  KW_TRY(xstart_bytes(ctx, slot, send, recv, rows * f.PX * sizeof(float2)));
  return xstart_bytes(ctx, slot + KW_COMM_SLOTS, send + f.side_off, recv + f.side_off, rows * sizeof(float2));
}
kw_status xwait(kw_ctx* ctx, int slot)
{
  const auto& f = ctx->fused;
  KW_TRY(xwait_one(ctx, slot));
  // callbacks (a start / wait pair, or a piece callback on the whole-array schedule): the side piece went on a slot of its own
  if (f.side_off != 0 && (f.exchange_start != nullptr || f.exchange_piece != nullptr)) KW_TRY(xwait_one(ctx, slot + KW_COMM_SLOTS));
  return KW_OK;
}
kw_status xwait_one(kw_ctx* ctx, int slot)
{
  const auto& f = ctx->fused;
  if (f.exchange_piece == nullptr && f.exchange_start == nullptr && f.exchange == nullptr) return kw_comm_exchange_wait(ctx, slot);
  if (f.exchange_piece != nullptr ? f.exchange_wait != nullptr : f.exchange_start != nullptr)
  {
    const int rc = f.exchange_wait(f.exchange_user, slot);
    if (rc != 0) { kw_set_error("slab exchange: the caller's wait callback failed (status %d)", rc); return KW_ERR_COMM; }
  }
  return KW_OK;
}

// ---- pipelined slab schedule (fused_plan::pipelined) -------------------------------------------------------------
// Buffer roles: s[] plane layout [nz local][ny][P] (x / y passes), t[] per-peer chunks [peer][nz local][nyl][PX] (packed
// y-pass output = forward send; backward receive = packed y-inverse input), r[] transposed [nz global][nyl][PX] (forward
// receive = z-pass in / out = backward send).  An exchange moves the planes of one chunk (or of all chunks) of one
// array: per peer q the bytes at (q * nz local + z0) * nyl * PX of both layouts, plus the same planes of the side array.
enum { X_FWD = 0, X_BACK = 1 };
constexpr int KW_ZSHIFT_SLOT = KW_COMM_SLOTS - 1;
inline int pslot(int dir, int a, int c) { return (dir * 3 + a) * KW_XCHUNKS_MAX + c; }

// planes [z0, z0 + nzp) of the arrays arrs[0..na) in one exchange
kw_status xpieces_start(kw_ctx* ctx, int slot, int dir, const int* arrs, int na, uint32_t z0, uint32_t nzp)
{
  const auto& f = ctx->fused;
  const size_t all = static_cast<size_t>(ctx->c.nz) * f.nyl, first = static_cast<size_t>(z0) * f.nyl, rows = static_cast<size_t>(nzp) * f.nyl;
  const size_t rb = f.PX * sizeof(float2);
  kw_comm_piece pc[6];
  int n = 0;
  for (int i = 0; i < na; i++)
  {
    float2* send = (dir == X_FWD) ? f.t[arrs[i]] : f.r[arrs[i]];
    float2* recv = (dir == X_FWD) ? f.r[arrs[i]] : f.t[arrs[i]];
    pc[n++] = kw_comm_piece{ send, recv, all * rb, first * rb, rows * rb };
    if (f.side_off != 0)
      pc[n++] = kw_comm_piece{ send + f.side_off, recv + f.side_off, all * sizeof(float2), first * sizeof(float2), rows * sizeof(float2) };
  }
  if (f.exchange_piece == nullptr) return kw_comm_exchange_start_pieces(ctx, slot, pc, n);
  for (int i = 0; i < n; i++)
  {
    const int rc = f.exchange_piece(f.exchange_user, const_cast<void*>(pc[i].send), pc[i].recv, pc[i].stride, pc[i].offset,
                                    pc[i].bytes, slot + i * KW_COMM_SLOTS);
    if (rc != 0) { kw_set_error("slab exchange: the caller's piece callback failed (status %d)", rc); return KW_ERR_COMM; }
  }
  return KW_OK;
}
kw_status xpieces_wait(kw_ctx* ctx, int slot, int npieces)
{
  const auto& f = ctx->fused;
  if (f.exchange_piece == nullptr) return kw_comm_exchange_wait(ctx, slot);
  if (f.exchange_wait == nullptr) return KW_OK; // blocking piece callback
  for (int i = 0; i < npieces; i++)
  {
    const int rc = f.exchange_wait(f.exchange_user, slot + i * KW_COMM_SLOTS);
    if (rc != 0) { kw_set_error("slab exchange: the caller's wait callback failed (status %d)", rc); return KW_ERR_COMM; }
  }
  return KW_OK;
}
// chunks [c0, c0 + nc) of the arrays arrs[0..na) in one exchange
kw_status pstart_multi(kw_ctx* ctx, int dir, const int* arrs, int na, int c0, int nc)
{
  auto& f = ctx->fused;
  const uint32_t nzc = ctx->c.nz / f.xchunks;
  const int slot = pslot(dir, arrs[0], c0);
  KW_TRY(xpieces_start(ctx, slot, dir, arrs, na, c0 * nzc, nc * nzc));
  for (int i = 0; i < na; i++)
    for (int c = c0; c < c0 + nc; c++) f.xslot[dir][arrs[i]][c] = static_cast<int8_t>(slot);
  f.slot_waited[slot] = false;
  f.slot_pieces[slot] = static_cast<int8_t>(na * (f.side_off != 0 ? 2 : 1));
  return KW_OK;
}
kw_status pstart(kw_ctx* ctx, int dir, int a, int c0, int nc) { return pstart_multi(ctx, dir, &a, 1, c0, nc); }
// the arrays [a0, a0 + na): one exchange when batching, else one each
kw_status pstart_arrays(kw_ctx* ctx, int dir, int a0, int na, int c0, int nc)
{
  const int arrs[3] = { a0, a0 + 1, a0 + 2 };
  if (ctx->fused.xbatch) return pstart_multi(ctx, dir, arrs, na, c0, nc);
  for (int i = 0; i < na; i++) KW_TRY(pstart(ctx, dir, a0 + i, c0, nc));
  return KW_OK;
}
kw_status pwait(kw_ctx* ctx, int dir, int a, int c)
{
  auto& f = ctx->fused;
  const int slot = f.xslot[dir][a][c];
  if (slot < 0) { kw_set_error("slab pipeline: chunk %d of array %d awaited before its exchange was started", c, a); return KW_ERR_STATE; }
  if (!f.slot_waited[slot])
  {
    KW_TRY(xpieces_wait(ctx, slot, f.slot_pieces[slot]));
    f.slot_waited[slot] = true;
  }
  return KW_OK;
}
kw_status pwait_all(kw_ctx* ctx, int dir, int a)
{
  for (uint32_t c = 0; c < ctx->fused.xchunks; c++) KW_TRY(pwait(ctx, dir, a, static_cast<int>(c)));
  return KW_OK;
}
// forward exchanges a producer started for a consumer that never came (e.g. a run that ended in between): order the
// buffers' reuse after them
kw_status drain_ahead(kw_ctx* ctx)
{
  auto& f = ctx->fused;
  for (int a = 0; a < f.fwd_ahead; a++) KW_TRY(pwait_all(ctx, X_FWD, a));
  f.fwd_ahead = 0;
  return KW_OK;
}
// forward half up to "exchanges started": from real arrays (x-forward first), from chained x-spectra in s[], or nothing
// to do when the producer's tail already sent them chunk by chunk
kw_status pforward_start(kw_ctx* ctx, int narr, const float* const* in)
{
  auto& f = ctx->fused;
  if (in == nullptr && f.fwd_ahead == narr) return KW_OK;
  if (f.fwd_ahead != 0) KW_TRY(drain_ahead(ctx));
  if (f.xbatch)
  { // small messages: multi-array kernels, one exchange for the lot
    if (in != nullptr) KW_TRY(launch_xfwd(ctx, narr, in, f.s));
    KW_TRY(launch_ypass(ctx, -1, narr, f.s, f.t, false, true));
    return pstart_arrays(ctx, X_FWD, 0, narr, 0, static_cast<int>(f.xchunks));
  }
  for (int a = 0; a < narr; a++)
  {
    if (in != nullptr) KW_TRY(launch_xfwd(ctx, 1, in + a, f.s + a));
    KW_TRY(launch_ypass(ctx, -1, 1, f.s + a, f.t + a, false, true));
    KW_TRY(pstart(ctx, X_FWD, a, 0, static_cast<int>(f.xchunks)));
  }
  return KW_OK;
}
// forward + z-pass per array + backward exchanges started chunk-major (chunk 0 of every array first: the tail's first
// chunk is complete after narr chunk transfers, the rest travel while it computes)
template<int MODE> kw_status pslab_chain(kw_ctx* ctx, int narr, const float* const* in, ZArgs z)
{
  auto& f = ctx->fused;
  const int C = static_cast<int>(f.xchunks);
  KW_TRY(pforward_start(ctx, narr, in));
  if (f.xbatch)
  {
    for (int a = 0; a < narr; a++) KW_TRY(pwait_all(ctx, X_FWD, a));
    f.fwd_ahead = 0;
    z.arr0 = 0;
    KW_TRY(launch_zfused<MODE>(ctx, narr, z));
    return pstart_arrays(ctx, X_BACK, 0, narr, 0, C);
  }
  for (int a = 0; a < narr; a++)
  {
    KW_TRY(pwait_all(ctx, X_FWD, a));
    z.arr0 = a;
    KW_TRY(launch_zfused<MODE>(ctx, 1, z));
    KW_TRY(pstart(ctx, X_BACK, a, 0, 1));
  }
  f.fwd_ahead = 0;
  for (int c = 1; c < C; c++)
    for (int a = 0; a < narr; a++) KW_TRY(pstart(ctx, X_BACK, a, c, 1));
  return KW_OK;
}
// plane-local tail per chunk: backward receive -> y-inverse -> x-inverse + epilogue -> (chained) y-forward -> forward send
template<int EPI, bool CHAIN, int TERMS = 0>
kw_status pslab_tail(kw_ctx* ctx, int narr, int ncomp, const XinvArgs& x, int nchain)
{
  auto& f = ctx->fused;
  const uint32_t C = f.xchunks, nzc = ctx->c.nz / C;
  for (uint32_t c = 0; c < C; c++)
  {
    if (f.xbatch || narr == 1)
    {
      for (int a = 0; a < narr; a++) KW_TRY(pwait(ctx, X_BACK, a, static_cast<int>(c)));
      KW_TRY(launch_ypass(ctx, +1, narr, f.t, f.s, true, false, c * nzc, nzc));
    }
    else
    { // every array's y-inverse as soon as that array is back: only the last one stays between the wire and the epilogue
      for (int a = 0; a < narr; a++)
      {
        KW_TRY(pwait(ctx, X_BACK, a, static_cast<int>(c)));
        KW_TRY(launch_ypass(ctx, +1, 1, f.t + a, f.s + a, true, false, c * nzc, nzc));
      }
    }
    KW_TRY((launch_xinv<EPI, CHAIN, TERMS>(ctx, ncomp, x, c * nzc, nzc)));
    if (CHAIN)
    {
      KW_TRY(launch_ypass(ctx, -1, nchain, f.s, f.t, false, true, c * nzc, nzc));
      KW_TRY(pstart_arrays(ctx, X_FWD, 0, nchain, static_cast<int>(c), 1));
    }
  }
  if (CHAIN) f.fwd_ahead = nchain;
  return KW_OK;
}

// Slab mode, narr independent arrays (velocity gradient, absorption, source scaling): software-pipelined per array so
// that the all-to-all of one array is in flight while the y / z passes of the others run.
template<int MODE> kw_status slab_chain(kw_ctx* ctx, int narr, const float* const* in, ZArgs z)
{
  auto& f = ctx->fused;
  if (f.pipelined) return pslab_chain<MODE>(ctx, narr, in, z); // (the caller's tail is pslab_tail)
  for (int a = 0; a < narr; a++)
  {
    if (in != nullptr) KW_TRY(launch_xfwd(ctx, 1, in + a, f.s + a));
    KW_TRY(launch_ypass(ctx, -1, 1, f.s + a, f.t + a, false, true));
    KW_TRY(xstart(ctx, a, f.t[a], f.s[a]));
  }
  for (int a = 0; a < narr; a++)
  {
    KW_TRY(xwait(ctx, a));
    z.arr0 = a;
    KW_TRY(launch_zfused<MODE>(ctx, 1, z));
    KW_TRY(xstart(ctx, a, f.s[a], f.t[a]));
  }
  for (int a = 0; a < narr; a++)
  {
    KW_TRY(xwait(ctx, a));
    KW_TRY(launch_ypass(ctx, +1, 1, f.t + a, f.s + a, true, false));
  }
  return KW_OK;
}

// forward half of a 3-D transform for narr real arrays: x-forward, y-forward, transpose.  Spectra end up in S[]
// ([nz][ny][P] with one rank, transposed [nz_global][nyl][P] in slab mode).
kw_status forward_xy(kw_ctx* ctx, int narr, const float* const* in, int s0 = 0)
{
  auto& f = ctx->fused;
  const int y_done = f.y_done;
  f.y_done = 0;
  if (f.slab && f.pipelined)
  { // (s0 == 0 on slabs) — ends with the transposed spectra in r[]
    KW_TRY(pforward_start(ctx, narr, in));
    for (int i = 0; i < narr; i++) KW_TRY(pwait_all(ctx, X_FWD, i));
    f.fwd_ahead = 0;
    return KW_OK;
  }
  if (in != nullptr) KW_TRY(launch_xfwd(ctx, narr, in, f.s + s0)); // nullptr: x-spectra were chained into S[] already
  else if (y_done >= s0 + narr) return KW_OK;                      // ... and so was their y-pass (chunked producer)
  if (f.two_d) return KW_OK;                                        // the y transform is inside the fused pass
  if (!f.slab) return launch_ypass(ctx, -1, narr, f.s + s0, f.s + s0, false, false);
  KW_TRY(launch_ypass(ctx, -1, narr, f.s + s0, f.t + s0, false, true));
  for (int i = 0; i < narr; i++) KW_TRY(xstart(ctx, s0 + i, f.t[s0 + i], f.s[s0 + i]));
  for (int i = 0; i < narr; i++) KW_TRY(xwait(ctx, s0 + i));
  return KW_OK;
}

// Single rank: the plane-local tail of a stage — y-inverse, x-inverse + epilogue and, when the epilogue chains the
// x-spectra of its results into S[0..nchain), their forward y-pass — runs per chunk of planes, so that what one kernel
// writes is still in the Infinity Cache when the next one reads it.
template<int EPI, bool CHAIN, int TERMS = 0>
kw_status plane_local_tail(kw_ctx* ctx, int narr, int ncomp, const XinvArgs& x, int nchain,
                                                         float2* const* yin = nullptr, float2* const* yout = nullptr,
                                                         const float2* const* ymul = nullptr)
{
  auto& f = ctx->fused;
  const kw_constants& c = ctx->c;
  if (f.plane)
  { // small grids: one launch — every block takes a z-plane and does its y transforms around the x kernels' work
    XinvArgs xp = x;
    for (int i = 0; i < narr; i++)
    { // y-pass i reads yin[i] (times ymul[i]) and leaves its result where some x-inverse reads it: that one takes both over
      const float2* from = yin ? yin[i] : f.s[i];
      const float2* to   = yout ? yout[i] : f.s[i];
      for (int k = 0; k < 3; k++)
        if (x.in[k] == to) { xp.in[k] = from; xp.ymul[k] = ymul ? ymul[i] : nullptr; }
    }
    KW_TRY((launch_xinv<EPI, CHAIN, TERMS>(ctx, ncomp, xp, 0, 0, true)));
    if (CHAIN) f.y_done = nchain;
    return KW_OK;
  }
  uint32_t nch = static_cast<uint32_t>(ctx->tuning.tail_chunks > 0 ? ctx->tuning.tail_chunks : 1);
  while (nch > 1 && (c.nz % nch != 0 || (c.nz / nch * c.ny) % (2 * nl_x(c.nx)) != 0)) nch--;
  const uint32_t nzc = c.nz / nch;
  for (uint32_t ch = 0; ch < nch; ch++)
  {
    KW_TRY(launch_ypass(ctx, +1, narr, yin ? yin : f.s, yout ? yout : f.s, false, false, ch * nzc, nzc, ymul, ymul != nullptr));
    KW_TRY((launch_xinv<EPI, CHAIN, TERMS>(ctx, ncomp, x, ch * nzc, nzc)));
    if (CHAIN) KW_TRY(launch_ypass(ctx, -1, nchain, f.s, f.s, false, false, ch * nzc, nzc));
  }
  if (CHAIN) f.y_done = nchain;
  return KW_OK;
}

// Way back of the pressure gradient after launch_zfused<Z_PGRAD>: S[0] = Q = F_z^-1{kappa F{p}}, S[2] = G_z (x and y
// still transformed).  d/dx and d/dy share Q: the y-inverse produces F_y^-1{ddy Q} into S[1] and F_y^-1{Q} into S[0]
// (one read of Q), the x-inverse of component 0 applies ddx(kx) to its rows.  Two transposes instead of three in slab
// mode, one array less written by the z-pass and read by the y-pass everywhere.
template<int EPI, bool CHAIN> kw_status gradient_tail(kw_ctx* ctx, XinvArgs x, const float2* ddx, const float2* ddy)
{
  auto& f = ctx->fused;
  x.mulx[0] = ddx;
  if (f.two_d)
  { // 2-D: the fused pass along y left Q in S[0] (d/dx: x ddx(kx) in the x-inverse) and G_y in S[2]; two components
    x.in[1] = f.s[2];
    return launch_xinv<EPI, CHAIN>(ctx, 2, x);
  }
  const float2* mul[3] = { ddy, nullptr, nullptr };
  if (f.slab && f.pipelined && f.xbatch)
  { // small messages: Q and G_z come back in one exchange, one multi-array launch per pass, one exchange forward
    const int back[2] = { 0, 2 };
    KW_TRY(pstart_multi(ctx, X_BACK, back, 2, 0, static_cast<int>(f.xchunks)));
    KW_TRY(pwait_all(ctx, X_BACK, 0));
    KW_TRY(pwait_all(ctx, X_BACK, 2));
    float2* yin[3]  = { f.t[0], f.t[0], f.t[2] };
    float2* yout[3] = { f.s[1], f.s[0], f.s[2] };
    KW_TRY(launch_ypass(ctx, +1, 3, yin, yout, true, false, 0, 0, mul, false));
    x.comp0 = 0;
    KW_TRY((launch_xinv<EPI, CHAIN>(ctx, 3, x)));
    if (CHAIN)
    {
      KW_TRY(launch_ypass(ctx, -1, 3, f.s, f.t, false, true));
      KW_TRY(pstart_arrays(ctx, X_FWD, 0, 3, 0, static_cast<int>(f.xchunks)));
      f.fwd_ahead = 3;
    }
    return KW_OK;
  }
  if (f.slab && f.pipelined)
  { // Q (array 0) and G_z (array 2) come back chunk by chunk; the three components leave again as their rows are done
    const uint32_t C = f.xchunks, nzc = ctx->c.nz / C;
    for (uint32_t ch = 0; ch < C; ch++)
    {
      KW_TRY(pstart(ctx, X_BACK, 0, static_cast<int>(ch), 1));
      KW_TRY(pstart(ctx, X_BACK, 2, static_cast<int>(ch), 1));
    }
    float2* yin[2]  = { f.t[0], f.t[0] };
    float2* yout[2] = { f.s[1], f.s[0] };
    for (uint32_t ch = 0; ch < C; ch++)
    {
      const int c = static_cast<int>(ch);
      KW_TRY(pwait(ctx, X_BACK, 0, c));
      KW_TRY(launch_ypass(ctx, +1, 2, yin, yout, true, false, ch * nzc, nzc, mul, false));
      x.comp0 = 0;
      KW_TRY((launch_xinv<EPI, CHAIN>(ctx, 2, x, ch * nzc, nzc)));
      if (CHAIN)
      {
        KW_TRY(launch_ypass(ctx, -1, 2, f.s, f.t, false, true, ch * nzc, nzc));
        KW_TRY(pstart(ctx, X_FWD, 0, c, 1));
        KW_TRY(pstart(ctx, X_FWD, 1, c, 1));
      }
      KW_TRY(pwait(ctx, X_BACK, 2, c));
      KW_TRY(launch_ypass(ctx, +1, 1, f.t + 2, f.s + 2, true, false, ch * nzc, nzc));
      x.comp0 = 2;
      KW_TRY((launch_xinv<EPI, CHAIN>(ctx, 1, x, ch * nzc, nzc)));
      if (CHAIN)
      {
        KW_TRY(launch_ypass(ctx, -1, 1, f.s + 2, f.t + 2, false, true, ch * nzc, nzc));
        KW_TRY(pstart(ctx, X_FWD, 2, c, 1));
      }
    }
    if (CHAIN) f.fwd_ahead = 3;
    return KW_OK;
  }
  if (f.slab)
  {
    KW_TRY(xstart(ctx, 0, f.s[0], f.t[0]));
    KW_TRY(xstart(ctx, 2, f.s[2], f.t[2]));
    KW_TRY(xwait(ctx, 0));
    float2* yin[2]  = { f.t[0], f.t[0] };
    float2* yout[2] = { f.s[1], f.s[0] };
    KW_TRY(launch_ypass(ctx, +1, 2, yin, yout, true, false, 0, 0, mul, false)); // out of place: no ordering needed
    x.comp0 = 0;
    KW_TRY((launch_xinv<EPI, CHAIN>(ctx, 2, x)));
    KW_TRY(xwait(ctx, 2));
    KW_TRY(launch_ypass(ctx, +1, 1, f.t + 2, f.s + 2, true, false));
    x.comp0 = 2;
    return launch_xinv<EPI, CHAIN>(ctx, 1, x);
  }
  float2* yin[3]  = { f.s[0], f.s[0], f.s[2] };
  float2* yout[3] = { f.s[1], f.s[0], f.s[2] };
  return plane_local_tail<EPI, CHAIN>(ctx, 3, 3, x, CHAIN ? 3 : 0, yin, yout, mul);
}

// inverse half: transpose back, y-inverse; leaves [nz][ny][P] spectra (x still transformed) in S[]
kw_status inverse_y(kw_ctx* ctx, int narr, int s0 = 0)
{
  auto& f = ctx->fused;
  if (f.two_d) return KW_OK;
  if (!f.slab) return launch_ypass(ctx, +1, narr, f.s + s0, f.s + s0, false, false);
  if (f.pipelined)
  { // whole arrays: r[] -> t[] -> y-inverse into s[]
    KW_TRY(pstart_arrays(ctx, X_BACK, s0, narr, 0, static_cast<int>(f.xchunks)));
    for (int i = 0; i < narr; i++) KW_TRY(pwait_all(ctx, X_BACK, s0 + i));
    return launch_ypass(ctx, +1, narr, f.t + s0, f.s + s0, true, false);
  }
  for (int i = 0; i < narr; i++) KW_TRY(xstart(ctx, s0 + i, f.s[s0 + i], f.t[s0 + i]));
  for (int i = 0; i < narr; i++) KW_TRY(xwait(ctx, s0 + i));
  return launch_ypass(ctx, +1, narr, f.t + s0, f.s + s0, true, false);
}

kw_status alloc_scratch(kw_ctx* ctx, void* const s[3], void* const t[3])
{
  auto& f = ctx->fused;
  const kw_constants& c = ctx->c;
  const size_t elems = static_cast<size_t>(f.Palloc) * c.ny * c.nz;
  f.owns_scratch     = (s == nullptr);
  for (int i = 0; i < 3; i++)
  {
    if (f.frames && i > 0) break; // the one stage of a frames context works on s[0] alone
    if (f.owns_scratch)
    {
      KW_HIP(hipMalloc(reinterpret_cast<void**>(&f.s[i]), elems * sizeof(float2)));
      if (f.slab) KW_HIP(hipMalloc(reinterpret_cast<void**>(&f.t[i]), elems * sizeof(float2)));
    }
    else
    {
      KW_REQUIRE(s[i] != nullptr && (!f.slab || (t != nullptr && t[i] != nullptr)));
      f.s[i] = static_cast<float2*>(s[i]);
      f.t[i] = (f.slab) ? static_cast<float2*>(t[i]) : nullptr;
    }
    KW_HIP(hipMemsetAsync(f.s[i], 0, elems * sizeof(float2), ctx->stream));
    if (f.t[i]) KW_HIP(hipMemsetAsync(f.t[i], 0, elems * sizeof(float2), ctx->stream));
    if (f.pipelined)
    { // the transposed set is always the library's own
      KW_HIP(hipMalloc(reinterpret_cast<void**>(&f.r[i]), elems * sizeof(float2)));
      KW_HIP(hipMemsetAsync(f.r[i], 0, elems * sizeof(float2), ctx->stream));
    }
  }
  return KW_OK;
}

kw_status create_impl(kw_ctx* ctx, void* const s[3], void* const t[3])
{
  KW_CHECK_CONSTS(ctx);
  int ok = 0;
  kw_fused_supported(ctx, &ok);
  if (!ok)
  {
    kw_set_error("kw_fused_create: grid %ux%ux%u (x %u ranks) is not supported by the fused pipeline", ctx->c.nx,
                 ctx->c.ny, ctx->c.nz, ctx->fused.nranks);
    return KW_ERR_INVALID;
  }
  // keep the slab description across the reset
  const auto slab = ctx->fused;
  kw_fused_destroy(ctx);
  auto& f = ctx->fused;
  f.slab = slab.slab; f.nranks = slab.nranks; f.rank = slab.rank; f.exchange = slab.exchange; f.exchange_user = slab.exchange_user;
  f.exchange_start = slab.exchange_start; f.exchange_wait = slab.exchange_wait; f.exchange_piece = slab.exchange_piece;
  f.frames = slab.frames;
  KW_HIP(hipSetDevice(ctx->device));
  const kw_constants& c = ctx->c;
  f.nz_global = (f.slab) ? slab.nz_global : c.nz;
  f.nyl       = c.ny / f.nranks;
  f.two_d     = (!f.slab && !f.frames && c.nz == 1); // (frames mode: x-pass, the pass along y by frames, x-pass, for any Nz)
  if (f.two_d)
  { // 2-D: the z-pass kernels run along y — one "row" per plane, lines of Ny elements with stride P
    f.nz_global = c.ny;
    f.nyl       = 1;
  }
  f.Palloc    = (c.nx_complex + NLMAX - 1) / NLMAX * NLMAX;
  {
    // x-Nyquist column apart (see tile_coord) whenever it is the one bin beyond whole tiles.  On slabs the exchange then
    // moves two pieces per peer — the row chunk [nz local][nyl][Nx/2] and the side chunk [nz local][nyl] — i.e. exactly
    // the Nx/2 + 1 bins per row, in aligned rows.  kw_tuning::side_array = 0 keeps the column in the (padded) rows.
    const bool side = (ctx->tuning.side_array != 0) && (c.nx_complex % NLMAX == 1u) && (c.nx_complex > NLMAX) && !f.two_d;
    f.nxm      = side ? c.nx_complex - 1u : c.nx_complex;
    f.P        = side ? f.nxm : f.Palloc;
    f.side_off = side ? f.P * c.ny * c.nz : 0u;
  }
  // Exchange-side row pitch = the pipeline's pitch: every 16-column tile segment of the packed y-passes and of the
  // transposed z-pass is one aligned 128-B line.  (Rows sent without their padding — nx/2+1 complex — would save 5-10 % of
  // the wire bytes of a grid without a side array, but their tile segments straddle two lines: measured on one rank at
  // 256^3 the z-pass then takes 67 us per array instead of 30 and the packed y-passes 35-42 us instead of 23-27.)
  f.PX = f.P;
  memset(f.xslot, -1, sizeof(f.xslot));
  {
    // Pipelined schedule: whenever the exchange can move plane chunks (the library's own transports, or a piece
    // callback).  kw_tuning::slab_pipeline = 0 keeps the whole-array schedule; slab_chunks sets the chunk count (chunks
    // are whole planes and whole x tiles).
    const kw_tuning& tn = ctx->tuning;
    const bool can = f.slab && (f.exchange_piece != nullptr || (f.exchange == nullptr && f.exchange_start == nullptr));
    f.pipelined    = can && tn.slab_pipeline != 0;
    // Plane chunks are off by default (slab_chunks = 1): a step on 8 GPUs is bound by the links, and every RCCL group
    // has a fixed cost on the wire (~30 us measured on one rank) and on the launching thread (~44 us); with the links
    // modelled (tools/emulate_rank.py) two chunks gain 3-4 % at a 10 us fixed cost and lose 6 % at 30 us.
    uint32_t nch = static_cast<uint32_t>(tn.slab_chunks > 0 ? tn.slab_chunks : 1);
    if (nch > KW_XCHUNKS_MAX) nch = KW_XCHUNKS_MAX;
    while (nch > 1 && (c.nz % nch != 0 || (c.nz / nch * c.ny) % (2 * nl_x(c.nx)) != 0)) nch--;
    f.xchunks = f.pipelined ? nch : 1u;
    // Below 4 MB per peer and array the exchanges are latency- and launch-bound: all arrays of a stage then travel in
    // one exchange per direction (6 per step instead of 13) and the passes run as multi-array launches (slab_batch).
    const size_t per_peer = static_cast<size_t>(c.nz) * f.nyl * c.nx_complex * sizeof(float2);
    f.xbatch = f.pipelined && ((tn.slab_batch >= 0) ? (tn.slab_batch == 1) : (per_peer < (4u << 20)));
    if (f.xbatch) f.xchunks = 1u;
  }
  KW_TRY(alloc_scratch(ctx, s, t));
  const uint32_t lens[3] = { c.nx, c.ny, f.nz_global };
  for (int i = 0; i < (f.frames ? 2 : 3); i++) // (frames mode: no transform along z)
  {
    std::vector<float2> tw(lens[i]);
    for (uint32_t m = 0; m < lens[i]; m++)
    {
      const double ph = -2.0 * M_PI * static_cast<double>(m) / static_cast<double>(lens[i]);
      tw[m]           = make_float2(static_cast<float>(std::cos(ph)), static_cast<float>(std::sin(ph)));
    }
    KW_HIP(hipMalloc(reinterpret_cast<void**>(&f.tw[i]), lens[i] * sizeof(float2)));
    KW_HIP(hipMemcpyAsync(f.tw[i], tw.data(), lens[i] * sizeof(float2), hipMemcpyHostToDevice, ctx->stream));
    KW_HIP(hipStreamSynchronize(ctx->stream));
  }
  f.split512 = (ctx->tuning.split512 != 0);
  // whole-plane x kernels (k_xinv PLANE): square planes of 32 / 64, one GPU, 3-D
  f.plane = (ctx->tuning.plane_kernels != 0) && !f.slab && !f.two_d && !f.frames && c.nx == c.ny && plane_len(static_cast<int>(c.nx)) &&
            supported_len(c.nx);
  if (f.plane)
  {
    const size_t elems = static_cast<size_t>(f.Palloc) * c.ny * c.nz;
    KW_HIP(hipMalloc(reinterpret_cast<void**>(&f.s4), elems * sizeof(float2)));
    KW_HIP(hipMemsetAsync(f.s4, 0, elems * sizeof(float2), ctx->stream));
  }
  f.ready = true;
  return KW_OK;
}

} // namespace

extern "C" {

kw_status kw_fused_set_slab(kw_ctx* ctx, uint32_t nranks, uint32_t rank, uint32_t nz_global, kw_exchange_fn fn, void* user)
{
  KW_CHECK_CTX(ctx);
  KW_REQUIRE(nranks >= 1 && rank < nranks);
  if (ctx->fused.ready) { kw_set_error("kw_fused_set_slab: must be called before kw_fused_create"); return KW_ERR_STATE; }
  if (ctx->fused.frames) { kw_set_error("kw_fused_set_slab: the context is in frames mode (kw_fused_set_frames)"); return KW_ERR_INVALID; }
  uint32_t comm_ranks = 0, comm_rank = 0;
  KW_TRY(kw_comm_info(ctx, &comm_ranks, &comm_rank, nullptr));
  if (fn == nullptr && nranks > 1 && comm_ranks == 0)
  {
    kw_set_error("kw_fused_set_slab: %u ranks need an exchange: call kw_comm_init first or pass a callback", nranks);
    return KW_ERR_STATE;
  }
  if (fn == nullptr && comm_ranks != 0 && (comm_ranks != nranks || comm_rank != rank))
  {
    kw_set_error("kw_fused_set_slab: rank %u of %u does not match the communicator (rank %u of %u)", rank, nranks, comm_rank, comm_ranks);
    return KW_ERR_INVALID;
  }
  // one rank with an exchange (callback or communicator) = the slab path against itself
  ctx->fused.slab          = (nranks > 1) || (fn != nullptr) || (comm_ranks != 0);
  ctx->fused.nranks        = nranks;
  ctx->fused.rank          = rank;
  ctx->fused.nz_global     = nz_global;
  ctx->fused.exchange      = fn;
  ctx->fused.exchange_user = user;
  return KW_OK;
}

kw_status kw_fused_set_slab_async(kw_ctx* ctx, kw_exchange_start_fn start, kw_exchange_wait_fn wait)
{
  KW_CHECK_CTX(ctx);
  KW_REQUIRE((start == nullptr) == (wait == nullptr));
  if (ctx->fused.ready) { kw_set_error("kw_fused_set_slab_async: must be called before kw_fused_create"); return KW_ERR_STATE; }
  ctx->fused.exchange_start = start;
  ctx->fused.exchange_wait  = wait;
  return KW_OK;
}

kw_status kw_fused_set_slab_pieces(kw_ctx* ctx, kw_exchange_piece_fn start, kw_exchange_wait_fn wait)
{
  KW_CHECK_CTX(ctx);
  KW_REQUIRE(start != nullptr || wait == nullptr);
  if (ctx->fused.ready) { kw_set_error("kw_fused_set_slab_pieces: must be called before kw_fused_create"); return KW_ERR_STATE; }
  ctx->fused.exchange_piece = start;
  if (start != nullptr) { ctx->fused.exchange_start = nullptr; ctx->fused.exchange_wait = wait; }
  return KW_OK;
}

// frames mode: the z axis of the constants is a batch of independent planes [ny][nx] (kw_fused_line_recon)
kw_status kw_fused_set_frames(kw_ctx* ctx, int on)
{
  KW_CHECK_CTX(ctx);
  if (ctx->fused.ready) { kw_set_error("kw_fused_set_frames: must be called before kw_fused_create"); return KW_ERR_STATE; }
  if (on && ctx->fused.slab) { kw_set_error("kw_fused_set_frames: the context is in slab mode (kw_fused_set_slab)"); return KW_ERR_INVALID; }
  ctx->fused.frames = (on != 0);
  return KW_OK;
}

kw_status kw_fused_supported(kw_ctx* ctx, int* out)
{
  KW_CHECK_CONSTS(ctx);
  KW_REQUIRE(out != nullptr);
  const kw_constants& c = ctx->c;
  const auto& f         = ctx->fused;
  const uint32_t nzg    = (f.slab) ? f.nz_global : c.nz;
  // (the x kernels work on tiles of 2 * NL rows; a row count Ny * Nz that is no whole number of tiles ends in one masked tile)
  bool ok = supported_len(c.nx) && supported_len(c.ny) && supported_len(nzg);
  if (!f.slab && c.nz == 1) ok = supported_len(c.nx) && supported_len(c.ny); // 2-D: x-pass, fused y-pass, x-pass
  if (f.frames) ok = supported_len(c.nx) && supported_len(c.ny) && c.nz <= KW_FRAMES_MAX; // no transform along z, any Nz >= 1
  if (f.slab) ok = ok && (nzg == c.nz * f.nranks) && (c.ny % f.nranks == 0);
  if (ok && !has_partial_x_tiles(static_cast<int>(c.nx))) ok = (c.ny * c.nz) % (2u * static_cast<uint32_t>(nl_x(c.nx))) == 0;
  const uint64_t P64 = (c.nx_complex + NLMAX - 1) / NLMAX * NLMAX;
  ok = ok && (P64 * c.ny * c.nz < (1ull << 32)) && (static_cast<uint64_t>(c.nx) * c.ny * c.nz < (1ull << 32));
  // frames mode: the pass along t holds the frame's offset in the 32-bit BYTE offset of its lanes (load_lines, store_lines),
  // so the scratch array, side array included, ends below 4 GiB: 2^29 complex elements
  if (f.frames) ok = ok && (P64 * c.ny * c.nz < (1ull << 29));
  *out = ok ? 1 : 0;
  return KW_OK;
}

kw_status kw_fused_destroy(kw_ctx* ctx)
{
  KW_CHECK_CTX(ctx);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  (void)kw_comm_sync(ctx); // forward exchanges started ahead by the last stage may still be on the communication stream
  kw_comm_buffers_gone(ctx);
  auto& f = ctx->fused;
  for (int i = 0; i < 3; i++)
  {
    if (f.r[i]) (void)hipFree(f.r[i]);
    f.r[i] = nullptr;
    if (i == 0 && f.s4) { (void)hipFree(f.s4); f.s4 = nullptr; }
    if (f.owns_scratch)
    {
      if (f.s[i]) (void)hipFree(f.s[i]);
      if (f.t[i]) (void)hipFree(f.t[i]);
    }
    if (f.tw[i]) (void)hipFree(f.tw[i]);
    f.s[i] = f.t[i] = nullptr;
    f.tw[i] = nullptr;
  }
  f = kw_ctx::fused_plan();
  return KW_OK;
}

kw_status kw_fused_create(kw_ctx* ctx) { return create_impl(ctx, nullptr, nullptr); }

kw_status kw_fused_create_with_scratch(kw_ctx* ctx, void* const s[3], void* const t[3])
{
  KW_CHECK_CTX(ctx);
  KW_REQUIRE(s != nullptr);
  return create_impl(ctx, s, t);
}

kw_status kw_fused_scratch_bytes(kw_ctx* ctx, size_t* out)
{
  KW_CHECK_CONSTS(ctx);
  KW_REQUIRE(out != nullptr);
  const uint32_t P = (ctx->c.nx_complex + NLMAX - 1) / NLMAX * NLMAX;
  *out             = static_cast<size_t>(P) * ctx->c.ny * ctx->c.nz * sizeof(float2);
  return KW_OK;
}

kw_status kw_fused_reduced_elems(kw_ctx* ctx, size_t* out)
{
  KW_FUSED_READY(ctx);
  KW_REQUIRE(out != nullptr);
  *out = static_cast<size_t>(ctx->fused.Palloc) * ctx->c.ny * ctx->c.nz;
  return KW_OK;
}

// src is [rows][nxc] with rows = ny*nz (one rank: [nz][ny]; slab mode: the transposed [nz_global][nyl]) — same count
kw_status kw_fused_import_reduced(kw_ctx* ctx, float* dst_padded, const float* src)
{
  KW_FUSED_READY(ctx);
  KW_REQUIRE(dst_padded && src);
  const kw_constants& c = ctx->c;
  // factorisation of the z lines, as the z-pass kernels are instantiated
  const bool split = (ctx->fused.nz_global == 512 && ctx->fused.split512);
  uint32_t r1 = Fac<256>::R1, r2 = Fac<256>::R2; // the split lines are built on the 256-point transform
  if (!split)
    switch (ctx->fused.nz_global)
    {
#define X(LEN) case LEN: r1 = Fac<LEN>::R1; r2 = Fac<LEN>::R2; break;
      KW_FUSED_LENGTHS(X)
#undef X
      default: kw_set_error("kw_fused_import_reduced: unsupported length %u", ctx->fused.nz_global); return KW_ERR_INVALID;
    }
  const uint32_t vec = static_cast<uint32_t>(op_vec(static_cast<int>(split ? 2 * r2 : r2)));
  const auto& f = ctx->fused;
  const size_t main_total = static_cast<size_t>(c.ny) * c.nz * f.P; // (f.P = row pitch of the main part: nxm rounded up to 16)
  KW_REQUIRE(f.nz_global <= 1024);
  // columns beyond the imported ones and the unused tail of the array read as zero
  KW_HIP(hipMemsetAsync(dst_padded, 0, static_cast<size_t>(f.Palloc) * c.ny * c.nz * sizeof(float), ctx->stream)); // = kw_fused_reduced_elems
  LAUNCH(k_import_reduced, dim3(f.nyl * (f.P / NLMAX)), dim3(256), dst_padded, src, c.nx_complex, f.nxm, f.P, f.nyl, f.nz_global,
         r1, vec, split ? 1u : 0u);
  if (f.side_off != 0)
  { // ceil(nyl / 16) tiles of 16 ky x nz values
    const size_t side_total = static_cast<size_t>((f.nyl + NLMAX - 1) / NLMAX) * NLMAX * f.nz_global;
    LAUNCH(k_import_reduced_side, dim3(ctx->cu_count * 2), dim3(256), dst_padded + main_total, src, c.nx_complex, f.nyl,
           f.nz_global, side_total, r1, vec, split ? 1u : 0u);
  }
  return KW_OK;
}

// A1-A4: u <- pml_sg*(pml_sg*u - dt/rho0_sg * ifftn(ddk_pos * kappa * fftn(p)) / N)
kw_status kw_fused_velocity(kw_ctx* ctx, const float* p, float* ux, float* uy, float* uz, const float* dtx,
                            const float* dty, const float* dtz, const float* pmlx, const float* pmly, const float* pmlz,
                            const float* kappa_padded, const float* ddx, const float* ddy, const float* ddz,
                            int chain_u_spectra)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_velocity");
  KW_REQUIRE(p && ux && uy && uz && pmlx && pmly && pmlz && kappa_padded && ddx && ddy && ddz);
  KW_REQUIRE((dtx == nullptr) == (dty == nullptr) && (dtx == nullptr) == (dtz == nullptr));
  float2** S = ctx->fused.s;
  const float* in1[1] = { p };
  const bool p_in_scratch = (chain_u_spectra & KW_FUSED_P_IN_SCRATCH) != 0;
  chain_u_spectra &= KW_FUSED_CHAIN_U;
  KW_TRY(forward_xy(ctx, 1, p_in_scratch ? nullptr : in1));
  ZArgs z{};
  z.in[0] = S[0];
  for (int i = 0; i < 3; i++) z.out[i] = S[i];
  z.op[0] = kappa_padded;
  z.dd[0] = (const float2*)ddx; z.dd[1] = (const float2*)ddy; z.dd[2] = (const float2*)ddz;
  KW_TRY(launch_zfused<Z_PGRAD>(ctx, 1, z));
  XinvArgs x{};
  float* u[3] = { ux, uy, uz };
  const float* dt[3] = { dtx, dty, dtz };
  const float* pml[3] = { pmlx, pmly, pmlz };
  for (int i = 0; i < 3; i++) { x.in[i] = S[i]; x.out[i] = u[i]; x.m0[i] = dt[i]; x.m1[i] = pml[i]; x.fout[i] = S[i]; }
  // whole-plane kernels: the block of u_x would overwrite the plane of Q that the block of u_y reads: its chained spectrum
  // goes to a fourth array, where the density stage picks it up
  if (ctx->fused.plane) x.fout[0] = ctx->fused.s4;
  // chained: the updated velocity rows are forward-transformed along x (and y) on the spot (valid as long as nothing
  // else writes u before kw_fused_density(..., KW_FUSED_U_IN_SCRATCH))
  if (chain_u_spectra) return gradient_tail<EPI_VELOCITY, true>(ctx, x, (const float2*)ddx, (const float2*)ddy);
  return gradient_tail<EPI_VELOCITY, false>(ctx, x, (const float2*)ddx, (const float2*)ddy);
}

// A12 second half: u <- +0.5*dt/rho0_sg * ifftn(ddk_pos * kappa * fftn(p)) / N
kw_status kw_fused_initial_velocity(kw_ctx* ctx, const float* p, float* ux, float* uy, float* uz, const float* dtx,
                                    const float* dty, const float* dtz, const float* kappa_padded, const float* ddx,
                                    const float* ddy, const float* ddz)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_initial_velocity");
  KW_REQUIRE(p && ux && uy && uz && kappa_padded && ddx && ddy && ddz);
  float2** S = ctx->fused.s;
  const float* in1[1] = { p };
  KW_TRY(forward_xy(ctx, 1, in1));
  ZArgs z{};
  z.in[0] = S[0];
  for (int i = 0; i < 3; i++) z.out[i] = S[i];
  z.op[0] = kappa_padded;
  z.dd[0] = (const float2*)ddx; z.dd[1] = (const float2*)ddy; z.dd[2] = (const float2*)ddz;
  KW_TRY(launch_zfused<Z_PGRAD>(ctx, 1, z));
  XinvArgs x{};
  float* u[3] = { ux, uy, uz };
  const float* dt[3] = { dtx, dty, dtz };
  for (int i = 0; i < 3; i++) { x.in[i] = S[i]; x.out[i] = u[i]; x.m0[i] = dt[i]; }
  return gradient_tail<EPI_INITVEL, false>(ctx, x, (const float2*)ddx, (const float2*)ddy);
}

// A6-A9 (+ the term kernels of A11 when terms != 0): du = ifftn(ddk_neg*kappa*fftn(u))/N; rho update; pressure terms
kw_status kw_fused_density(kw_ctx* ctx, int nonlinear, const float* ux, const float* uy, const float* uz, float* rx,
                           float* ry, float* rz, const float* pmlx, const float* pmly, const float* pmlz,
                           const float* rho0, const float* kappa_padded, const float* ddx, const float* ddy,
                           const float* ddz, float* duxdx, float* duydy, float* duzdz, int terms, const float* bona,
                           float* t0, float* t1, float* t2, int flags)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_density");
  const bool u_in_scratch = (flags & KW_FUSED_U_IN_SCRATCH) != 0;
  const bool chain_terms  = (flags & KW_FUSED_CHAIN_TERMS) != 0;
  KW_REQUIRE(!chain_terms || terms != 0);
  KW_REQUIRE(ux && uy && uz && rx && ry && rz && pmlx && pmly && pmlz && kappa_padded && ddx && ddy && ddz);
  KW_REQUIRE((duxdx == nullptr) == (duydy == nullptr) && (duxdx == nullptr) == (duzdz == nullptr));
  KW_REQUIRE(terms >= 0 && terms <= 6);
  KW_REQUIRE(terms == 0 || terms >= 3 || (t0 && t1 && (terms == 1 || t2)));
  KW_REQUIRE(!(terms == 3 || terms == 4) || t0 != nullptr);
  if (terms >= 5)
  { // one-term power law: `first` (t0 linear, t1 nonlinear) and, unless chained, the array the one term is stored in
    KW_REQUIRE(nonlinear ? t1 != nullptr : t0 != nullptr);
    KW_REQUIRE(chain_terms || (terms == 5 ? (nonlinear ? t2 : t1) != nullptr : t0 != nullptr));
  }
  float2** S = ctx->fused.s;
  const float* in3[3] = { ux, uy, uz };
  ZArgs z{};
  for (int i = 0; i < 3; i++) { z.in[i] = S[i]; z.out[i] = S[i]; }
  if (u_in_scratch && ctx->fused.plane) z.in[0] = ctx->fused.s4; // (see kw_fused_velocity)
  z.op[0] = kappa_padded;
  z.dd[0] = (const float2*)ddx; z.dd[1] = (const float2*)ddy; z.dd[2] = (const float2*)ddz;
  // 2-D: u_z is identically zero; its spectrum travels as zeros (chained stages leave G_y of the velocity stage in S[2])
  if (ctx->fused.two_d && u_in_scratch)
    KW_HIP(hipMemsetAsync(S[2], 0, static_cast<size_t>(ctx->fused.Palloc) * ctx->c.ny * sizeof(float2), ctx->stream));
  if (ctx->fused.slab)
  {
    KW_TRY(slab_chain<Z_VGRAD>(ctx, 3, u_in_scratch ? nullptr : in3, z));
  }
  else
  {
    KW_TRY(forward_xy(ctx, 3, u_in_scratch ? nullptr : in3));
    KW_TRY(launch_zfused<Z_VGRAD>(ctx, 3, z));
  }
  const bool tail_chunked = (!ctx->fused.slab && !ctx->fused.two_d);
  XinvArgs x{};
  float* rho[3] = { rx, ry, rz };
  const float* pml[3] = { pmlx, pmly, pmlz };
  float* du[3] = { duxdx, duydy, duzdz };
  float* t[3] = { t0, t1, t2 };
  for (int i = 0; i < 3; i++) { x.in[i] = S[i]; x.out[i] = rho[i]; x.m1[i] = pml[i]; x.aux[i] = du[i]; x.t[i] = t[i]; }
  x.m0[0]     = rho0;
  x.m0[1]     = bona;
  x.m0[2]     = (terms == 3 || terms == 4) ? t1 : nullptr; // lossless / Stokes pressure: t0 = p (out), t1 = c2 array or NULL (in),
                                             // Stokes: t2 = absorb_tau array or NULL (in; travels as x.t[2], never written)
  x.nonlinear = nonlinear;
  x.terms     = terms;
  x.which     = (terms == 6) ? 1 : 0; // one-term power law: 5 no_dispersion, 6 no_absorption — one kernel set (TERMS == 5)
  x.fout[0]   = S[0]; // chained: x-spectrum of rho0 * sum(du) (terms == 6: of sum(rho), the one chained array)
  x.fout[1]   = S[1]; //          x-spectrum of sum(rho)
  // one specialised kernel per pressure-term mode
#define DENSITY_TAIL(T)                                                                                                \
  do {                                                                                                                 \
    if (tail_chunked)                                                                                                  \
    {                                                                                                                  \
      if (chain_terms) KW_TRY((plane_local_tail<EPI_DENSITY, true, (T) == 0 ? 1 : (T)>(ctx, 3, 1, x, (T) >= 3 ? 1 : 2))); \
      else KW_TRY((plane_local_tail<EPI_DENSITY, false, (T)>(ctx, 3, 1, x, 0)));                                       \
    }                                                                                                                  \
    else if (ctx->fused.pipelined)                                                                                     \
    {                                                                                                                  \
      if (chain_terms) KW_TRY((pslab_tail<EPI_DENSITY, true, (T) == 0 ? 1 : (T)>(ctx, 3, 1, x, (T) >= 3 ? 1 : 2)));    \
      else KW_TRY((pslab_tail<EPI_DENSITY, false, (T)>(ctx, 3, 1, x, 0)));                                             \
    }                                                                                                                  \
    else if (chain_terms) KW_TRY((launch_xinv<EPI_DENSITY, true, (T) == 0 ? 1 : (T)>(ctx, 1, x)));                      \
    else KW_TRY((launch_xinv<EPI_DENSITY, false, (T)>(ctx, 1, x)));                                                    \
  } while (0)
  switch (terms)
  {
    case 0: DENSITY_TAIL(0); break; // (chain_terms requires terms != 0: checked above)
    case 1: DENSITY_TAIL(1); break;
    case 2: DENSITY_TAIL(2); break;
    case 3: DENSITY_TAIL(3); break;
    case 4: DENSITY_TAIL(4); break;
    default: DENSITY_TAIL(5); break;
  }
#undef DENSITY_TAIL
  return KW_OK;
}

// A6-A8 only: du_i/dx_i = ifftn(ddk_i_neg * kappa * fftn(u_i)) / N stored as arrays — for callers that put something
// between the gradient and the density update (non-uniform grids: duxdx *= dxudxn, SolverCudaKernels.cu:1285-1301)
kw_status kw_fused_velocity_gradient(kw_ctx* ctx, const float* ux, const float* uy, const float* uz, float* duxdx,
                                     float* duydy, float* duzdz, const float* kappa_padded, const float* ddx, const float* ddy,
                                     const float* ddz, int flags)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_velocity_gradient");
  KW_REQUIRE(ux && uy && uz && duxdx && duydy && duzdz && kappa_padded && ddx && ddy && ddz);
  const bool u_in_scratch = (flags & KW_FUSED_U_IN_SCRATCH) != 0;
  float2** S = ctx->fused.s;
  const float* in3[3] = { ux, uy, uz };
  ZArgs z{};
  for (int i = 0; i < 3; i++) { z.in[i] = S[i]; z.out[i] = S[i]; }
  if (u_in_scratch && ctx->fused.plane) z.in[0] = ctx->fused.s4; // (see kw_fused_velocity)
  z.op[0] = kappa_padded;
  z.dd[0] = (const float2*)ddx; z.dd[1] = (const float2*)ddy; z.dd[2] = (const float2*)ddz;
  if (ctx->fused.two_d && u_in_scratch)
    KW_HIP(hipMemsetAsync(S[2], 0, static_cast<size_t>(ctx->fused.Palloc) * ctx->c.ny * sizeof(float2), ctx->stream));
  if (ctx->fused.slab) KW_TRY(slab_chain<Z_VGRAD>(ctx, 3, u_in_scratch ? nullptr : in3, z));
  else
  {
    KW_TRY(forward_xy(ctx, 3, u_in_scratch ? nullptr : in3));
    KW_TRY(launch_zfused<Z_VGRAD>(ctx, 3, z));
    KW_TRY(inverse_y(ctx, 3));
  }
  XinvArgs x{};
  float* du[3] = { duxdx, duydy, duzdz };
  for (int i = 0; i < 3; i++) { x.in[i] = S[i]; x.out[i] = du[i]; }
  if (ctx->fused.slab && ctx->fused.pipelined) return pslab_tail<EPI_STORE, false>(ctx, 3, 3, x, 0);
  return launch_xinv<EPI_STORE>(ctx, 3, x);
}

// A11 absorbing branch after the terms: p = c2*(first + d*(tau*ifftn(nabla1*fftn(vel_grad_term)) - eta*ifftn(nabla2*fftn(density_sum))))
kw_status kw_fused_absorption_pressure(kw_ctx* ctx, float* p, const float* vel_grad_term, const float* density_sum,
                                       const float* first, const float* nabla1_padded, const float* nabla2_padded,
                                       const float* c2, const float* tau, const float* eta, int flags)
{
  const bool terms_in_scratch = (flags & KW_FUSED_TERMS_IN_SCRATCH) != 0;
  const bool chain_p          = (flags & KW_FUSED_CHAIN_P) != 0;
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_absorption_pressure");
  KW_REQUIRE(p && first && nabla1_padded && nabla2_padded);
  KW_REQUIRE(terms_in_scratch || (vel_grad_term && density_sum));
  KW_REQUIRE((tau == nullptr) == (eta == nullptr));
  float2** S = ctx->fused.s;
  const float* in2[2] = { vel_grad_term, density_sum };
  ZArgs z{};
  for (int i = 0; i < 2; i++) { z.in[i] = S[i]; z.out[i] = S[i]; }
  z.op[0] = nabla1_padded;
  z.op[1] = nabla2_padded;
  if (ctx->fused.slab)
  {
    KW_TRY(slab_chain<Z_ABSORB>(ctx, 2, terms_in_scratch ? nullptr : in2, z));
  }
  else
  {
    KW_TRY(forward_xy(ctx, 2, terms_in_scratch ? nullptr : in2));
    KW_TRY(launch_zfused<Z_ABSORB>(ctx, 2, z));
  }
  XinvArgs x{};
  x.in[0] = S[0]; x.in[1] = S[1];
  x.out[0] = p;
  x.m0[0] = first; x.m0[1] = c2;
  x.m1[0] = tau;   x.m1[1] = eta;
  x.fout[0] = S[0]; // chained: x-spectrum of the new p
  if (!ctx->fused.slab && !ctx->fused.two_d)
  {
    if (chain_p) KW_TRY((plane_local_tail<EPI_PSUM, true>(ctx, 2, 1, x, 1)));
    else KW_TRY((plane_local_tail<EPI_PSUM, false>(ctx, 2, 1, x, 0)));
  }
  else if (ctx->fused.slab && ctx->fused.pipelined)
  {
    if (chain_p) KW_TRY((pslab_tail<EPI_PSUM, true>(ctx, 2, 1, x, 1)));
    else KW_TRY((pslab_tail<EPI_PSUM, false>(ctx, 2, 1, x, 0)));
  }
  else if (chain_p) KW_TRY((launch_xinv<EPI_PSUM, true>(ctx, 1, x)));
  else KW_TRY(launch_xinv<EPI_PSUM>(ctx, 1, x));
  return KW_OK;
}

// The absorbing branch with one term (absorbing_flag 3 / 4): p = c2*(first + d*(tau*ifftn(nabla1*fftn(term)))) for which == 0
// (no_dispersion: term = rho0 * sum du), p = c2*(first - d*(eta*ifftn(nabla2*fftn(term)))) for which == 1 (no_absorption:
// term = sum rho) — one array through every pass of the stage, one exchange each way on slabs
kw_status kw_fused_absorption_pressure_one(kw_ctx* ctx, float* p, const float* term, const float* first,
                                           const float* nabla_padded, const float* c2, const float* coef, int which, int flags)
{
  const bool terms_in_scratch = (flags & KW_FUSED_TERMS_IN_SCRATCH) != 0;
  const bool chain_p          = (flags & KW_FUSED_CHAIN_P) != 0;
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_absorption_pressure_one");
  KW_REQUIRE(p && first && nabla_padded);
  KW_REQUIRE(terms_in_scratch || term != nullptr);
  KW_REQUIRE(which == 0 || which == 1);
  KW_REQUIRE((flags & ~(KW_FUSED_TERMS_IN_SCRATCH | KW_FUSED_CHAIN_P)) == 0);
  float2** S = ctx->fused.s;
  const float* in1[1] = { term };
  ZArgs z{};
  z.in[0] = S[0]; z.out[0] = S[0];
  z.op[0] = nabla_padded;
  if (ctx->fused.slab)
  {
    KW_TRY(slab_chain<Z_ABSORB>(ctx, 1, terms_in_scratch ? nullptr : in1, z));
  }
  else
  {
    KW_TRY(forward_xy(ctx, 1, terms_in_scratch ? nullptr : in1));
    KW_TRY(launch_zfused<Z_ABSORB>(ctx, 1, z));
  }
  XinvArgs x{};
  x.in[0] = S[0];
  x.out[0] = p;
  x.m0[0] = first; x.m0[1] = c2;
  x.m1[0] = coef;
  x.which = which;
  x.fout[0] = S[0]; // chained: x-spectrum of the new p
  if (!ctx->fused.slab && !ctx->fused.two_d)
  {
    if (chain_p) KW_TRY((plane_local_tail<EPI_PSUM1, true>(ctx, 1, 1, x, 1)));
    else KW_TRY((plane_local_tail<EPI_PSUM1, false>(ctx, 1, 1, x, 0)));
  }
  else if (ctx->fused.slab && ctx->fused.pipelined)
  {
    if (chain_p) KW_TRY((pslab_tail<EPI_PSUM1, true>(ctx, 1, 1, x, 1)));
    else KW_TRY((pslab_tail<EPI_PSUM1, false>(ctx, 1, 1, x, 0)));
  }
  else if (chain_p) KW_TRY((launch_xinv<EPI_PSUM1, true>(ctx, 1, x)));
  else KW_TRY(launch_xinv<EPI_PSUM1>(ctx, 1, x));
  return KW_OK;
}

// The Z_SHIFT pass of kw_fused_shift_velocity: the real array is read as nx/2 complex columns (no side array); `lines`
// lines of `len` elements along `axis`, whose elements are lrows rows of nx/2 apart and whose neighbours brows rows.
// (Z_SHIFT reads neither ZArgs::ny nor ::nz.)
static kw_status launch_zshift(kw_ctx* ctx, const float* in, float* out, const float* filter, int axis, uint32_t len, uint32_t lines,
                        uint32_t lrows, uint32_t brows)
{
  ZArgs z{};
  z.in[0]   = reinterpret_cast<const float2*>(in);
  z.out[0]  = reinterpret_cast<float2*>(out);
  z.dd[2]   = reinterpret_cast<const float2*>(filter);
  z.tw      = ctx->fused.tw[axis];
  z.nxc     = ctx->c.nx / 2;
  z.P       = ctx->c.nx / 2;
  z.narr    = 1;
  z.lstride = lrows * z.P;
  z.bstride = brows * z.P;
  return KW_LAUNCH_ZPASS((k_zfused<LEN, Z_SHIFT>), len, dim3(z_tiles(z.nxc, len), lines, 1), z);
}

// computeVelocityShiftInX/Y/Z + the two 1-D transforms around it (KSpaceFirstOrderSolver.cpp:2714-2735,
// SolverCudaKernels.cu:2617-2710) in one kernel per axis: out = F_axis^-1{ H .* F_axis{in} }, H = full-length Hermitian
// filter with the 1/N of the transform pair folded in (see kwave_hip.h)
kw_status kw_fused_shift_velocity(kw_ctx* ctx, int axis, const float* in, float* out, const float* filter)
{
  KW_FUSED_READY(ctx);
  auto& f = ctx->fused;
  const kw_constants& c = ctx->c;
  KW_REQUIRE(axis >= 0 && axis <= 2 && in != nullptr && out != nullptr && filter != nullptr);
  static const char* const names[3] = { "k_xshift", "k_zfused_shift_y", "k_zfused_shift_z" };
  KW_PROF(ctx, names[axis]);
  if (f.slab && axis == 2)
  { // lines along z cross the slabs: the real array travels as [nz local][ny / P rows per peer][nx] chunks to the
    // owner of each row range ([nz global][nyl][nx] there), is shifted along z and travels back — two exchanges of one
    // real array per sampled step (KSpaceFirstOrderSolver.cpp:2731-2733 on the decomposed grid).  x and y lines are
    // slab-local.  Staging: scratch pair 1 (only S[0] carries a chained spectrum between stages).
    const uint32_t nyl = f.nyl, nzl = c.nz, P = f.nranks;
    const size_t   row = static_cast<size_t>(c.nx) * sizeof(float), chunk = static_cast<size_t>(nzl) * nyl * c.nx;
    float* snd = reinterpret_cast<float*>(f.s[1]);
    float* rcv = reinterpret_cast<float*>(f.t[1]);
    for (uint32_t q = 0; q < P; q++)
      KW_HIP(hipMemcpy2DAsync(snd + q * chunk, nyl * row, in + static_cast<size_t>(q) * nyl * c.nx, c.ny * row, nyl * row, nzl,
                              hipMemcpyDeviceToDevice, ctx->stream));
    KW_TRY(xstart_bytes(ctx, KW_ZSHIFT_SLOT, snd, rcv, chunk * sizeof(float)));
    KW_TRY(xwait_one(ctx, KW_ZSHIFT_SLOT));
    KW_TRY(launch_zshift(ctx, rcv, rcv, filter, 2, f.nz_global, nyl, nyl, 1));
    KW_TRY(xstart_bytes(ctx, KW_ZSHIFT_SLOT, rcv, snd, chunk * sizeof(float)));
    KW_TRY(xwait_one(ctx, KW_ZSHIFT_SLOT));
    for (uint32_t q = 0; q < P; q++)
      KW_HIP(hipMemcpy2DAsync(out + static_cast<size_t>(q) * nyl * c.nx, c.ny * row, snd + q * chunk, nyl * row, nyl * row, nzl,
                              hipMemcpyDeviceToDevice, ctx->stream));
    return KW_OK;
  }
  if (axis == 0)
  {
    XshiftArgs a{ in, out, f.tw[0], reinterpret_cast<const float2*>(filter), c.ny * c.nz, 0u };
    const uint32_t rows_per_tile = 2u * static_cast<uint32_t>(nl_x(c.nx)), full = a.nrows / rows_per_tile;
    if (full > 0)
    {
      const dim3 grid(full, 1, 1);
#define M(LEN) LAUNCH((k_xshift<LEN, false>), grid, dim3(GeoX<LEN>::THREADS), a)
      KW_LEN_SWITCH(c.nx, M)
#undef M
    }
    if (a.nrows % rows_per_tile != 0)
    {
      a.tile0 = full;
#define M(LEN) if constexpr (!has_partial_x_tiles(LEN)) KW_NO_TAIL(LEN) else LAUNCH((k_xshift<LEN, true>), dim3(1, 1, 1), dim3(GeoX<LEN>::THREADS), a)
      KW_LEN_SWITCH(c.nx, M)
#undef M
    }
    return KW_OK;
  }
  // y / z: the real array is read as nx/2 complex columns; lines run along the axis with the matching stride
  if (axis == 1) return launch_zshift(ctx, in, out, filter, 1, c.ny, c.nz, 1, c.ny);
  return launch_zshift(ctx, in, out, filter, 2, c.nz, c.ny, c.ny, 1);
}

// The stages that run on one GPU and a 3-D grid only refuse anything else here; `what` names what the stage works on.
static kw_status single_gpu_only(const kw_ctx* ctx, const char* name, const char* what = "3-D only")
{
  if (!(ctx->fused.slab || ctx->fused.two_d)) return KW_OK;
  kw_set_error("%s: single GPU and %s (no Z-slabs, no Nz == 1)", name, what);
  return KW_ERR_INVALID;
}

// scratch array 0 -> the real array `out`: the storing x-inverse, after the y-inverse where the stage has one
static kw_status store_scratch0(kw_ctx* ctx, float* out, bool y_inverse = true)
{
  if (y_inverse) KW_TRY(inverse_y(ctx, 1));
  XinvArgs x{};
  x.in[0]  = ctx->fused.s[0];
  x.out[0] = out;
  return launch_xinv<EPI_STORE>(ctx, 1, x);
}

// scaleSource body (KSpaceFirstOrderSolver.cpp:2346-2351): scaled <- ifftn(sourceKappa*fftn(scaled))/N, in place
kw_status kw_fused_scale_source(kw_ctx* ctx, float* scaled, const float* source_kappa_padded)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_scale_source");
  KW_REQUIRE(scaled && source_kappa_padded);
  float2** S = ctx->fused.s;
  const float* in1[1] = { scaled };
  KW_TRY(forward_xy(ctx, 1, in1));
  ZArgs z{};
  z.in[0] = S[0]; z.out[0] = S[0];
  z.op[0] = source_kappa_padded;
  KW_TRY(launch_zfused<Z_SOURCE>(ctx, 1, z));
  return store_scratch0(ctx, scaled);
}

// CW field propagator (kw_cw.hip): the complex field re + i im through one 3-D round trip with the complex operator
// G = g_re + i g_im (real, reduced, imported: a function of |k|), as two real transforms —
//   re <- ifftn(g_re fftn(re) - g_im fftn(im)),   im <- ifftn(g_im fftn(re) + g_re fftn(im)),   in place;
// the operators carry the 1/N.  kw_fused_scale_source's schedule with two arrays and the pair kernel as its z-pass.
kw_status kw_fused_cw_pair(kw_ctx* ctx, float* re, float* im, const float* g_re_padded, const float* g_im_padded)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_cw_pair");
  KW_REQUIRE(re && im && g_re_padded && g_im_padded && re != im);
  KW_TRY(single_gpu_only(ctx, __func__));
  float2** S = ctx->fused.s;
  const float* in2[2] = { re, im };
  KW_TRY(forward_xy(ctx, 2, in2));
  ZArgs z{};
  for (int i = 0; i < 2; i++) { z.in[i] = S[i]; z.out[i] = S[i]; }
  z.op[0] = g_re_padded;
  z.op[1] = g_im_padded;
  KW_TRY(zfused_pair(ctx, z));
  KW_TRY(inverse_y(ctx, 2));
  XinvArgs x{};
  x.in[0] = S[0]; x.in[1] = S[1];
  x.out[0] = re;  x.out[1] = im;
  KW_TRY(launch_xinv<EPI_STORE>(ctx, 2, x));
  return KW_OK;
}

// Angular-spectrum projector (kw_angular.hip).  The source plane is transformed once: x-forward of the leading planes of
// re / im that make whole x tiles (plane 0 holds the source; the others ride along and are dropped), the forward y-pass of
// plane 0 alone, and a copy of that plane's rows and side column into the compact 2-D spectra
// (kw_fused_angular_elems complex values each).
kw_status kw_fused_angular_elems(kw_ctx* ctx, size_t* out)
{
  KW_FUSED_READY(ctx);
  KW_REQUIRE(out != nullptr);
  const auto& f = ctx->fused;
  *out = static_cast<size_t>(f.P) * ctx->c.ny + (f.side_off != 0 ? ctx->c.ny : 0u);
  return KW_OK;
}

kw_status kw_fused_angular_forward(kw_ctx* ctx, const float* re, const float* im, float* spec_re, float* spec_im)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_angular_forward");
  KW_REQUIRE(re && im && spec_re && spec_im && spec_re != spec_im);
  KW_TRY(single_gpu_only(ctx, __func__, "a chunk of planes only"));
  const kw_constants& c = ctx->c;
  const auto& f = ctx->fused;
  const uint32_t rows_per_tile = 2u * static_cast<uint32_t>(nl_x(c.nx));
  uint32_t np = 1;
  while (np < c.nz && (c.ny * np) % rows_per_tile != 0) np++; // whole x tiles: no masked tile is ever needed
  const float* in2[2] = { re, im };
  KW_TRY(launch_xfwd(ctx, 2, in2, f.s, np));
  KW_TRY(launch_ypass(ctx, -1, 2, f.s, f.s, false, false, 0, 1));
  float* const spec[2] = { spec_re, spec_im };
  const size_t main_elems = static_cast<size_t>(f.P) * c.ny;
  for (int i = 0; i < 2; i++)
  {
    float2* dst = reinterpret_cast<float2*>(spec[i]);
    KW_HIP(hipMemcpyAsync(dst, f.s[i], main_elems * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
    if (f.side_off != 0)
      KW_HIP(hipMemcpyAsync(dst + main_elems, f.s[i] + f.side_off, c.ny * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return KW_OK;
}

// One chunk of planes: planes j0 ... j0 + Nz - 1 (Nz = the context's plane count) of
//   re + i im <- ifft2( (spec_re^ + i spec_im^) H(., ., z_j) )
// as k_yinv_angular (H from the imported tables, the 2x2 mix, both y-inverses) and the x-inverse of the two arrays.
kw_status kw_fused_angular_planes(kw_ctx* ctx, const float* spec_re, const float* spec_im, const uint32_t* tables_imported,
                                  uint32_t j0, float* re, float* im)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_angular_planes");
  KW_REQUIRE(spec_re && spec_im && tables_imported && re && im && re != im);
  KW_REQUIRE(static_cast<uint64_t>(j0) + ctx->c.nz <= (1ull << 31));
  KW_TRY(single_gpu_only(ctx, __func__, "a chunk of planes only"));
  float2** S = ctx->fused.s;
  AngArgs a{};
  a.in[0]  = reinterpret_cast<const float2*>(spec_re);
  a.in[1]  = reinterpret_cast<const float2*>(spec_im);
  a.out[0] = S[0];
  a.out[1] = S[1];
  a.tab    = tables_imported;
  a.j0     = j0;
  KW_TRY(yinv_angular(ctx, a));
  XinvArgs x{};
  x.in[0] = S[0]; x.in[1] = S[1];
  x.out[0] = re;  x.out[1] = im;
  KW_TRY(launch_xinv<EPI_STORE>(ctx, 2, x));
  return KW_OK;
}

// Time-domain angular-spectrum projector (kw_angular_time.hip).  The record [Lt][Ey][Ex] is transformed along x and y once
// and the (kx, ky, t) half-spectrum kept aside; every plane is kw_fused_scale_source's second half with k_zfused_time as
// its z-pass, reading the kept spectrum.
// complex values of a kept half-spectrum: scratch array 0, side array included
static size_t kept_elems(const kw_ctx* ctx) { return static_cast<size_t>(ctx->fused.Palloc) * ctx->c.ny * ctx->c.nz; }

kw_status kw_fused_angular_time_elems(kw_ctx* ctx, size_t* out)
{
  KW_FUSED_READY(ctx);
  KW_REQUIRE(out != nullptr);
  *out = kept_elems(ctx);
  return KW_OK;
}

// kept <- the (kx, ky, z) half-spectrum of vol: the x- and y-forward of the one array, then a copy of scratch array 0, side
// array included (kw_fused_angular_time_forward and kw_fused_second_order_forward, after their own checks)
static kw_status keep_forward_xy(kw_ctx* ctx, const float* vol, float* kept)
{
  const float* in1[1] = { vol };
  KW_TRY(forward_xy(ctx, 1, in1));
  KW_HIP(hipMemcpyAsync(kept, ctx->fused.s[0], kept_elems(ctx) * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
  return KW_OK;
}

kw_status kw_fused_angular_time_forward(kw_ctx* ctx, const float* vol, float* kept)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_angular_time_forward");
  KW_REQUIRE(vol && kept);
  KW_TRY(single_gpu_only(ctx, __func__));
  return keep_forward_xy(ctx, vol, kept);
}

kw_status kw_fused_angular_time_plane(kw_ctx* ctx, const float* kept, const kw_angular_time_op* op, float* vol_out)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_angular_time_plane");
  KW_REQUIRE(kept && op && vol_out);
  KW_TRY(single_gpu_only(ctx, __func__));
  KW_REQUIRE(op->dx > 0.0 && op->dy > 0.0 && op->dt > 0.0 && op->c0 > 0.0 && op->z >= 0.0);
  KW_TRY(zfused_time(ctx, reinterpret_cast<const float2*>(kept), ctx->fused.s[0], op));
  return store_scratch0(ctx, vol_out);
}

// Exact k-space propagator (kw_second_order.hip): the projector's shape with the volume's own z axis — the (kx, ky, z)
// half-spectrum of the embedded p0 kept aside, every output time one z-pass k_zfused_second_order that reads it, the
// y-inverse and the storing x-inverse.
kw_status kw_fused_second_order_elems(kw_ctx* ctx, size_t* out)
{
  KW_FUSED_READY(ctx);
  KW_REQUIRE(out != nullptr);
  *out = kept_elems(ctx);
  return KW_OK;
}

kw_status kw_fused_second_order_forward(kw_ctx* ctx, const float* vol, float* kept)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_second_order_forward");
  KW_REQUIRE(vol && kept);
  KW_TRY(single_gpu_only(ctx, __func__));
  return keep_forward_xy(ctx, vol, kept);
}

kw_status kw_fused_second_order_time(kw_ctx* ctx, const float* kept, const kw_second_order_op* op, float* vol_out)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_second_order_time");
  KW_REQUIRE(kept && op && vol_out);
  KW_TRY(single_gpu_only(ctx, __func__));
  KW_REQUIRE(op->dx > 0.0 && op->dy > 0.0 && op->dz > 0.0 && op->c0 > 0.0 && op->t >= 0.0);
  KW_REQUIRE(op->absorbing == 0 || (op->a >= 0.0 && op->alpha_power >= 0.0 && op->alpha_power != 1.0));
  KW_TRY(zfused_second_order(ctx, reinterpret_cast<const float2*>(kept), ctx->fused.s[0], op));
  return store_scratch0(ctx, vol_out);
}

// The same stage with dp0/dt as a second initial condition (kw_second_order_pair.hip): `kept_v` is the kept spectrum of the
// embedded dp0dt (kw_fused_second_order_forward into an array of its own); k_zfused_second_order_pair carries both forward,
// mixes them in registers and runs one inverse, so the y-inverse and the x-inverse are the single stage's.
kw_status kw_fused_second_order_time_pair(kw_ctx* ctx, const float* kept_p, const float* kept_v, const kw_second_order_op* op,
                                          float* vol_out)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_second_order_time_pair");
  KW_REQUIRE(kept_p && kept_v && op && vol_out);
  KW_TRY(single_gpu_only(ctx, __func__));
  KW_REQUIRE(op->dx > 0.0 && op->dy > 0.0 && op->dz > 0.0 && op->c0 > 0.0 && op->t >= 0.0);
  KW_REQUIRE(op->absorbing == 0 || (op->a >= 0.0 && op->alpha_power >= 0.0 && op->alpha_power != 1.0));
  KW_TRY(zfused_second_order_pair(ctx, reinterpret_cast<const float2*>(kept_p), reinterpret_cast<const float2*>(kept_v),
                                  ctx->fused.s[0], op));
  return store_scratch0(ctx, vol_out);
}

// k-space plane reconstruction (kw_plane_recon.hip): kw_fused_scale_source's round trip with k_zfused_recon as its z-pass —
// the weight and the gather from w to kz happen along the line the z-pass holds in LDS.
kw_status kw_fused_plane_recon(kw_ctx* ctx, const float* vol_even, const kw_plane_recon_op* op, float* vol_out)
{
  KW_FUSED_READY(ctx);
  KW_PROF(ctx, "fused_plane_recon");
  KW_REQUIRE(vol_even && op && vol_out);
  KW_TRY(single_gpu_only(ctx, __func__));
  KW_REQUIRE(op->dx > 0.0 && op->dy > 0.0 && op->dt > 0.0 && op->c0 > 0.0 && (op->interp == 0 || op->interp == 1));
  const float* in1[1] = { vol_even };
  KW_TRY(forward_xy(ctx, 1, in1));
  KW_TRY(zfused_recon(ctx, ctx->fused.s[0], op));
  return store_scratch0(ctx, vol_out);
}

// Batched k-space line reconstruction (kw_line_recon.hip), frames mode: the x-forward over all Ny * Nz rows, ONE launch of
// k_yfused_line_recon (forward along t, weight, gather, inverse along t, each frame's lines apart), the storing x-inverse.
kw_status kw_fused_line_recon(kw_ctx* ctx, const float* vol_even, const kw_plane_recon_op* op, float* vol_out)
{
  KW_CHECK_CONSTS(ctx);
  if (!ctx->fused.ready) { kw_set_error("kw_fused_line_recon: kw_fused_create has not been called"); return KW_ERR_STATE; }
  KW_PROF(ctx, "fused_line_recon");
  KW_REQUIRE(vol_even && op && vol_out);
  if (!ctx->fused.frames)
  {
    kw_set_error("kw_fused_line_recon: needs a context in frames mode (kw_fused_set_frames before kw_fused_create)");
    return KW_ERR_INVALID;
  }
  KW_REQUIRE(op->dx > 0.0 && op->dt > 0.0 && op->c0 > 0.0 && (op->interp == 0 || op->interp == 1));
  float2** S = ctx->fused.s;
  const float* in1[1] = { vol_even };
  KW_TRY(launch_xfwd(ctx, 1, in1, S));
  KW_TRY(yfused_line_recon(ctx, S[0], op));
  return store_scratch0(ctx, vol_out, false);
}

// Batched 2-D exact k-space propagator (kw_second_order.hip), frames mode: F planes [Ey][Ex], no transform along z.  The
// (kx, y, frame) half-spectrum of the embedded p0 is kept aside; every output time is ONE launch of k_yfused_second_order
// that reads it (forward along y, H, inverse along y into scratch array 0) and the storing x-inverse.
#define KW_FRAMES_STAGE_READY(ctx)                                                                                     \
  do {                                                                                                                 \
    KW_CHECK_CONSTS(ctx);                                                                                              \
    if (!(ctx)->fused.ready) { kw_set_error("%s: kw_fused_create has not been called", __func__); return KW_ERR_STATE; } \
    if (!(ctx)->fused.frames)                                                                                          \
    {                                                                                                                  \
      kw_set_error("%s: needs a context in frames mode (kw_fused_set_frames before kw_fused_create)", __func__);       \
      return KW_ERR_INVALID;                                                                                           \
    }                                                                                                                  \
  } while (0)

kw_status kw_fused_second_order_frames_elems(kw_ctx* ctx, size_t* out)
{
  KW_FRAMES_STAGE_READY(ctx);
  KW_REQUIRE(out != nullptr);
  *out = kept_elems(ctx);
  return KW_OK;
}

kw_status kw_fused_second_order_frames_forward(kw_ctx* ctx, const float* vol, float* kept)
{
  KW_FRAMES_STAGE_READY(ctx);
  KW_PROF(ctx, "fused_second_order_frames_forward");
  KW_REQUIRE(vol && kept);
  const float* in1[1] = { vol };
  KW_TRY(launch_xfwd(ctx, 1, in1, ctx->fused.s));
  KW_HIP(hipMemcpyAsync(kept, ctx->fused.s[0], kept_elems(ctx) * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
  return KW_OK;
}

kw_status kw_fused_second_order_frames_time(kw_ctx* ctx, const float* kept, const kw_second_order_op* op, float* vol_out)
{
  KW_FRAMES_STAGE_READY(ctx);
  KW_PROF(ctx, "fused_second_order_frames_time");
  KW_REQUIRE(kept && op && vol_out);
  KW_REQUIRE(op->dx > 0.0 && op->dy > 0.0 && op->c0 > 0.0 && op->t >= 0.0); // (dz is not looked at)
  KW_REQUIRE(op->absorbing == 0 || (op->a >= 0.0 && op->alpha_power >= 0.0 && op->alpha_power != 1.0));
  KW_TRY(yfused_second_order(ctx, reinterpret_cast<const float2*>(kept), ctx->fused.s[0], op));
  return store_scratch0(ctx, vol_out, false);
}

// with dp0/dt: ONE launch of k_yfused_second_order_pair over both kept spectra and the storing x-inverse
kw_status kw_fused_second_order_frames_time_pair(kw_ctx* ctx, const float* kept_p, const float* kept_v,
                                                 const kw_second_order_op* op, float* vol_out)
{
  KW_FRAMES_STAGE_READY(ctx);
  KW_PROF(ctx, "fused_second_order_frames_time_pair");
  KW_REQUIRE(kept_p && kept_v && op && vol_out);
  KW_REQUIRE(op->dx > 0.0 && op->dy > 0.0 && op->c0 > 0.0 && op->t >= 0.0); // (dz is not looked at)
  KW_REQUIRE(op->absorbing == 0 || (op->a >= 0.0 && op->alpha_power >= 0.0 && op->alpha_power != 1.0));
  KW_TRY(yfused_second_order_pair(ctx, reinterpret_cast<const float2*>(kept_p), reinterpret_cast<const float2*>(kept_v),
                                  ctx->fused.s[0], op));
  return store_scratch0(ctx, vol_out, false);
}

// Pass-level probe for tuning (tools/probe_passes.py): launches ONE pass over the scratch arrays, no physics.
//   0: y-pass forward on s[0] (in place)          1: the same line kernel along z (stride ny*P) on s[0]
//   2: z-fused (forward, x sourceKappa-style multiply with op, inverse) on s[0]   3: y-pass on s[0..2] (3 arrays)
// `op` = a padded reduced real array (e.g. kappa).  Single rank only.  The others (10-16, 20-23, 30-37: memory patterns
// of a pass without its arithmetic) are in kw_fused_probe.hip.
kw_status kw_fused_probe(kw_ctx* ctx, int which, const float* op)
{
  KW_FUSED_READY(ctx);
  auto& f = ctx->fused;
  KW_REQUIRE(!f.slab);
  const kw_constants& c = ctx->c;
  if (which == 0) return launch_ypass(ctx, -1, 1, f.s, f.s, false, false);
  if (which == 3) return launch_ypass(ctx, -1, 3, f.s, f.s, false, false);
  if (which == 1)
  {
    KW_REQUIRE(c.nz == c.ny); // same line-length template
    PassArgs a{};
    a.in[0] = f.s[0]; a.out[0] = f.s[0];
    a.tw  = f.tw[2];
    a.nxc = f.nxm;
    a.P   = f.P;
    a.narr = 1;
    a.ain = a.aout = RowAddr{0u, 0u, 0u, 1u, c.ny}; // element k of line (ky = blockIdx.y): row k*ny + ky
    const dim3 grid(f.P / nl_yz(c.nz), c.ny, 1);
#define M(LEN) LAUNCH((k_ypass<LEN, kFwd, false, false>), grid, dim3(Geo<LEN>::THREADS), a)
    KW_LEN_SWITCH(c.nz, M)
#undef M
    return KW_OK;
  }
  if (which == 2)
  {
    KW_REQUIRE(op != nullptr);
    ZArgs z{};
    z.in[0] = f.s[0]; z.out[0] = f.s[0];
    z.op[0] = op;
    return launch_zfused<Z_SOURCE>(ctx, 1, z);
  }
  return probe_patterns(ctx, which, op);
}

} // extern "C"
