// kw_fused.hip — the MI355X-fused spectral pipeline: hand-written 3-D FFT passes with the element-wise physics
// folded into them.  This is the fast path of the per-step loop; it computes exactly the stages of
// KSpaceFirstOrderSolver::computeVelocity / computeVelocityGradient / computeDensity* / computePressure*
// (KSpaceSolver/KSpaceFirstOrderSolver.cpp:2087-2245) with the arithmetic of the SolverCudaKernels.cu lines cited at
// each epilogue, but organised around memory traffic instead of around one kernel per MATLAB statement:
//
//   x-forward   real rows -> half-spectrum rows (two real rows ride one complex FFT)          R  -> C
//   y-pass      in-place complex FFT along y on 16-column tiles (128-B segments)              C <-> C
//   z-fused     forward FFT along z, spectral multiply (kappa*ddk, nabla, sourceKappa), inverse FFT along z,
//               all in registers/LDS — the spectrum never makes a round trip to HBM            C  -> C (x1..3)
//   y-pass^-1   in-place inverse along y
//   x-inverse   half-spectrum rows -> real rows + epilogue: velocity update / density update (+ pressure terms) /
//               pressure sum — the gradients never exist in HBM as separate arrays
//
// vs. the reference order (14 library FFTs + 7 element-wise kernels, each a full HBM round trip).
// Internal spectral scratch is private to the pipeline: rows are whole 16-complex tiles (128-B segments) — for even Nx
// exactly Nx/2 bins, the x-Nyquist bin of every row living in a compact side array behind them (tile_coord); kappa /
// nabla operators are imported once into the per-thread run layout their z-pass reads (load_op_run).
// Supported: each of Nx, Ny, Nz one of the lengths of KW_FUSED_LENGTHS (2^a 3^b 5^c with a two-factor split into 4- to
// 32-point register DFTs, 16 ... 1024; axes independent); anything else uses the rocFFT path (kw_fft.hip +
// kw_solver_kernels.hip).  Multi-GPU: Z-slabs, see "pipelined slab schedule" in kw_fused_main.hip and kw_comm.hip.
// This file is the pipeline's device code: the line-length and tuning tables, tile geometry, the pass kernels and their
// launch helpers.  It is no code object of its own: each one includes it and instantiates only what it launches —
// kw_fused_main.hip (y-, z-, x-forward, x-shift and import kernels, host schedule, C-ABI), kw_fused_probe.hip (tuning
// probes) and eight kw_fused_xinv_*.hip with the x-inverse + epilogue kernels, the bulk of the compile time and code
// size (one kernel per epilogue variant and line length).  Those compile side by side and the runtime loads a code object
// at the first launch out of it, so a run pays for the variants it uses (launch_xinv in kw_fused_main.hip picks one).
// Kernels stay in the unnamed namespace (no host stub shared between code objects); the plain-data argument structs are
// in kwfused, so that host functions of different code objects can pass them.
#ifndef KW_FUSED_HIP
#define KW_FUSED_HIP

#include "kw_fft_device.h"
#include "kw_internal.h"

#include <cmath>
#include <type_traits>

using namespace kwfft;

#define KW_LONG_LINES 432 /* kw_fused_xinv_density_*_long.hip hold the density epilogues of the x lines from this length on */

namespace kwfused {

// Row addressing of a y-line element.  Natural layout: row(z, ky) = z*ny + ky.  Packed layout (slab mode, the send /
// receive side of the all-to-all): row(z, ky) = ((ky / nyl) * nzl + z) * nyl + ky % nyl, i.e. one contiguous chunk
// [nzl][nyl][P] per peer rank.  Both are  q * qstride + (ky - q * nyl) + z * zmul  with q = ky / nyl taken as
// (ky * magic) >> 20, magic = 2^20 / nyl + 1: exact while ky * nyl < 2^20 (lines have at most 1024 elements); the natural
// layout has magic = 0, hence q = 0.
struct RowAddr
{
  uint32_t magic, nyl, qstride, zmul;
  uint32_t estride; // 1 for y-lines; ny for lines along z (probe / plain z transform)
  // 32-bit element indices throughout the pipeline: every scratch / field array has < 2^32 elements (checked in
  // kw_fused_supported), so addresses are "uniform base + 32-bit lane offset" and need no 64-bit VALU arithmetic
  __device__ __forceinline__ uint32_t row(uint32_t z, uint32_t ky) const
  {
    const uint32_t q = (ky * magic) >> 20;
    return q * qstride + (ky - q * nyl) * estride + z * zmul;
  }
};

struct PassArgs
{
  const float2* in[3];
  float2*       out[3];
  const float2* tw;
  uint32_t      nxc, P;
  uint32_t      PX;   // row pitch of the packed (exchange) side (= P unless rows travel without their padding)
  uint32_t      narr; // arrays per block (grid.z * narr arrays in the launch)
  uint32_t      z0;   // first plane of this launch (chunked plane-local passes)
  uint32_t      side_off; // element offset of the x-Nyquist side array, 0 = the column lives in the rows (see tile_coord)
  const float2* mul[3]; // per array: optional factor mul[ky] applied to the line before its transform (ddy of the gradient)
  RowAddr       ain, aout;
};

struct ZArgs
{
  const float2* in[3];
  float2*       out[3];
  const float*  op[2];  // padded reduced real operators: kappa (PGRAD/VGRAD), nabla1/nabla2 (ABSORB), sourceKappa
  const float2* dd[3];  // ddx[kx], ddy[ky], ddz[kz]
  const float2* tw;
  float         divider;
  uint32_t      nxc, P, ny, nz;
  uint32_t      Pop;  // row pitch of the operator arrays (always padded; P is the unpadded exchange pitch in slab mode)
  uint32_t      arr0; // first array of this launch
  uint32_t      narr; // arrays processed back to back by each block (VGRAD / ABSORB)
  uint32_t      ky0;  // global ky of local row 0 (slab mode: rank * ny/nranks); ny above = number of LOCAL rows
  uint32_t      lstride, bstride; // Z_SHIFT: element stride along a line, offset per blockIdx.y (both in complex units)
  uint32_t      side_off;    // element offset of the x-Nyquist side array in the scratch arrays (0: none; see tile_coord)
  uint32_t      op_side_off; // float offset of the side column's values in the imported operators
  uint32_t      axis_of[3];  // VGRAD: derivative axis of array i (0 ddx[kx], 1 ddy[ky], 2 along the line: dd[2][k]); 3-D: 0 1 2
};

struct XfwdArgs
{
  const float*  in[3];
  float2*       out[3];
  const float2* tw;
  uint32_t      nx, P;
  uint32_t      nrows, tile0; // rows of the grid (ny * nz); first tile of this launch
  uint32_t      side_off;     // element offset of the x-Nyquist side array in out[] (0: the bin stays in its row)
};

struct XinvArgs
{
  const float2* in[3];
  const float2* tw;
  kw_constants  c;
  uint32_t      P;
  // EPI_STORE: out[0]; EPI_VELOCITY/INITVEL: u[3], dtrho[3] (NULL -> scalar), pml[3]
  // EPI_DENSITY: rho[3] in/out, pml[3], rho0, bona, du[3] (optional store), t[3] terms outputs, flags
  // EPI_PSUM: p, first, c2, tau, eta
  // EPI_PSUM1: p, first, c2, the one coefficient (tau or eta by `which`)
  float*        out[3];
  const float*  m0[3]; // dtrho / (rho0, bona, -) / (first, c2, -)
  const float*  m1[3]; // pml / (tau, eta, -) / (tau or eta, -, -)
  float*        aux[3]; // du stores / -
  float*        t[3];  // pressure-term outputs
  int           nonlinear;
  int           terms; // 0 none, 1 linear (t0 = sum rho, t1 = rho0*sum du), 2 nonlinear (t0, t1 = nonlinear term, t2),
                       // 3 lossless pressure (t0 = p, m0[2] = c2), 4 Stokes pressure (as 3, and t[2] = absorb_tau array or NULL: INPUT),
                       // 5 one-term power law (`which` below; first -> t0 linear / t1 nonlinear; the one term as 1 / 2 place it)
  uint32_t      comp0; // first component of this launch (per-array launches)
  float2*       fout[3]; // CHAIN: where the forward x-transform of the epilogue's result goes (scratch rows)
  uint32_t      tile0;   // first 2*NL-row tile of this launch (chunked plane-local passes)
  const float2* mulx[3]; // per component: optional factor mulx[kx] applied to the rows before the inverse (ddx of the gradient)
  uint32_t      nrows;      // rows of the grid (ny * nz): bounds the partial last tile (TAIL kernels)
  uint32_t      side_off;   // element offset of the x-Nyquist side array in in[] / fout[] (0: none)
  const float2* ymul[3];    // PLANE kernels: optional factor ymul[ky] applied to array i before its y-inverse (ddy of the gradient)
  int           which;      // one-term power law (density terms == 5, EPI_PSUM1), the same for every wave: 0 no_dispersion
                            // (the term is rho0 * sum du, its coefficient tau), 1 no_absorption (sum rho, eta)
};

// the y-inverse of the angular-spectrum projector (kw_angular.hip)
struct AngArgs
{
  const float2*   in[2];  // the source's 2-D spectra Sr^, Si^ in the plane layout: rows [ky][P], side column at side_off2
  float2*         out[2]; // scratch arrays of the chunk: planes [z][ky][P], side array at side_off
  const uint32_t* tab;    // five tables (a0, a1, b0, b1, alive) of tab_elems words each, in the plane layout
  const float2*   tw;
  uint32_t        nxc, P, ny;
  uint32_t        side_off, side_off2, tab_elems;
  uint32_t        j0;     // plane index of the chunk's first plane
  float           divider; // 1 / (Ex Ey)
};

// the geometry of a pass over the scratch layout: what the operator passes (k_zfused_time, k_zfused_second_order,
// k_yfused_second_order, k_zfused_recon, k_yfused_line_recon) take from the context (pass_geo)
struct PassGeo
{
  const float2* tw;                 // the twiddle table of the line's axis
  uint32_t      nxc, P, side_off;   // columns of a row, row pitch, element offset of the x-Nyquist side array (0: none)
};

struct XshiftArgs
{
  const float*  in;
  float*        out;
  const float2* tw;
  const float2* H; // L complex: shift[k] / L on 0 < k < L/2, conjugate above, real parts at k = 0 and L/2
  uint32_t      nrows, tile0;
};

// x-inverse + epilogue entry points, one code object each (kw_fused_xinv_*.hip): launch the kernels of `ntiles` x tiles
// from tile0 on (whole-plane forms: z-planes from plane0 on)
kw_status xinv_density_chain_short(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_chain_long(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_chain_tail(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_plain_short(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_plain_long(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_plain_tail(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
// the Stokes pressure epilogue (terms == 4), plain and chained, in code objects of its own (kw_fused_xinv_density_stokes_*.hip)
kw_status xinv_density_stokes_short(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_stokes_long(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_stokes_tail(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_stokes_plane(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t plane0, uint32_t nplanes);
// the one-term power law (absorbing_flag 3 / 4): its density epilogue (terms == 5; kw_fused_xinv_density_oneterm_*.hip) and
// its pressure sum over one inverse (EPI_PSUM1; kw_fused_xinv_psum_one*.hip), plain and chained, in code objects of their own
kw_status xinv_density_oneterm_short(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_oneterm_long(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_oneterm_tail(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_density_oneterm_plane(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t plane0, uint32_t nplanes);
kw_status xinv_psum_one(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_psum_one_tail(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_psum_one_plane(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t plane0, uint32_t nplanes);
kw_status xinv_other(int epi, int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
kw_status xinv_other_tail(int epi, int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles);
// whole-plane tiles (small grids, see k_xinv); with density-chain-short and other
kw_status xinv_density_plane(int chain, int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t plane0, uint32_t nplanes);
kw_status xinv_other_plane(int epi, int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t plane0, uint32_t nplanes);
// the z-pass of kw_fused_cw_pair: two spectra forward along z, the 2x2 mix with two real operators, both inverses (kw_cw.hip)
kw_status zfused_pair(kw_ctx* ctx, ZArgs a);
// the y-inverse of kw_fused_angular_planes: H of each plane formed from the tables, the 2x2 mix, both inverses (kw_angular.hip)
kw_status yinv_angular(kw_ctx* ctx, AngArgs a);
// the z-pass of kw_fused_angular_time_plane: one spectrum forward along t, H of the plane formed in registers, the inverse
// (kw_angular_time.hip): lines of `in` (the kept spectrum) to `out`
kw_status zfused_time(kw_ctx* ctx, const float2* in, float2* out, const kw_angular_time_op* op);
// the z-pass of kw_fused_second_order_time: one spectrum forward along z, the real H(|k|; t) formed in registers, the inverse
// (kw_second_order.hip): lines of `in` (the kept spectrum) to `out`
kw_status zfused_second_order(kw_ctx* ctx, const float2* in, float2* out, const kw_second_order_op* op);
// the z-pass of kw_fused_plane_recon: lines of `s` forward along t, the weight, the gather from w to kz along each line,
// the inverse, in place (kw_plane_recon.hip)
kw_status zfused_recon(kw_ctx* ctx, float2* s, const kw_plane_recon_op* op);
// the pass along t of kw_fused_line_recon (frames context): lines of `s` along y, one frame per tile position, the plane
// reconstruction's weight and gather with rho2 of the column alone, in place (kw_line_recon.hip; op->dx = the sensor pitch)
kw_status yfused_line_recon(kw_ctx* ctx, float2* s, const kw_plane_recon_op* op);
// the pass along y of kw_fused_second_order_frames_time (frames context): lines of `in` (the kept spectrum of the frames)
// forward along y, the real H(|k|; t) of the plane formed in registers, the inverse, to `out` (kw_second_order.hip)
kw_status yfused_second_order(kw_ctx* ctx, const float2* in, float2* out, const kw_second_order_op* op);
// the same two passes with dp0/dt as a second initial condition (kw_second_order_pair.hip): lines of both kept spectra
// forward, Hc in_p + Hs in_v in registers, ONE inverse, to `out`
kw_status zfused_second_order_pair(kw_ctx* ctx, const float2* in_p, const float2* in_v, float2* out, const kw_second_order_op* op);
kw_status yfused_second_order_pair(kw_ctx* ctx, const float2* in_p, const float2* in_v, float2* out, const kw_second_order_op* op);
// the tuning probes of kw_fused_probe that launch no pipeline kernel (kw_fused_probe.hip)
kw_status probe_patterns(kw_ctx* ctx, int which, const float* op);

} // namespace kwfused
using namespace kwfused;

namespace {

constexpr int NLMAX = 16; // widest tile: 16 complex = 128-B segments (also the row-pitch granule)
// x passes, rows per block = 2 * nl_x.  Chosen per line length from a measured matrix (every length from 160 up, both
// orientations of its factor pair, 8 / 10 / 12 / 16 line pairs; 4 / 8 / 16 from 96 to 144: profiles/r03_length_tuning.txt).
// What the matrix shows: a block should be a whole number of 4 waves or less — the 5- and 6-wave blocks of 18, 20 and 24
// threads per line at 16 line pairs are rarely co-resident (one wave more on one SIMD than on the others), 240^3: x-inverse
// kernels 1.4-1.5x faster at 12 line pairs — and the long lines want the small block's register budget.
// (tuning builds: -DKW_TUNE_NLX=<n> overrides the table, -DKW_TUNE_SWAP the orientation table in kw_fft_device.h)
#ifdef KW_TUNE_NLX
constexpr int nl_x(int) { return KW_TUNE_NLX; }
#else
constexpr int nl_x(int L)
{
  switch (L)
  {
    case 100: case 108: case 140: case 160: case 168: case 196: case 200: case 224: case 288: case 336: case 384: case 392: return 8;
    case 280: case 300: case 320: case 432: case 480: case 500: case 600: return 10;
    case 180: case 216: case 240: case 252: case 324: case 360: case 400: return 12;
    case 896: return 16;
    default: return L >= 400 ? 8 : 16;
  }
}
#endif
// Every fast-path length is a multiple of 4, so the Ny * Nz rows of a 3-D grid on one GPU are a multiple of 16 and x tiles of
// 8 line pairs (16 rows) always divide it: only 2-D grids and slabs with Ny * Nz(local) off a multiple of 16 ever need the
// masked (TAIL) kernels of such a length.  For the long lines added in round 3 — the most expensive kernels of the file to
// compile — those are not built; kw_fused_supported sends such a grid to the rocFFT path.
constexpr bool has_partial_x_tiles(int L)
{
  switch (L)
  {
    case 672: case 700: case 720: case 756: case 784: case 800: case 840: case 864: case 900: case 960: return false;
    default: return true;
  }
}
#define KW_NO_TAIL(LEN)                                                                                                \
  { kw_set_error("fused pipeline: rows of %d elements have no partial x tiles", LEN); return KW_ERR_INVALID; }

// y / z passes, columns per tile: 16 (128-B row segments) at every length.  500^3 measured with 8-column tiles (64-B
// segments) for the long lines: y passes 1.5x, z-fused 1.25x slower; 240^3 with 12- and 8-column tiles (4- and 3-wave
// blocks instead of 5): step 11 % and 15 % slower.
constexpr int nl_yz(int) { return 16; }
// ... except the z-fused kernels of 240- and 400-point lines (20 threads per line: 5-wave blocks, of which a CU mostly
// holds one): 32-column tiles — one 10-wave block, 256-B row segments — take 16 % / 10 % off them (the y-passes of the
// same lengths lose with 32 columns, every other length loses in both: profiles/r03_length_tuning.txt)
#ifdef KW_TUNE_NLZ
constexpr int nl_z(int) { return KW_TUNE_NLZ; }
#else
constexpr int nl_z(int L) { return (L == 240 || L == 400) ? 32 : 16; }
#endif
// tiles of nl_z columns over the P (a multiple of 16) columns of a row
constexpr uint32_t z_tiles(uint32_t P, uint32_t len) { return (P + static_cast<uint32_t>(nl_z(len)) - 1u) / static_cast<uint32_t>(nl_z(len)); }

constexpr int cmax(int a, int b) { return a > b ? a : b; }
// 20- to 32-point register DFTs next to a multi-array epilogue want more than 256 VGPRs, which leaves ONE wave per SIMD
// (nothing to hide a memory round trip behind): hold those kernels to the two-wave budget instead
constexpr int big_line_waves(int L) { return L >= 400 ? 2 : 1; }
// largest divisor of n that is <= want
constexpr int gq_pick(int n, int want) { return (n % want == 0) ? want : gq_pick(n, want - 1); }

template<int L, int NLV = nl_yz(L)> struct Geo
{
  static constexpr int R1 = Fac<L>::R1, R2 = Fac<L>::R2;
  static constexpr int NL      = NLV;
  static constexpr int TPL     = cmax(R1, R2);
  static constexpr int THREADS = NL * TPL;
  // y/z passes: the R2 threads per line of a step-A region (line loads and stores) are whole waves — see ACTW, ld_uni<PIN>
  static constexpr bool WA     = (R2 == TPL) || ((NL * R2) % 64 == 0 && 64 % NL == 0);
  // y/z passes: LDS[k1][n2][c]; +16 complex per k1 block keeps the step-B reads conflict-free
  static constexpr int PADB    = NL;
  static constexpr int SF      = R2 * NL + PADB; // stride per k1 (forward and inverse use the same cells, see inverse_from_regs)
  static constexpr int LDSB    = R1 * SF;
  // x passes: LDS[c][k1][n2] (pitch LP per line) aliased with a natural-order line buffer (pitch ZP)
  static constexpr int LP0  = R1 * (R2 + 1);
  static constexpr int LP   = LP0 + ((16 - LP0 % 32) + 32) % 32;
  static constexpr int ZP   = L + 16;
  static constexpr int LDSX = NL * cmax(LP, ZP);
  // inter-step twiddles, LDS-resident: T[k][n] = W_L^(k*n), k < R1, n < R2, pitch TP (odd: conflict-free both ways)
  static constexpr int TP   = R2 + 1;
  static constexpr int TWN  = R1 * TP;
};

// "thread t takes part in a step of R threads per line": compile-time true when every thread of a line does (R == TPL),
// so that the common L = 256 kernels carry no divergent regions (and no phi-separated register sets) at all.
template<int L> using GeoX = Geo<L, nl_x(L)>; // geometry of the x passes

#define ACT(R, t) ((R) == G::TPL || (t) < (R))
// the same for the y / z kernels, whose threads are laid out t = j * NL + c: when NL * R is a whole number of waves the
// participants of a step are whole waves, and the test is made on a wave-uniform value (a scalar branch, no exec masking)
#define ACTW(R, j) ((R) == G::TPL || (((G::NL * (R)) % 64 == 0 && 64 % G::NL == 0) ? __builtin_amdgcn_readfirstlane(j) < (R) : (j) < (R)))

// Roles of the x kernels' threads.  A step with R participants per line (R2 in step A, R1 in step B) is taken by the FIRST
// NL * R threads of the block, R consecutive ones per line: with R < TPL (12 x 20, 12 x 18 ... factorisations) the idle
// threads are whole trailing waves instead of masked lanes inside every wave.  Everything crosses LDS between the steps,
// so the line a thread works on may change from step to step; with R == TPL this is the plain (c, f) = (t / TPL, t % TPL).
template<class G, int R> struct XRole
{
  int  c, f;
  bool on;
  __device__ __forceinline__ XRole()
  {
    c  = static_cast<int>(threadIdx.x) / R;
    f  = static_cast<int>(threadIdx.x) - c * R;
    on = (R == G::TPL) || static_cast<int>(threadIdx.x) < G::NL * R;
  }
};

// Block barrier that orders LDS traffic only.  __syncthreads() also drains every outstanding global load and store
// (vmcnt(0)) — here all cross-thread communication goes through LDS, and global stores / prefetched loads should stay in
// flight across the exchange steps.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// State and medium arrays are touched once per step and not again for a whole step (> 5 GB of traffic later): they are
// streamed past the caches (non-temporal), which leaves the 256 MB Infinity Cache to the spectral scratch that the very
// next kernel re-reads.  Measured: +5.4 % on the whole step against plain accesses; the same for the reduced operators
// (+2.6 %).  Spectra stay on plain accesses: marking their last-use reads non-temporal costs 0.6-2 % in every pass type.
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float* p)
{
  const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4(float* p, const float4& v)
{
  v4f t = { v.x, v.y, v.z, v.w };
  __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(p));
}
__device__ __forceinline__ float ldop(const float* p) { return __builtin_nontemporal_load(p); }
#define LDOP(p) ldop(p) // reduced real operators (kappa, nabla): one or two reads per step each (+2.6 % measured)

// Reduced operators are stored for the z-pass that consumes them: [ky][kx tile of 16][q][j][c][V] — thread (c, j) of the
// block owning that tile finds the values of ITS bins (kz = j + R1*k2, k2 = q*V + r; 2 x 256 split lines: kz = 2j + h +
// 2*R1*k2 with run index 2*k2 + h) as RUN / V vectors of V floats, and the 64 lanes of a wave read one contiguous
// 64 * V * 4-byte piece per load instruction.  V = 4 when the per-thread run length allows, else 2 or 1 (V = 1 is
// plain [kz][c] order).
constexpr int op_vec(int run) { return (run % 4 == 0) ? 4 : (run % 2 == 0) ? 2 : 1; }
template<int RUN, int R1> __device__ __forceinline__ void load_op_run(float (&dst)[RUN], const float* __restrict__ op, uint32_t base)
{ // base: index (in floats) of vector q = 0 of this thread; consecutive q are R1 * 16 vectors apart
  constexpr int V = op_vec(RUN);
  typedef float vf __attribute__((ext_vector_type(V)));
#pragma unroll
  for (int q = 0; q < RUN / V; q++)
  {
    if constexpr (V == 1) dst[q] = LDOP(op + base + static_cast<uint32_t>(q * R1 * NLMAX));
    else
    {
      const vf t = __builtin_nontemporal_load(reinterpret_cast<const vf*>(op + base + static_cast<uint32_t>(q * R1 * NLMAX * V)));
#pragma unroll
      for (int r = 0; r < V; r++) dst[q * V + r] = t[r];
    }
  }
}


// Element e of a lane plus a wave-uniform element offset: "SGPR base + 32-bit lane offset" addressing.  The uniform part
// (array base + n * line stride) is 64-bit scalar arithmetic, the lane part one VGPR holding a byte offset — written
// this way the loads / stores of a tile cost no vector ALU work at all (as  p[lane + n * stride]  every access pays a
// v_add_u32 and a 64-bit v_lshl_add_u64: a sixth of the vector instructions of a z-pass, whose VALU is ~75 % busy).
// (the empty asm pins the uniform part to an SGPR pair: left alone, the compiler re-associates it into a chain of 64-bit
// vector adds)
// PIN = false: inside a region only some lanes of a wave enter (a step whose participants are not whole waves) the
// compiler may hold the base in vector registers, which the "s" constraint cannot take: there the base is read back
// from the first active lane instead (two v_readfirstlane; folded away when the value already is scalar).
template<bool PIN = true>
__device__ __forceinline__ float2 ld_uni(const float2* __restrict__ p, uint64_t uniform_elems, uint32_t lane_bytes)
{
  typedef float v2 __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(1))) char* gptr; // global address space survives the asm (else: flat loads)
  gptr b = (gptr)(p + uniform_elems);
  if constexpr (PIN) asm volatile("" : "+s"(b));
  else
  {
    const uint64_t bits = reinterpret_cast<uint64_t>(p + uniform_elems);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(bits));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(bits >> 32));
    b = (gptr)((static_cast<uint64_t>(hi) << 32) | lo);
  }
  const v2 t = *(const __attribute__((address_space(1))) v2*)(b + lane_bytes);
  return make_float2(t.x, t.y);
}
template<bool PIN = true>
__device__ __forceinline__ void st_uni(float2* __restrict__ p, uint64_t uniform_elems, uint32_t lane_bytes, const float2& v)
{
  typedef float v2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(1))) char* gptr;
  gptr b = (gptr)(p + uniform_elems);
  if constexpr (PIN) asm volatile("" : "+s"(b));
  else
  {
    const uint64_t bits = reinterpret_cast<uint64_t>(p + uniform_elems);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(bits));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(bits >> 32));
    b = (gptr)((static_cast<uint64_t>(hi) << 32) | lo);
  }
  *(__attribute__((address_space(1))) v2*)(b + lane_bytes) = v2{ v.x, v.y };
}

// Tile coordinates of a block of a y- or z-pass.  Regular tiles: NL consecutive columns kx at one line position (the
// plane z of a y-pass, the row ky of a z-pass; blockIdx.y).
//
// Side tile.  A half-spectrum row has nxc = Nx/2 + 1 bins: for every Nx that is a multiple of 32 that is a whole number
// of 16-column tiles plus ONE bin, the x-Nyquist column.  Kept in the rows it costs a ninth tile of 16 lanes with one
// useful lane at 256^3 (11 % of every y- and z-pass; 20 % at 128^3).  The pipeline therefore stores that column apart,
// as a compact array N[line position][y] behind the main part (rows of Nx/2 bins, no padding at all), and the passes
// handle it with one extra tile index whose blocks take the column at NL line positions each: lane c <-> position
// NL * blockIdx.y + c.  Same kernel, same LDS traffic; the lanes of a side block read 8-B neighbours of one array.
// (Tried before, with the column left in the padded rows: every wave-level access then touches 64 different cache
// lines and those blocks become the critical path — y-passes +12 %, step -4 %.)
struct TileCoord
{
  uint32_t kx;    // true column index (operator lookups along kx)
  uint32_t col;   // column used for addressing: min(kx, last main column), 0 in a side block
  uint32_t pos;   // line position: z (y-pass) / ky (z-pass)
  uint32_t pitch; // row pitch of the region this block works in: P, or 1 (side array)
  uint32_t off;   // element offset of that region in the scratch array
  bool     valid, dead, side;
};
template<int NL>
__device__ __forceinline__ TileCoord tile_coord(uint32_t nxc, uint32_t P, uint32_t side_off, uint32_t npos, int c)
{
  TileCoord t;
  if (side_off != 0 && blockIdx.x == gridDim.x - 1)
  {
    const uint32_t p = blockIdx.y * NL + c;
    t.dead  = blockIdx.y * NL >= npos;
    t.kx    = nxc; // the bin after the nxc main columns
    t.col   = 0;
    t.valid = p < npos;
    t.pos   = min(p, npos - 1u); // lanes past the last position re-read it; their results are never stored
    t.pitch = 1;
    t.off   = side_off;
    t.side  = true;
  }
  else
  {
    t.kx    = blockIdx.x * NL + c;
    t.col   = min(t.kx, nxc - 1u); // pad lanes re-read the last column (no branch, no extra sector); never stored
    t.valid = t.kx < nxc;
    t.pos   = blockIdx.y;
    t.pitch = P;
    t.off   = 0;
    t.dead  = false;
    t.side  = false;
  }
  return t;
}

// ---- register-level steps -------------------------------------------------------------------------------------------
// Fill the block's twiddle table from the global one (tw[m] = exp(-2*pi*i*m/L)); the caller's next lds_barrier()
// publishes it.  Every use below is "one VGPR base + compile-time offset", so twiddles cost neither address registers
// nor global-memory requests.
template<int L> __device__ __forceinline__ void load_twiddles(float2* twl, const float2* __restrict__ tw)
{
  using G = Geo<L>;
  for (int e = threadIdx.x; e < G::R1 * G::R2; e += blockDim.x)
  {
    const int k = e / G::R2, n = e - k * G::R2;
    twl[k * G::TP + n] = tw[k * n];
  }
}

template<int L, int DIR> __device__ __forceinline__ void step_a(float2 (&v)[Fac<L>::R1], int n2, const float2* twl)
{
  Dft<Fac<L>::R1, DIR>::run(v);
#pragma unroll
  for (int k1 = 1; k1 < Fac<L>::R1; k1++) v[k1] = apply_tw<DIR>(v[k1], twl[k1 * Geo<L>::TP + n2]);
}

// ---- line-tile steps ------------------------------------------------------------------------------------------------
// What a y- or z-pass kernel is assembled from: the block's tile, the line loads and stores, and the two exchanges of a
// four-step transform through the block's buffer lds[G::LDSB].  A kernel's body keeps what is its own — which arrays,
// what happens to a bin between the transforms — and the order of loads, barriers and stores.
// On the steps: k_zfused_split, k_zfused_pair_split (kw_cw.hip), k_zfused_time (kw_angular_time.hip), k_zfused_second_order
// and k_yfused_second_order (kw_second_order.hip), their pair forms (kw_second_order_pair.hip), k_zfused_recon (kw_plane_recon.hip), k_yfused_line_recon (kw_line_recon.hip); k_ypass and k_ypass_split take the tile and keep their
// RowAddr loads and stores.  k_zfused, k_zfused_pair (kw_cw.hip) and k_yinv_angular (kw_angular.hip) spell the same steps out in their bodies: assembled from
// the functions below the compiler allocates their guarded (non-whole-wave) and spilling instantiations differently — an
// occupancy step lost at some lengths, scratch bytes gained at others — so they stay as they were written.  A change to
// a step below is a change to those three bodies as well.
//
// Who calls a step.  Threads are laid out t = j * NL + c.  A thread with ACTW(R2, j) is "column thread" n2 = j of its
// line (c): it holds the R1 elements x[n1 * R2 + j] before a forward transform and after an inverse.  A thread with
// ACTW(R1, j) is "row thread" k1 = j: it holds the R2 bins X[j + R1 * k2] between them.  load_lines and
// fwd_cols are for column threads, fwd_rows is for row threads, and the kernel calls them under that guard (it usually
// has more to do under the same one); store_lines and inverse_from_regs make the test themselves and are called by
// every thread.
//
// Exchange-buffer discipline.  Cell (k1, n2) of column c is lds[k1 * SF + n2 * NL + c].  In a forward exchange column
// thread n2 writes the cells (k1, n2) for all k1 ("its column") and, after a barrier, row thread k1 reads (k1, n2) for
// all n2 ("its row").  inverse_from_regs runs that backwards over the same cells: row thread k1 writes its row — cells
// nobody else has read — and, after a barrier, column thread q1 reads its column.  A thread therefore only ever
// overwrites what it read last itself: no barrier is needed between a forward read and the inverse's write, nor between
// the inverse's read and the next forward write.  Two exchanges of the same direction in a row do need one (the second
// one's writers overwrite cells other threads may still be reading), unless the second runs transposed (ROWWRITE /
// COLWRITE, square factorisations), which restores "writes what it has just read".

// The block's tile and this thread's place in it.  Element n of the thread's line (position pos, column c of the tile)
// is element base + n * lstride of a scratch array; loads use basel instead, whose pad lanes re-read the last column.
struct LineTile
{
  int       c, j;    // column of the tile; thread row (n2 = j as a column thread, k1 = j as a row thread)
  TileCoord tc;
  uint32_t  pos;     // line position: ky (z-pass) / z (y-pass), the launch's first position included
  bool      valid;   // the column exists (or, in a side block, the position): its results are stored
  uint32_t  lstride; // element stride along the line
  uint32_t  base, basel;
};
// lmul / bmul: strides along the line and from one line position to the next, in rows of the block's region (its pitch:
// P, or 1 in the side array).  z-pass: (ny, 1); y-pass: (1, ny); lines with free strides and no side array (Z_SHIFT):
// P = 1 and the strides in elements.  The caller returns at once when tc.dead (a side block past the last position).
template<class G>
__device__ __forceinline__ LineTile line_tile(uint32_t nxc, uint32_t P, uint32_t side_off, uint32_t lmul, uint32_t bmul,
                                              uint32_t pos0 = 0)
{
  LineTile t;
  t.c       = threadIdx.x % G::NL;
  t.j       = threadIdx.x / G::NL;
  t.tc      = tile_coord<G::NL>(nxc, P, side_off, gridDim.y, t.c);
  t.pos     = t.tc.pos + pos0;
  t.valid   = t.tc.valid;
  t.lstride = lmul * t.tc.pitch;
  const uint32_t bstride = bmul * t.tc.pitch;
  t.base    = t.pos * bstride + (t.tc.side ? 0u : t.tc.kx) + t.tc.off;
  t.basel   = t.pos * bstride + t.tc.col + t.tc.off;
  return t;
}

// Operators live in a tile-blocked layout [ky][kx tile][kz][16]: the 16 x nz values of a z-pass block's tile are one
// contiguous run (k_import_reduced), instead of 64-B pieces a whole plane apart.  Index of vector q = 0 of row thread
// t.j's run of RUN values (load_op_run); side blocks: the side column's values are stored like one more row of tiles
// whose columns are the ky, op_side_off floats into the array.
template<int RUN, int R1>
__device__ __forceinline__ uint32_t op_run_base(const LineTile& t, uint32_t Pop, uint32_t op_side_off)
{
  constexpr int  OPV = op_vec(RUN);
  const uint32_t ky  = t.pos;
  return t.tc.side ? op_side_off + (((ky / NLMAX) * (RUN / OPV) * R1 + t.j) * NLMAX + ky % NLMAX) * OPV
                   : (((ky * (Pop / NLMAX) + t.tc.col / NLMAX) * (RUN / OPV) * R1 + t.j) * NLMAX + t.tc.col % NLMAX) * OPV;
}

// Column thread: its R1 line elements x[n1 * R2 + j].  PIN as in ld_uni: G::WA wherever the guard can split a wave.
// The lane part of the address is a 32-bit BYTE offset that holds the whole line position (t.basel): the array must end
// below 2^29 elements wherever the line position is not bounded by a line length — a 3-D grid's is (every axis is at most
// 1024 long), a frames context's is not, hence the limit in kw_fused_supported.  store_lines: the same.
template<class G, bool PIN = G::WA>
__device__ __forceinline__ void load_lines(float2 (&v)[G::R1], const float2* __restrict__ in, const LineTile& t)
{
  const uint32_t lb = (t.basel + static_cast<uint32_t>(t.j) * t.lstride) * static_cast<uint32_t>(sizeof(float2));
#pragma unroll
  for (int n1 = 0; n1 < G::R1; n1++) v[n1] = ld_uni<PIN>(in, static_cast<uint64_t>(n1 * G::R2) * t.lstride, lb);
}
// Every thread: a column thread's x[j + R2 * q2] after an inverse, where the column is valid.  The element index is
// laundered through an empty asm, which makes the address arithmetic per store (and, in the kernels that request the
// next array's lines inside their loop, per load): left alone the compiler hoists it, and 16 hoisted 64-bit addresses
// cost an occupancy step.
template<class G, bool PIN = G::WA>
__device__ __forceinline__ void store_lines(float2* __restrict__ out, const LineTile& t, const float2 (&r)[G::R1])
{
  if (ACTW(G::R2, t.j) && t.valid)
  {
    uint32_t ob = t.base + static_cast<uint32_t>(t.j) * t.lstride;
    asm volatile("" : "+v"(ob));
#pragma unroll
    for (int q2 = 0; q2 < G::R1; q2++) st_uni<PIN>(out, static_cast<uint64_t>(G::R2 * q2) * t.lstride, ob * static_cast<uint32_t>(sizeof(float2)), r[q2]);
  }
}

// The forward exchange of an L-point transform of sign DIR, in two halves around the kernel's lds_barrier().
// Column thread: step A on its registers, then its column of the buffer.  ROWWRITE: the transposed cell assignment.
template<int L, int DIR, int NLV = nl_yz(L), bool ROWWRITE = false>
__device__ __forceinline__ void fwd_cols(float2 (&v)[Fac<L>::R1], float2* lds, int c, int j, const float2* twl)
{
  using G = Geo<L, NLV>;
  static_assert(!ROWWRITE || G::R1 == G::R2, "transposed exchange needs a square factorisation");
  step_a<L, DIR>(v, j, twl);
#pragma unroll
  for (int k1 = 0; k1 < G::R1; k1++) lds[ROWWRITE ? j * G::SF + k1 * G::NL + c : k1 * G::SF + j * G::NL + c] = v[k1];
}
// Row thread: its row of the buffer, then step B; ends with X[j + R1 * k2].
template<int L, int DIR, int NLV = nl_yz(L), bool ROWWRITE = false>
__device__ __forceinline__ void fwd_rows(float2 (&X)[Fac<L>::R2], const float2* lds, int c, int j)
{
  using G = Geo<L, NLV>;
#pragma unroll
  for (int n2 = 0; n2 < G::R2; n2++) X[n2] = lds[ROWWRITE ? n2 * G::SF + j * G::NL + c : j * G::SF + n2 * G::NL + c];
  Dft<G::R2, DIR>::run(X);
}
// Both halves for a block all of whose threads are column and row threads (R1 == R2 == TPL): the transform of the step-A
// registers v, X[j + R1 * k2] in w.  ROWWRITE: for a transform that follows an exchange whose read was by rows, so that
// no barrier is needed in between.  Otherwise the buffer must be free on entry.
template<int H, int DIR, bool ROWWRITE = false, int NLV = nl_yz(H)>
__device__ __forceinline__ void line_fft(float2 (&v)[Fac<H>::R1], float2 (&w)[Fac<H>::R2], float2* lds, int c, int j,
                                         const float2* twl)
{
  fwd_cols<H, DIR, NLV, ROWWRITE>(v, lds, c, j, twl);
  lds_barrier();
  fwd_rows<H, DIR, NLV, ROWWRITE>(w, lds, c, j);
}

// Every thread: inverse along the line, started from the row threads' registers (X[j + R1 * k2] in w); the column
// threads end with x[j + R2 * q2], q2 < R1, in v.  The exchange is the forward one run backwards (see above).
// COLWRITE (square factorisations only, used by the 2 x 256 split kernels): the transposed cell assignment — thread k1
// writes its column and thread q1 reads its row — for an exchange that follows one whose read was by columns.
template<int L, bool COLWRITE = false, int NLV = nl_yz(L)>
__device__ __forceinline__ void inverse_from_regs(float2 (&w)[Fac<L>::R2], float2 (&v)[Fac<L>::R1], float2* lds, int c,
                                                  int j, const float2* twl)
{
  using G = Geo<L, NLV>;
  constexpr int R1 = G::R1, R2 = G::R2;
  static_assert(!COLWRITE || R1 == R2, "transposed exchange needs a square factorisation");
  if (ACTW(R1, j))
  {
    Dft<R2, kInv>::run(w);
#pragma unroll
    for (int q1 = 0; q1 < R2; q1++)
    {
      const float2 t = (q1 == 0) ? w[0] : apply_tw<kInv>(w[q1], twl[j * G::TP + q1]);
      if (COLWRITE) lds[q1 * G::SF + j * G::NL + c] = t;
      else lds[j * G::SF + q1 * G::NL + c] = t;
    }
  }
  lds_barrier();
  if (ACTW(R2, j))
  {
#pragma unroll
    for (int k1 = 0; k1 < R1; k1++)
      v[k1] = COLWRITE ? lds[j * G::SF + k1 * G::NL + c] : lds[k1 * G::SF + j * G::NL + c];
    Dft<R1, kInv>::run(v);
  }
}

// =====================================================================================================================
// y-pass: in-place complex FFT along y (stride P) for tile (z = blockIdx.y, kx tile = blockIdx.x), array blockIdx.z
// =====================================================================================================================

// PIN / POUT: packed (per-peer chunk) addressing on the input / output side; the natural layout is the cheap
// compile-time-strided case  element(k) = base + k * P.  Both go through the launch's RowAddr (ain / aout), so the line
// loads and stores are this kernel's own; the tile is line_tile's.  The exchange is fwd_cols / fwd_rows spelt out (written
// with the two steps the compiler allocates a register more or less at most lengths, and an occupancy step with it at
// some).
//   per array:  [mul] write columns | next array's lines requested | barrier | read rows -> store | barrier (buffer reused)
template<int L, int DIR, bool PIN, bool POUT>
__global__ __launch_bounds__(Geo<L>::THREADS) void k_ypass(PassArgs a)
{
  using G = Geo<L>;
  constexpr int R1 = G::R1, R2 = G::R2;
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  load_twiddles<L>(twl, a.tw);
  // RowAddr addressing (natural or packed) is this kernel's own: zero strides leave t.lstride / t.base / t.basel inert;
  // only c, j, tc, pos and valid are used
  const LineTile t     = line_tile<G>(a.nxc, a.P, a.side_off, 0u, 0u, a.z0);
  if (t.tc.dead) return;
  const int      c     = t.c, j = t.j;
  const uint32_t kx    = t.tc.side ? 0u : t.tc.kx; // addressing column (side blocks: the one column of the side array)
  const uint32_t kxl   = t.tc.col;
  const uint32_t z     = t.pos;
  const uint32_t Pe    = t.tc.pitch, soff = t.tc.off; // row pitch / offset of the region (main rows, or the side array)
  const uint32_t PXe   = t.tc.side ? 1u : a.PX;       // the same on the packed (exchange) side: per-peer chunks of the side array
  const uint32_t arr0  = blockIdx.z * a.narr; // each block takes a.narr arrays back to back (next one's lines prefetched)

  auto ld = [&](float2 (&v)[R1], const float2* __restrict__ Sin) {
    if (PIN)
    {
#pragma unroll
      for (int n1 = 0; n1 < R1; n1++) v[n1] = Sin[a.ain.row(z, n1 * R2 + j) * PXe + kxl + soff];
    }
    else
    {
      uint32_t b = (z * a.ain.zmul + j * a.ain.estride) * Pe + kxl + soff; // estride = 1 (y lines) or ny (z probe)
      asm volatile("" : "+v"(b));
      const uint32_t step = R2 * a.ain.estride * Pe;
#pragma unroll
      for (int n1 = 0; n1 < R1; n1++)
        v[n1] = ld_uni(Sin, static_cast<uint64_t>(n1) * step, b * static_cast<uint32_t>(sizeof(float2)));
    }
  };

  float2 v[R1];
  if (ACTW(R2, j)) ld(v, a.in[arr0]);
  lds_barrier(); // twiddle table visible (the line loads stay in flight across it)
#pragma unroll 1
  for (uint32_t ia = 0; ia < a.narr; ia++)
  {
    if (ACTW(R2, j))
    {
      const float2* __restrict__ m = a.mul[arr0 + ia];
      if (m != nullptr)
      {
#pragma unroll
        for (int n1 = 0; n1 < R1; n1++) v[n1] = cmulf(v[n1], m[n1 * R2 + j]);
      }
      step_a<L, DIR>(v, j, twl);
#pragma unroll
      for (int k1 = 0; k1 < R1; k1++) lds[k1 * G::SF + j * G::NL + c] = v[k1];
      if (ia + 1 < a.narr) ld(v, a.in[arr0 + ia + 1]);
    }
    lds_barrier();
    if (ACTW(R1, j))
    {
      float2 w[R2];
#pragma unroll
      for (int n2 = 0; n2 < R2; n2++) w[n2] = lds[j * G::SF + n2 * G::NL + c];
      Dft<R2, DIR>::run(w);
      if (t.valid)
      {
        float2* __restrict__ Sout = a.out[arr0 + ia];
        if (POUT)
        {
#pragma unroll
          for (int k2 = 0; k2 < R2; k2++) Sout[a.aout.row(z, j + R1 * k2) * PXe + kx + soff] = w[k2];
        }
        else
        {
          uint32_t b = (z * a.aout.zmul + j * a.aout.estride) * Pe + kx + soff;
          asm volatile("" : "+v"(b));
          const uint32_t step = R1 * a.aout.estride * Pe;
#pragma unroll
          for (int k2 = 0; k2 < R2; k2++) st_uni(Sout, static_cast<uint64_t>(k2) * step, b * static_cast<uint32_t>(sizeof(float2)), w[k2]);
        }
      }
    }
    if (ia + 1 < a.narr) lds_barrier(); // exchange buffer reused by the next array
  }
}

// =====================================================================================================================
// z-fused: forward along z, spectral multiply, inverse along z.  Tile (y = blockIdx.y, kx tile = blockIdx.x).
// =====================================================================================================================
// Z_SHIFT: plain "transform along a line, multiply bin k by a complex H[k], transform back" on lines with arbitrary
// strides — the half-cell shift of a staggered velocity (computeVelocityShiftInY / InZ) done on pairs of real
// x-neighbours packed as one complex value
enum ZMode { Z_PGRAD = 0, Z_VGRAD = 1, Z_ABSORB = 2, Z_SOURCE = 3, Z_SHIFT = 4 };


// One block owns the z-lines of tile (ky = blockIdx.y, kx tile = blockIdx.x) of `narr` arrays (VGRAD: the three velocity
// spectra, ABSORB: the two pressure terms), processed back to back: the lines of array i+1 are in flight while array i
// is transformed, and kappa is fetched once for all three velocity components.  PGRAD has one input and three outputs.
// The body spells the line-tile steps out (see there for why): tile set-up = line_tile, opbase = op_run_base, the first
// load = load_lines, the exchange = fwd_cols / fwd_rows, the store = store_lines; its own are the operator multiply, the
// axis handling and the prefetch of the next array.
//   per array:  write columns | next array's lines requested | barrier | read rows -> multiply |
//               per output: inverse_from_regs -> store | barrier before the next output's inverse
template<int L, int MODE> __global__ __launch_bounds__((Geo<L, nl_z(L)>::THREADS), big_line_waves(L)) void k_zfused(ZArgs a)
{
  using G = Geo<L, nl_z(L)>;
  constexpr int R1 = G::R1, R2 = G::R2;
  constexpr bool WA = G::WA;
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  load_twiddles<L>(twl, a.tw);
  const int      c      = threadIdx.x % G::NL;
  const int      j      = threadIdx.x / G::NL;
  const TileCoord tc    = tile_coord<G::NL>(a.nxc, a.P, (MODE == Z_SHIFT) ? 0u : a.side_off, gridDim.y, c);
  if (tc.dead) return;
  const uint32_t ky     = tc.pos;
  const bool     valid  = tc.valid;
  const uint32_t zstr   = (MODE == Z_SHIFT) ? a.lstride : a.ny * tc.pitch;
  const uint32_t bstr   = (MODE == Z_SHIFT) ? a.bstride : tc.pitch;
  const uint32_t kxl    = tc.kx < a.nxc ? tc.kx : (tc.side ? a.nxc : a.nxc - 1u); // true column (ddx lookups)
  const uint32_t base   = ky * bstr + (tc.side ? 0u : tc.kx) + tc.off;
  const uint32_t basel  = ky * bstr + tc.col + tc.off;
  // operators live in a tile-blocked layout [ky][kx tile][kz][16]: the 16 x nz values of this block's tile are one
  // contiguous run (k_import_reduced), instead of 64-B pieces a whole plane apart
  constexpr int  OPV    = op_vec(R2);
  // side blocks: the side column's operator values are stored like one more row of tiles whose columns are the ky
  const uint32_t opbase = tc.side ? a.op_side_off + (((ky / NLMAX) * (R2 / OPV) * R1 + j) * NLMAX + ky % NLMAX) * OPV
                                  : (((ky * (a.Pop / NLMAX) + tc.col / NLMAX) * (R2 / OPV) * R1 + j) * NLMAX + tc.col % NLMAX) * OPV;
  constexpr bool MULTI  = (MODE == Z_VGRAD || MODE == Z_ABSORB);
  const uint32_t arr0   = MULTI ? a.arr0 + blockIdx.z * a.narr : 0; // (grid.z > 1: small grids, one array per block)
  const uint32_t narr   = MULTI ? a.narr : 1;
  // PGRAD: the x- and y-gradients share one z-inverse — ddx(kx), ddy(ky) do not depend on kz, so they are applied after
  // the way back (y-pass / x-pass); only Q = F_z^-1{kappa X} and G_z = F_z^-1{ddz kappa X} leave this kernel
  constexpr int  NOUT   = (MODE == Z_PGRAD) ? 2 : 1;

  float2 v[R1];
  const float2* __restrict__ in0 = a.in[arr0]; // (array pointers are picked outside the thread-dependent regions: SGPR bases)
  if (ACTW(R2, j))
  {
    const float2* __restrict__ in = in0;
    const uint32_t lb = (basel + static_cast<uint32_t>(j) * zstr) * static_cast<uint32_t>(sizeof(float2));
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++)
      v[n1] = ld_uni<WA>(in, static_cast<uint64_t>(n1 * R2) * zstr, lb);
  }
  // spectral operator of the elements this thread will hold after the forward transform (kz = j + R1*k2)
  float kap[R2];
  if (MODE != Z_SHIFT && ACTW(R1, j))
  {
    load_op_run<R2, R1>(kap, a.op[(MODE == Z_ABSORB) ? arr0 : 0], opbase);
  }
  lds_barrier(); // twiddle table visible (the loads above stay in flight across it)

#pragma unroll 1
  for (uint32_t ia = 0; ia < narr; ia++)
  {
    const uint32_t arr = arr0 + ia;
    const float2* __restrict__ in_next = a.in[min(arr + 1u, arr0 + narr - 1u)];
    if (ACTW(R2, j))
    {
      step_a<L, kFwd>(v, j, twl);
#pragma unroll
      for (int k1 = 0; k1 < R1; k1++) lds[k1 * G::SF + j * G::NL + c] = v[k1];
    }
    // next array's lines: in flight during this array's two transforms
    if (MULTI && ia + 1 < narr && ACTW(R2, j))
    {
      const float2* __restrict__ in = in_next;
      uint32_t lb = basel + static_cast<uint32_t>(j) * zstr;
      asm volatile("" : "+v"(lb)); // per-iteration address arithmetic instead of 16 loop-invariant address registers
#pragma unroll
      for (int n1 = 0; n1 < R1; n1++)
        v[n1] = ld_uni<WA>(in, static_cast<uint64_t>(n1 * R2) * zstr, lb * static_cast<uint32_t>(sizeof(float2)));
    }
    lds_barrier();
    float2 X[R2];
    if (ACTW(R1, j))
    {
#pragma unroll
      for (int n2 = 0; n2 < R2; n2++) X[n2] = lds[j * G::SF + n2 * G::NL + c];
      Dft<R2, kFwd>::run(X);
      //   Z_PGRAD  SolverCudaKernels.cu:1149-1155  e = X*kappa;            out_d = e (x) dd_d_pos
      //   Z_VGRAD  :1220-1236                      e = X*(kappa*divider);  out   = e (x) dd_neg of this array's own axis
      //   Z_ABSORB :1817-1818                      out = X*nabla
      //   Z_SOURCE :742-744                        out = X*(sourceKappa*divider)
      if (MODE == Z_SHIFT)
      { // SolverCudaKernels.cu:2617-2710: bin k times shift[k] / N (both folded into H by the host)
#pragma unroll
        for (int k2 = 0; k2 < R2; k2++) X[k2] = cmulf(X[k2], a.dd[2][j + R1 * k2]);
      }
      else
      {
#pragma unroll
        for (int k2 = 0; k2 < R2; k2++)
        {
          float sc = kap[k2];
          if (MODE == Z_VGRAD || MODE == Z_SOURCE) sc *= a.divider;
          X[k2] = make_float2(X[k2].x * sc, X[k2].y * sc);
        }
      }
      if (MODE == Z_ABSORB && ia + 1 < narr)
      {
        uint32_t lb = opbase;
        asm volatile("" : "+v"(lb));
        load_op_run<R2, R1>(kap, a.op[arr + 1], lb);
      }
    }

#pragma unroll 1
    for (int o = 0; o < NOUT; o++)
    {
      float2 w[R2];
      if (ACTW(R1, j))
      {
        if (MODE == Z_PGRAD || MODE == Z_VGRAD)
        {
          const uint32_t axis = (MODE == Z_PGRAD) ? (o == 0 ? 3u : 2u) : a.axis_of[arr];
          if (axis == 3)
          {
#pragma unroll
            for (int k2 = 0; k2 < R2; k2++) w[k2] = X[k2];
          }
          else if (axis == 2)
          {
            uint32_t jz = j;
            asm volatile("" : "+v"(jz)); // keeps the 16 ddz loads inside this pass instead of hoisted registers
#pragma unroll
            for (int k2 = 0; k2 < R2; k2++) w[k2] = cmulf(X[k2], a.dd[2][jz + R1 * k2]);
          }
          else
          {
            const float2 dxy = (axis == 0) ? a.dd[0][kxl] : a.dd[1][ky + a.ky0];
#pragma unroll
            for (int k2 = 0; k2 < R2; k2++) w[k2] = cmulf(X[k2], dxy);
          }
        }
        else
        {
#pragma unroll
          for (int k2 = 0; k2 < R2; k2++) w[k2] = X[k2];
        }
      }
      float2 r[R1];
      inverse_from_regs<L, false, G::NL>(w, r, lds, c, j, twl);
      float2* __restrict__ out = a.out[(MODE == Z_PGRAD) ? 2 * o : arr];
      if (ACTW(R2, j) && valid)
      {
        uint32_t ob = base + static_cast<uint32_t>(j) * zstr;
        asm volatile("" : "+v"(ob)); // recomputed per output: 16 hoisted 64-bit addresses cost an occupancy step
#pragma unroll
        for (int q2 = 0; q2 < R1; q2++) st_uni<WA>(out, static_cast<uint64_t>(R2 * q2) * zstr, ob * static_cast<uint32_t>(sizeof(float2)), r[q2]);
      }
      // the next output's inverse writes rows while other threads may still read their columns: barrier; the next
      // array's forward transform writes the column this thread has just read: none
      if (o + 1 < NOUT) lds_barrier();
    }
  }
}

// =====================================================================================================================
// Lines of 512 = 2 x 256.  One radix-2 decimation-in-frequency stage in registers around two 256-point four-step
// transforms that use the block's exchange buffer one after the other:
//   forward / standalone (either sign):  a[n] = x[n] + x[n+H],  b[n] = (x[n] - x[n+H]) * W_L^(DIR*n),
//                                        X[2k] = F_H(a)[k],     X[2k+1] = F_H(b)[k]
//   inverse started from spectrum registers:  a = F_H^-1(X[2k]),  b = F_H^-1(X[2k+1]),
//                                        x[n] = a[n] + W_L^(+n) b[n],   x[n+H] = a[n] - W_L^(+n) b[n]
// 16 lines x 16 threads with 32 elements per thread: the tile width (128-B segments), block size and LDS footprint of the
// 256-point kernels, instead of 32-point register DFTs whose register demand leaves one or two waves per SIMD.
// =====================================================================================================================
template<int L> __device__ __forceinline__ void load_twiddles_split(float2* twl, float2* tw2, const float2* __restrict__ tw)
{
  using G = Geo<L / 2>;
  for (int e = threadIdx.x; e < G::R1 * G::R2; e += G::THREADS)
  {
    const int k = e / G::R2, n = e - k * G::R2;
    twl[k * G::TP + n] = tw[2 * k * n]; // W_H^(kn) = W_L^(2kn)
  }
  for (int e = threadIdx.x; e < L / 2; e += G::THREADS) tw2[e] = tw[e];
}

// The steps of the split lines' z-passes (every thread of the block is a column and a row thread of the H-point
// transforms).  The lower and the upper half of the thread's line: x[n1 * R2 + j] in va, x[H + n1 * R2 + j] in vb ...
template<int L>
__device__ __forceinline__ void load_split_halves(float2 (&va)[Fac<L / 2>::R1], float2 (&vb)[Fac<L / 2>::R1],
                                                  const float2* __restrict__ in, const LineTile& t)
{
  constexpr int H = L / 2;
  using G = Geo<H>;
  const uint32_t lb = (t.basel + static_cast<uint32_t>(t.j) * t.lstride) * static_cast<uint32_t>(sizeof(float2));
#pragma unroll
  for (int n1 = 0; n1 < G::R1; n1++)
  {
    va[n1] = ld_uni(in, static_cast<uint64_t>(n1 * G::R2) * t.lstride, lb);
    vb[n1] = ld_uni(in, static_cast<uint64_t>(H + n1 * G::R2) * t.lstride, lb);
  }
}
// ... their radix-2 stage on the way in, once tw2 is visible: va <- a, vb <- b, the step-A registers of the two halves
template<int L>
__device__ __forceinline__ void split_butterfly(float2 (&va)[Fac<L / 2>::R1], float2 (&vb)[Fac<L / 2>::R1], int j, const float2* tw2)
{
  using G = Geo<L / 2>;
#pragma unroll
  for (int n1 = 0; n1 < G::R1; n1++)
  {
    const float2 lo = va[n1], hi = vb[n1];
    va[n1] = cadd(lo, hi);
    vb[n1] = apply_tw<kFwd>(csub(lo, hi), tw2[n1 * G::R2 + j]);
  }
}
// ... and the recombination of the two inverse halves ra = a[j + R2 * q2], rb = b[j + R2 * q2] on the way out
template<int L>
__device__ __forceinline__ void store_split_halves(float2* __restrict__ out, const LineTile& t, const float2 (&ra)[Fac<L / 2>::R1],
                                                   const float2 (&rb)[Fac<L / 2>::R1], const float2* tw2)
{
  constexpr int H = L / 2;
  using G = Geo<H>;
  if (t.valid)
  {
    uint32_t ob = t.base + static_cast<uint32_t>(t.j) * t.lstride;
    asm volatile("" : "+v"(ob)); // (see store_lines)
#pragma unroll
    for (int q2 = 0; q2 < G::R1; q2++)
    { // n = j + R2*q2
      const float2 w = apply_tw<kInv>(rb[q2], tw2[t.j + G::R2 * q2]);
      st_uni(out, static_cast<uint64_t>(G::R2 * q2) * t.lstride, ob * static_cast<uint32_t>(sizeof(float2)), cadd(ra[q2], w));
      st_uni(out, static_cast<uint64_t>(H + G::R2 * q2) * t.lstride, ob * static_cast<uint32_t>(sizeof(float2)), csub(ra[q2], w));
    }
  }
}

// The y-pass of the split lines: forward-only (no recombination), with the optional factor folded into its radix-2
// stage, and RowAddr addressing on both sides as in k_ypass — so the halves' loads and stores are its own.
template<int L, int DIR, bool PIN, bool POUT>
__global__ __launch_bounds__(Geo<L / 2>::THREADS) void k_ypass_split(PassArgs a)
{
  constexpr int H = L / 2;
  using G = Geo<H>;
  constexpr int R1 = G::R1, R2 = G::R2;
  static_assert(R1 == R2 && G::TPL == R1 && H == R1 * R2, "split lines are built on the balanced 256-point transform");
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  __shared__ float2 tw2[H];
  load_twiddles_split<L>(twl, tw2, a.tw);
  // RowAddr addressing (natural or packed) is this kernel's own: zero strides leave t.lstride / t.base / t.basel inert;
  // only c, j, tc, pos and valid are used
  const LineTile t     = line_tile<G>(a.nxc, a.P, a.side_off, 0u, 0u, a.z0);
  if (t.tc.dead) return;
  const int      c     = t.c, j = t.j;
  const uint32_t kx    = t.tc.side ? 0u : t.tc.kx;
  const bool     valid = t.valid;
  const uint32_t kxl   = t.tc.col;
  const uint32_t z     = t.pos;
  const uint32_t Pe    = t.tc.pitch, soff = t.tc.off;
  const uint32_t PXe   = t.tc.side ? 1u : a.PX;
  const float2* __restrict__ Sin = a.in[blockIdx.z];
  float2* __restrict__ Sout      = a.out[blockIdx.z];

  float2 va[R1], vb[R1];
  if (PIN)
  {
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++)
    {
      va[n1] = Sin[a.ain.row(z, n1 * R2 + j) * PXe + kxl + soff];
      vb[n1] = Sin[a.ain.row(z, H + n1 * R2 + j) * PXe + kxl + soff];
    }
  }
  else
  {
    const uint32_t b    = (z * a.ain.zmul + j * a.ain.estride) * Pe + kxl + soff;
    const uint32_t step = R2 * a.ain.estride * Pe;
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++)
    {
      va[n1] = ld_uni(Sin, static_cast<uint64_t>(n1) * step, b * static_cast<uint32_t>(sizeof(float2)));
      vb[n1] = ld_uni(Sin, static_cast<uint64_t>(R1 + n1) * step, b * static_cast<uint32_t>(sizeof(float2)));
    }
  }
  lds_barrier(); // twiddle tables visible (the line loads stay in flight across it)
  const float2* __restrict__ m = a.mul[blockIdx.z];
#pragma unroll
  for (int n1 = 0; n1 < R1; n1++)
  {
    float2 lo = va[n1], hi = vb[n1];
    if (m != nullptr) { lo = cmulf(lo, m[n1 * R2 + j]); hi = cmulf(hi, m[H + n1 * R2 + j]); }
    va[n1] = cadd(lo, hi);
    vb[n1] = apply_tw<DIR>(csub(lo, hi), tw2[n1 * R2 + j]);
  }
  float2 wa[R2], wb[R2];
  line_fft<H, DIR>(va, wa, lds, c, j, twl);
  line_fft<H, DIR, true>(vb, wb, lds, c, j, twl); // writes the rows the first transform just read: no barrier
  if (valid)
  {
    if (POUT)
    {
#pragma unroll
      for (int k2 = 0; k2 < R2; k2++)
      {
        Sout[a.aout.row(z, 2 * (j + R1 * k2)) * PXe + kx + soff]     = wa[k2];
        Sout[a.aout.row(z, 2 * (j + R1 * k2) + 1) * PXe + kx + soff] = wb[k2];
      }
    }
    else
    {
      const uint32_t b    = (z * a.aout.zmul + 2 * j * a.aout.estride) * Pe + kx + soff;
      const uint32_t one  = a.aout.estride * Pe;
      const uint32_t step = 2 * R1 * one;
#pragma unroll
      for (int k2 = 0; k2 < R2; k2++)
      {
        st_uni(Sout, static_cast<uint64_t>(k2) * step, b * static_cast<uint32_t>(sizeof(float2)), wa[k2]);
        st_uni(Sout, static_cast<uint64_t>(k2) * step + one, b * static_cast<uint32_t>(sizeof(float2)), wb[k2]);
      }
    }
  }
}

template<int L, int MODE> __global__ __launch_bounds__(Geo<L / 2>::THREADS) void k_zfused_split(ZArgs a)
{
  constexpr int H = L / 2;
  using G = Geo<H>;
  constexpr int R1 = G::R1, R2 = G::R2;
  static_assert(R1 == R2 && G::TPL == R1 && H == R1 * R2, "split lines are built on the balanced 256-point transform");
  __shared__ float2 lds[G::LDSB];
  __shared__ float2 twl[G::TWN];
  __shared__ float2 tw2[H];
  load_twiddles_split<L>(twl, tw2, a.tw);
  const LineTile t      = line_tile<G>(a.nxc, a.P, a.side_off, a.ny, 1u);
  if (t.tc.dead) return;
  const int      c      = t.c, j = t.j;
  const uint32_t ky     = t.pos;
  const uint32_t kxl    = t.tc.kx < a.nxc ? t.tc.kx : (t.tc.side ? a.nxc : a.nxc - 1u); // true column (ddx lookups)
  const uint32_t opbase = op_run_base<2 * R2, R1>(t, a.Pop, a.op_side_off); // run: bins 2*(j + R1*k2) + h at run index 2*k2 + h
  constexpr bool MULTI  = (MODE == Z_VGRAD || MODE == Z_ABSORB);
  const uint32_t arr    = MULTI ? a.arr0 + blockIdx.z : 0;
  // PGRAD: the x- and y-gradients share one z-inverse — ddx(kx), ddy(ky) do not depend on kz, so they are applied after
  // the way back (y-pass / x-pass); only Q = F_z^-1{kappa X} and G_z = F_z^-1{ddz kappa X} leave this kernel
  constexpr int  NOUT   = (MODE == Z_PGRAD) ? 2 : 1;

  float2 Xa[R2], Xb[R2]; // after the forward transform: X[2*(j + R1*k2)], X[2*(j + R1*k2) + 1]
  {
    float2 va[R1], vb[R1];
    load_split_halves<L>(va, vb, a.in[arr], t);
    lds_barrier(); // twiddle tables visible
    split_butterfly<L>(va, vb, j, tw2);
    // four exchanges per line and output (two forward, two inverse halves), each writing exactly the cells its thread
    // read in the one before (column / row / column / row ...): the only barriers left are the ones inside them
    line_fft<H, kFwd>(va, Xa, lds, c, j, twl);
    line_fft<H, kFwd, true>(vb, Xb, lds, c, j, twl);
  }
  { // spectral operator (see k_zfused for the reference lines), kz = 2*(j + R1*k2) (+1)
    float run[2 * R2];
    load_op_run<2 * R2, R1>(run, a.op[(MODE == Z_ABSORB) ? arr : 0], opbase);
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++)
    {
      float sa = run[2 * k2];
      float sb = run[2 * k2 + 1];
      if (MODE == Z_VGRAD || MODE == Z_SOURCE) { sa *= a.divider; sb *= a.divider; }
      Xa[k2] = make_float2(Xa[k2].x * sa, Xa[k2].y * sa);
      Xb[k2] = make_float2(Xb[k2].x * sb, Xb[k2].y * sb);
    }
  }
#pragma unroll 1
  for (int o = 0; o < NOUT; o++)
  {
    const uint32_t axis = (MODE == Z_PGRAD) ? (o == 0 ? 3u : 2u) : a.axis_of[arr];
    float2 ra[R1], rb[R1];
#pragma unroll
    for (int half = 0; half < 2; half++)
    {
      float2 w[R2];
      if (MODE == Z_PGRAD || MODE == Z_VGRAD)
      {
        if (axis == 3)
        {
#pragma unroll
          for (int k2 = 0; k2 < R2; k2++) w[k2] = half ? Xb[k2] : Xa[k2];
        }
        else if (axis == 2)
        {
          uint32_t jz = 2 * j + half;
          asm volatile("" : "+v"(jz));
#pragma unroll
          for (int k2 = 0; k2 < R2; k2++) w[k2] = cmulf(half ? Xb[k2] : Xa[k2], a.dd[2][jz + 2 * R1 * k2]);
        }
        else
        {
          const float2 dxy = (axis == 0) ? a.dd[0][kxl] : a.dd[1][ky + a.ky0];
#pragma unroll
          for (int k2 = 0; k2 < R2; k2++) w[k2] = cmulf(half ? Xb[k2] : Xa[k2], dxy);
        }
      }
      else
      {
#pragma unroll
        for (int k2 = 0; k2 < R2; k2++) w[k2] = half ? Xb[k2] : Xa[k2];
      }
      if (half == 0) inverse_from_regs<H, true>(w, ra, lds, c, j, twl); // after a read by columns: write columns
      else inverse_from_regs<H>(w, rb, lds, c, j, twl);                  // after a read by rows: write rows
    }
    store_split_halves<L>(a.out[(MODE == Z_PGRAD) ? 2 * o : arr], t, ra, rb, tw2);
  }
}

// =====================================================================================================================
// x-forward: two real rows per complex line -> two half-spectrum rows
// =====================================================================================================================

// The x kernels work on tiles of 2 * NL rows.  A grid whose row count ny * nz is not a whole number of tiles ends in a
// partial tile: that one tile is launched on its own with TAIL = true — row loads clamp to the last row, every store is
// predicated on the row — so the full tiles keep their unmasked kernels.

// forward line FFT of this block's 16 complex lines (= 32 real rows) from the step-A registers v (of role XRole<G, R2>),
// split into the two half-spectra and stored to rows tile_row0.. of `out`.  Called by every thread of the block; the
// exchange buffer must be free on entry and is free again on exit (trailing barrier).
// NLX: line pairs per block.  PLANE (the tile is a whole z-plane, see k_xinv): the half-spectrum rows go to the block's
// plane buffer in LDS ([row][L / 2 + 1], `out`) instead of to the scratch array.
template<int L, bool TAIL = false, int NLX = nl_x(L), bool PLANE = false>
__device__ __forceinline__ void xfwd_tail(float2 (&v)[Fac<L>::R1], float2* lds,
                                          const float2* tw, float2* __restrict__ out, uint32_t P, uint32_t tile,
                                          uint32_t nrows = 0, uint32_t side_off = 0)
{
  using G = Geo<L, NLX>;
  constexpr int R1 = G::R1, R2 = G::R2, HALF = L / 2 + 1;
  const XRole<G, R2> sa; // v: the step-A registers of line sa.c, column sa.f
  const XRole<G, R1> sb;
  if (sa.on)
  {
    step_a<L, kFwd>(v, sa.f, tw);
#pragma unroll
    for (int k1 = 0; k1 < R1; k1++) lds[sa.c * G::LP + k1 * (R2 + 1) + sa.f] = v[k1];
  }
  lds_barrier();
  float2 w[R2];
  if (sb.on)
  {
#pragma unroll
    for (int n2 = 0; n2 < R2; n2++) w[n2] = lds[sb.c * G::LP + sb.f * (R2 + 1) + n2];
    Dft<R2, kFwd>::run(w);
  }
  lds_barrier();
  if (sb.on)
  {
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++) lds[sb.c * G::ZP + sb.f + R1 * k2] = w[k2];
  }
  lds_barrier();
  const uint32_t tile_row0 = tile * G::NL * 2;
  for (int e = threadIdx.x; e < G::NL * HALF; e += G::THREADS)
  {
    const int    cc = e / HALF;
    const int    k  = e - cc * HALF;
    const float2 zk = lds[cc * G::ZP + k];
    const float2 zn = lds[cc * G::ZP + (k == 0 ? 0 : L - k)];
    const float2 xa = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
    const float2 xb = make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x));
    if (PLANE)
    {
      out[(2 * cc) * HALF + k]     = xa;
      out[(2 * cc + 1) * HALF + k] = xb;
      continue;
    }
    const uint32_t r = tile_row0 + 2 * cc;
    // the x-Nyquist bin of a row goes to the side array N[row] when the pipeline keeps that column apart (tile_coord)
    const bool     ny_bin = (side_off != 0) && (k == L / 2);
    const uint32_t ia = ny_bin ? side_off + r : r * P + k;
    const uint32_t ib = ny_bin ? ia + 1u : ia + P;
    if (!TAIL || r < nrows) out[ia] = xa;
    if (!TAIL || r + 1 < nrows) out[ib] = xb;
  }
  lds_barrier();
}

template<int L, bool TAIL = false> __global__ __launch_bounds__(GeoX<L>::THREADS) void k_xfwd(XfwdArgs a)
{
  using G = GeoX<L>;
  constexpr int R1 = G::R1, R2 = G::R2;
  __shared__ float2 lds[G::LDSX];
  __shared__ float2 twl[G::TWN];
  load_twiddles<L>(twl, a.tw);
  const XRole<G, R2> sa;
  const float* __restrict__ in = a.in[blockIdx.y];
  const uint32_t tile = blockIdx.x + a.tile0;
  const uint32_t row0 = (tile * G::NL + sa.c) * 2;
  float2 v[R1];
  if (sa.on)
  {
    const float* __restrict__ ra = in + (TAIL ? min(row0, a.nrows - 1u) : row0) * L;
    const float* __restrict__ rb = TAIL ? in + min(row0 + 1u, a.nrows - 1u) * L : ra + L;
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++) v[n1] = make_float2(ra[n1 * R2 + sa.f], rb[n1 * R2 + sa.f]);
  }
  lds_barrier(); // twiddle table visible
  xfwd_tail<L, TAIL>(v, lds, twl, a.out[blockIdx.y], a.P, tile, a.nrows, a.side_off);
}

// =====================================================================================================================
// x-inverse + epilogue
// =====================================================================================================================
enum Epi { EPI_STORE = 0, EPI_VELOCITY = 1, EPI_INITVEL = 2, EPI_DENSITY = 3, EPI_PSUM = 4, EPI_PSUM1 = 5 };

// Line lengths whose density and pressure-sum epilogues let values wait in the real tile in LDS instead of in registers
// (see k_xinv: LAST_IN_LDS, FW0_IN_LDS, FRESH_XT): the pressure sum's chained row, the density epilogue's last inverse,
// the pressure sum's last inverse.  On where it buys an occupancy step at no scratch AND measures faster (DESIGN.md
// §3b, §6: 256 so far; the register table of the other lengths is there); a length left off compiles to the kernels it
// had before.  (tuning builds: -DKW_TUNE_XLDS=<bits> overrides the three tables for every length: 1, 2, 4 in that
// order; -DKW_TUNE_XWAVES=<n> the waves per SIMD asked for the two epilogues)
#ifdef KW_TUNE_XLDS
constexpr bool psum_row_in_lds(int) { return (KW_TUNE_XLDS & 1) != 0; }
constexpr bool last_inverse_in_lds(int) { return (KW_TUNE_XLDS & 2) != 0; }
constexpr bool psum_last_in_lds(int) { return (KW_TUNE_XLDS & 4) != 0; }
#else
constexpr bool psum_row_in_lds(int L) { return L == 256; }
constexpr bool last_inverse_in_lds(int L) { return L == 256; }
constexpr bool psum_last_in_lds(int) { return false; }
#endif
// waves per SIMD asked of the allocator.  256 points: the LDS forms of the two epilogues fit the 128 registers of four
// waves with no scratch, but the allocator only aims for them when asked; the register form of the density epilogue sits
// two registers above the three-wave step
constexpr int xinv_waves(int L, int EPI)
{
#ifdef KW_TUNE_XWAVES
  if (EPI == EPI_DENSITY || EPI == EPI_PSUM) return KW_TUNE_XWAVES;
#endif
  if (L == 256 && EPI == EPI_DENSITY) return last_inverse_in_lds(L) ? 4 : 3;
  if (L == 256 && EPI == EPI_PSUM && psum_row_in_lds(L)) return 4;
  return big_line_waves(L);
}


// standalone inverse of one array for this block's 32 rows; the thread of role sb = XRole<G, R1> ends with
// x[sb.f + R1*k2] of rows (2 sb.c, 2 sb.c + 1)
// PLANE: the rows come from the block's plane buffer in LDS ([row][L / 2 + 1], `src`), where the y-inverse left them
template<int L, int NGRP = 1, bool TAIL = false, int NLX = nl_x(L), bool PLANE = false, bool FRESH = false>
__device__ __forceinline__ void xinv_lines(const float2* __restrict__ src, uint32_t P, float2* lds,
                                           const float2* tw, float2 (&w)[Fac<L>::R2], uint32_t tile,
                                           const float2* __restrict__ mulx = nullptr, uint32_t nrows = 0,
                                           uint32_t side_off = 0)
{
  using G = Geo<L, NLX>;
  constexpr int R1 = G::R1, R2 = G::R2, HALF = L / 2 + 1;
  const uint32_t tile_row0 = tile * G::NL * 2;
  // all row loads of the tile are requested before the first one is consumed (a load-use loop would expose the memory
  // latency once per iteration); the last, partial iteration re-reads the final element instead of being predicated
  constexpr int NE = (G::NL * HALF + G::THREADS - 1) / G::THREADS;
  constexpr int NG = (NE + NGRP - 1) / NGRP; // iterations per group (NGRP > 1: fewer loads in flight, fewer registers)
  // FRESH: the row offsets are worked out again for every array of a multi-array kernel instead of waiting in registers
  int tx = static_cast<int>(threadIdx.x);
  if (FRESH) asm volatile("" : "+v"(tx));
#pragma unroll
  for (int g0 = 0; g0 < NE; g0 += NG)
  {
    float2 A[NG], B[NG];
#pragma unroll
    for (int it = 0; it < NG; it++)
    {
      const int e  = min(tx + (g0 + it) * G::THREADS, G::NL * HALF - 1);
      const int cc = e / HALF;
      const int k  = e - cc * HALF;
      const uint32_t r = tile_row0 + 2 * cc;
      const uint32_t ra = TAIL ? min(r, nrows - 1u) : r, rb = TAIL ? min(r + 1u, nrows - 1u) : r + 1u;
      if (PLANE)
      {
        A[it] = src[(2 * cc) * HALF + k];
        B[it] = src[(2 * cc + 1) * HALF + k];
        continue;
      }
      const bool     ny_bin = (side_off != 0) && (k == L / 2); // the x-Nyquist bin lives in the side array N[row]
      A[it] = src[ny_bin ? side_off + ra : ra * P + k];
      B[it] = src[ny_bin ? side_off + rb : rb * P + k];
    }
#pragma unroll
    for (int it = 0; it < NG; it++)
    {
      const int e = static_cast<int>(threadIdx.x) + (g0 + it) * G::THREADS;
      if (g0 + it < NE && e < G::NL * HALF)
      {
        const int cc = e / HALF;
        const int k  = e - cc * HALF;
        float2 a = A[it], b = B[it];
        if (mulx != nullptr) { const float2 d = mulx[k]; a = cmulf(a, d); b = cmulf(b, d); }
        if (k == 0 || k == L / 2) { a.y = 0.f; b.y = 0.f; } // C2R ignores the imaginary part of DC / Nyquist
        lds[cc * G::ZP + k] = make_float2(a.x - b.y, a.y + b.x);
        if (k != 0 && k != L / 2) lds[cc * G::ZP + L - k] = make_float2(a.x + b.y, b.x - a.y);
      }
    }
  }
  lds_barrier();
  const XRole<G, R2> sa;
  const XRole<G, R1> sb;
  float2 v[R1];
  if (sa.on)
  {
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++) v[n1] = lds[sa.c * G::ZP + n1 * R2 + sa.f];
  }
  lds_barrier();
  if (sa.on)
  {
    step_a<L, kInv>(v, sa.f, tw);
#pragma unroll
    for (int k1 = 0; k1 < R1; k1++) lds[sa.c * G::LP + k1 * (R2 + 1) + sa.f] = v[k1];
  }
  lds_barrier();
  if (sb.on)
  {
#pragma unroll
    for (int n2 = 0; n2 < R2; n2++) w[n2] = lds[sb.c * G::LP + sb.f * (R2 + 1) + n2];
    Dft<R2, kInv>::run(w);
  }
  lds_barrier();
}

__device__ __forceinline__ float  f4get(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ void   f4put(float4& v, int k, float s)
{
  if (k == 0) v.x = s; else if (k == 1) v.y = s; else if (k == 2) v.z = s; else v.w = s;
}


// ---- small grids: a whole z-plane per block -------------------------------------------------------------------------------
// When a half-spectrum plane [L][L / 2 + 1] (Nx == Ny == L <= 64) fits the LDS next to the x kernels' line buffers, the
// block of an x-inverse + epilogue kernel takes a whole plane as its tile and does the plane's y transforms itself: the
// y-inverse of every input array before its x-inverse, the y-forward of every chained array after its x-forward — same
// small DFTs, same twiddles, same order of operations as k_ypass (bit-identical results), but the stage's tail is ONE
// launch instead of three.  32^3 and 64^3 are bound by launches and by kernels that are over before the chip has filled
// (13 kernels of 5-15 us per step): this takes six of them away and the spectra of a stage's tail never leave the CU.
// plane buffer Y[ky][kx], kx < L / 2 + 1 (the x-Nyquist bin sits in its row here: no side array in LDS)
template<int L> __device__ __forceinline__ void plane_load(float2* Y, const float2* __restrict__ src, uint32_t plane, uint32_t P,
                                                           uint32_t side_off, const float2* __restrict__ mul, int threads)
{ // rows plane*L .. of the scratch array (+ their side-array bins) -> Y, times mul[ky] where given (ddy of the gradient)
  constexpr int HALF = L / 2 + 1;
  const uint32_t row0 = plane * L;
  if (side_off != 0)
  { // rows of exactly L / 2 bins
    for (int e = threadIdx.x; e < L * (L / 2); e += threads)
    {
      const int ky = e / (L / 2), k = e % (L / 2);
      float2 v = src[(row0 + ky) * P + k];
      if (mul != nullptr) v = cmulf(v, mul[ky]);
      Y[ky * HALF + k] = v;
    }
    for (int ky = threadIdx.x; ky < L; ky += threads)
    {
      float2 v = src[side_off + row0 + ky];
      if (mul != nullptr) v = cmulf(v, mul[ky]);
      Y[ky * HALF + L / 2] = v;
    }
  }
  else
  {
    for (int e = threadIdx.x; e < L * HALF; e += threads)
    {
      const int ky = e / HALF, k = e - ky * HALF;
      float2 v = src[(row0 + ky) * P + k];
      if (mul != nullptr) v = cmulf(v, mul[ky]);
      Y[e] = v;
    }
  }
}
template<int L> __device__ __forceinline__ void plane_store(const float2* Y, float2* __restrict__ dst, uint32_t plane, uint32_t P,
                                                            uint32_t side_off, int threads)
{
  constexpr int HALF = L / 2 + 1;
  const uint32_t row0 = plane * L;
  if (side_off != 0)
  {
    for (int e = threadIdx.x; e < L * (L / 2); e += threads)
    {
      const int ky = e / (L / 2), k = e % (L / 2);
      dst[(row0 + ky) * P + k] = Y[ky * HALF + k];
    }
    for (int ky = threadIdx.x; ky < L; ky += threads) dst[side_off + row0 + ky] = Y[ky * HALF + L / 2];
  }
  else
  {
    for (int e = threadIdx.x; e < L * HALF; e += threads)
    {
      const int ky = e / HALF, k = e - ky * HALF;
      dst[(row0 + ky) * P + k] = Y[e];
    }
  }
}
// in-place transform of the L / 2 + 1 columns of Y along y: the four-step of k_ypass with the plane buffer itself as the
// exchange buffer.  (L / 2) * TPL threads: thread (c, j) of the main columns, then the first TPL threads once more for the
// x-Nyquist column.  Y must be complete on entry (barrier before); complete again on exit (trailing barrier).
template<int L, int DIR> __device__ __forceinline__ void plane_yfft(float2* Y, const float2* twl)
{
  using G = Geo<L, L / 2>;
  constexpr int R1 = G::R1, R2 = G::R2, HALF = L / 2 + 1, TPL = G::TPL;
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++)
  {
    const bool on = (pass == 0) || (threadIdx.x < TPL);
    const int  c  = (pass == 0) ? static_cast<int>(threadIdx.x) % (L / 2) : L / 2;
    const int  j  = (pass == 0) ? static_cast<int>(threadIdx.x) / (L / 2) : static_cast<int>(threadIdx.x);
    if (on && ACT(R2, j))
    { // step A on rows n1 * R2 + j; the results go back to the same cells (index k1 in place of n1)
      float2 v[R1];
#pragma unroll
      for (int n1 = 0; n1 < R1; n1++) v[n1] = Y[(n1 * R2 + j) * HALF + c];
      step_a<L, DIR>(v, j, twl);
#pragma unroll
      for (int k1 = 0; k1 < R1; k1++) Y[(k1 * R2 + j) * HALF + c] = v[k1];
    }
    lds_barrier();
    float2 w[R2];
    if (on && ACT(R1, j))
    {
#pragma unroll
      for (int n2 = 0; n2 < R2; n2++) w[n2] = Y[(j * R2 + n2) * HALF + c];
      Dft<R2, DIR>::run(w);
    }
    lds_barrier(); // every cell has been read before the natural-order results overwrite them
    if (on && ACT(R1, j))
    {
#pragma unroll
      for (int k2 = 0; k2 < R2; k2++) Y[(j + R1 * k2) * HALF + c] = w[k2];
    }
    lds_barrier();
  }
}
// (128: one 1024-thread block per CU, held to 128 VGPRs — measured 14 % slower than the three-launch form; 32 and 64 gain)
constexpr bool plane_len(int L) { return L == 32 || L == 64; }

// The inverse leaves each thread with x = f + R1*k2 of two rows — a 64-B-segment pattern.  The results are restaged
// through LDS as a plain real tile [32 rows][L] and re-read as float4 in a row-contiguous mapping, so that every
// epilogue access to the state / medium arrays is a 16-B-per-lane coalesced access.
// (waves per SIMD asked of the allocator: xinv_waves)
// TERMS: compile-time value of a.terms for the density epilogue (one specialised kernel per pressure-term mode)
// PLANE: the tile is a whole z-plane (L / 2 line pairs) and the kernel does the plane's y transforms too — see above.
template<int L, int EPI, bool CHAIN, int TERMS = 0, bool TAIL = false, bool PLANE = false>
__global__ __launch_bounds__((Geo<L, PLANE ? L / 2 : nl_x(L)>::THREADS), xinv_waves(L, EPI)) void k_xinv(XinvArgs a)
{
  constexpr int terms = TERMS;
  constexpr int NLX = PLANE ? L / 2 : nl_x(L); // (the registers a thread needs follow from L / TPL, not from the lines per block)
  using G = Geo<L, NLX>;
  constexpr int R1 = G::R1, R2 = G::R2;
  constexpr int NA  = (EPI == EPI_DENSITY) ? 3 : (EPI == EPI_PSUM) ? 2 : 1;
  constexpr int RP  = L + 8;                       // real-tile row pitch (floats): conflict-free 4-B scatter
  constexpr int Q4  = L / 4;                       // float4 per row
  constexpr int TOT4 = 2 * G::NL * Q4;              // float4 of the real tile
  constexpr int NQ  = (TOT4 + G::THREADS - 1) / G::THREADS;  // float4 per thread
  // L / 2 not a multiple of the threads per line (25 x 28, 27 x 28, 25 x 32, 27 x 32): the tile does not divide by the block;
  // the surplus lanes of the last round read the tile's last float4 (XE) and store nothing (XE_OK)
  constexpr bool QPART = (TOT4 % G::THREADS) != 0;
#define XE(q) (QPART ? min(xt + (q) * G::THREADS, TOT4 - 1) : xt + (q) * G::THREADS)
#define XE_OK(q) (!QPART || xt + (q) * G::THREADS < TOT4)
  // xt: the thread's index in the block as the float4 mapping sees it.  FRESH_XT: every read-out loop and every operand
  // group derives its cells from a fresh copy, so that no row index or LDS address waits in a register across a transform
#define XT_FRESH() do { xt = static_cast<int>(threadIdx.x); if (FRESH_XT) asm volatile("" : "+v"(xt)); } while (0)
  __shared__ float2 lds[G::LDSX];
  __shared__ float2 twl[G::TWN];
  __shared__ float2 Yp[PLANE ? L * (L / 2 + 1) : 1]; // PLANE: the plane's half-spectrum between its y and x transforms
  load_twiddles<L>(twl, a.tw); // published by the first barrier of xinv_lines (PLANE: of the plane's y transform)
  float* ldsr = reinterpret_cast<float*>(lds);
  const XRole<G, R2> sa; // (see XRole: who takes part in the R2- and in the R1-participant steps)
  const XRole<G, R1> sb;
  const uint32_t comp = (NA == 1) ? blockIdx.y + a.comp0 : 0; // component / array index for single-array epilogues
  const uint32_t tile = blockIdx.x + a.tile0;
  // the last inverse (the density epilogue's duz, the pressure sum's eta term) stays in the real tile: each float4 is
  // read where the epilogue uses it, just before the same thread overwrites the cell with a chained row (no read-out
  // loop and no barrier after it; a surplus lane of a QPART tile may read a cell its owner has rewritten: it stores nothing)
  constexpr bool LAST_IN_LDS = !PLANE && ((EPI == EPI_DENSITY && last_inverse_in_lds(L)) || (EPI == EPI_PSUM && psum_last_in_lds(L)));
  float4 res[LAST_IN_LDS ? NA - 1 : NA][NQ];
  constexpr bool FRESH_XT = LAST_IN_LDS || (EPI == EPI_PSUM && !PLANE && psum_row_in_lds(L));
  int xt = static_cast<int>(threadIdx.x);
  constexpr int NF = CHAIN ? ((EPI == EPI_DENSITY) ? 2 : 1) : 1; // chained forward transforms
  // rows to chain: kept in registers, except the first of the density epilogue's two (and, where psum_row_in_lds, the
  // pressure sum's one), which goes straight into the real tile in LDS (free once the last inverse has been read out)
  // — 32 registers less at the kernel's widest point
  constexpr bool FW0_IN_LDS = CHAIN && ((EPI == EPI_DENSITY) || (EPI == EPI_PSUM && !PLANE && psum_row_in_lds(L)));
  float4 fw[FW0_IN_LDS ? 1 : NF][NQ];
#pragma unroll
  for (int i = 0; i < NA; i++)
  {
    float2 w[R2];
    if constexpr (PLANE)
    { // this array's plane: scratch -> LDS (x ddy[ky] for the y-gradient), inverse along y, then rows out of LDS
      const uint32_t ia = (NA == 1) ? comp : i;
      plane_load<L>(Yp, a.in[ia], tile, a.P, a.side_off, a.ymul[ia], G::THREADS);
      lds_barrier();
      plane_yfft<L, kInv>(Yp, twl);
      xinv_lines<L, 1, false, NLX, true>(Yp, a.P, lds, twl, w, tile, (NA == 1) ? a.mulx[comp] : nullptr);
    }
    else
    xinv_lines<L, (EPI == EPI_DENSITY) ? 2 : 1, TAIL, NLX, false, LAST_IN_LDS>(a.in[(NA == 1) ? comp : i], a.P, lds, twl, w, tile,
                                                            (NA == 1) ? a.mulx[comp] : nullptr, a.nrows, a.side_off); // ends with a barrier
    if (sb.on)
    {
#pragma unroll
      for (int k2 = 0; k2 < R2; k2++)
      {
        ldsr[(2 * sb.c) * RP + sb.f + R1 * k2]     = w[k2].x;
        ldsr[(2 * sb.c + 1) * RP + sb.f + R1 * k2] = w[k2].y;
      }
    }
    lds_barrier();
    if (LAST_IN_LDS && i == NA - 1) break;
    XT_FRESH();
#pragma unroll
    for (int q = 0; q < NQ; q++)
    {
      const int e   = XE(q);
      const int row = e / Q4;
      const int x4  = e - row * Q4;
      res[LAST_IN_LDS ? min(i, NA - 2) : i][q] = *reinterpret_cast<const float4*>(&ldsr[row * RP + 4 * x4]);
    }
    lds_barrier();
  }

  const kw_constants& k = a.c;
  const uint32_t tile_row0 = tile * G::NL * 2;
  // The operands of the epilogue are requested for a group of GQ float4 per thread before the first one is used: a
  // load - use - store loop per float4 exposes one memory round trip each time (and vmcnt also waits for the stores
  // issued before the loads).  GQ is bounded by the register budget of each epilogue.
  // measured on one box: density 1 (2 spills registers: -1 %), pressure sum 2 (1 gives a fourth wave but -1.4 %),
  // velocity 4 (8: -1 %)
  constexpr int GQ = gq_pick(NQ, (EPI == EPI_DENSITY) ? 1 : (EPI == EPI_PSUM || EPI == EPI_PSUM1) ? 2 : 4);
  // power-of-two rows: x is the same for every float4 of a thread (one PML-x load per thread); the 3 * 2^m rows whose
  // float4 count does not divide the block take x (and the PML-x operand) per float4
  constexpr bool XFIX = (G::THREADS % Q4 == 0);
  XT_FRESH();
  const uint32_t xfix = 4u * (static_cast<uint32_t>(xt) % Q4);
  float4 pmlx4 = make_float4(1.f, 1.f, 1.f, 1.f);
  if (XFIX && ((EPI == EPI_VELOCITY && comp == 0) || EPI == EPI_DENSITY)) pmlx4 = ld4(a.m1[0] + xfix);
  const bool hetRho0 = (EPI == EPI_DENSITY) && (a.m0[0] != nullptr);
  const bool hetBonA = (EPI == EPI_DENSITY) && (terms == 2 || ((terms == 3 || terms == 4 || terms == 5) && a.nonlinear)) && (a.m0[1] != nullptr);
  const bool hetC2   = (EPI == EPI_DENSITY) && (terms == 3 || terms == 4) && (a.m0[2] != nullptr);
  const bool hetTau  = (EPI == EPI_DENSITY) && (terms == 4) && (a.t[2] != nullptr);
#pragma unroll
  for (int q0 = 0; q0 < NQ; q0 += GQ)
  {
    float4 op0[GQ], op1[GQ], op2[GQ], op3[GQ], op4[GQ], op5[GQ], opx[GQ];
    XT_FRESH();
    float  sy[GQ], sz[GQ];
#pragma unroll
    for (int g = 0; g < GQ; g++)
    {
      const int      e   = XE(q0 + g);
      const uint32_t r   = TAIL ? min(tile_row0 + e / Q4, a.nrows - 1u) : tile_row0 + e / Q4; // operands of a masked row: the last row's
      const uint32_t z   = r / k.ny;
      const uint32_t y   = r - z * k.ny;
      const uint32_t x   = XFIX ? xfix : 4u * (e % Q4);
      const uint32_t i   = r * L + x;
      if (!XFIX && ((EPI == EPI_VELOCITY && comp == 0) || EPI == EPI_DENSITY)) opx[g] = ld4(a.m1[0] + x);
      if (EPI == EPI_VELOCITY)
      {
        op0[g] = ld4(a.out[comp] + i);
        if (a.m0[comp] != nullptr) op1[g] = ld4(a.m0[comp] + i);
        if (comp == 1) sy[g] = a.m1[1][y];
        if (comp == 2) sy[g] = a.m1[2][z];
      }
      else if (EPI == EPI_INITVEL)
      {
        if (a.m0[comp] != nullptr) op1[g] = ld4(a.m0[comp] + i);
      }
      else if (EPI == EPI_DENSITY)
      {
        op0[g] = ld4(a.out[0] + i);
        op1[g] = ld4(a.out[1] + i);
        op2[g] = ld4(a.out[2] + i);
        if (hetRho0) op3[g] = ld4(a.m0[0] + i);
        if (hetBonA) op4[g] = ld4(a.m0[1] + i);
        if (hetC2 && terms == 3) op5[g] = ld4(a.m0[2] + i);
        sy[g] = a.m1[1][y];
        sz[g] = a.m1[2][z];
      }
      else if (EPI == EPI_PSUM)
      {
        op0[g] = ld4(a.m0[0] + i);
        if (a.m0[1] != nullptr) op1[g] = ld4(a.m0[1] + i);
        if (a.m1[0] != nullptr) op2[g] = ld4(a.m1[0] + i);
        if (a.m1[1] != nullptr) op3[g] = ld4(a.m1[1] + i);
      }
      else if (EPI == EPI_PSUM1)
      {
        op0[g] = ld4(a.m0[0] + i);
        if (a.m0[1] != nullptr) op1[g] = ld4(a.m0[1] + i);
        if (a.m1[0] != nullptr) op2[g] = ld4(a.m1[0] + i);
      }
    }
#pragma unroll
    for (int g = 0; g < GQ; g++)
    {
      const int      q = q0 + g;
      const int      e = XE(q);
      const uint32_t r = tile_row0 + e / Q4;
      const uint32_t x = XFIX ? xfix : 4u * (e % Q4);
      const uint32_t i = r * L + x;
      const bool     e_ok   = XE_OK(q);                          // (the chained rows in LDS are predicated on it)
      const bool     row_ok = (!TAIL || r < a.nrows) && e_ok;     // every global store below is predicated on it
      const float4   pmx = XFIX ? pmlx4 : opx[g];
      if (EPI == EPI_STORE)
      {
        if (row_ok) st4(a.out[comp] + i, res[0][q]);
      }
      else if (EPI == EPI_VELOCITY)
      { // SolverCudaKernels.cu:199-212 (heterogeneous) / :287-305 (homogeneous)
        float4       vu   = op0[g];
        const float4 gr   = res[0][q];
        const float4 pml4 = (comp == 0) ? pmx : make_float4(sy[g], sy[g], sy[g], sy[g]);
        if (a.m0[comp] != nullptr)
        {
          const float4 d = op1[g];
#pragma unroll
          for (int t = 0; t < 4; t++)
          {
            const float ee = k.fft_divider * f4get(gr, t) * f4get(d, t);
            const float pm = f4get(pml4, t);
            f4put(vu, t, (f4get(vu, t) * pm - ee) * pm);
          }
        }
        else
        {
          const float dtr     = (comp == 0) ? k.dt_rho0_sgx : (comp == 1) ? k.dt_rho0_sgy : k.dt_rho0_sgz;
          const float divider = dtr * k.fft_divider;
#pragma unroll
          for (int t = 0; t < 4; t++)
          {
            const float pm = f4get(pml4, t);
            f4put(vu, t, (f4get(vu, t) * pm - divider * f4get(gr, t)) * pm);
          }
        }
        if (row_ok) st4(a.out[comp] + i, vu);
        if constexpr (CHAIN) fw[0][q] = vu;
      }
      else if (EPI == EPI_INITVEL)
      { // :957-980: u = ifft * (dtRho0Sg * (fftDivider*0.5)) | u = ifft * (fftDivider*0.5*dtRho0Sg)
        const float4 gr = res[0][q];
        float4       o;
        if (a.m0[comp] != nullptr)
        {
          const float4 d = op1[g];
#pragma unroll
          for (int t = 0; t < 4; t++) f4put(o, t, f4get(gr, t) * (f4get(d, t) * (k.fft_divider * 0.5f)));
        }
        else
        {
          const float dtr = (comp == 0) ? k.dt_rho0_sgx : (comp == 1) ? k.dt_rho0_sgy : k.dt_rho0_sgz;
#pragma unroll
          for (int t = 0; t < 4; t++) f4put(o, t, f4get(gr, t) * (k.fft_divider * 0.5f * dtr));
        }
        if (row_ok) st4(a.out[comp] + i, o);
      }
      else if (EPI == EPI_DENSITY)
      { // :1368-1392 (nonlinear) / :1480-1496 (linear); du already carries fftDivider (applied in k-space, :1220)
        const float4 dux = res[0][q], duy = res[1][q];
        const float4 duz = LAST_IN_LDS ? *reinterpret_cast<const float4*>(&ldsr[(e / Q4) * RP + x]) : res[LAST_IN_LDS ? 0 : 2][q];
        const float  py = sy[g], pz = sz[g];
        const float4 rx = op0[g], ry = op1[g], rz = op2[g];
        const float4 r04 = hetRho0 ? op3[g] : make_float4(k.rho0, k.rho0, k.rho0, k.rho0);
        float4 nrx, nry, nrz;
#pragma unroll
        for (int t = 0; t < 4; t++)
        {
          const float px = f4get(pmx, t);
          const float r0 = f4get(r04, t);
          const float erx = f4get(rx, t), ery = f4get(ry, t), erz = f4get(rz, t);
          if (a.nonlinear)
          {
            const float sumRhosDt = (2.0f * (erx + ery + erz) + r0) * k.dt;
            f4put(nrx, t, px * ((px * erx) - sumRhosDt * f4get(dux, t)));
            f4put(nry, t, py * ((py * ery) - sumRhosDt * f4get(duy, t)));
            f4put(nrz, t, pz * ((pz * erz) - sumRhosDt * f4get(duz, t)));
          }
          else
          {
            const float dtRho0 = hetRho0 ? k.dt * r0 : k.dt_rho0;
            f4put(nrx, t, px * (px * erx - dtRho0 * f4get(dux, t)));
            f4put(nry, t, py * (py * ery - dtRho0 * f4get(duy, t)));
            f4put(nrz, t, pz * (pz * erz - dtRho0 * f4get(duz, t)));
          }
        }
        if (row_ok) st4(a.out[0] + i, nrx);
        if (row_ok) st4(a.out[1] + i, nry);
        if (row_ok) st4(a.out[2] + i, nrz);
        if (a.aux[0] != nullptr)
        {
          if (row_ok) st4(a.aux[0] + i, dux);
          if (row_ok) st4(a.aux[1] + i, duy);
          if (row_ok) st4(a.aux[2] + i, duz);
        }
        if (terms == 2)
        { // :1588-1601 with the updated densities
          const float4 b4 = hetBonA ? op4[g] : make_float4(k.b_on_a, k.b_on_a, k.b_on_a, k.b_on_a);
          float4 o0, o1, o2;
#pragma unroll
          for (int t = 0; t < 4; t++)
          {
            const float eBonA   = f4get(b4, t);
            const float r0      = f4get(r04, t);
            const float eRhoSum = (f4get(nrx, t) + f4get(nry, t) + f4get(nrz, t));
            const float eDuSum  = (f4get(dux, t) + f4get(duy, t) + f4get(duz, t));
            f4put(o0, t, eRhoSum);
            f4put(o1, t, ((eBonA * eRhoSum * eRhoSum) / (2.0f * r0)) + eRhoSum);
            f4put(o2, t, r0 * eDuSum);
          }
          if (row_ok) st4(a.t[1] + i, o1); // the nonlinear term is read again by the pressure sum (a stage later: cached or not, same time)
          if constexpr (CHAIN) { if (e_ok) *reinterpret_cast<float4*>(&ldsr[(e / Q4) * RP + x]) = o2; fw[0][q] = o0; }
          else { if (row_ok) st4(a.t[0] + i, o0); if (row_ok) st4(a.t[2] + i, o2); }
        }
        else if (terms == 3)
        { // lossless equation of state on the updated densities: sumPressureNonlinearLossless (:2067-2084) /
          // sumPressureLinearLossless (:2224-2236); the new p is chained like the pressure sum's
          const float4 b4  = hetBonA ? op4[g] : make_float4(k.b_on_a, k.b_on_a, k.b_on_a, k.b_on_a);
          const float4 c24 = hetC2 ? op5[g] : make_float4(k.c2, k.c2, k.c2, k.c2);
          float4 pn;
#pragma unroll
          for (int t = 0; t < 4; t++)
          {
            const float rhoSum = f4get(nrx, t) + f4get(nry, t) + f4get(nrz, t);
            if (a.nonlinear) f4put(pn, t, f4get(c24, t) * (rhoSum + (f4get(b4, t) * (rhoSum * rhoSum) / (2.0f * f4get(r04, t)))));
            else f4put(pn, t, f4get(c24, t) * rhoSum);
          }
          if (row_ok) st4(a.t[0] + i, pn);
          if constexpr (CHAIN) { if (e_ok) *reinterpret_cast<float4*>(&ldsr[(e / Q4) * RP + x]) = pn; }
        }
        else if (terms == 4)
        { // Stokes absorption (alpha_power == 2) on the updated densities and the gradients of this step: kw_stokes_pressure
          // (kw_internal.h), the arithmetic of kw_sum_pressure_stokes_*; the new p is stored and chained like the lossless one
          const float4 b4   = hetBonA ? op4[g] : make_float4(k.b_on_a, k.b_on_a, k.b_on_a, k.b_on_a);
          // c2 and tau are requested here, once the density update has released the registers of the old densities, not
          // with the operand group above: the epilogue then needs no more registers than the lossless one
          // (a masked row reads nothing: its p is 0 and is neither stored nor chained past the grid's last row)
          const bool   in_grid = !TAIL || r < a.nrows;
          const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 c24  = hetC2 ? (in_grid ? ld4(a.m0[2] + i) : zero4) : make_float4(k.c2, k.c2, k.c2, k.c2);
          const float4 tau4 = hetTau ? (in_grid ? ld4(a.t[2] + i) : zero4) : make_float4(k.absorb_tau, k.absorb_tau, k.absorb_tau, k.absorb_tau);
          float4 pn;
#pragma unroll
          for (int t = 0; t < 4; t++)
          {
            const float rhoSum = f4get(nrx, t) + f4get(nry, t) + f4get(nrz, t);
            const float duSum  = f4get(dux, t) + f4get(duy, t) + f4get(duz, t);
            f4put(pn, t, kw_stokes_pressure(a.nonlinear != 0, f4get(c24, t), f4get(tau4, t), f4get(r04, t), f4get(b4, t), rhoSum, duSum));
          }
          if (row_ok) st4(a.t[0] + i, pn);
          if constexpr (CHAIN) { if (e_ok) *reinterpret_cast<float4*>(&ldsr[(e / Q4) * RP + x]) = pn; }
        }
        else if (terms == 5)
        { // one-term power law: `first` goes where the pressure sum reads it (t0 linear, t1 nonlinear: as terms 1 and 2 put
          // it) and ONE array takes the absorption round trip: rho0 * sum du (no_dispersion) or sum rho (no_absorption,
          // where rho0 * sum du is not computed).  Chained, that array's row goes through the real tile like the first
          // chained row of terms 1 / 2; plain, it is stored where terms 1 / 2 store it (t1 | t2, t0).
          const float4 b4 = hetBonA ? op4[g] : make_float4(k.b_on_a, k.b_on_a, k.b_on_a, k.b_on_a);
          float4 fi, tm;
#pragma unroll
          for (int t = 0; t < 4; t++)
          {
            const float eRhoSum = (f4get(nrx, t) + f4get(nry, t) + f4get(nrz, t));
            if (a.nonlinear) f4put(fi, t, ((f4get(b4, t) * eRhoSum * eRhoSum) / (2.0f * f4get(r04, t))) + eRhoSum);
            else f4put(fi, t, eRhoSum);
            f4put(tm, t, eRhoSum);
          }
          if (a.which == 0)
          {
#pragma unroll
            for (int t = 0; t < 4; t++) f4put(tm, t, f4get(r04, t) * (f4get(dux, t) + f4get(duy, t) + f4get(duz, t)));
          }
          if (row_ok) st4((a.nonlinear ? a.t[1] : a.t[0]) + i, fi);
          if constexpr (CHAIN) { if (e_ok) *reinterpret_cast<float4*>(&ldsr[(e / Q4) * RP + x]) = tm; }
          else
          {
            if (a.which == 0) { if (row_ok) st4((a.nonlinear ? a.t[2] : a.t[1]) + i, tm); }
            else if (a.nonlinear) { if (row_ok) st4(a.t[0] + i, tm); } // (linear: sum rho is `first`, stored above)
          }
        }
        else if (terms == 1)
        { // :1733-1741
          float4 o0, o1;
#pragma unroll
          for (int t = 0; t < 4; t++)
          {
            f4put(o0, t, f4get(nrx, t) + f4get(nry, t) + f4get(nrz, t));
            const float duSum = f4get(dux, t) + f4get(duy, t) + f4get(duz, t);
            f4put(o1, t, f4get(r04, t) * duSum);
          }
          if (row_ok) st4(a.t[0] + i, o0); // the density sum is read again by the pressure sum
          if constexpr (CHAIN) { if (e_ok) *reinterpret_cast<float4*>(&ldsr[(e / Q4) * RP + x]) = o1; fw[0][q] = o0; }
          else if (row_ok) st4(a.t[1] + i, o1);
        }
      }
      else if (EPI == EPI_PSUM)
      { // :1877 / :1978: p = c2*(first + (fftDivider*((tauTerm*tau) - (etaTerm*eta))))
        const float4 tt = res[0][q];
        const float4 et = LAST_IN_LDS ? *reinterpret_cast<const float4*>(&ldsr[(e / Q4) * RP + x]) : res[LAST_IN_LDS ? 0 : 1][q];
        const float4 fi = op0[g];
        const float4 c24  = (a.m0[1] != nullptr) ? op1[g] : make_float4(k.c2, k.c2, k.c2, k.c2);
        const float4 tau4 = (a.m1[0] != nullptr) ? op2[g] : make_float4(k.absorb_tau, k.absorb_tau, k.absorb_tau, k.absorb_tau);
        const float4 eta4 = (a.m1[1] != nullptr) ? op3[g] : make_float4(k.absorb_eta, k.absorb_eta, k.absorb_eta, k.absorb_eta);
        float4 o;
#pragma unroll
        for (int t = 0; t < 4; t++)
          f4put(o, t, f4get(c24, t) * (f4get(fi, t) + (k.fft_divider * ((f4get(tt, t) * f4get(tau4, t)) - (f4get(et, t) * f4get(eta4, t))))));
        if (row_ok) st4(a.out[0] + i, o);
        if constexpr (FW0_IN_LDS) { if (e_ok) *reinterpret_cast<float4*>(&ldsr[(e / Q4) * RP + x]) = o; }
        else if constexpr (CHAIN) fw[0][q] = o;
      }
      else if (EPI == EPI_PSUM1)
      { // the power law's sum with one term (kw_one_term_pressure, kw_internal.h): the arithmetic of kw_sum_pressure_terms_one_*
        const float4 tm = res[0][q];
        const float4 fi = op0[g];
        const float  cs = a.which ? k.absorb_eta : k.absorb_tau;
        const float4 c24 = (a.m0[1] != nullptr) ? op1[g] : make_float4(k.c2, k.c2, k.c2, k.c2);
        const float4 co4 = (a.m1[0] != nullptr) ? op2[g] : make_float4(cs, cs, cs, cs);
        float4 o;
#pragma unroll
        for (int t = 0; t < 4; t++)
          f4put(o, t, kw_one_term_pressure(a.which, f4get(c24, t), f4get(fi, t), k.fft_divider, f4get(tm, t), f4get(co4, t)));
        if (row_ok) st4(a.out[0] + i, o);
        if constexpr (CHAIN) fw[0][q] = o;
      }
    }
  }

  // ---- chained forward x-transform of what the epilogue just produced (rows are still in registers): the consumer
  // stage finds the spectra in the scratch arrays and skips its own x-forward pass and the HBM round trip ----
  if constexpr (CHAIN)
  {
    constexpr int R1c = G::R1, R2c = G::R2;
#pragma unroll
    for (int jf = 0; jf < NF; jf++)
    {
      if (EPI == EPI_DENSITY && jf == 1 && terms >= 3) break; // lossless / Stokes: only p is chained; one-term power law: one term
      if (!(FW0_IN_LDS && jf == 0))
      {
        XT_FRESH();
#pragma unroll
        for (int q = 0; q < NQ; q++)
        {
          const int e   = XE(q);
          const int row = e / Q4;
          const int x4  = e - row * Q4;
          if (XE_OK(q)) *reinterpret_cast<float4*>(&ldsr[row * RP + 4 * x4]) = fw[FW0_IN_LDS ? 0 : jf][q];
        }
      }
      lds_barrier();
      float2 v[R1c];
      if (sa.on)
      {
#pragma unroll
        for (int n1 = 0; n1 < R1c; n1++)
          v[n1] = make_float2(ldsr[(2 * sa.c) * RP + n1 * R2c + sa.f], ldsr[(2 * sa.c + 1) * RP + n1 * R2c + sa.f]);
      }
      lds_barrier(); // the real tile aliases the exchange buffer
      if constexpr (PLANE)
      { // rows into the plane buffer, forward along y, plane -> scratch (the consumer's z-pass comes next)
        xfwd_tail<L, false, NLX, true>(v, lds, twl, Yp, a.P, tile);
        plane_yfft<L, kFwd>(Yp, twl);
        plane_store<L>(Yp, a.fout[(NA == 1) ? comp : jf], tile, a.P, a.side_off, G::THREADS);
        lds_barrier(); // the plane buffer is reused by the second chained array
      }
      else
      xfwd_tail<L, TAIL, NLX>(v, lds, twl, a.fout[(NA == 1) ? comp : jf], a.P, tile, a.nrows, a.side_off);
    }
  }
}

// Half-cell shift along x (computeVelocityShiftInX, SolverCudaKernels.cu:2617-2640): rows 2c and 2c+1 travel as the
// real and imaginary part of one complex line — the filter H is Hermitian with a real Nyquist bin (what the reference's
// R2C -> multiply -> C2R applies to each row), so it acts on both parts independently.  One read and one write of the
// array; loads as in k_xfwd, stores as coalesced float4 through the real tile like the x-inverse epilogues.

template<int L, bool TAIL = false> __global__ __launch_bounds__(GeoX<L>::THREADS) void k_xshift(XshiftArgs a)
{
  using G = GeoX<L>;
  constexpr int R1 = G::R1, R2 = G::R2;
  constexpr int RP = L + 8, Q4 = L / 4, TOT4 = 2 * G::NL * Q4, NQ = (TOT4 + G::THREADS - 1) / G::THREADS;
  constexpr bool QPART = (TOT4 % G::THREADS) != 0; // (see k_xinv)
  __shared__ float2 lds[G::LDSX];
  __shared__ float2 twl[G::TWN];
  load_twiddles<L>(twl, a.tw);
  float* ldsr = reinterpret_cast<float*>(lds);
  const XRole<G, R2> sa;
  const XRole<G, R1> sb;
  const uint32_t tile_row0 = (blockIdx.x + a.tile0) * G::NL * 2;
  const int xt = static_cast<int>(threadIdx.x); // (XE / XE_OK)
  float2 v[R1];
  if (sa.on)
  {
    const uint32_t row0 = tile_row0 + 2 * sa.c;
    const float* __restrict__ ra = a.in + (TAIL ? min(row0, a.nrows - 1u) : row0) * L;
    const float* __restrict__ rb = TAIL ? a.in + min(row0 + 1u, a.nrows - 1u) * L : ra + L;
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++) v[n1] = make_float2(ra[n1 * R2 + sa.f], rb[n1 * R2 + sa.f]);
  }
  lds_barrier(); // twiddle table visible
  if (sa.on)
  {
    step_a<L, kFwd>(v, sa.f, twl);
#pragma unroll
    for (int k1 = 0; k1 < R1; k1++) lds[sa.c * G::LP + k1 * (R2 + 1) + sa.f] = v[k1];
  }
  lds_barrier();
  float2 w[R2];
  if (sb.on)
  {
#pragma unroll
    for (int n2 = 0; n2 < R2; n2++) w[n2] = lds[sb.c * G::LP + sb.f * (R2 + 1) + n2];
    Dft<R2, kFwd>::run(w);
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++) w[k2] = cmulf(w[k2], a.H[sb.f + R1 * k2]);
  }
  lds_barrier();
  if (sb.on)
  { // natural-order spectrum of the line, the starting point of the inverse (as in xinv_lines)
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++) lds[sb.c * G::ZP + sb.f + R1 * k2] = w[k2];
  }
  lds_barrier();
  if (sa.on)
  {
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++) v[n1] = lds[sa.c * G::ZP + n1 * R2 + sa.f];
  }
  lds_barrier();
  if (sa.on)
  {
    step_a<L, kInv>(v, sa.f, twl);
#pragma unroll
    for (int k1 = 0; k1 < R1; k1++) lds[sa.c * G::LP + k1 * (R2 + 1) + sa.f] = v[k1];
  }
  lds_barrier();
  if (sb.on)
  {
#pragma unroll
    for (int n2 = 0; n2 < R2; n2++) w[n2] = lds[sb.c * G::LP + sb.f * (R2 + 1) + n2];
    Dft<R2, kInv>::run(w);
  }
  lds_barrier();
  if (sb.on)
  {
#pragma unroll
    for (int k2 = 0; k2 < R2; k2++)
    {
      ldsr[(2 * sb.c) * RP + sb.f + R1 * k2]     = w[k2].x;
      ldsr[(2 * sb.c + 1) * RP + sb.f + R1 * k2] = w[k2].y;
    }
  }
  lds_barrier();
#pragma unroll
  for (int q = 0; q < NQ; q++)
  {
    const int e   = XE(q);
    const int row = e / Q4;
    const int x4  = e - row * Q4;
    if ((!TAIL || tile_row0 + row < a.nrows) && XE_OK(q))
      st4(a.out + (tile_row0 + row) * L + 4 * x4, *reinterpret_cast<const float4*>(&ldsr[row * RP + 4 * x4]));
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// line lengths with a two-factor register decomposition L = R1 * R2, R1, R2 in {4 ... 32} with at most one odd prime
// power (3, 9, 27, 5, 25, 7) each: 2^m, 3 * 2^m, 9 * 2^m, 27 * 2^m, 81 * 4, 5 * 2^m, 15 * 2^m, 25 * 2^m, 75 * 2^m, 125 * 4,
// 45 * 2^m (180, 360), 135 * 4 (540), 7 * 2^m (112 ... 896), 21 * 2^m (168, 336, 672), 35 * 2^m (140, 280, 560), 49 * 2^m
// (196, 392, 784), 63 * 2^m (252, 504), 105 * 2^m (420, 840), 45 * 16 (720), 225 * 4 (900), 15 * 64 (960: 30 x 32, the
// 15 * 2^m register DFTs), 175 * 4 (700), 189 * 4 (756), 25 * 32 (800), 27 * 32 (864); the x kernels need L % 4 == 0 (where
// L / 2 is no multiple of the threads per line their float4 tile ends in a partial round: QPART in k_xinv)
#define KW_FUSED_LENGTHS_SHORT(X) X(16) X(32) X(48) X(64) X(72) X(80) X(96) X(100) X(108) X(112) X(120) X(128) X(140)  \
  X(144) X(160) X(168) X(180) X(192) X(196) X(200) X(216) X(224) X(240) X(252) X(256) X(280) X(288) X(300) X(320) X(324)  \
  X(336) X(360) X(384) X(392) X(400) X(420)
#define KW_FUSED_LENGTHS_LONG(X) X(432) X(448) X(480) X(500) X(504) X(512) X(540) X(560) X(576) X(600) X(640) X(648)     \
  X(672) X(700) X(720) X(756) X(768) X(784) X(800) X(840) X(864) X(896) X(900) X(960) X(1024)
#ifdef KW_FUSED_ONLY /* tuning builds: one line length only (-DKW_FUSED_ONLY=256), compiles in seconds */
#define KW_FUSED_LENGTHS(X) X(KW_FUSED_ONLY)
#else
#define KW_FUSED_LENGTHS(X) KW_FUSED_LENGTHS_SHORT(X) KW_FUSED_LENGTHS_LONG(X)
#endif

// dispatch on a runtime line length; the call sites define the per-length launch macro under the name M
#define KW_LEN_CASE(LEN) case LEN: M(LEN); break;
#define KW_LEN_SWITCH(len, MACRO)                                                                                      \
  switch (len)                                                                                                         \
  {                                                                                                                    \
    KW_FUSED_LENGTHS(KW_LEN_CASE)                                                                                      \
    default: kw_set_error("fused pipeline: unsupported length %u", (unsigned)(len)); return KW_ERR_INVALID;            \
  }

#define LAUNCH(kernel, grid, block, ...)                                                                               \
  do {                                                                                                                 \
    hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, __VA_ARGS__);                                              \
    KW_LAUNCH_CHECK();                                                                                                 \
  } while (0)

// f(std::integral_constant<int, LEN>) for the runtime line length len
template<class F> kw_status with_length(uint32_t len, F&& f)
{
#define M(LEN) return f(std::integral_constant<int, LEN>())
  KW_LEN_SWITCH(len, M)
#undef M
}
// Grid of a z-pass over the pipeline's scratch layout: the tiles of a row plus one tile index for the blocks of the
// x-Nyquist side array (tile_coord), by the local rows, by `nz` (arrays, where each block takes one).  `nl`: columns per
// tile of the kernel launched — nl_z(length) for the kernels on Geo<L, nl_z(L)>, NLMAX for the 2 x 256 split kernels.
inline dim3 z_pass_grid(const kw_ctx* ctx, uint32_t nl, uint32_t nz = 1)
{
  const auto& f = ctx->fused;
  return dim3((f.P + nl - 1u) / nl + (f.side_off != 0 ? 1u : 0u), f.nyl, nz);
}
// the geometry of an operator pass along `axis` (1: y, 2: z) over the context's scratch layout
inline PassGeo pass_geo(const kw_ctx* ctx, int axis)
{
  const auto& f = ctx->fused;
  return PassGeo{ f.tw[axis], f.nxm, f.P, f.side_off };
}
// Launch of z-pass kernel K at the runtime line length len (a kw_status): K names the kernel with LEN for its length,
// as in  return KW_LAUNCH_ZPASS((k_zfused_pair<LEN>), f.nz_global, z_pass_grid(ctx, nl_z(f.nz_global)), a);
#define KW_LAUNCH_ZPASS(K, len, grid, ...)                                                                             \
  with_length(len, [&](auto kw_len) -> kw_status {                                                                     \
    constexpr int LEN = decltype(kw_len)::value;                                                                       \
    LAUNCH(K, grid, dim3((Geo<LEN, nl_z(LEN)>::THREADS)), __VA_ARGS__);                                                \
    return KW_OK;                                                                                                      \
  })

// the x lines whose x-inverse kernels a code object holds: every length, those below KW_LONG_LINES, those from it on
enum XLines { X_ALL, X_SHORT, X_LONG };
constexpr bool holds_lines(int lines, int L) { return lines == X_ALL || (lines == X_SHORT) == (L < KW_LONG_LINES); }

// PLANE: whole-plane tiles (tile0 / ntiles count z-planes), 32- and 64-point rows only
template<int EPI, bool CHAIN, int TERMS, bool TAIL, int LINES = X_ALL, bool PLANE = false>
kw_status launch_xinv_impl(kw_ctx* ctx, int ncomp, XinvArgs a, uint32_t tile0, uint32_t ntiles)
{
  a.tile0 = tile0;
  const dim3 grid(ntiles, ncomp, 1);
#define M(LEN)                                                                                                         \
  if constexpr (!holds_lines(LINES, LEN) || (PLANE && !plane_len(LEN)))                                                \
  { kw_set_error("fused pipeline: no such x-inverse kernel for rows of %d", LEN); return KW_ERR_INVALID; }              \
  else if constexpr (TAIL && !has_partial_x_tiles(LEN)) KW_NO_TAIL(LEN)                                                \
  else LAUNCH((k_xinv<LEN, EPI, CHAIN, TERMS, TAIL, PLANE>), grid, dim3((Geo<LEN, PLANE ? LEN / 2 : nl_x(LEN)>::THREADS)), a)
  KW_LEN_SWITCH(ctx->c.nx, M)
#undef M
  return KW_OK;
}

// the bodies of the x-inverse entry points (kw_fused_xinv_*.hip): density epilogues by their number of pressure terms
// (chained: 1 ... 3, plain: 0 ... 3; the Stokes pressure epilogue, 4, has entry points of its own), the other epilogues
// by epilogue and chaining
template<bool CHAIN, bool TAIL, int LINES, bool PLANE = false>
kw_status launch_xinv_density(int terms, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  switch (terms)
  {
    case 0: if constexpr (!CHAIN) return launch_xinv_impl<EPI_DENSITY, false, 0, TAIL, LINES, PLANE>(ctx, ncomp, a, tile0, ntiles); break;
    case 1: return launch_xinv_impl<EPI_DENSITY, CHAIN, 1, TAIL, LINES, PLANE>(ctx, ncomp, a, tile0, ntiles);
    case 2: return launch_xinv_impl<EPI_DENSITY, CHAIN, 2, TAIL, LINES, PLANE>(ctx, ncomp, a, tile0, ntiles);
    case 3: return launch_xinv_impl<EPI_DENSITY, CHAIN, 3, TAIL, LINES, PLANE>(ctx, ncomp, a, tile0, ntiles);
  }
  kw_set_error("fused pipeline: no density epilogue for chain = %d, terms = %d", CHAIN ? 1 : 0, terms);
  return KW_ERR_INVALID;
}

template<bool TAIL, int LINES, bool PLANE = false>
kw_status launch_xinv_density_stokes(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return chain ? launch_xinv_impl<EPI_DENSITY, true, 4, TAIL, LINES, PLANE>(ctx, ncomp, a, tile0, ntiles)
               : launch_xinv_impl<EPI_DENSITY, false, 4, TAIL, LINES, PLANE>(ctx, ncomp, a, tile0, ntiles);
}

// the one-term power law's epilogues: density (terms == 5) and pressure sum over one inverse
template<bool TAIL, int LINES, bool PLANE = false>
kw_status launch_xinv_density_oneterm(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return chain ? launch_xinv_impl<EPI_DENSITY, true, 5, TAIL, LINES, PLANE>(ctx, ncomp, a, tile0, ntiles)
               : launch_xinv_impl<EPI_DENSITY, false, 5, TAIL, LINES, PLANE>(ctx, ncomp, a, tile0, ntiles);
}

template<bool TAIL, bool PLANE = false>
kw_status launch_xinv_psum_one(int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  return chain ? launch_xinv_impl<EPI_PSUM1, true, 0, TAIL, X_ALL, PLANE>(ctx, ncomp, a, tile0, ntiles)
               : launch_xinv_impl<EPI_PSUM1, false, 0, TAIL, X_ALL, PLANE>(ctx, ncomp, a, tile0, ntiles);
}

template<bool TAIL, bool PLANE = false>
kw_status launch_xinv_other(int epi, int chain, kw_ctx* ctx, int ncomp, const XinvArgs& a, uint32_t tile0, uint32_t ntiles)
{
  switch (2 * epi + chain)
  {
    case 2 * EPI_STORE: return launch_xinv_impl<EPI_STORE, false, 0, TAIL, X_ALL, PLANE>(ctx, ncomp, a, tile0, ntiles);
    case 2 * EPI_VELOCITY: return launch_xinv_impl<EPI_VELOCITY, false, 0, TAIL, X_ALL, PLANE>(ctx, ncomp, a, tile0, ntiles);
    case 2 * EPI_VELOCITY + 1: return launch_xinv_impl<EPI_VELOCITY, true, 0, TAIL, X_ALL, PLANE>(ctx, ncomp, a, tile0, ntiles);
    case 2 * EPI_INITVEL: return launch_xinv_impl<EPI_INITVEL, false, 0, TAIL, X_ALL, PLANE>(ctx, ncomp, a, tile0, ntiles);
    case 2 * EPI_PSUM: return launch_xinv_impl<EPI_PSUM, false, 0, TAIL, X_ALL, PLANE>(ctx, ncomp, a, tile0, ntiles);
    case 2 * EPI_PSUM + 1: return launch_xinv_impl<EPI_PSUM, true, 0, TAIL, X_ALL, PLANE>(ctx, ncomp, a, tile0, ntiles);
    default: kw_set_error("fused pipeline: no epilogue %d with chain = %d", epi, chain); return KW_ERR_INVALID;
  }
}

} // namespace

#endif // KW_FUSED_HIP
