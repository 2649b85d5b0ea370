// kw_offgrid.hip — element weights of an off-grid transducer array from its geometry (kwave_hip.h, "Off-grid elements").
// An element is a set of integration points; every point spreads a truncated band-limited interpolant (a separable sinc
// stencil of (2R + 1)^3 grid points) over the grid and an element's weights are the sums over its points.  That is a
// scatter-accumulate followed by a sparse compaction:
//   k_offgrid_accumulate  every contribution is computed in fp32, converted to 64-bit fixed point (2^-40) and added with an
//                         integer atomic into the element's zeroed bounding box — integer sums are exact, so the result does
//                         not depend on the order in which the adds arrive (run to run, or under a permutation of the points)
//   k_offgrid_count       non-zero cells per 256-cell block of the boxes
//   k_offgrid_scan        exclusive scan of the block counts (one block)
//   k_offgrid_emit        (grid index, fp32 weight) of every non-zero cell, boxes in element order and cells in ascending
//                         grid index: the rows of the CSR, already in order
// As many element boxes as fit the scratch budget share one round: a memset and these four launches, then one host round
// trip of two synchronisations (the entry count, which sizes the host arrays, then the entries).
#include "kw_internal.h"

#include <algorithm>
#include <cmath>
#include <exception>
#include <new>

namespace {

constexpr uint32_t kBlock      = 256;          // threads per block; the compaction takes one cell per thread
constexpr uint32_t kWaves      = kBlock / 64;  // the accumulation takes one integration point per wave and pass
constexpr uint32_t kPointsPerBlock = 32;       // integration points per accumulate block
constexpr int      kMaxRadius  = 64;           // stencil radius the factor table in LDS is sized for (bli_tolerance >= 0.005)
constexpr int      kMaxWidth   = 2 * kMaxRadius + 1;
constexpr uint64_t kCellBytes  = 8 + 8 + 4;    // accumulator + emitted index + emitted weight
constexpr double   kFixedOne   = 1099511627776.0;         // 2^40
constexpr float    kFixedStep  = 9.094947017729282e-13f;  // 2^-40
constexpr uint64_t kMaxPoints  = 1ull << 32;   // integration points of one build (48 GB of host arrays beside the caller's)
constexpr double   kMaxAbsSum  = 4194304.0;    // 2^22: sum over an element's points of |scale| stays below it

// bounding box of one element: the clipped min / max of its points' nearest indices, dilated by the radius
struct Box
{
  int32_t  lo[3];
  uint32_t dim[3];
  uint64_t cells;       // dim[0] * dim[1] * dim[2]
  float    scale;
  uint32_t first_block; // of the round: the box starts at cell first_block * 256 of the scratch (boxes are padded to blocks)
};

// one block's share of the accumulation: `count` points of element `box` (index within the round) from point `begin`
struct Work
{
  uint64_t begin;
  uint32_t count;
  uint32_t box;
};

struct Grid
{
  uint32_t n[3];
  int32_t  radius[3]; // 0 on an axis of one point
};

// s(d, f) = sinc(d - f) as (-1)^d sin(pi f) / (pi (f - d)): one sine per point and axis (sin_pif), exactly 0 off the point's
// own index when f == 0; every operation rounded on its own so that the value depends on (d, f) alone
__device__ __forceinline__ float sinc_factor(int d, float f, float sin_pif)
{
#pragma clang fp contract(off)
  const float t = f - static_cast<float>(d);
  if (t == 0.0f) return 1.0f;
  const float s = sin_pif / (3.14159265358979323846f * t);
  return (d & 1) ? -s : s;
}

__global__ __launch_bounds__(256) void k_offgrid_accumulate(unsigned long long* __restrict__ acc, const Work* __restrict__ work,
                                                            const Box* __restrict__ boxes, const int32_t* __restrict__ pn,
                                                            const float* __restrict__ pf, Grid g)
{
  __shared__ float fac[kWaves][3][kMaxWidth];
  const Work     w    = work[blockIdx.x];
  const Box      b    = boxes[w.box];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t wx = 2 * g.radius[0] + 1, wy = 2 * g.radius[1] + 1, wz = 2 * g.radius[2] + 1;
  const uint32_t total = wx * wy * wz;
  unsigned long long* const box_acc = acc + static_cast<uint64_t>(b.first_block) * kBlock;
  for (uint32_t first = 0; first < w.count; first += kWaves) // the same trip count for every wave of the block
  {
    const bool     active = first + wave < w.count;
    const uint64_t p      = w.begin + first + wave;
    int32_t n[3] = {0, 0, 0};
    if (active)
    {
      n[0] = pn[3 * p], n[1] = pn[3 * p + 1], n[2] = pn[3 * p + 2];
      // the 1-D factors of this wave's point, once: lanes 0 .. wx + wy + wz - 1
      for (uint32_t i = lane; i < wx + wy + wz; i += 64)
      {
        const uint32_t axis = (i < wx) ? 0 : ((i < wx + wy) ? 1 : 2);
        const uint32_t k    = i - ((axis == 0) ? 0 : ((axis == 1) ? wx : wx + wy));
        float s = 1.0f;
        if (g.n[axis] > 1)
        {
#pragma clang fp contract(off)
          const float f = pf[3 * p + axis];
          s = sinc_factor(static_cast<int>(k) - g.radius[axis], f, sinf(3.14159265358979323846f * f));
        }
        fac[wave][axis][k] = s;
      }
    }
    __syncthreads();
    if (active)
    {
      // the stencil with x fastest: 64 consecutive stencil cells are runs of contiguous box cells
      for (uint32_t t = lane; t < total; t += 64)
      {
        const uint32_t ix = t % wx, r = t / wx, iy = r % wy, iz = r / wy;
        const int32_t  gx = n[0] - g.radius[0] + static_cast<int32_t>(ix);
        const int32_t  gy = n[1] - g.radius[1] + static_cast<int32_t>(iy);
        const int32_t  gz = n[2] - g.radius[2] + static_cast<int32_t>(iz);
        if (static_cast<uint32_t>(gx) >= g.n[0] || static_cast<uint32_t>(gy) >= g.n[1] || static_cast<uint32_t>(gz) >= g.n[2])
          continue; // clipped at the grid's faces
        float c;
        {
#pragma clang fp contract(off)
          c = ((b.scale * fac[wave][0][ix]) * fac[wave][1][iy]) * fac[wave][2][iz];
        }
        const long long v = __double2ll_rn(static_cast<double>(c) * kFixedOne);
        const uint32_t bx = static_cast<uint32_t>(gx - b.lo[0]), by = static_cast<uint32_t>(gy - b.lo[1]),
                       bz = static_cast<uint32_t>(gz - b.lo[2]);
        // the box holds every in-grid stencil cell of its points; the test keeps a wrong table from writing elsewhere
        if (v != 0 && bx < b.dim[0] && by < b.dim[1] && bz < b.dim[2])
          atomicAdd(box_acc + (static_cast<uint64_t>(bz) * b.dim[1] + by) * b.dim[0] + bx, static_cast<unsigned long long>(v));
      }
    }
    __syncthreads(); // before the next pass overwrites the factors
  }
}

__global__ __launch_bounds__(256) void k_offgrid_count(uint32_t* __restrict__ count, const long long* __restrict__ acc)
{
  const int n = __syncthreads_count(acc[static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x] != 0);
  if (threadIdx.x == 0) count[blockIdx.x] = static_cast<uint32_t>(n);
}

// offset[i] = count[0] + ... + count[i - 1] for i = 0 .. n (one block: each thread a contiguous run, the run sums through LDS)
__global__ __launch_bounds__(1024) void k_offgrid_scan(uint64_t* __restrict__ offset, const uint32_t* __restrict__ count,
                                                       uint32_t n)
{
  __shared__ uint64_t run[1024];
  const uint32_t per = (n + 1023) / 1024;
  const uint32_t lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
  uint64_t sum = 0;
  for (uint32_t i = lo; i < hi; i++) sum += count[i];
  run[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    uint64_t before = 0;
    for (uint32_t t = 0; t < 1024; t++)
    {
      const uint64_t s = run[t];
      run[t] = before;
      before += s;
    }
    offset[n] = before;
  }
  __syncthreads();
  uint64_t at = run[threadIdx.x];
  for (uint32_t i = lo; i < hi; i++)
  {
    offset[i] = at;
    at += count[i];
  }
}

// one cell per thread; a block's non-zero cells go to offset[block] + (non-zero cells before this one in the block)
__global__ __launch_bounds__(256) void k_offgrid_emit(uint64_t* __restrict__ index, float* __restrict__ weight,
                                                      const long long* __restrict__ acc, const uint64_t* __restrict__ offset,
                                                      const Box* __restrict__ boxes, uint32_t n_boxes, Grid g)
{
  __shared__ uint32_t wave_count[kWaves];
  const uint32_t  wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long v    = acc[static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x];
  const unsigned long long set = __ballot(v != 0);
  if (lane == 0) wave_count[wave] = static_cast<uint32_t>(__popcll(set));
  __syncthreads();
  if (v == 0) return;
  uint32_t before = static_cast<uint32_t>(__popcll(set & ((1ull << lane) - 1ull)));
  for (uint32_t q = 0; q < wave; q++) before += wave_count[q];
  // the box this block belongs to: the last one with first_block <= blockIdx.x (boxes without cells share their successor's)
  uint32_t lo = 0, hi = n_boxes;
  while (hi - lo > 1)
  {
    const uint32_t mid = (lo + hi) >> 1;
    if (boxes[mid].first_block <= blockIdx.x) lo = mid;
    else hi = mid;
  }
  const Box      b     = boxes[lo];
  const uint64_t local = static_cast<uint64_t>(blockIdx.x - b.first_block) * kBlock + threadIdx.x;
  if (local >= b.cells) return; // padding of the box: never written, so never non-zero
  const uint64_t row = local / b.dim[0];
  const uint64_t gx = static_cast<uint64_t>(b.lo[0]) + (local - row * b.dim[0]);
  const uint64_t gy = static_cast<uint64_t>(b.lo[1]) + row % b.dim[1];
  const uint64_t gz = static_cast<uint64_t>(b.lo[2]) + row / b.dim[1];
  const uint64_t at = offset[blockIdx.x] + before;
  index[at]  = gx + g.n[0] * (gy + g.n[1] * gz);
  weight[at] = __ll2float_rn(v) * kFixedStep; // the one rounding of the sum (the scaling by 2^-40 is exact)
}

// device buffers of one build, released on every way out
struct Buffers
{
  std::vector<void*> all;
  ~Buffers()
  {
    for (void* p : all) (void)hipFree(p);
  }
  template<typename T> hipError_t get(T** out, uint64_t count)
  {
    *out = nullptr;
    if (count == 0) return hipSuccess;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e == hipSuccess)
    {
      all.push_back(p);
      *out = static_cast<T*>(p);
    }
    return e;
  }
};

struct Round // the elements whose boxes share one accumulate / count / scan / emit
{
  uint64_t first_element, n_elements, first_work, n_work;
  uint32_t blocks; // 256-cell blocks of its boxes
};

} // namespace

struct kw_offgrid
{
  std::vector<uint64_t> ptr, index;
  std::vector<float>    weight;
};

extern "C" {

kw_status kw_offgrid_build(kw_ctx* ctx, const double* coords, const uint64_t* point_ptr, const float* scale, uint64_t n_elements,
                           uint32_t nx, uint32_t ny, uint32_t nz, double bli_tolerance, uint64_t scratch_bytes, kw_offgrid** out)
{
  KW_CHECK_CTX(ctx);
  KW_REQUIRE(out != nullptr);
  *out = nullptr;
  KW_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= (1u << 30) && ny <= (1u << 30) && nz <= (1u << 30));
  KW_REQUIRE(n_elements == 0 || (point_ptr != nullptr && scale != nullptr));
  KW_REQUIRE(n_elements < 0xFFFFFFFFull);
  if (!(bli_tolerance > 0.0 && bli_tolerance < 1.0))
  {
    kw_set_error("kw_offgrid_build: bli_tolerance %g is outside (0, 1)", bli_tolerance);
    return KW_ERR_INVALID;
  }
  const int radius = static_cast<int>(std::ceil(1.0 / (M_PI * bli_tolerance)));
  if (radius > kMaxRadius)
  {
    kw_set_error("kw_offgrid_build: bli_tolerance %g needs a stencil radius of %d grid points, above the %d supported", bli_tolerance,
                 radius, kMaxRadius);
    return KW_ERR_INVALID;
  }
  // a round's blocks are counted in 32 bits
  const uint64_t budget = std::min<uint64_t>(scratch_bytes ? scratch_bytes : ctx->tuning.offgrid_scratch_bytes,
                                             0x7FFFFFFFull * kBlock * kCellBytes);
  Grid g{};
  g.n[0] = nx, g.n[1] = ny, g.n[2] = nz;
  for (int a = 0; a < 3; a++) g.radius[a] = (g.n[a] > 1) ? radius : 0;

  kw_offgrid* h = new (std::nothrow) kw_offgrid;
  if (h == nullptr) { kw_set_error("kw_offgrid_build: out of host memory"); return KW_ERR_ALLOC; }
  struct Owner { kw_offgrid* h; ~Owner() { delete h; } } owner{h}; // dropped on every failing way out
  try
  {
    h->ptr.assign(n_elements + 1, 0);
    // ---- the points: nearest index and offset, split in float64; the elements' boxes ---------------------------------------
    if (n_elements > 0 && point_ptr[0] != 0)
    {
      kw_set_error("kw_offgrid_build: point_ptr[0] is %llu, not 0 (element 0)", (unsigned long long)point_ptr[0]);
      return KW_ERR_INVALID;
    }
    for (uint64_t e = 0; e < n_elements; e++)
      if (point_ptr[e + 1] < point_ptr[e])
      {
        kw_set_error("kw_offgrid_build: point_ptr is not monotone at element %llu (%llu after %llu)", (unsigned long long)e,
                     (unsigned long long)point_ptr[e + 1], (unsigned long long)point_ptr[e]);
        return KW_ERR_INVALID;
      }
    const uint64_t n_points = n_elements ? point_ptr[n_elements] : 0;
    KW_REQUIRE(n_points == 0 || coords != nullptr);
    if (n_points > kMaxPoints)
    {
      kw_set_error("kw_offgrid_build: point_ptr names %llu integration points, above the %llu supported",
                   (unsigned long long)n_points, (unsigned long long)kMaxPoints);
      return KW_ERR_INVALID;
    }
    std::vector<int32_t> pn(3 * n_points);
    std::vector<float>   pf(3 * n_points);
    std::vector<Box>     boxes(n_elements);
    std::vector<Work>    work;
    std::vector<Round>   rounds;
    uint64_t round_cells = 0; // padded cells of the round being filled
    for (uint64_t e = 0; e < n_elements; e++)
    {
      const uint64_t p0 = point_ptr[e], p1 = point_ptr[e + 1];
      Box& b = boxes[e];
      b = Box{};
      b.scale = scale[e];
      if (!std::isfinite(scale[e]) || std::fabs(static_cast<double>(scale[e])) * static_cast<double>(p1 - p0) >= kMaxAbsSum)
      {
        kw_set_error("kw_offgrid_build: element %llu: scale %g over %llu points: the sum of |scale| must stay below 2^22",
                     (unsigned long long)e, scale[e], (unsigned long long)(p1 - p0));
        return KW_ERR_INVALID;
      }
      int64_t lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
      for (uint64_t p = p0; p < p1; p++)
        for (int a = 0; a < 3; a++)
        {
          const double u = coords[3 * p + a];
          if (!std::isfinite(u))
          {
            kw_set_error("kw_offgrid_build: element %llu, point %llu: coordinate %d is not finite", (unsigned long long)e,
                         (unsigned long long)(p - p0), a);
            return KW_ERR_INVALID;
          }
          const double nearest = std::floor(u + 0.5);
          if (!(nearest >= 0.0 && nearest <= static_cast<double>(g.n[a] - 1)))
          {
            kw_set_error("kw_offgrid_build: element %llu, point %llu: coordinate %d = %.17g lies outside the grid (0 .. %u)",
                         (unsigned long long)e, (unsigned long long)(p - p0), a, u, g.n[a] - 1);
            return KW_ERR_INVALID;
          }
          const int64_t n = static_cast<int64_t>(nearest);
          pn[3 * p + a] = static_cast<int32_t>(n);
          pf[3 * p + a] = static_cast<float>(u - nearest);
          if (p == p0) lo[a] = hi[a] = n;
          else lo[a] = std::min(lo[a], n), hi[a] = std::max(hi[a], n);
        }
      if (p1 > p0)
      {
        b.cells = 1;
        for (int a = 0; a < 3; a++)
        {
          const int64_t l = std::max<int64_t>(lo[a] - g.radius[a], 0);
          const int64_t u = std::min<int64_t>(hi[a] + g.radius[a], static_cast<int64_t>(g.n[a]) - 1);
          b.lo[a]  = static_cast<int32_t>(l);
          b.dim[a] = static_cast<uint32_t>(u - l + 1);
          b.cells *= b.dim[a];
        }
      }
      const uint64_t padded = (b.cells + kBlock - 1) / kBlock * kBlock;
      if (padded * kCellBytes > budget)
      {
        kw_set_error("kw_offgrid_build: element %llu: its box of %u x %u x %u grid points needs %llu bytes of scratch, the budget "
                     "is %llu", (unsigned long long)e, b.dim[0], b.dim[1], b.dim[2], (unsigned long long)(padded * kCellBytes),
                     (unsigned long long)budget);
        return KW_ERR_ALLOC;
      }
      if (rounds.empty() || (round_cells + padded) * kCellBytes > budget)
      {
        rounds.push_back(Round{e, 0, work.size(), 0, 0});
        round_cells = 0;
      }
      Round& r = rounds.back();
      b.first_block = static_cast<uint32_t>(round_cells / kBlock);
      round_cells += padded;
      r.blocks = static_cast<uint32_t>(round_cells / kBlock);
      for (uint64_t p = p0; p < p1; p += kPointsPerBlock)
        work.push_back(Work{p, static_cast<uint32_t>(std::min<uint64_t>(kPointsPerBlock, p1 - p)),
                            static_cast<uint32_t>(e - r.first_element)});
      r.n_elements = e + 1 - r.first_element;
      r.n_work     = work.size() - r.first_work;
    }
    uint32_t max_blocks = 0;
    for (const Round& r : rounds) max_blocks = std::max(max_blocks, r.blocks);
    if (max_blocks == 0) // no element has a point: empty rows
    {
      owner.h = nullptr;
      *out    = h;
      return KW_OK;
    }

    // ---- device: points, tables, the scratch of the largest round ----------------------------------------------------------
    KW_HIP(hipSetDevice(ctx->device));
    Buffers   dev;
    int32_t*  d_pn = nullptr;
    float*    d_pf = nullptr;
    Box*      d_boxes = nullptr;
    Work*     d_work = nullptr;
    long long* d_acc = nullptr;
    uint32_t* d_count = nullptr;
    uint64_t *d_offset = nullptr, *d_index = nullptr;
    float*    d_weight = nullptr;
    const uint64_t max_cells = static_cast<uint64_t>(max_blocks) * kBlock;
    KW_HIP(dev.get(&d_pn, pn.size()));
    KW_HIP(dev.get(&d_pf, pf.size()));
    KW_HIP(dev.get(&d_boxes, boxes.size()));
    KW_HIP(dev.get(&d_work, work.size()));
    KW_HIP(dev.get(&d_acc, max_cells));
    KW_HIP(dev.get(&d_count, static_cast<uint64_t>(max_blocks)));
    KW_HIP(dev.get(&d_offset, static_cast<uint64_t>(max_blocks) + 1));
    KW_HIP(dev.get(&d_index, max_cells));
    KW_HIP(dev.get(&d_weight, max_cells));
    hipStream_t s = ctx->stream;
    KW_HIP(hipMemcpyAsync(d_pn, pn.data(), pn.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    KW_HIP(hipMemcpyAsync(d_pf, pf.data(), pf.size() * sizeof(float), hipMemcpyHostToDevice, s));
    KW_HIP(hipMemcpyAsync(d_boxes, boxes.data(), boxes.size() * sizeof(Box), hipMemcpyHostToDevice, s));
    KW_HIP(hipMemcpyAsync(d_work, work.data(), work.size() * sizeof(Work), hipMemcpyHostToDevice, s));

    std::vector<uint64_t> offset;
    for (const Round& r : rounds)
    {
      if (r.blocks == 0) // elements without points only
      {
        for (uint64_t e = r.first_element; e < r.first_element + r.n_elements; e++) h->ptr[e + 1] = h->index.size();
        continue;
      }
      const uint64_t cells = static_cast<uint64_t>(r.blocks) * kBlock;
      const Box*     rb    = d_boxes + r.first_element;
      KW_HIP(hipMemsetAsync(d_acc, 0, cells * sizeof(long long), s));
      if (r.n_work > 0)
      {
        KW_REQUIRE(r.n_work <= 0x7FFFFFFFull);
        hipLaunchKernelGGL(k_offgrid_accumulate, dim3(static_cast<uint32_t>(r.n_work)), dim3(kBlock), 0, s,
                           reinterpret_cast<unsigned long long*>(d_acc), d_work + r.first_work, rb, d_pn, d_pf, g);
        KW_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL(k_offgrid_count, dim3(r.blocks), dim3(kBlock), 0, s, d_count, d_acc);
      KW_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_offgrid_scan, dim3(1), dim3(1024), 0, s, d_offset, d_count, r.blocks);
      KW_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_offgrid_emit, dim3(r.blocks), dim3(kBlock), 0, s, d_index, d_weight, d_acc, d_offset, rb,
                         static_cast<uint32_t>(r.n_elements), g);
      KW_LAUNCH_CHECK();
      offset.resize(static_cast<size_t>(r.blocks) + 1);
      KW_HIP(hipMemcpyAsync(offset.data(), d_offset, offset.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
      KW_HIP(hipStreamSynchronize(s)); // the round's entry count sizes the host arrays
      const uint64_t base = h->index.size(), nnz = offset[r.blocks];
      KW_REQUIRE(nnz <= cells);
      h->index.resize(base + nnz);
      h->weight.resize(base + nnz);
      if (nnz > 0)
      {
        KW_HIP(hipMemcpyAsync(h->index.data() + base, d_index, nnz * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        KW_HIP(hipMemcpyAsync(h->weight.data() + base, d_weight, nnz * sizeof(float), hipMemcpyDeviceToHost, s));
        KW_HIP(hipStreamSynchronize(s)); // before the next round overwrites the staging arrays
      }
      for (uint64_t i = 0; i < r.n_elements; i++)
      {
        const uint64_t e   = r.first_element + i;
        const uint32_t end = (i + 1 < r.n_elements) ? boxes[e + 1].first_block : r.blocks;
        h->ptr[e + 1] = base + offset[end];
      }
    }
  }
  catch (const std::exception&) // bad_alloc or length_error of the host arrays: nothing may cross the C boundary
  {
    kw_set_error("kw_offgrid_build: out of host memory");
    return KW_ERR_ALLOC;
  }
  owner.h = nullptr;
  *out    = h;
  return KW_OK;
}

kw_status kw_offgrid_size(kw_ctx* ctx, const kw_offgrid* h, uint64_t* out_n_elements, uint64_t* out_nnz)
{
  KW_CHECK_CTX(ctx);
  KW_REQUIRE(h != nullptr);
  if (out_n_elements) *out_n_elements = h->ptr.size() - 1;
  if (out_nnz) *out_nnz = h->index.size();
  return KW_OK;
}

kw_status kw_offgrid_ptr(kw_ctx* ctx, const kw_offgrid* h, uint64_t* out_ptr)
{
  KW_CHECK_CTX(ctx);
  KW_REQUIRE(h != nullptr && out_ptr != nullptr);
  memcpy(out_ptr, h->ptr.data(), h->ptr.size() * sizeof(uint64_t));
  return KW_OK;
}

kw_status kw_offgrid_entries(kw_ctx* ctx, const kw_offgrid* h, uint64_t* out_index, float* out_weight)
{
  KW_CHECK_CTX(ctx);
  KW_REQUIRE(h != nullptr);
  if (h->index.empty()) return KW_OK;
  if (out_index) memcpy(out_index, h->index.data(), h->index.size() * sizeof(uint64_t));
  if (out_weight) memcpy(out_weight, h->weight.data(), h->weight.size() * sizeof(float));
  return KW_OK;
}

kw_status kw_offgrid_free(kw_ctx* ctx, kw_offgrid* h)
{
  KW_CHECK_CTX(ctx);
  delete h;
  return KW_OK;
}

} // extern "C"
