// kw_element_kernels.hip — weighted transducer arrays (kwave_hip.h, "Weighted transducer arrays"): the element signals
// expanded to per-point source values, and the sampled pressure reduced to one value per element.  Both are gathers over
// a CSR matrix whose entries are (uint32 column, float weight) pairs, so each entry is one 8-byte load and no output is
// written by more than one thread: the summation order is fixed by the CSR alone.
#include "kw_internal.h"

namespace {

constexpr uint32_t kBlock = 256;                          // 4 waves
constexpr uint32_t kChunk = KW_ELEMENT_CHUNK;             // entries per block of the sensor reduction
static_assert(kChunk % kBlock == 0, "a chunk is a whole number of block-wide passes");

} // namespace

// one thread per source point: its row of the CSR in order, fp32 fma from 0
__global__ __launch_bounds__(256) void k_element_source_row(float* __restrict__ row, const float* __restrict__ signal_t,
                                                            const uint32_t* __restrict__ ptr,
                                                            const uint2* __restrict__ entries, uint32_t n_points)
{
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n_points; k += gridDim.x * blockDim.x)
  {
    const uint32_t end = ptr[k + 1];
    float acc = 0.0f;
    for (uint32_t j = ptr[k]; j < end; j++)
    {
      const uint2 e = entries[j];
      acc = __fmaf_rn(__uint_as_float(e.y), signal_t[e.x], acc);
    }
    row[k] = acc;
  }
}

// one block per (element, chunk): lane l of the block sums entries begin + l, begin + l + 256, ... with fp32 fma, then a
// butterfly over the 64 lanes of each wave and the four wave sums in a fixed pairing give the chunk's partial sum
__global__ __launch_bounds__(256) void k_sample_elements(float* __restrict__ partials, const float* __restrict__ p,
                                                         const uint32_t* __restrict__ ptr, const uint2* __restrict__ entries,
                                                         const uint32_t* __restrict__ chunk_ptr, uint32_t n_elements)
{
  const uint32_t b = blockIdx.x;
  // the element whose chunks include b: the largest e with chunk_ptr[e] <= b (rows without chunks are skipped over)
  uint32_t lo = 0, hi = n_elements;
  while (hi - lo > 1)
  {
    const uint32_t mid = (lo + hi) >> 1;
    if (chunk_ptr[mid] <= b) lo = mid;
    else hi = mid;
  }
  const uint32_t row_end = ptr[lo + 1];
  const uint32_t begin   = ptr[lo] + (b - chunk_ptr[lo]) * kChunk;
  const uint32_t end     = (begin >= row_end) ? begin : ((row_end - begin > kChunk) ? begin + kChunk : row_end);
  float acc = 0.0f;
  for (uint32_t j = begin + threadIdx.x; j < end; j += kBlock)
  {
    const uint2 e = entries[j];
    acc = __fmaf_rn(__uint_as_float(e.y), p[e.x], acc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  __shared__ float wave_sum[kBlock / 64];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[b] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// one thread per element: its chunk partials in chunk order (0 for an empty row)
__global__ __launch_bounds__(256) void k_sample_elements_sum(float* __restrict__ out, const float* __restrict__ partials,
                                                             const uint32_t* __restrict__ chunk_ptr, uint32_t n_elements)
{
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elements) return;
  const uint32_t end = chunk_ptr[e + 1];
  float acc = 0.0f;
  for (uint32_t c = chunk_ptr[e]; c < end; c++) acc += partials[c];
  out[e] = acc;
}

// ---- the velocity components: one index set and one weight matrix for up to three fields, every entry read once --------
struct ElementRows
{
  float*       row[3];    // nullptr: the component is not written ...
  const float* signal[3]; // ... and its signal row is not read
};
struct ElementFields
{
  float*       out[3];
  const float* field[3];
};

// k_element_source_row for the components X / Y / Z chosen at compile time: per component the same fma chain from 0 over
// the row in CSR order, so each row carries the bits the one-component kernel gives
template<bool X, bool Y, bool Z>
__device__ __forceinline__ void element_source_rows_body(const ElementRows& a, const uint32_t* __restrict__ ptr,
                                                         const uint2* __restrict__ entries, uint32_t n_points)
{
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n_points; k += gridDim.x * blockDim.x)
  {
    const uint32_t end = ptr[k + 1];
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    for (uint32_t j = ptr[k]; j < end; j++)
    {
      const uint2 e = entries[j];
      const float w = __uint_as_float(e.y);
      if (X) ax = __fmaf_rn(w, a.signal[0][e.x], ax);
      if (Y) ay = __fmaf_rn(w, a.signal[1][e.x], ay);
      if (Z) az = __fmaf_rn(w, a.signal[2][e.x], az);
    }
    if (X) a.row[0][k] = ax;
    if (Y) a.row[1][k] = ay;
    if (Z) a.row[2][k] = az;
  }
}

// the component pointers are kernel arguments: the switch is one scalar branch per wave, taken before the loops
__global__ __launch_bounds__(256) void k_element_source_rows(ElementRows a, const uint32_t* __restrict__ ptr,
                                                             const uint2* __restrict__ entries, uint32_t n_points)
{
  const uint32_t mask = (a.row[0] ? 1u : 0u) | (a.row[1] ? 2u : 0u) | (a.row[2] ? 4u : 0u);
  switch (mask)
  {
    case 1: element_source_rows_body<true, false, false>(a, ptr, entries, n_points); break;
    case 2: element_source_rows_body<false, true, false>(a, ptr, entries, n_points); break;
    case 3: element_source_rows_body<true, true, false>(a, ptr, entries, n_points); break;
    case 4: element_source_rows_body<false, false, true>(a, ptr, entries, n_points); break;
    case 5: element_source_rows_body<true, false, true>(a, ptr, entries, n_points); break;
    case 6: element_source_rows_body<false, true, true>(a, ptr, entries, n_points); break;
    case 7: element_source_rows_body<true, true, true>(a, ptr, entries, n_points); break;
    default: break;
  }
}

// k_sample_elements with one accumulator per field: the same chunk, lane stride, butterfly and wave pairing, so field f's
// partial of chunk b (partials[f * n_chunks + b]) carries the bits k_sample_elements gives on that field alone
template<int NF>
__global__ __launch_bounds__(256) void k_sample_elements_multi(float* __restrict__ partials, ElementFields a,
                                                               const uint32_t* __restrict__ ptr,
                                                               const uint2* __restrict__ entries,
                                                               const uint32_t* __restrict__ chunk_ptr, uint32_t n_elements,
                                                               uint32_t n_chunks)
{
  const uint32_t b = blockIdx.x;
  uint32_t lo = 0, hi = n_elements;
  while (hi - lo > 1)
  {
    const uint32_t mid = (lo + hi) >> 1;
    if (chunk_ptr[mid] <= b) lo = mid;
    else hi = mid;
  }
  const uint32_t row_end = ptr[lo + 1];
  const uint32_t begin   = ptr[lo] + (b - chunk_ptr[lo]) * kChunk;
  const uint32_t end     = (begin >= row_end) ? begin : ((row_end - begin > kChunk) ? begin + kChunk : row_end);
  float acc[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) acc[f] = 0.0f;
  for (uint32_t j = begin + threadIdx.x; j < end; j += kBlock)
  {
    const uint2 e = entries[j];
    const float w = __uint_as_float(e.y);
#pragma unroll
    for (int f = 0; f < NF; f++) acc[f] = __fmaf_rn(w, a.field[f][e.x], acc[f]);
  }
  __shared__ float wave_sum[NF][kBlock / 64];
#pragma unroll
  for (int f = 0; f < NF; f++)
  {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[f] += __shfl_xor(acc[f], off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[f][threadIdx.x >> 6] = acc[f];
  }
  __syncthreads();
  if (threadIdx.x < NF)
  {
    const float* s = wave_sum[threadIdx.x];
    partials[threadIdx.x * n_chunks + b] = (s[0] + s[1]) + (s[2] + s[3]);
  }
}

// one thread per element: per field, its chunk partials in chunk order (0 for an empty row)
__global__ __launch_bounds__(256) void k_sample_elements_multi_sum(ElementFields a, uint32_t n_fields,
                                                                   const float* __restrict__ partials,
                                                                   const uint32_t* __restrict__ chunk_ptr,
                                                                   uint32_t n_elements, uint32_t n_chunks)
{
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elements) return;
  const uint32_t begin = chunk_ptr[e], end = chunk_ptr[e + 1];
#pragma unroll
  for (uint32_t f = 0; f < 3; f++) // unrolled: a.out[f] stays a kernel argument, not an indexed copy
  {
    if (f >= n_fields) break;
    float acc = 0.0f;
    for (uint32_t c = begin; c < end; c++) acc += partials[f * n_chunks + c];
    a.out[f][e] = acc;
  }
}

// ---- per-entry time delays -------------------------------------------------------------------------------------------
struct ElementDelayedRows
{
  float*       row[3];    // nullptr: the component is not written ...
  const float* signal[3]; // ... and its signals (steps[c] rows of n_elements values) are not read
  uint64_t     steps[3];
};

// element_source_rows_body with entry j reading signal row t - delays[j]: the same fma chain from 0 in CSR order, an entry
// whose row lies before the signal's start or past its end is left out of the chain
template<bool X, bool Y, bool Z>
__device__ __forceinline__ void element_source_rows_delayed_body(const ElementDelayedRows& a, const uint32_t* __restrict__ ptr,
                                                                 const uint2* __restrict__ entries,
                                                                 const uint32_t* __restrict__ delays, uint32_t n_points,
                                                                 uint32_t n_elements, uint64_t t)
{
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n_points; k += gridDim.x * blockDim.x)
  {
    const uint32_t end = ptr[k + 1];
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    for (uint32_t j = ptr[k]; j < end; j++)
    {
      const uint2    e = entries[j];
      const uint64_t d = delays[j];
      if (d > t) continue;
      const uint64_t s   = t - d;
      const size_t   at  = static_cast<size_t>(s) * n_elements + e.x;
      const float    w   = __uint_as_float(e.y);
      if (X && s < a.steps[0]) ax = __fmaf_rn(w, a.signal[0][at], ax);
      if (Y && s < a.steps[1]) ay = __fmaf_rn(w, a.signal[1][at], ay);
      if (Z && s < a.steps[2]) az = __fmaf_rn(w, a.signal[2][at], az);
    }
    if (X) a.row[0][k] = ax;
    if (Y) a.row[1][k] = ay;
    if (Z) a.row[2][k] = az;
  }
}

__global__ __launch_bounds__(256) void k_element_source_rows_delayed(ElementDelayedRows a, const uint32_t* __restrict__ ptr,
                                                                     const uint2* __restrict__ entries,
                                                                     const uint32_t* __restrict__ delays, uint32_t n_points,
                                                                     uint32_t n_elements, uint64_t t)
{
  const uint32_t mask = (a.row[0] ? 1u : 0u) | (a.row[1] ? 2u : 0u) | (a.row[2] ? 4u : 0u);
  switch (mask)
  {
    case 1: element_source_rows_delayed_body<true, false, false>(a, ptr, entries, delays, n_points, n_elements, t); break;
    case 2: element_source_rows_delayed_body<false, true, false>(a, ptr, entries, delays, n_points, n_elements, t); break;
    case 3: element_source_rows_delayed_body<true, true, false>(a, ptr, entries, delays, n_points, n_elements, t); break;
    case 4: element_source_rows_delayed_body<false, false, true>(a, ptr, entries, delays, n_points, n_elements, t); break;
    case 5: element_source_rows_delayed_body<true, false, true>(a, ptr, entries, delays, n_points, n_elements, t); break;
    case 6: element_source_rows_delayed_body<false, true, true>(a, ptr, entries, delays, n_points, n_elements, t); break;
    case 7: element_source_rows_delayed_body<true, true, true>(a, ptr, entries, delays, n_points, n_elements, t); break;
    default: break;
  }
}

struct ElementRings
{
  float* out[3];
  float* ring[3]; // ring_rows x n_elements floats per field
};

// one thread per element: each of its groups' chunk partials in chunk order from 0, added to the ring row the group's
// delay points at; then the row of this step is emitted and cleared.  Column e of every ring row belongs to this thread
// alone, so the additions need no atomics and arrive in a fixed order.
__global__ __launch_bounds__(256) void k_sample_elements_ring(ElementRings a, uint32_t n_fields,
                                                              const float* __restrict__ partials,
                                                              const uint32_t* __restrict__ element_group_ptr,
                                                              const uint32_t* __restrict__ group_delay,
                                                              const uint32_t* __restrict__ chunk_ptr, uint32_t n_elements,
                                                              uint32_t n_chunks, uint32_t ring_rows, uint32_t row_now)
{
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elements) return;
  const uint32_t g_begin = element_group_ptr[e], g_end = element_group_ptr[e + 1];
#pragma unroll
  for (uint32_t f = 0; f < 3; f++) // unrolled: a.ring[f] and a.out[f] stay kernel arguments
  {
    if (f >= n_fields) break;
    float* ring = a.ring[f];
    for (uint32_t g = g_begin; g < g_end; g++)
    {
      const uint32_t end = chunk_ptr[g + 1];
      float acc = 0.0f;
      for (uint32_t c = chunk_ptr[g]; c < end; c++) acc += partials[f * n_chunks + c];
      // row_now < ring_rows and the remainder of the delay keep the row inside the ring whatever the delay holds
      const uint32_t r = static_cast<uint32_t>((static_cast<uint64_t>(row_now) + group_delay[g]) % ring_rows);
      const size_t  at = static_cast<size_t>(r) * n_elements + e;
      ring[at] += acc;
    }
    const size_t now = static_cast<size_t>(row_now) * n_elements + e;
    a.out[f][e] = ring[now];
    ring[now]   = 0.0f;
  }
}

extern "C" {

kw_status kw_element_source_rows(kw_ctx* ctx, float* const rows[3], const float* const element_inputs[3],
                                 const uint32_t* ptr, const kw_csr_entry* entries, uint32_t n_points, uint32_t n_elements,
                                 uint64_t time_index)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "element_source_rows");
  KW_REQUIRE(rows && element_inputs);
  ElementRows a{};
  bool any = false;
  for (int c = 0; c < 3; c++)
  {
    if (rows[c] == nullptr) continue; // skipped: element_inputs[c] is not looked at
    KW_REQUIRE(element_inputs[c] != nullptr);
    a.row[c]    = rows[c];
    a.signal[c] = element_inputs[c] + time_index * n_elements;
    any         = true;
  }
  if (n_points == 0 || !any) return KW_OK;
  KW_REQUIRE(ptr && entries && n_elements > 0);
  uint32_t grid = (n_points + kBlock - 1) / kBlock;
  const uint32_t cap = static_cast<uint32_t>(ctx->cu_count) * 8;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(k_element_source_rows, dim3(grid), dim3(kBlock), 0, ctx->stream, a, ptr,
                     reinterpret_cast<const uint2*>(entries), n_points);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_sample_elements_multi(kw_ctx* ctx, uint32_t n_fields, float* const outs[], const float* const fields[],
                                   const uint32_t* ptr, const kw_csr_entry* entries, uint32_t n_elements, uint64_t nnz,
                                   const uint32_t* chunk_ptr, uint32_t n_chunks, float* partials)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "sample_elements_multi");
  KW_REQUIRE(n_fields >= 1 && n_fields <= 3 && outs && fields);
  if (n_elements == 0) return KW_OK;
  KW_REQUIRE(ptr && chunk_ptr && nnz <= 0xFFFFFFFFull);
  KW_REQUIRE(static_cast<uint64_t>(n_fields) * n_chunks <= 0xFFFFFFFFull);
  KW_REQUIRE(n_chunks == 0 || (entries && partials));
  ElementFields a{};
  for (uint32_t f = 0; f < n_fields; f++)
  {
    KW_REQUIRE(outs[f] && (n_chunks == 0 || fields[f]));
    a.out[f]   = outs[f];
    a.field[f] = fields[f];
  }
  if (n_chunks > 0)
  {
    const uint2* e = reinterpret_cast<const uint2*>(entries);
    if (n_fields == 1)
      hipLaunchKernelGGL(k_sample_elements_multi<1>, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, partials, a, ptr, e,
                         chunk_ptr, n_elements, n_chunks);
    else if (n_fields == 2)
      hipLaunchKernelGGL(k_sample_elements_multi<2>, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, partials, a, ptr, e,
                         chunk_ptr, n_elements, n_chunks);
    else
      hipLaunchKernelGGL(k_sample_elements_multi<3>, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, partials, a, ptr, e,
                         chunk_ptr, n_elements, n_chunks);
    KW_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_sample_elements_multi_sum, dim3((n_elements + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, a,
                     n_fields, partials, chunk_ptr, n_elements, n_chunks);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_element_source_row(kw_ctx* ctx, float* row, const float* element_input, const uint32_t* ptr,
                                const kw_csr_entry* entries, uint32_t n_points, uint32_t n_elements, uint64_t time_index)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "element_source_row");
  if (n_points == 0) return KW_OK;
  KW_REQUIRE(row && element_input && ptr && entries && n_elements > 0);
  static_assert(sizeof(kw_csr_entry) == sizeof(uint2), "an entry is one 8-byte load");
  uint32_t grid = (n_points + kBlock - 1) / kBlock;
  const uint32_t cap = static_cast<uint32_t>(ctx->cu_count) * 8;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(k_element_source_row, dim3(grid), dim3(kBlock), 0, ctx->stream, row,
                     element_input + time_index * n_elements, ptr, reinterpret_cast<const uint2*>(entries), n_points);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_sample_elements(kw_ctx* ctx, float* out, const float* p, const uint32_t* ptr, const kw_csr_entry* entries,
                             uint32_t n_elements, uint64_t nnz, const uint32_t* chunk_ptr, uint32_t n_chunks,
                             float* partials)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "sample_elements");
  if (n_elements == 0) return KW_OK;
  KW_REQUIRE(out && ptr && chunk_ptr && nnz <= 0xFFFFFFFFull);
  KW_REQUIRE(n_chunks == 0 || (p && entries && partials));
  if (n_chunks > 0)
  {
    hipLaunchKernelGGL(k_sample_elements, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, partials, p, ptr,
                       reinterpret_cast<const uint2*>(entries), chunk_ptr, n_elements);
    KW_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_sample_elements_sum, dim3((n_elements + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, out,
                     partials, chunk_ptr, n_elements);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_element_source_rows_delayed(kw_ctx* ctx, float* const rows[3], const float* const element_inputs[3],
                                         const uint64_t signal_steps[3], const uint32_t* ptr, const kw_csr_entry* entries,
                                         const uint32_t* delays, uint32_t n_points, uint32_t n_elements, uint64_t time_index)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "element_source_rows_delayed");
  KW_REQUIRE(rows && element_inputs && signal_steps);
  ElementDelayedRows a{};
  bool any = false;
  for (int c = 0; c < 3; c++)
  {
    if (rows[c] == nullptr) continue; // skipped: element_inputs[c] and signal_steps[c] are not looked at
    KW_REQUIRE(element_inputs[c] != nullptr);
    a.row[c]    = rows[c];
    a.signal[c] = element_inputs[c];
    a.steps[c]  = signal_steps[c];
    any         = true;
  }
  if (n_points == 0 || !any) return KW_OK;
  KW_REQUIRE(ptr && entries && delays && n_elements > 0);
  uint32_t grid = (n_points + kBlock - 1) / kBlock;
  const uint32_t cap = static_cast<uint32_t>(ctx->cu_count) * 8;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(k_element_source_rows_delayed, dim3(grid), dim3(kBlock), 0, ctx->stream, a, ptr,
                     reinterpret_cast<const uint2*>(entries), delays, n_points, n_elements, time_index);
  KW_LAUNCH_CHECK();
  return KW_OK;
}

kw_status kw_sample_elements_delayed(kw_ctx* ctx, uint32_t n_fields, float* const outs[], const float* const fields[],
                                     const uint32_t* group_ptr, const kw_csr_entry* entries, const uint32_t* group_delay,
                                     const uint32_t* element_group_ptr, uint32_t n_elements, uint32_t n_groups, uint64_t nnz,
                                     const uint32_t* chunk_ptr, uint32_t n_chunks, float* partials, float* const rings[],
                                     uint32_t ring_rows, uint64_t rows_emitted)
{
  KW_CHECK_CTX(ctx);
  KW_PROF(ctx, "sample_elements_delayed");
  KW_REQUIRE(n_fields >= 1 && n_fields <= 3 && outs && fields && rings);
  if (n_elements == 0) return KW_OK;
  KW_REQUIRE(ring_rows >= 1 && element_group_ptr && nnz <= 0xFFFFFFFFull);
  KW_REQUIRE(static_cast<uint64_t>(n_fields) * n_chunks <= 0xFFFFFFFFull);
  KW_REQUIRE(n_groups == 0 || (group_ptr && group_delay && chunk_ptr));
  KW_REQUIRE(n_chunks == 0 || (n_groups > 0 && entries && partials));
  ElementFields a{};
  ElementRings  r{};
  for (uint32_t f = 0; f < n_fields; f++)
  {
    KW_REQUIRE(outs[f] && rings[f] && (n_chunks == 0 || fields[f]));
    a.field[f] = fields[f];
    r.out[f]   = outs[f];
    r.ring[f]  = rings[f];
  }
  if (n_chunks > 0)
  {
    // the groups as rows of k_sample_elements_multi: a group's partials carry the bits its row would
    const uint2* e = reinterpret_cast<const uint2*>(entries);
    if (n_fields == 1)
      hipLaunchKernelGGL(k_sample_elements_multi<1>, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, partials, a, group_ptr, e,
                         chunk_ptr, n_groups, n_chunks);
    else if (n_fields == 2)
      hipLaunchKernelGGL(k_sample_elements_multi<2>, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, partials, a, group_ptr, e,
                         chunk_ptr, n_groups, n_chunks);
    else
      hipLaunchKernelGGL(k_sample_elements_multi<3>, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, partials, a, group_ptr, e,
                         chunk_ptr, n_groups, n_chunks);
    KW_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_sample_elements_ring, dim3((n_elements + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, r,
                     n_fields, partials, element_group_ptr, group_delay, chunk_ptr, n_elements, n_chunks, ring_rows,
                     static_cast<uint32_t>(rows_emitted % ring_rows));
  KW_LAUNCH_CHECK();
  return KW_OK;
}

} // extern "C"
