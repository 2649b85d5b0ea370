// ElementArrays.cpp — see ElementArrays.h.
#include "ElementArrays.h"

#include <vector>

#include "HipError.h"
#include "Parameters.h"

static kw_ctx* ctx() { return Parameters::getInstance().getHipParameters().getContext(); }

void ElementCsr::upload(const size_t* ptr, size_t rows, const size_t* cols1, const float* weights, size_t nnz, bool chunks,
                        size_t fields)
{
  release();
  mRows = rows;
  mNnz  = nnz;
  std::vector<uint32_t> p(rows + 1), cp(rows + 1, 0);
  for (size_t r = 0; r <= rows; r++) p[r] = static_cast<uint32_t>(ptr[r]);
  std::vector<kw_csr_entry> e(nnz);
  for (size_t j = 0; j < nnz; j++) e[j] = kw_csr_entry{static_cast<uint32_t>(cols1[j] - 1), weights[j]};
  for (size_t r = 0; r < rows; r++) cp[r + 1] = cp[r] + (p[r + 1] - p[r] + KW_ELEMENT_CHUNK - 1) / KW_ELEMENT_CHUNK;
  mChunks = cp[rows];
  auto put = [](const void* src, size_t bytes) {
    void* d = nullptr;
    kwCheck(kw_malloc(ctx(), bytes, &d));
    if (bytes) kwCheck(kw_memcpy_h2d(ctx(), d, src, bytes));
    return d;
  };
  mPtr     = static_cast<uint32_t*>(put(p.data(), p.size() * sizeof(uint32_t)));
  mEntries = static_cast<kw_csr_entry*>(put(e.data(), e.size() * sizeof(kw_csr_entry)));
  if (chunks)
  {
    mChunkPtr = static_cast<uint32_t*>(put(cp.data(), cp.size() * sizeof(uint32_t)));
    void* d   = nullptr;
    kwCheck(kw_malloc(ctx(), fields * mChunks * sizeof(float), &d));
    mPartials = static_cast<float*>(d);
  }
}

namespace {
void* put(const void* src, size_t bytes)
{
  void* d = nullptr;
  kwCheck(kw_malloc(ctx(), bytes, &d));
  if (bytes) kwCheck(kw_memcpy_h2d(ctx(), d, src, bytes));
  return d;
}
} // namespace

void ElementCsr::uploadWithDelays(const size_t* ptr, size_t rows, const size_t* cols1, const float* weights,
                                  const size_t* delays, size_t nnz)
{
  upload(ptr, rows, cols1, weights, nnz, false);
  std::vector<uint32_t> d(nnz);
  for (size_t j = 0; j < nnz; j++) d[j] = static_cast<uint32_t>(delays[j]);
  mDelays = static_cast<uint32_t*>(put(d.data(), d.size() * sizeof(uint32_t)));
}

void ElementCsr::uploadDelayed(const size_t* ptr, size_t rows, const size_t* cols1, const float* weights, const size_t* delays,
                               size_t nnz, size_t fields)
{
  release();
  mRows = rows;
  mNnz  = nnz;
  mGrouped = true;
  const ElementGroups g = regroup(ptr, rows, delays);
  std::vector<kw_csr_entry> e(nnz);
  for (size_t j = 0; j < nnz; j++) e[j] = kw_csr_entry{static_cast<uint32_t>(cols1[g.order[j]] - 1), weights[g.order[j]]};
  uint32_t maxDelay = 0;
  for (uint32_t d : g.groupDelay) maxDelay = (d > maxDelay) ? d : maxDelay;
  mGroups   = static_cast<uint32_t>(g.groups());
  mChunks   = g.chunkPtr.back();
  mRingRows = maxDelay + 1;
  mPtr             = static_cast<uint32_t*>(put(g.groupPtr.data(), g.groupPtr.size() * sizeof(uint32_t)));
  mEntries         = static_cast<kw_csr_entry*>(put(e.data(), e.size() * sizeof(kw_csr_entry)));
  mChunkPtr        = static_cast<uint32_t*>(put(g.chunkPtr.data(), g.chunkPtr.size() * sizeof(uint32_t)));
  mDelays          = static_cast<uint32_t*>(put(g.groupDelay.data(), g.groupDelay.size() * sizeof(uint32_t)));
  mElementGroupPtr = static_cast<uint32_t*>(put(g.elementGroupPtr.data(), g.elementGroupPtr.size() * sizeof(uint32_t)));
  void* d = nullptr;
  kwCheck(kw_malloc(ctx(), fields * mChunks * sizeof(float), &d));
  mPartials = static_cast<float*>(d);
  const size_t ringBytes = fields * mRingRows * rows * sizeof(float);
  kwCheck(kw_malloc(ctx(), ringBytes, &d));
  mRing = static_cast<float*>(d);
  if (ringBytes) kwCheck(kw_memset(ctx(), mRing, 0, ringBytes));
}

void ElementCsr::release()
{
  if (ctx())
    for (void* d : {static_cast<void*>(mPtr), static_cast<void*>(mEntries), static_cast<void*>(mChunkPtr),
                    static_cast<void*>(mPartials), static_cast<void*>(mDelays), static_cast<void*>(mElementGroupPtr),
                    static_cast<void*>(mRing)})
      if (d) kw_free(ctx(), d);
  mPtr = nullptr;
  mEntries = nullptr;
  mChunkPtr = nullptr;
  mPartials = nullptr;
  mDelays = nullptr;
  mElementGroupPtr = nullptr;
  mRing = nullptr;
  mGroups = mRingRows = 0;
  mGrouped = false;
  mRows = mNnz = 0;
  mChunks = 0;
}
