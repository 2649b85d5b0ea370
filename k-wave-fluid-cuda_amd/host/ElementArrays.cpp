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

void ElementCsr::release()
{
  if (ctx())
    for (void* d : {static_cast<void*>(mPtr), static_cast<void*>(mEntries), static_cast<void*>(mChunkPtr),
                    static_cast<void*>(mPartials)})
      if (d) kw_free(ctx(), d);
  mPtr = nullptr;
  mEntries = nullptr;
  mChunkPtr = nullptr;
  mPartials = nullptr;
  mRows = mNnz = 0;
  mChunks = 0;
}
