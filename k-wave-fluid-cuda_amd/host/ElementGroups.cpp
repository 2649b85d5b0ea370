// ElementGroups.cpp — ElementCsr::regroup (ElementArrays.h): host arithmetic alone, so that a program without a device can
// call it.
#include <algorithm>
#include <numeric>

#include "ElementArrays.h"

ElementGroups ElementCsr::regroup(const size_t* ptr, size_t rows, const size_t* delays)
{
  ElementGroups g;
  const size_t nnz = (rows > 0) ? ptr[rows] : 0;
  g.order.resize(nnz);
  std::iota(g.order.begin(), g.order.end(), 0u);
  g.elementGroupPtr.assign(rows + 1, 0);
  g.groupPtr.push_back(0);
  g.chunkPtr.push_back(0);
  for (size_t r = 0; r < rows; r++)
  {
    std::stable_sort(g.order.begin() + ptr[r], g.order.begin() + ptr[r + 1],
                     [&](uint32_t a, uint32_t b) { return delays[a] < delays[b]; });
    for (size_t j = ptr[r]; j < ptr[r + 1]; j++)
    {
      const bool last = (j + 1 == ptr[r + 1]) || (delays[g.order[j + 1]] != delays[g.order[j]]);
      if (!last) continue;
      const uint32_t length = static_cast<uint32_t>(j + 1) - g.groupPtr.back();
      g.groupDelay.push_back(static_cast<uint32_t>(delays[g.order[j]]));
      g.groupPtr.push_back(static_cast<uint32_t>(j + 1));
      g.chunkPtr.push_back(g.chunkPtr.back() + (length + KW_ELEMENT_CHUNK - 1) / KW_ELEMENT_CHUNK);
    }
    g.elementGroupPtr[r + 1] = static_cast<uint32_t>(g.groupDelay.size());
  }
  return g;
}
