// ElementArrays.h — device form of the CSR weight matrices of a weighted transducer array (kwave_hip.h, "Weighted
// transducer arrays").  New with this build; the reference takes such an array only in expanded form (one series per
// grid point, p_source_many = 1, and -p over every point).
#ifndef KW_HOST_ELEMENT_ARRAYS_H
#define KW_HOST_ELEMENT_ARRAYS_H
#include <cstddef>
#include <cstdint>

#include "kwave_hip.h"

/// One CSR matrix on the device: uint32 row offsets, packed (0-based column, weight) entries and, for the sensor
/// reduction, the chunk offsets of kw_sample_elements with its partial-sum workspace.  Built from the input datasets
/// (0-based uint64 offsets, 1-based uint64 columns), which Parameters::init has checked already.
class ElementCsr
{
 public:
  ElementCsr() = default;
  ~ElementCsr() { release(); }
  ElementCsr(const ElementCsr&)            = delete;
  ElementCsr& operator=(const ElementCsr&) = delete;

  /// fields: how many fields one kw_sample_elements_multi call reduces over this matrix (sizes the partial sums)
  void upload(const size_t* ptr, size_t rows, const size_t* cols1, const float* weights, size_t nnz, bool chunks,
              size_t fields = 1);
  void release();

  size_t               rows() const { return mRows; }
  size_t               nnz() const { return mNnz; }
  const uint32_t*      ptr() const { return mPtr; }
  const kw_csr_entry*  entries() const { return mEntries; }
  const uint32_t*      chunkPtr() const { return mChunkPtr; }
  uint32_t             chunks() const { return mChunks; }
  float*               partials() const { return mPartials; }

 private:
  size_t        mRows = 0, mNnz = 0;
  uint32_t      mChunks = 0;
  uint32_t*     mPtr = nullptr;
  kw_csr_entry* mEntries = nullptr;
  uint32_t*     mChunkPtr = nullptr;
  float*        mPartials = nullptr;
};
#endif
