// ElementArrays.h — device form of the CSR weight matrices of a weighted transducer array (kwave_hip.h, "Weighted
// transducer arrays").  New with this build; the reference takes such an array only in expanded form (one series per
// grid point, p_source_many = 1, and -p over every point).
#ifndef KW_HOST_ELEMENT_ARRAYS_H
#define KW_HOST_ELEMENT_ARRAYS_H
#include <cstddef>
#include <cstdint>
#include <vector>

#include "kwave_hip.h"

/// The entries of a delayed sensor regrouped by delay (kwave_hip.h, kw_sample_elements_delayed): inside a row the entries
/// are ordered by ascending delay, stably, so CSR order is kept inside a group; a group is a row's entries of one delay.
struct ElementGroups
{
  std::vector<uint32_t> order;           ///< regrouped position -> entry of the CSR (nnz values)
  std::vector<uint32_t> groupPtr;        ///< groups + 1 offsets into the regrouped entries
  std::vector<uint32_t> groupDelay;      ///< one delay per group
  std::vector<uint32_t> elementGroupPtr; ///< rows + 1 offsets into the groups
  std::vector<uint32_t> chunkPtr;        ///< groups + 1 prefix sums of ceil(group length / KW_ELEMENT_CHUNK)
  size_t groups() const { return groupDelay.size(); }
};

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
  /// a weighted source with per-entry delays (one per entry): upload() plus the delays as a uint32 array beside the entries
  void uploadWithDelays(const size_t* ptr, size_t rows, const size_t* cols1, const float* weights, const size_t* delays,
                        size_t nnz);
  /// a weighted sensor with per-entry delays: the regrouped entries, the groups as the rows of the reduction (ptr(),
  /// chunkPtr(), partials() are over groups), the groups' delays, the elements' group offsets and one zeroed ring of
  /// ringRows() x rows floats per field, ringRows() = the largest delay + 1
  void uploadDelayed(const size_t* ptr, size_t rows, const size_t* cols1, const float* weights, const size_t* delays,
                     size_t nnz, size_t fields);
  /// pure host function: no device, no Parameters
  static ElementGroups regroup(const size_t* ptr, size_t rows, const size_t* delays);
  void release();

  size_t               rows() const { return mRows; }
  size_t               nnz() const { return mNnz; }
  const kw_csr_entry*  entries() const { return mEntries; }   // uploadDelayed: the regrouped entries
  float*               partials() const { return mPartials; }
  // upload / uploadWithDelays: the rows of the matrix.  NULL / 0 after uploadDelayed, whose reduction runs over groups
  const uint32_t*      ptr() const { return mGrouped ? nullptr : mPtr; }
  const uint32_t*      chunkPtr() const { return mGrouped ? nullptr : mChunkPtr; }
  uint32_t             chunks() const { return mGrouped ? 0 : mChunks; }
  const uint32_t*      entryDelays() const { return mGrouped ? nullptr : mDelays; } // uploadWithDelays: one delay per entry
  // uploadDelayed alone (NULL / 0 otherwise): the groups as the rows of the reduction, their delays, the elements' groups
  const uint32_t*      groupPtr() const { return mGrouped ? mPtr : nullptr; }
  const uint32_t*      groupChunkPtr() const { return mGrouped ? mChunkPtr : nullptr; }
  uint32_t             groupChunks() const { return mGrouped ? mChunks : 0; }
  const uint32_t*      groupDelays() const { return mGrouped ? mDelays : nullptr; }
  const uint32_t*      elementGroupPtr() const { return mElementGroupPtr; }
  uint32_t             groups() const { return mGroups; }
  uint32_t             ringRows() const { return mRingRows; }
  float*               ring(size_t field) const { return mRing + field * mRingRows * mRows; }

 private:
  size_t        mRows = 0, mNnz = 0;
  uint32_t      mChunks = 0;
  uint32_t*     mPtr = nullptr;
  kw_csr_entry* mEntries = nullptr;
  uint32_t*     mChunkPtr = nullptr;
  float*        mPartials = nullptr;
  uint32_t*     mDelays = nullptr;
  uint32_t*     mElementGroupPtr = nullptr;
  float*        mRing = nullptr;
  uint32_t      mGroups = 0, mRingRows = 0;
  bool          mGrouped = false; // uploadDelayed: mPtr / mChunkPtr / mDelays are over groups
};
#endif
