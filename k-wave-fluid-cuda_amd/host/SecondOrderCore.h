// SecondOrderCore.h — what the two exact k-space propagators do alike (SecondOrder: 3-D; SecondOrderFrames: a batch of
// planes): the context, the volume, the kept spectrum, the crop, the record and the aggregates, with setP0, setDp0dt, field,
// run and get once.  A form says what differs: the six sizes handed to embed and crop, the rocFFT path's divider, the operator
// without its time, and the device entry points (which have the same signatures in both forms).
#ifndef KW_HOST_SECOND_ORDER_CORE_H
#define KW_HOST_SECOND_ORDER_CORE_H
#include <string>
#include <vector>

#include "DeviceGrid.h"
#include "GridRules.h"

/// the device entry points of one form
struct SecondOrderEntries
{
  bool framesContext; ///< the pipeline in frames mode and the batched 2-D plans; otherwise the 3-D ones
  kw_status (*elems)(kw_ctx*, size_t*);
  kw_status (*forward)(kw_ctx*, const float*, float*);
  kw_status (*time)(kw_ctx*, const float*, const kw_second_order_op*, float*);
  kw_status (*mix)(kw_ctx*, float*, const float*, const kw_second_order_op*, float);
  kw_status (*timePair)(kw_ctx*, const float*, const float*, const kw_second_order_op*, float*);       ///< with dp0/dt
  kw_status (*mixPair)(kw_ctx*, float*, const float*, const float*, const kw_second_order_op*, float);
  kw_status (*r2c)(kw_ctx*, const float*, float*);
  kw_status (*c2r)(kw_ctx*, float*, float*);
};

struct SecondOrderForm
{
  size_t ex, ey, ez, nx, ny, nz;     ///< the expanded grid and the domain; ez = nz = F for a batch of planes
  float  divider;                    ///< rocFFT path: 1 / the points of one transform, as the form computes it
  kw_second_order_op op;             ///< dx, dy, dz, c0, a, alpha_power, absorbing; t is set per call
  const SecondOrderEntries* entries;
  size_t nDomain() const { return nx * ny * nz; }
  size_t nExpanded() const { return ex * ey * ez; }
  size_t nReduced() const { return (ex / 2 + 1) * ey * ez; }
};

class SecondOrderCore
{
 public:
  /// rules: the device, fastPath and the aggregates wanted; index: the sensor points in the expanded grid, one row of the
  /// record (empty: no record)
  SecondOrderCore(const SecondOrderRules& rules, const SecondOrderForm& form, const std::vector<uint64_t>& index);
  SecondOrderCore(const SecondOrderCore&) = delete;
  SecondOrderCore& operator=(const SecondOrderCore&) = delete;

  void setP0(const float* p0);
  /// dp/dt at t = 0 [Pa/s], the domain's shape: embedded, transformed and kept in a second array that exists from the first
  /// call on; nullptr clears the condition (the single passes again).  Independent of setP0: either may be called again in
  /// any order, neither resets the other.
  void setDp0dt(const float* dp0dt);
  bool hasDp0dt() const { return mHaveDp0dt; }
  void field(double t, float* dst);
  void run(const double* times, size_t nTimes);
  void get(const std::string& name, float* dst, size_t n);
  size_t runs() const { return mRuns; }
  kw_second_order_op op(double t) const;
  DeviceGrid&  grid() { return mGrid; }
  const DeviceGrid& grid() const { return mGrid; }
  kw_ctx*      ctx() const { return mGrid.ctx(); }
  const float* vol() const { return mVol; }
  const float* kept() const { return mKept; }

 private:
  void keep(const float* src, float* kept); // kept <- the spectrum of the domain array src on the host, embedded (through mP, mVol)
  void propagate(double t); // mVol <- the expanded field at time t
  void crop();              // mP <- the domain corner of mVol

  const SecondOrderForm mForm;
  const size_t mRow;        // sensor points of one row of the record
  DeviceGrid mGrid;         // the context, the pipeline and every device array below
  bool       mHaveInput = false, mHaveField = false, mHaveDp0dt = false;
  size_t     mKeptFloats = 0;   // floats of a kept spectrum
  size_t     mRuns = 0, mTimes = 0, mRawCapacity = 0;
  float*     mVol = nullptr;    // Ez Ey Ex: the embedded p0, then each time's field
  float*     mKept = nullptr;   // the kept spectrum
  float*     mKeptV = nullptr;  // the kept spectrum of dp0dt, from the first setDp0dt on
  float*     mSpec = nullptr;   // rocFFT path: the spectrum of one time
  float*     mP = nullptr;      // the domain: p0 as handed in, then the crop
  uint64_t*  mIndex = nullptr;  // the sensor points in the expanded grid
  float*     mRaw = nullptr;    // [n_times][mRow]
  float     *mMax = nullptr, *mMin = nullptr, *mRms = nullptr, *mFinal = nullptr; // the domain each, where asked for
};
#endif
