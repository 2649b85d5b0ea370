// DeviceGrid.h — the one owner of a kw_ctx for the operators that bring their own context (ThermalSolver, CwPropagator,
// AngularSpectrum, AngularSpectrumTime, PlaneRecon, LineRecon, and SecondOrderCore for SecondOrder and SecondOrderFrames):
// the context, its FFT pipeline and every device allocation, released by the destructor.  Held as a member: when the
// enclosing constructor throws, what was built so far goes the same way.
#ifndef KW_HOST_DEVICE_GRID_H
#define KW_HOST_DEVICE_GRID_H
#include <cstddef>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "kwave_hip.h"

/// a failing device call with its kw_status (the kwh_*_create entry points hand KW_ERR_NO_DEVICE through)
struct DeviceError : std::runtime_error
{
  kw_status status;
  DeviceError(kw_status s, const std::string& what) : std::runtime_error(what), status(s) {}
};

/// the constants of a real-to-complex grid nx x ny x nz; everything else zero.  Callers amend it before setConstants.
kw_constants gridConstants(size_t nx, size_t ny, size_t nz);

class DeviceGrid
{
 public:
  explicit DeviceGrid(int deviceIdx);
  /// sync, every owned pointer, the fused pipeline (also after a failed create: destroy frees what it left), the context
  ~DeviceGrid();
  DeviceGrid(const DeviceGrid&) = delete;
  DeviceGrid& operator=(const DeviceGrid&) = delete;

  /// KW_ERR_ALLOC -> std::bad_alloc, any other failure -> DeviceError with kw_last_error()
  void check(kw_status s) const;
  void setConstants(const kw_constants& k) { check(kw_set_constants(mCtx, &k)); }
  /// the fused pipeline when wanted and supported for the constants set, the 3-D rocFFT plans otherwise — those for
  /// `unfusedConstants` where given (a pipeline and plans of different shapes); returns fused()
  bool choosePipeline(bool wantFused, const kw_constants* unfusedConstants = nullptr);

  /// the same choice for a pipeline with a mode of its own (LineRecon's frames context): setMode(true) comes before the
  /// support query, and where the pipeline is not taken setMode(false) and makePlans() replace the 3-D plans; both call
  /// the device library themselves and report through check; returns fused()
  bool choosePipeline(bool wantFused, const std::function<void(bool)>& setMode, const std::function<void()>& makePlans);

  void*  bytes(size_t nBytes);
  float* array(size_t nFloats) { return static_cast<float*>(bytes(nFloats * sizeof(float))); }
  float* upload(const std::vector<float>& host);
  /// frees one owned pointer now
  void   release(void* p);
  /// a reduced operator on the device copied into the fused pipeline's padded layout (a new owned array)
  float* importReduced(const float* reducedDevice);

  kw_ctx* ctx() const { return mCtx; }
  bool    fused() const { return mFused; }

 private:
  kw_ctx* mCtx = nullptr;
  bool    mFused = false; // kw_fused_create has been called
  std::vector<void*> mOwned;
};
#endif
