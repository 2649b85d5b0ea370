// SecondOrder.h — exact k-space propagator: an initial pressure p0[z][y][x] in a homogeneous medium, lossless or power-law
// absorbing, to the pressure at any time with no time loop (DESIGN.md "Exact k-space propagator"; what k-Wave's
// kspaceSecondOrder computes).  Owns its context through a DeviceGrid.
//
//   setP0: embed p0 into the zero-filled volume Ez x Ey x Ex (kw_angular_time_embed), transform it once and keep the
//         result — fast path: kw_fused_second_order_forward (the (kx, ky, z) half-spectrum); others: kw_fft_r2c_3d
//   field(t): fast path: kw_fused_second_order_time; others: kw_second_order_mix and kw_fft_c2r_3d — then the crop to the
//         domain (kw_plane_recon_crop), which stays on the device
//   run(times): for every time in the given order the three passes, the sample at the sensor points into row i of the
//         record (kw_sample_index on the expanded volume, indices translated once) and, where asked for, the crop and
//         kw_sample_all into the running max, min, sum of squares and the final field — all exact and in a fixed order.
//
// Device memory, E = Ex Ey Ez points, R = (Ex/2 + 1) Ey Ez bins, N the domain: the volume 4 E, the kept spectrum (8 R; a
// scratch array on the fast path) and the pipeline's three scratch arrays (fast path) or one more spectrum 8 R (rocFFT);
// the crop 4 N and 4 N per aggregate; the record 4 n_times n_sensor.
#ifndef KW_HOST_SECOND_ORDER_H
#define KW_HOST_SECOND_ORDER_H
#include <string>

#include "DeviceGrid.h"
#include "SecondOrderParameters.h"

class SecondOrder
{
 public:
  explicit SecondOrder(const SecondOrderParameters& parameters);
  SecondOrder(const SecondOrder&) = delete;
  SecondOrder& operator=(const SecondOrder&) = delete;

  /// p0: Nx Ny Nz floats on the host, [Nz][Ny][Nx]; may be called again
  void setP0(const float* p0);
  /// the pressure at time t on the domain; dst: Nx Ny Nz floats on the host or NULL (the crop stays on the device)
  void field(double t, float* dst);
  /// every time in the given order: the record's row, the aggregates
  void run(const double* times, size_t nTimes);
  /// "p_raw" [n_times][n_sensor], "p_max", "p_min", "p_rms", "p_final" of the last run, "p" (the last field computed)
  void get(const std::string& name, float* dst, size_t n);
  bool    usesFusedPipeline() const { return mGrid.fused(); }
  size_t  runs() const { return mRuns; }
  kw_ctx* context() const { return mGrid.ctx(); }
  const SecondOrderParameters& parameters() const { return mPar; }

 private:
  void propagate(double t); // mVol <- the expanded field at time t
  void crop();              // mP <- the domain corner of mVol

  SecondOrderParameters mPar;
  DeviceGrid mGrid; // the context, the pipeline and every device array below
  bool       mHaveInput = false, mHaveField = false;
  size_t     mRuns = 0, mTimes = 0, mRawCapacity = 0;
  float*     mVol = nullptr;    // Ez Ey Ex: the embedded p0, then each time's field
  float*     mKept = nullptr;   // the kept spectrum
  float*     mSpec = nullptr;   // rocFFT path: the spectrum of one time
  float*     mP = nullptr;      // the domain: p0 as handed in, then the crop
  uint64_t*  mIndex = nullptr;  // the sensor points in the expanded volume
  float*     mRaw = nullptr;    // [n_times][n_sensor]
  float     *mMax = nullptr, *mMin = nullptr, *mRms = nullptr, *mFinal = nullptr; // the domain each, where asked for
};
#endif
