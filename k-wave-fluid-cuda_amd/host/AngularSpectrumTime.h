// AngularSpectrumTime.h — time-domain angular-spectrum projector: a pressure record p0[t][y][x] on a plane carried to
// parallel planes at the distances z_j of a homogeneous, possibly absorbing medium (DESIGN.md "Time-domain
// angular-spectrum projector"; what k-Wave's angularSpectrum computes).  Owns its context through a DeviceGrid.
//
//   setInput: embed the record into the zero-filled volume Lt x Ey x Ex (kw_angular_time_embed), transform it once and keep
//         the result — fast path: kw_fused_angular_time_forward (the (kx, ky, t) half-spectrum); others: kw_fft_r2c_3d
//   project: per plane — fast path: kw_fused_angular_time_plane; others: kw_angular_time_mix and kw_fft_c2r_3d — then
//         kw_angular_time_reduce into p_max[j], p_min[j].  run = setInput + project.
//   series(j): plane j alone, recomputed, with the cropped record as third output.  No Nz x Nt volume is ever held.
//
// Device memory, E = Ex Ey Lt points, R = (Ex/2 + 1) Ey Lt bins: the volume 4 E, the kept spectrum (8 R; a scratch array
// on the fast path) and the pipeline's three scratch arrays (fast path) or one more spectrum 8 R (rocFFT); the record and
// one series 4 Nx Ny Nt each; p_max and p_min 4 Nx Ny per plane each.
#ifndef KW_HOST_ANGULAR_SPECTRUM_TIME_H
#define KW_HOST_ANGULAR_SPECTRUM_TIME_H
#include <string>

#include "AngularTimeParameters.h"
#include "DeviceGrid.h"

class AngularSpectrumTime
{
 public:
  explicit AngularSpectrumTime(const AngularTimeParameters& parameters);
  AngularSpectrumTime(const AngularSpectrumTime&) = delete;
  AngularSpectrumTime& operator=(const AngularSpectrumTime&) = delete;

  /// p0: Nx Ny Nt floats on the host, [Nt][Ny][Nx]
  void setInput(const float* p0);
  /// setInput and every plane
  void run(const float* p0);
  /// the planes alone, from the kept spectrum as it stands (tools/bench_angular_time.py)
  void project();
  /// "p_max" or "p_min" of the last run: n = Nx Ny n_planes
  void get(const std::string& name, float* dst, size_t n);
  /// plane j recomputed: dst [Nt][Ny][Nx], n = Nx Ny Nt
  void series(size_t j, float* dst, size_t n);
  bool    usesFusedPipeline() const { return mGrid.fused(); }
  size_t  runs() const { return mRuns; }
  kw_ctx* context() const { return mGrid.ctx(); }
  const AngularTimeParameters& parameters() const { return mPar; }

 private:
  void plane(size_t j, float* pMax, float* pMin, float* series);

  AngularTimeParameters mPar;
  DeviceGrid   mGrid; // the context, the pipeline and every device array below
  bool         mHaveInput = false;
  size_t       mRuns = 0;
  float*  mVol = nullptr;     // Lt Ey Ex: the embedded record, then each plane's record
  float*  mKept = nullptr;    // the kept spectrum
  float*  mSpec = nullptr;    // rocFFT path: the plane's spectrum
  float*  mRecord = nullptr;  // the record as handed in / one series
  double* mAk = nullptr;      // alpha k log2(e) per temporal bin; NULL: lossless
  float  *mMax = nullptr, *mMin = nullptr; // [n_planes][Ny][Nx]
};
#endif
