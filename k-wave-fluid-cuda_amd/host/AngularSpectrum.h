// AngularSpectrum.h — angular-spectrum CW projector: a complex pressure plane carried to the planes z_j = z0 + j dz of a
// homogeneous, possibly absorbing medium (DESIGN.md "Angular-spectrum projector"; what k-Wave's angularSpectrumCW
// computes).  Owns its context through a DeviceGrid and builds the operator tables once; every run reuses them.
//
//   run:  embed the plane into the zero-filled expanded pair (kw_cw_embed, one plane), transform it once
//         (kw_fused_angular_forward, or kw_fft_r2c_3d on the 2-D plans), then project()
//   project: per chunk of Zc planes — fast path: kw_fused_angular_planes;  others: kw_angular_mix and one 2-D C2R
//         transform per plane and part — and the crop of the chunk into the domain-sized result (kw_cw_extract)
//   outputs: kw_cw_extract on the domain-sized pair (|P|, the float64 atan2 phase and Q stay one implementation)
//
// Device memory, E = Ex Ey points of a plane, R = (Ex/2 + 1) Ey bins: the chunk 8 E Zc bytes (the pair) + the pipeline's
// three spectra 24 R Zc (fast path) or two spectra 16 R Zc (rocFFT); tables 20 R (twice on the fast path); the source's
// spectra 16 R; and the result, 8 bytes per domain point, plus one staging array of that size.
#ifndef KW_HOST_ANGULAR_SPECTRUM_H
#define KW_HOST_ANGULAR_SPECTRUM_H
#include <string>

#include "AngularParameters.h"
#include "DeviceGrid.h"

class AngularSpectrum
{
 public:
  explicit AngularSpectrum(const AngularParameters& parameters);
  AngularSpectrum(const AngularSpectrum&) = delete;
  AngularSpectrum& operator=(const AngularSpectrum&) = delete;

  /// parts: a = Re P0, b = Im P0; otherwise a = amplitude, b = phase [rad]; Nx Ny floats each, on the host
  void run(const float* a, const float* b, bool parts);
  /// the result of the last run: "re", "im", "amplitude", "phase"; n = Nx Ny Nz
  void get(const std::string& name, float* dst, size_t n);
  /// Q = q |P|^2: q per point (n floats on the host), or NULL and qScalar
  void heat(const float* q, float qScalar, float* dst, size_t n);
  /// the chunks alone, from the source spectra as they stand (tools/bench_angular.py)
  void project();
  bool    usesFusedPipeline() const { return mGrid.fused(); }
  size_t  runs() const { return mRuns; }
  kw_ctx* context() const { return mGrid.ctx(); }
  const AngularParameters& parameters() const { return mPar; }

 private:
  AngularParameters mPar;
  DeviceGrid   mGrid; // the context, the pipeline and every device array below
  size_t       mRuns = 0;
  float *mRe = nullptr, *mIm = nullptr;         // the chunk: Ex Ey Zc each
  uint32_t *mTab = nullptr, *mTabImported = nullptr;
  float *mSrcRe = nullptr, *mSrcIm = nullptr;   // the source's 2-D spectra (pipeline layout, or [Ey][Ex/2 + 1])
  float *mSpecRe = nullptr, *mSpecIm = nullptr; // rocFFT path: the chunk's half spectra
  float *mA = nullptr, *mB = nullptr;           // the plane as handed in
  float *mOutRe = nullptr, *mOutIm = nullptr;   // the result on the domain
  float *mOut = nullptr, *mQ = nullptr;         // domain: staging of one output, per-point q
};
#endif
