// CwPropagator.h — steady-state pressure of a continuous-wave source in a homogeneous lossless medium in one FFT round
// trip (DESIGN.md "CW field propagator"; what k-Wave's acousticFieldPropagator computes).  Owns its context through
// a DeviceGrid and builds the operator G exp(-i w T) / N once; every run reuses it.
//
//   run:  embed the source into the zero-filled expanded pair (kw_cw_embed)
//         fast-path grids: kw_fused_cw_pair;   others: kw_fft_r2c_3d x 2, kw_cw_mix, kw_fft_c2r_3d x 2
//         the outputs crop the domain back out of the pair (kw_cw_extract)
//
// Device memory, E = Ex Ey Ez points, R = (Ex/2 + 1) Ey Ez bins, Rp = R with the rows padded to 16 bins:
//   fast path:  8 E (the pair) + 8 Rp (the two operators) + 24 Rp (the pipeline's three spectra; a fourth on square planes
//               of 32 or 64) — about 24 E bytes; 8 R more while the operators are built
//   rocFFT:     8 E + 8 R (operators) + 16 R (two spectra) + the library's work buffer — about 20 E bytes
// plus four arrays of the DOMAIN's size (two inputs, two staging outputs).
#ifndef KW_HOST_CW_PROPAGATOR_H
#define KW_HOST_CW_PROPAGATOR_H
#include <string>

#include "CwParameters.h"
#include "DeviceGrid.h"

class CwPropagator
{
 public:
  explicit CwPropagator(const CwParameters& parameters);
  CwPropagator(const CwPropagator&) = delete;
  CwPropagator& operator=(const CwPropagator&) = delete;

  /// parts: a = Re S, b = Im S; otherwise a = amplitude, b = phase [rad]; n = Nx Ny Nz floats each, on the host
  void run(const float* a, const float* b, bool parts);
  /// the result of the last run cropped to the domain: "re", "im", "amplitude", "phase"
  void get(const std::string& name, float* dst, size_t n);
  /// Q = q |P|^2: q per point (n floats on the host), or NULL and qScalar
  void heat(const float* q, float qScalar, float* dst, size_t n);
  bool    usesFusedPipeline() const { return mGrid.fused(); }
  size_t  runs() const { return mRuns; }
  kw_ctx* context() const { return mGrid.ctx(); }
  const CwParameters& parameters() const { return mPar; }
  /// the pair stage alone on the expanded pair as it stands (tools/bench_cw.py)
  void propagate();

 private:
  CwParameters mPar;
  DeviceGrid   mGrid; // the context, the pipeline and every device array below
  size_t       mRuns = 0;
  float *mRe = nullptr, *mIm = nullptr;     // the expanded pair
  float *mGRe = nullptr, *mGIm = nullptr;   // operators: imported (fast path) or reduced (rocFFT path)
  float *mSpecRe = nullptr, *mSpecIm = nullptr; // rocFFT path: half spectra
  float *mA = nullptr, *mB = nullptr;       // domain: the source as handed in
  float *mOut = nullptr, *mQ = nullptr;     // domain: staging of one output, per-point q
};
#endif
