// ThermalSolver.h — explicit k-space time stepping of the Pennes bioheat equation on a periodic grid, with the CEM43
// thermal dose accumulated on the GPU (DESIGN.md "Bioheat"; what k-Wave's kWaveDiffusion computes).  A second solver
// beside KSpaceFirstOrderSolver: it owns its own kw_ctx (a DeviceGrid), so acoustic and thermal solvers can share a process.
//
// One step = the diffusion term by FFT stages of the device library, then kw_thermal_update:
//   Laplacian form (scalar K):  L = F^-1{ -|k|^2 kappa_d F{T} }                   kw_fused_scale_source | rocFFT twins
//   flux form (array K):        F_i = K_sg_i F^-1{ kappa_d i k_i e^{+i k_i d_i/2} F{T} }   kw_fused_initial_velocity | ...
//                               d_i = F^-1{ i k_i e^{-i k_i d_i/2} F{F_i} }                kw_fused_velocity_gradient | ...
#ifndef KW_HOST_THERMAL_SOLVER_H
#define KW_HOST_THERMAL_SOLVER_H
#include <string>
#include <vector>

#include "DeviceGrid.h"
#include "ThermalParameters.h"

class ThermalSolver
{
 public:
  explicit ThermalSolver(const ThermalParameters& parameters);
  ThermalSolver(const ThermalSolver&) = delete;
  ThermalSolver& operator=(const ThermalSolver&) = delete;

  /// n steps; heatOn = false leaves Q out (cooling)
  void   run(size_t nSteps, bool heatOn);
  size_t timeIndex() const { return mTimeIndex; }
  bool   usesFusedPipeline() const { return mGrid.fused(); }
  kw_ctx* context() const { return mGrid.ctx(); }
  /// "T", "cem43", "T_max", "Q": n floats of the grid
  void   getMatrix(const std::string& name, float* dst, size_t n);
  void   setMatrix(const std::string& name, const float* src, size_t n);
  /// volume [m^3] of the points with cem43 >= thresholdMinutes, counted on the host
  double lesionVolume(float thresholdMinutes);
  /// "T_raw": T at the sensor points after each step, steps x points
  const std::vector<float>& series(const std::string& name) const;
  size_t sensorSize() const { return mPar.sensorIndex.size(); }

 private:
  float* matrix(const std::string& name, bool forWriting);
  void   diffusionTerm();

  ThermalParameters mPar;
  DeviceGrid        mGrid; // the context, the pipeline and every device array below
  size_t            mTimeIndex = 0;
  float *mT = nullptr, *mCem43 = nullptr, *mTMax = nullptr, *mQ = nullptr;
  float *mA = nullptr, *mP = nullptr, *mTa = nullptr;
  float* mD[3] = { nullptr, nullptr, nullptr };      // Laplacian (mD[0]) or the three terms of the divergence
  float* mFlux[3] = { nullptr, nullptr, nullptr };   // flux form: K_sg grad T
  float* mTwoKsg[3] = { nullptr, nullptr, nullptr };
  float* mSpectrum[3] = { nullptr, nullptr, nullptr }; // rocFFT path: half spectra
  float *mLaplacianOp = nullptr, *mKappaD = nullptr, *mOnes = nullptr; // reduced operators (fused path: imported)
  float* mDdPos[3] = { nullptr, nullptr, nullptr };
  float* mDdNeg[3] = { nullptr, nullptr, nullptr };
  uint64_t* mSensorIndex = nullptr;
  float*    mSensorBuffer = nullptr;
  std::vector<float> mTRaw;
};
#endif
