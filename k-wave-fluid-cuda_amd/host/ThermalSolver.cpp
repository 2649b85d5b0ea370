// ThermalSolver.cpp — the host loop of the bioheat solver around the device library's FFT stages and kw_thermal_update.
#include "ThermalSolver.h"

#include <stdexcept>

ThermalSolver::ThermalSolver(const ThermalParameters& parameters) : mPar(parameters), mGrid(mPar.options.deviceIdx)
{
  const size_t n = mPar.nElements(), nr = mPar.nReduced();
  kw_constants k = gridConstants(mPar.nx, mPar.ny, mPar.nz);
  k.dt      = mPar.dt;
  k.dt_by_2 = mPar.dt * 2.0f;
  mGrid.setConstants(k);
  const bool fused = mGrid.choosePipeline(mPar.options.fusedKernels);

  // state
  mT     = mGrid.upload(mPar.T0);
  mCem43 = mGrid.array(n);
  mGrid.check(kw_memset(context(), mCem43, 0, n * sizeof(float)));
  if (mPar.hasQ) mQ = mGrid.upload(mPar.Q);
  if (mPar.a.isArray) mA = mGrid.upload(mPar.a.data);
  if (mPar.P.isArray) mP = mGrid.upload(mPar.P.data);
  if (mPar.Ta.isArray) mTa = mGrid.upload(mPar.Ta.data);

  // operators, generated in double and rounded once; the fused path reads them in its own padded layout
  std::vector<float> kappaD(nr), laplacian(nr);
  ThermalOperators::generate(mPar.nx, mPar.ny, mPar.nz, mPar.dx, mPar.dy, mPar.dz, mPar.dt, mPar.dRef, kappaD.data(),
                             laplacian.data());
  auto reducedOperator = [&](const std::vector<float>& host) {
    float* d = mGrid.upload(host);
    return fused ? mGrid.importReduced(d) : d;
  };
  const int nArrays = mPar.fluxForm ? 3 : 1;
  for (int i = 0; i < nArrays; i++) mD[i] = mGrid.array(n);
  if (!fused)
    for (int i = 0; i < nArrays; i++) mSpectrum[i] = mGrid.array(2 * nr);
  if (!mPar.fluxForm) mLaplacianOp = reducedOperator(laplacian);
  else
  {
    mKappaD = reducedOperator(kappaD);
    mOnes   = reducedOperator(std::vector<float>(nr, 1.0f)); // kappa_d is applied once, in the gradient stage
    const size_t dims[3]   = { mPar.nx, mPar.ny, mPar.nz };
    const float  delta[3]  = { mPar.dx, mPar.dy, mPar.dz };
    for (int i = 0; i < 3; i++)
    {
      mFlux[i]   = mGrid.array(n);
      mTwoKsg[i] = mGrid.upload(mPar.twoKsg[i]);
      const size_t count = (i == 0) ? dims[0] / 2 + 1 : dims[i]; // x: the half spectrum's bins
      std::vector<float> v(2 * count);
      ThermalOperators::derivative(dims[i], count, delta[i], true, v.data());
      mDdPos[i] = mGrid.upload(v);
      ThermalOperators::derivative(dims[i], count, delta[i], false, v.data());
      mDdNeg[i] = mGrid.upload(v);
    }
  }
  if (!mPar.sensorIndex.empty())
  {
    mSensorIndex = static_cast<uint64_t*>(mGrid.bytes(mPar.sensorIndex.size() * sizeof(uint64_t)));
    mGrid.check(kw_memcpy_h2d(context(), mSensorIndex, mPar.sensorIndex.data(), mPar.sensorIndex.size() * sizeof(uint64_t)));
    mSensorBuffer = mGrid.array(mPar.sensorIndex.size());
  }
  mGrid.check(kw_sync(context()));
}

void ThermalSolver::diffusionTerm()
{
  const size_t n = mPar.nElements();
  if (!mPar.fluxForm)
  { // L = F^-1{ -|k|^2 kappa_d F{T} } / N
    if (mGrid.fused())
    {
      mGrid.check(kw_memcpy_d2d(context(), mD[0], mT, n * sizeof(float))); // the stage works in place
      mGrid.check(kw_fused_scale_source(context(), mD[0], mLaplacianOp));
      return;
    }
    mGrid.check(kw_fft_r2c_3d(context(), mT, mSpectrum[0]));
    mGrid.check(kw_compute_source_gradient(context(), mSpectrum[0], mLaplacianOp)); // carries the 1/N
    mGrid.check(kw_fft_c2r_3d(context(), mSpectrum[0], mD[0]));
    return;
  }
  if (mGrid.fused())
  { // the epilogue of the gradient stage multiplies by 0.5 * (1/N) * (2 K_sg); the divergence stage carries its own 1/N
    mGrid.check(kw_fused_initial_velocity(context(), mT, mFlux[0], mFlux[1], mFlux[2], mTwoKsg[0], mTwoKsg[1], mTwoKsg[2], mKappaD,
                                          mDdPos[0], mDdPos[1], mDdPos[2]));
    mGrid.check(kw_fused_velocity_gradient(context(), mFlux[0], mFlux[1], mFlux[2], mD[0], mD[1], mD[2], mOnes, mDdNeg[0], mDdNeg[1],
                                           mDdNeg[2], 0));
    return;
  }
  mGrid.check(kw_fft_r2c_3d(context(), mT, mSpectrum[0]));
  mGrid.check(kw_compute_pressure_gradient(context(), mSpectrum[0], mSpectrum[1], mSpectrum[2], mKappaD, mDdPos[0], mDdPos[1], mDdPos[2]));
  for (int i = 0; i < 3; i++) mGrid.check(kw_fft_c2r_3d(context(), mSpectrum[i], mFlux[i]));
  // flux = gradient * (2 K_sg * 0.5 * (1/N))
  mGrid.check(kw_compute_initial_velocity(context(), mFlux[0], mFlux[1], mFlux[2], mTwoKsg[0], mTwoKsg[1], mTwoKsg[2]));
  for (int i = 0; i < 3; i++) mGrid.check(kw_fft_r2c_3d(context(), mFlux[i], mSpectrum[i]));
  mGrid.check(kw_compute_velocity_gradient(context(), mSpectrum[0], mSpectrum[1], mSpectrum[2], mOnes, mDdNeg[0], mDdNeg[1], mDdNeg[2])); // 1/N
  for (int i = 0; i < 3; i++) mGrid.check(kw_fft_c2r_3d(context(), mSpectrum[i], mD[i]));
}

void ThermalSolver::run(size_t nSteps, bool heatOn)
{
  const size_t n  = mPar.nElements();
  const size_t ns = mPar.sensorIndex.size();
  for (size_t step = 0; step < nSteps; step++)
  {
    diffusionTerm();
    mGrid.check(kw_thermal_update(context(), mT, mCem43, mTMax, mD[0], mD[1], mD[2], mPar.fluxForm ? 1.0f : mPar.conductivity, mA,
                                  mPar.a.scalar, mP, mPar.P.scalar, mTa, mPar.Ta.scalar, mQ, mPar.dt, heatOn ? 1 : 0, n));
    if (ns != 0)
    {
      mGrid.check(kw_sample_index(context(), KW_OP_NONE, mSensorBuffer, mT, mSensorIndex, ns));
      mTRaw.resize(mTRaw.size() + ns);
      mGrid.check(kw_memcpy_d2h(context(), mTRaw.data() + mTRaw.size() - ns, mSensorBuffer, ns * sizeof(float)));
    }
    mTimeIndex++;
  }
}

float* ThermalSolver::matrix(const std::string& name, bool forWriting)
{
  if (name == "T") return mT;
  if (name == "cem43") return mCem43;
  if (name == "T_max")
  {
    if (mTMax == nullptr && forWriting) mTMax = mGrid.array(mPar.nElements()); // switched on by the first write
    if (mTMax == nullptr) throw std::invalid_argument("T_max: the running maximum is off (set T_max once to switch it on)");
    return mTMax;
  }
  if (name == "Q")
  {
    if (mQ == nullptr && forWriting) mQ = mGrid.array(mPar.nElements());
    if (mQ == nullptr) throw std::invalid_argument("Q: this simulation has no heat source");
    return mQ;
  }
  throw std::invalid_argument("no thermal matrix named " + name + " (T, cem43, T_max, Q)");
}

void ThermalSolver::getMatrix(const std::string& name, float* dst, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for matrix " + name);
  mGrid.check(kw_memcpy_d2h(context(), dst, matrix(name, false), n * sizeof(float)));
}

void ThermalSolver::setMatrix(const std::string& name, const float* src, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for matrix " + name);
  mGrid.check(kw_memcpy_h2d(context(), matrix(name, true), src, n * sizeof(float)));
}

double ThermalSolver::lesionVolume(float thresholdMinutes)
{
  std::vector<float> dose(mPar.nElements());
  getMatrix("cem43", dose.data(), dose.size());
  size_t count = 0;
  for (float v : dose) count += (v >= thresholdMinutes) ? 1 : 0;
  return static_cast<double>(count) * static_cast<double>(mPar.dx) * static_cast<double>(mPar.dy) * static_cast<double>(mPar.dz);
}

const std::vector<float>& ThermalSolver::series(const std::string& name) const
{
  if (name != "T_raw") throw std::invalid_argument("no thermal stream named " + name + " (T_raw)");
  if (mPar.sensorIndex.empty()) throw std::invalid_argument("T_raw: the input has no sensor_mask_index");
  return mTRaw;
}
