// ThermalSolver.cpp — the host loop of the bioheat solver around the device library's FFT stages and kw_thermal_update.
#include "ThermalSolver.h"

#include <stdexcept>

#include "HipError.h"

ThermalSolver::ThermalSolver(const ThermalParameters& parameters) : mPar(parameters)
{
  kwCheck(kw_init(mPar.options.deviceIdx, &mCtx));
  try
  {
    const size_t n = mPar.nElements(), nr = mPar.nReduced();
    kw_constants k{};
    k.nx = static_cast<uint32_t>(mPar.nx);
    k.ny = static_cast<uint32_t>(mPar.ny);
    k.nz = static_cast<uint32_t>(mPar.nz);
    k.n_elements = static_cast<uint32_t>(n);
    k.nx_complex = static_cast<uint32_t>(mPar.nx / 2 + 1);
    k.ny_complex = k.ny;
    k.nz_complex = k.nz;
    k.n_elements_complex = static_cast<uint32_t>(nr);
    k.fft_divider   = 1.0f / static_cast<float>(n);
    k.fft_divider_x = 1.0f / static_cast<float>(mPar.nx);
    k.fft_divider_y = 1.0f / static_cast<float>(mPar.ny);
    k.fft_divider_z = 1.0f / static_cast<float>(mPar.nz);
    k.dt      = mPar.dt;
    k.dt_by_2 = mPar.dt * 2.0f;
    kwCheck(kw_set_constants(mCtx, &k));

    int fusedOk = 0;
    if (mPar.options.fusedKernels) kwCheck(kw_fused_supported(mCtx, &fusedOk));
    mFused = fusedOk != 0;
    if (mFused) kwCheck(kw_fused_create(mCtx));
    else kwCheck(kw_fft_create_plans_3d(mCtx));

    // state
    mT     = upload(mPar.T0);
    mCem43 = deviceArray(n);
    kwCheck(kw_memset(mCtx, mCem43, 0, n * sizeof(float)));
    if (mPar.hasQ) mQ = upload(mPar.Q);
    if (mPar.a.isArray) mA = upload(mPar.a.data);
    if (mPar.P.isArray) mP = upload(mPar.P.data);
    if (mPar.Ta.isArray) mTa = upload(mPar.Ta.data);

    // operators, generated in double and rounded once; the fused path reads them in its own padded layout
    std::vector<float> kappaD(nr), laplacian(nr);
    ThermalOperators::generate(mPar.nx, mPar.ny, mPar.nz, mPar.dx, mPar.dy, mPar.dz, mPar.dt, mPar.dRef, kappaD.data(),
                               laplacian.data());
    auto reducedOperator = [&](const std::vector<float>& host) {
      float* d = upload(host);
      return mFused ? importPadded(d) : d;
    };
    const int nArrays = mPar.fluxForm ? 3 : 1;
    for (int i = 0; i < nArrays; i++) mD[i] = deviceArray(n);
    if (!mFused)
      for (int i = 0; i < nArrays; i++) mSpectrum[i] = deviceArray(2 * nr);
    if (!mPar.fluxForm) mLaplacianOp = reducedOperator(laplacian);
    else
    {
      mKappaD = reducedOperator(kappaD);
      mOnes   = reducedOperator(std::vector<float>(nr, 1.0f)); // kappa_d is applied once, in the gradient stage
      const size_t dims[3]   = { mPar.nx, mPar.ny, mPar.nz };
      const float  delta[3]  = { mPar.dx, mPar.dy, mPar.dz };
      for (int i = 0; i < 3; i++)
      {
        mFlux[i]   = deviceArray(n);
        mTwoKsg[i] = upload(mPar.twoKsg[i]);
        const size_t count = (i == 0) ? dims[0] / 2 + 1 : dims[i]; // x: the half spectrum's bins
        std::vector<float> v(2 * count);
        ThermalOperators::derivative(dims[i], count, delta[i], true, v.data());
        mDdPos[i] = upload(v);
        ThermalOperators::derivative(dims[i], count, delta[i], false, v.data());
        mDdNeg[i] = upload(v);
      }
    }
    if (!mPar.sensorIndex.empty())
    {
      void* d = nullptr;
      kwCheck(kw_malloc(mCtx, mPar.sensorIndex.size() * sizeof(uint64_t), &d));
      mOwned.push_back(d);
      mSensorIndex = static_cast<uint64_t*>(d);
      kwCheck(kw_memcpy_h2d(mCtx, d, mPar.sensorIndex.data(), mPar.sensorIndex.size() * sizeof(uint64_t)));
      mSensorBuffer = deviceArray(mPar.sensorIndex.size());
    }
    kwCheck(kw_sync(mCtx));
  }
  catch (...)
  {
    for (void* p : mOwned) kw_free(mCtx, p);
    if (mFused) kw_fused_destroy(mCtx);
    kw_destroy(mCtx);
    throw;
  }
}

ThermalSolver::~ThermalSolver()
{
  if (mCtx == nullptr) return;
  kw_sync(mCtx);
  for (void* p : mOwned) kw_free(mCtx, p);
  if (mFused) kw_fused_destroy(mCtx); // the pipeline's scratch and twiddles
  kw_destroy(mCtx);                   // the FFT plans go with the context
}

float* ThermalSolver::deviceArray(size_t nFloats)
{
  void* d = nullptr;
  kwCheck(kw_malloc(mCtx, nFloats * sizeof(float), &d));
  mOwned.push_back(d);
  return static_cast<float*>(d);
}

float* ThermalSolver::upload(const std::vector<float>& host)
{
  float* d = deviceArray(host.size());
  kwCheck(kw_memcpy_h2d(mCtx, d, host.data(), host.size() * sizeof(float)));
  return d;
}

float* ThermalSolver::importPadded(const float* reducedDevice)
{
  size_t n = 0;
  kwCheck(kw_fused_reduced_elems(mCtx, &n));
  float* d = deviceArray(n);
  kwCheck(kw_fused_import_reduced(mCtx, d, reducedDevice));
  return d;
}

void ThermalSolver::diffusionTerm()
{
  const size_t n = mPar.nElements();
  if (!mPar.fluxForm)
  { // L = F^-1{ -|k|^2 kappa_d F{T} } / N
    if (mFused)
    {
      kwCheck(kw_memcpy_d2d(mCtx, mD[0], mT, n * sizeof(float))); // the stage works in place
      kwCheck(kw_fused_scale_source(mCtx, mD[0], mLaplacianOp));
      return;
    }
    kwCheck(kw_fft_r2c_3d(mCtx, mT, mSpectrum[0]));
    kwCheck(kw_compute_source_gradient(mCtx, mSpectrum[0], mLaplacianOp)); // carries the 1/N
    kwCheck(kw_fft_c2r_3d(mCtx, mSpectrum[0], mD[0]));
    return;
  }
  if (mFused)
  { // the epilogue of the gradient stage multiplies by 0.5 * (1/N) * (2 K_sg); the divergence stage carries its own 1/N
    kwCheck(kw_fused_initial_velocity(mCtx, mT, mFlux[0], mFlux[1], mFlux[2], mTwoKsg[0], mTwoKsg[1], mTwoKsg[2], mKappaD,
                                      mDdPos[0], mDdPos[1], mDdPos[2]));
    kwCheck(kw_fused_velocity_gradient(mCtx, mFlux[0], mFlux[1], mFlux[2], mD[0], mD[1], mD[2], mOnes, mDdNeg[0], mDdNeg[1],
                                       mDdNeg[2], 0));
    return;
  }
  kwCheck(kw_fft_r2c_3d(mCtx, mT, mSpectrum[0]));
  kwCheck(kw_compute_pressure_gradient(mCtx, mSpectrum[0], mSpectrum[1], mSpectrum[2], mKappaD, mDdPos[0], mDdPos[1], mDdPos[2]));
  for (int i = 0; i < 3; i++) kwCheck(kw_fft_c2r_3d(mCtx, mSpectrum[i], mFlux[i]));
  // flux = gradient * (2 K_sg * 0.5 * (1/N))
  kwCheck(kw_compute_initial_velocity(mCtx, mFlux[0], mFlux[1], mFlux[2], mTwoKsg[0], mTwoKsg[1], mTwoKsg[2]));
  for (int i = 0; i < 3; i++) kwCheck(kw_fft_r2c_3d(mCtx, mFlux[i], mSpectrum[i]));
  kwCheck(kw_compute_velocity_gradient(mCtx, mSpectrum[0], mSpectrum[1], mSpectrum[2], mOnes, mDdNeg[0], mDdNeg[1], mDdNeg[2])); // 1/N
  for (int i = 0; i < 3; i++) kwCheck(kw_fft_c2r_3d(mCtx, mSpectrum[i], mD[i]));
}

void ThermalSolver::run(size_t nSteps, bool heatOn)
{
  const size_t n  = mPar.nElements();
  const size_t ns = mPar.sensorIndex.size();
  for (size_t step = 0; step < nSteps; step++)
  {
    diffusionTerm();
    kwCheck(kw_thermal_update(mCtx, mT, mCem43, mTMax, mD[0], mD[1], mD[2], mPar.fluxForm ? 1.0f : mPar.conductivity, mA,
                              mPar.a.scalar, mP, mPar.P.scalar, mTa, mPar.Ta.scalar, mQ, mPar.dt, heatOn ? 1 : 0, n));
    if (ns != 0)
    {
      kwCheck(kw_sample_index(mCtx, KW_OP_NONE, mSensorBuffer, mT, mSensorIndex, ns));
      mTRaw.resize(mTRaw.size() + ns);
      kwCheck(kw_memcpy_d2h(mCtx, mTRaw.data() + mTRaw.size() - ns, mSensorBuffer, ns * sizeof(float)));
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
    if (mTMax == nullptr && forWriting) mTMax = deviceArray(mPar.nElements()); // switched on by the first write
    if (mTMax == nullptr) throw std::invalid_argument("T_max: the running maximum is off (set T_max once to switch it on)");
    return mTMax;
  }
  if (name == "Q")
  {
    if (mQ == nullptr && forWriting) mQ = deviceArray(mPar.nElements());
    if (mQ == nullptr) throw std::invalid_argument("Q: this simulation has no heat source");
    return mQ;
  }
  throw std::invalid_argument("no thermal matrix named " + name + " (T, cem43, T_max, Q)");
}

void ThermalSolver::getMatrix(const std::string& name, float* dst, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for matrix " + name);
  kwCheck(kw_memcpy_d2h(mCtx, dst, matrix(name, false), n * sizeof(float)));
}

void ThermalSolver::setMatrix(const std::string& name, const float* src, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for matrix " + name);
  kwCheck(kw_memcpy_h2d(mCtx, matrix(name, true), src, n * sizeof(float)));
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
