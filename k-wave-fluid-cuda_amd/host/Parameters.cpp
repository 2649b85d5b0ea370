// Parameters.cpp — see Parameters.h.  Follows Parameters/Parameters.cpp:194-459 (what is read, in which order,
// how scalar-vs-matrix medium is detected) and Parameters/CudaParameters.cpp:81-177,238-288.
#include "Parameters.h"
#include <algorithm>
#include <vector>

#include <ios>
#include <stdexcept>

#include "CompressHelper.h"
#include "HipError.h"
#include "MatrixNames.h"

namespace
{
thread_local Parameters* tBound = nullptr; // the set of the solver handle whose entry point this thread is inside
}

Parameters::Parameters() : mCompressHelper(new CompressHelper()) {}

Parameters::~Parameters()
{
  if (mDetached) mHipParameters.release();
}

Parameters& Parameters::getInstance()
{
  if (tBound != nullptr) return *tBound;
  static Parameters instance;
  return instance;
}

std::unique_ptr<Parameters> Parameters::createDetached()
{
  std::unique_ptr<Parameters> p(new Parameters());
  p->mDetached = true;
  return p;
}

Parameters::Scope::Scope(Parameters* p) : mPrevious(tBound)
{
  if (p != nullptr) tBound = p;
}

Parameters::Scope::~Scope() { tBound = mPrevious; }

void Parameters::init(const InputProvider& in, const Options& options)
{
  mOptions   = options;
  mTimeIndex = 0;
  const DimensionSizes scalarSizes(1, 1, 1);

  size_t x, y, z;
  in.readScalarValue(kNxName, x);
  in.readScalarValue(kNyName, y);
  in.readScalarValue(kNzName, z);
  mFullDimensionSizes    = DimensionSizes(x, y, z);
  mReducedDimensionSizes = DimensionSizes((x / 2) + 1, y, z);
  mGlobalDimensionSizes  = mFullDimensionSizes;
  if (isSlabDecomposed())
  {
    if (mOptions.nzGlobal != z * mOptions.slabRanks || mOptions.slabRank >= mOptions.slabRanks || y % mOptions.slabRanks != 0)
      throw std::invalid_argument("Z-slab decomposition: Nz_global must equal slabRanks * local Nz and Ny must divide by slabRanks");
    mGlobalDimensionSizes.nz = mOptions.nzGlobal;
  }
  if (!isSimulation3D())
  { // 2-D (Nz == 1): what this build carries over from the 3-D path; the rest says so instead of computing nonsense
    if (z != 1 || isSlabDecomposed())
      throw std::invalid_argument("2-D simulations need Nz == 1 and a single GPU");
  }

  in.readScalarValue(kNtName, mNt);
  if (mOptions.benchmarkTimeStepCount > 0) mNt = mOptions.benchmarkTimeStepCount; // Parameters.cpp:130-133
  // Parameters.cpp:135-139: sampling must start inside the run ("-s 0" arrives here as 0 - 1, i.e. wrapped around)
  if (mOptions.samplingStartTimeIndex > mNt)
    throw std::invalid_argument("Error: The beginning of data sampling is out of the simulation time span <1, " +
                                std::to_string(mNt) + ">.");
  in.readScalarValue(kDtName, mDt);
  in.readScalarValue(kDxName, mDx);
  in.readScalarValue(kDyName, mDy);
  mDz = 0.0f;
  if (isSimulation3D()) in.readScalarValue(kDzName, mDz); // a 2-D input file has no dz (Parameters.cpp:240-243)
  in.readScalarValue(kCRefName, mCRef);
  const char* const pmlSizeNames[3]  = {"pml_x_size", "pml_y_size", "pml_z_size"};
  const char* const pmlAlphaNames[3] = {"pml_x_alpha", "pml_y_alpha", "pml_z_alpha"};
  for (int a = 0; a < 3; a++)
  {
    if (in.datasetExists(pmlSizeNames[a])) in.readScalarValue(pmlSizeNames[a], mPmlSize[a]);
    if (in.datasetExists(pmlAlphaNames[a])) in.readScalarValue(pmlAlphaNames[a], mPmlAlpha[a]);
  }

  // sensor mask (file version 1.1: Parameters.cpp:262-312)
  mSensorMaskIndexSize = mSensorMaskCornersSize = 0;
  size_t maskType = 0;
  if (in.datasetExists(kSensorMaskTypeName)) in.readScalarValue(kSensorMaskTypeName, maskType);
  mSensorMaskType = (maskType == 1) ? SensorMaskType::kCorners : SensorMaskType::kIndex;
  if (mSensorMaskType == SensorMaskType::kIndex)
  {
    if (in.datasetExists(kSensorMaskIndexName)) mSensorMaskIndexSize = in.getDatasetSize(kSensorMaskIndexName);
  }
  else
  {
    mSensorMaskCornersSize = in.getDatasetDimensionSizes(kSensorMaskCornersName).ny;
  }

  in.readScalarValue(kPressureSourceFlagName, mPressureSourceFlag);
  in.readScalarValue(kInitialPressureSourceFlagName, mInitialPressureSourceFlag);
  // 2-D input files carry neither a transducer nor a z-velocity source (Parameters.cpp:300-320)
  mTransducerSourceFlag = 0;
  mVelocityZSourceFlag  = 0;
  if (isSimulation3D() || in.datasetExists(kTransducerSourceFlagName)) in.readScalarValue(kTransducerSourceFlagName, mTransducerSourceFlag);
  in.readScalarValue(kVelocityXSourceFlagName, mVelocityXSourceFlag);
  in.readScalarValue(kVelocityYSourceFlagName, mVelocityYSourceFlag);
  if (isSimulation3D() || in.datasetExists(kVelocityZSourceFlagName)) in.readScalarValue(kVelocityZSourceFlagName, mVelocityZSourceFlag);
  if (!isSimulation3D() && (mTransducerSourceFlag != 0 || mVelocityZSourceFlag != 0))
    throw std::invalid_argument("2-D simulations have no transducer or z-velocity source");
  in.readScalarValue(kNonUniformGridFlagName, mNonUniformGridFlag);
  in.readScalarValue(kAbsorbingFlagName, mAbsorbingFlag);
  if (mAbsorbingFlag > 4)
    throw std::invalid_argument(std::string("Error: Illegal value of ") + kAbsorbingFlagName + " (" + std::to_string(mAbsorbingFlag) +
                                "): 0 lossless, 1 power law, 2 Stokes, 3 no_dispersion, 4 no_absorption");
  in.readScalarValue(kNonLinearFlagName, mNonLinearFlag);
  if (mNonUniformGridFlag != 0 && !isSimulation3D())
    throw std::invalid_argument("Non-uniform grids are implemented for 3-D simulations only");

  mTransducerSourceInputSize = (mTransducerSourceFlag == 0) ? 0 : in.getDatasetSize(kTransducerSourceInputName);
  mVelocitySourceIndexSize   = 0;
  if ((mTransducerSourceFlag > 0) || (mVelocityXSourceFlag > 0) || (mVelocityYSourceFlag > 0) ||
      (mVelocityZSourceFlag > 0))
    mVelocitySourceIndexSize = in.getDatasetSize(kVelocitySourceIndexName);

  auto toMode = [](size_t v, const char* what) {
    if (v > 2) throw std::ios_base::failure(std::string("Error: bad ") + what + " source mode in the input");
    return static_cast<SourceMode>(v);
  };
  if ((mVelocityXSourceFlag > 0) || (mVelocityYSourceFlag > 0) || (mVelocityZSourceFlag > 0))
  {
    // weighted (readElementArrays checks that every active component then is): one row per step and component
    if (in.datasetExists(kVelocityXSourceElementInputName) || in.datasetExists(kVelocityYSourceElementInputName) ||
        in.datasetExists(kVelocityZSourceElementInputName))
      mVelocitySourceMany = 1;
    else in.readScalarValue(kVelocitySourceManyName, mVelocitySourceMany);
    size_t m = 0;
    in.readScalarValue(kVelocitySourceModeName, m);
    mVelocitySourceMode = toMode(m, "velocity");
  }
  else
  {
    mVelocitySourceMany = 0;
    mVelocitySourceMode = SourceMode::kDirichlet;
  }
  if (mPressureSourceFlag != 0)
  {
    if (in.datasetExists(kPressureSourceElementInputName)) mPressureSourceMany = 1; // weighted: one row per step
    else in.readScalarValue(kPressureSourceManyName, mPressureSourceMany);
    size_t m = 0;
    in.readScalarValue(kPressureSourceModeName, m);
    mPressureSourceMode      = toMode(m, "pressure");
    mPressureSourceIndexSize = in.getDatasetSize(kPressureSourceIndexName);
  }
  else
  {
    mPressureSourceMode      = SourceMode::kDirichlet;
    mPressureSourceMany      = 0;
    mPressureSourceIndexSize = 0;
  }

  mAlphaCoeffScalarFlag = true;
  mAlphaCoeffScalar = mAlphaPower = mAbsorbTauScalar = mAbsorbEtaScalar = 0.0f;
  if (mAbsorbingFlag != 0)
  {
    in.readScalarValue(kAlphaPowerName, mAlphaPower);
    if (mAlphaPower == 1.0f) throw std::invalid_argument("Error: Illegal value of alpha_power (must not equal to 1.0)");
    if (isStokesAbsorption() && mAlphaPower != 2.0f)
      throw std::invalid_argument(std::string("Error: Illegal value of ") + kAlphaPowerName + " (" + std::to_string(mAlphaPower) +
                                  "): " + kAbsorbingFlagName + " = 2 (Stokes absorption) needs " + kAlphaPowerName + " = 2");
    mAlphaCoeffScalarFlag = in.getDatasetDimensionSizes(kAlphaCoeffName) == scalarSizes;
    if (mAlphaCoeffScalarFlag) in.readScalarValue(kAlphaCoeffName, mAlphaCoeffScalar);
  }
  mC0ScalarFlag = in.getDatasetDimensionSizes(kC0Name) == scalarSizes;
  if (mC0ScalarFlag) in.readScalarValue(kC0Name, mC0Scalar);
  mBOnAScalarFlag = true;
  mBOnAScalar     = 0.0f;
  if (mNonLinearFlag)
  {
    mBOnAScalarFlag = in.getDatasetDimensionSizes(kBonAName) == scalarSizes;
    if (mBOnAScalarFlag) in.readScalarValue(kBonAName, mBOnAScalar);
  }
  if (mOptions.storePressureC || mOptions.storeVelocityNonStaggeredC || mOptions.storeIntensityAvgC || mOptions.storeQTermC ||
      mOptions.storeVelocityC)
  { // Parameters.cpp:462-551: the period (in time steps) is given (--period) or found from the pressure source signal:
    // the last <= 500 samples of the middle source point (:488-512)
    if (mOptions.period > 0.0f && mOptions.frequency > 0.0f) // :468-471
      throw std::ios_base::failure("Error: --period and --frequency cannot be given together");
    if (mOptions.frequency > 0.0f) mOptions.period = 1.0f / (mOptions.frequency * mDt); // :473-477
    if (!(mOptions.period > 0.0f))
    {
      if (!in.datasetExists(kPressureSourceInputName))
        throw std::ios_base::failure("Error: compression streams need --period (> 0) or a p_source_input to derive it from");
      const DimensionSizes size = in.getDatasetDimensionSizes(kPressureSourceInputName); // (nSrc | 1, Nt_src, 1)
      std::vector<float> all(size.nElements());
      in.readFloat(kPressureSourceInputName, all.data(), all.size());
      const size_t length = std::min<size_t>(size.ny, 500);
      std::vector<float> tail(length);
      for (size_t t = 0; t < length; t++) tail[t] = all[(size.ny - length + t) * size.nx + size.nx / 2];
      mOptions.period = CompressHelper::findPeriod(tail.data(), length);
    }
    CompressHelper::getInstance().init(mOptions.period, mOptions.mos, mOptions.harmonics, true);
  }
  readElementArrays(in);
  mRho0ScalarFlag = in.getDatasetDimensionSizes(kRho0Name) == scalarSizes;
  if (mRho0ScalarFlag)
  {
    in.readScalarValue(kRho0Name, mRho0Scalar);
    in.readScalarValue(kRho0SgxName, mRho0SgxScalar);
    in.readScalarValue(kRho0SgyName, mRho0SgyScalar);
    in.readScalarValue(kRho0SgzName, mRho0SgzScalar);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weighted transducer arrays: the CSR datasets are checked here, before anything is allocated on the device, because a
// bad offset or column would be an out-of-bounds gather in kw_element_source_row(s) / kw_sample_elements(_multi).  The device holds
// offsets and columns as 32-bit values (kw_csr_entry), which bounds the entry count and, for the sensor, the grid.
void Parameters::readElementArrays(const InputProvider& in)
{
  mPressureSourceElementCount = mPressureSourceElementNnz = 0;
  mVelocitySourceElementCount = mVelocitySourceElementNnz = 0;
  mSensorElementCount = mSensorElementNnz = 0;
  mPressureSourceElementDelayed = mVelocitySourceElementDelayed = mSensorElementDelayed = false;
  mPressureSourceElementMaxDelay = mVelocitySourceElementMaxDelay = mSensorElementMaxDelay = 0;
  const size_t gridPoints = mFullDimensionSizes.nElements();
  constexpr size_t kMax32 = 0xFFFFFFFFull;
  // ptr: rows + 1 non-decreasing 0-based offsets ending at nnz; columns: 1-based, 1 .. limit
  auto checkCsr = [&](const std::string& ptrName, size_t rows, const std::string& colName, const std::string& weightName,
                      size_t limit, const char* what) {
    for (const std::string* n : {&ptrName, &colName, &weightName})
      if (!in.datasetExists(*n)) throw std::invalid_argument(*n + ": dataset is missing (" + what + ")");
    const size_t nnz = in.getDatasetSize(colName);
    if (in.getDatasetSize(ptrName) != rows + 1)
      throw std::invalid_argument(ptrName + ": has " + std::to_string(in.getDatasetSize(ptrName)) + " entries, expected " +
                                  std::to_string(rows + 1));
    if (in.getDatasetSize(weightName) != nnz)
      throw std::invalid_argument(weightName + ": has " + std::to_string(in.getDatasetSize(weightName)) + " entries, but " +
                                  colName + " has " + std::to_string(nnz));
    if (nnz > kMax32) throw std::invalid_argument(colName + ": more than 2^32 - 1 entries");
    std::vector<size_t> ptr(rows + 1), col(nnz);
    in.readIndex(ptrName, ptr.data(), ptr.size());
    if (ptr[0] != 0) throw std::invalid_argument(ptrName + ": the first offset must be 0");
    for (size_t r = 0; r < rows; r++)
      if (ptr[r + 1] < ptr[r]) throw std::invalid_argument(ptrName + ": offsets are not monotone at row " + std::to_string(r));
    if (ptr[rows] != nnz)
      throw std::invalid_argument(ptrName + ": last offset " + std::to_string(ptr[rows]) + " differs from the " +
                                  std::to_string(nnz) + " entries of " + colName);
    if (nnz > 0) in.readIndex(colName, col.data(), col.size());
    for (size_t j = 0; j < nnz; j++)
      if (col[j] < 1 || col[j] > limit)
        throw std::invalid_argument(colName + ": entry " + std::to_string(j) + " = " + std::to_string(col[j]) +
                                    " lies outside 1.." + std::to_string(limit));
    return nnz;
  };

  // the delays of a CSR's entries: one per entry, at most KW_ELEMENT_MAX_DELAY; sets the flag and the largest delay
  auto checkDelays = [&](const std::string& delayName, const std::string& colName, size_t nnz, bool& delayed, size_t& maxDelay) {
    if (!in.datasetExists(delayName)) return;
    if (in.getDatasetSize(delayName) != nnz)
      throw std::invalid_argument(delayName + ": has " + std::to_string(in.getDatasetSize(delayName)) + " entries, but " +
                                  colName + " has " + std::to_string(nnz));
    std::vector<size_t> d(nnz);
    if (nnz > 0) in.readIndex(delayName, d.data(), d.size());
    for (size_t j = 0; j < nnz; j++)
    {
      if (d[j] > KW_ELEMENT_MAX_DELAY)
        throw std::invalid_argument(delayName + ": entry " + std::to_string(j) + " = " + std::to_string(d[j]) +
                                    " lies above the largest delay " + std::to_string(KW_ELEMENT_MAX_DELAY));
      maxDelay = std::max(maxDelay, d[j]);
    }
    delayed = true;
  };
  // the largest delay of the whole array, given where this input holds a part of its entries
  auto readHorizon = [&](const std::string& maxName, const std::string& delayName, bool delayed, size_t& maxDelay) {
    if (!in.datasetExists(maxName)) return;
    if (!delayed) throw std::invalid_argument(maxName + ": present without " + delayName);
    size_t horizon = 0;
    in.readScalarValue(maxName, horizon);
    if (horizon < maxDelay || horizon > KW_ELEMENT_MAX_DELAY)
      throw std::invalid_argument(maxName + ": " + std::to_string(horizon) + " lies outside " + std::to_string(maxDelay) +
                                  ".." + std::to_string(KW_ELEMENT_MAX_DELAY) + " (the largest delay of " + delayName + " and the limit)");
    maxDelay = horizon;
  };
  // ... and a delay dataset whose CSR is not part of the input
  auto refuseLoneDelays = [&](const std::string& delayName, const std::string& colName, const char* what) {
    if (in.datasetExists(delayName))
      throw std::invalid_argument(delayName + ": present without " + colName + " (the delays of a " + what + ")");
  };

  // a weighted source's element signals: not beside the plain series, many = 1 if given, (1, flag, E) with E >= 1
  auto checkElementInput = [&](const std::string& elementName, const std::string& plainName, const std::string& manyName,
                               size_t flag, const std::string& flagName) {
    if (in.datasetExists(plainName))
      throw std::invalid_argument(plainName + " and " + elementName + " cannot both be present");
    if (in.datasetExists(manyName))
    {
      size_t many = 0;
      in.readScalarValue(manyName, many);
      if (many != 1) throw std::invalid_argument(manyName + ": must be 1 with " + elementName);
    }
    const DimensionSizes dims = in.getDatasetDimensionSizes(elementName); // (E, Nt_src, 1)
    const size_t elements = dims.nx;
    if (elements == 0 || dims.nElements() != elements * flag)
      throw std::invalid_argument(elementName + ": expected (1, " + flagName + " = " + std::to_string(flag) + ", E) with E >= 1");
    return elements;
  };

  const bool sourceWeighted = in.datasetExists(kPressureSourceElementInputName);
  if (sourceWeighted && mPressureSourceFlag == 0)
    throw std::invalid_argument(kPressureSourceElementInputName + ": present, but p_source_flag is 0");
  if (sourceWeighted)
  {
    const size_t elements = checkElementInput(kPressureSourceElementInputName, kPressureSourceInputName, kPressureSourceManyName,
                                              mPressureSourceFlag, kPressureSourceFlagName);
    if (mPressureSourceIndexSize > kMax32) throw std::invalid_argument(kPressureSourceIndexName + ": more than 2^32 - 1 points");
    mPressureSourceElementNnz = checkCsr(kPressureSourceElementPtrName, mPressureSourceIndexSize, kPressureSourceElementIndexName,
                                         kPressureSourceElementWeightName, elements, "weighted pressure source");
    mPressureSourceElementCount = elements;
    checkDelays(kPressureSourceElementDelayName, kPressureSourceElementIndexName, mPressureSourceElementNnz,
                mPressureSourceElementDelayed, mPressureSourceElementMaxDelay);
    readHorizon(kPressureSourceElementDelayMaxName, kPressureSourceElementDelayName, mPressureSourceElementDelayed,
                mPressureSourceElementMaxDelay);
  }
  else refuseLoneDelays(kPressureSourceElementDelayName, kPressureSourceElementIndexName, "weighted pressure source");

  // velocity: the components share u_source_index and so one CSR; a component is active when its flag is above 0, and
  // the active ones are all weighted or all plain
  struct Component { const std::string& elementName; const std::string& plainName; const std::string& flagName; size_t flag; };
  const Component comps[3] = {
    {kVelocityXSourceElementInputName, kVelocityXSourceInputName, kVelocityXSourceFlagName, mVelocityXSourceFlag},
    {kVelocityYSourceElementInputName, kVelocityYSourceInputName, kVelocityYSourceFlagName, mVelocityYSourceFlag},
    {kVelocityZSourceElementInputName, kVelocityZSourceInputName, kVelocityZSourceFlagName, mVelocityZSourceFlag}};
  const Component* firstWeighted = nullptr;
  const Component* firstPlain    = nullptr;
  size_t velocityElements = 0;
  for (const Component& c : comps)
  {
    const bool present = in.datasetExists(c.elementName);
    if (present && c.flag == 0) throw std::invalid_argument(c.elementName + ": present, but " + c.flagName + " is 0");
    if (c.flag == 0) continue;
    if (!present)
    {
      if (firstPlain == nullptr) firstPlain = &c;
      continue;
    }
    const size_t elements = checkElementInput(c.elementName, c.plainName, kVelocitySourceManyName, c.flag, c.flagName);
    if (firstWeighted != nullptr && elements != velocityElements)
      throw std::invalid_argument(c.elementName + ": has " + std::to_string(elements) + " elements, but " +
                                  firstWeighted->elementName + " has " + std::to_string(velocityElements));
    if (firstWeighted == nullptr) firstWeighted = &c;
    velocityElements = elements;
  }
  if (firstWeighted != nullptr)
  {
    if (firstPlain != nullptr)
      throw std::invalid_argument(firstPlain->elementName + ": missing, although " + firstPlain->flagName + " is above 0 and " +
                                  firstWeighted->elementName + " is present (active velocity components are all weighted or all plain)");
    if (mTransducerSourceFlag != 0)
      throw std::invalid_argument(firstWeighted->elementName + ": a weighted velocity source cannot be combined with " +
                                  kTransducerSourceFlagName);
    if (mVelocitySourceIndexSize > kMax32) throw std::invalid_argument(kVelocitySourceIndexName + ": more than 2^32 - 1 points");
    mVelocitySourceElementNnz = checkCsr(kVelocitySourceElementPtrName, mVelocitySourceIndexSize, kVelocitySourceElementIndexName,
                                         kVelocitySourceElementWeightName, velocityElements, "weighted velocity source");
    mVelocitySourceElementCount = velocityElements;
    checkDelays(kVelocitySourceElementDelayName, kVelocitySourceElementIndexName, mVelocitySourceElementNnz,
                mVelocitySourceElementDelayed, mVelocitySourceElementMaxDelay);
    readHorizon(kVelocitySourceElementDelayMaxName, kVelocitySourceElementDelayName, mVelocitySourceElementDelayed,
                mVelocitySourceElementMaxDelay);
  }
  else refuseLoneDelays(kVelocitySourceElementDelayName, kVelocitySourceElementIndexName, "weighted velocity source");
  if (getStoreAnyElementsFlag())
  {
    const char* flag = mOptions.storePressureElements ? "--p_elements" : mOptions.storeVelocityElements ? "--u_elements" : "--u_non_staggered_elements";
    if (!in.datasetExists(kSensorElementPtrName) || !in.datasetExists(kSensorElementIndexName) ||
        !in.datasetExists(kSensorElementWeightName))
      throw std::invalid_argument(std::string(flag) + " needs the datasets " + kSensorElementPtrName + ", " + kSensorElementIndexName +
                                  " and " + kSensorElementWeightName);
    if (gridPoints > kMax32)
      throw std::invalid_argument(kSensorElementIndexName + ": the weighted sensor needs a grid of fewer than 2^32 points");
    const size_t rows = in.getDatasetSize(kSensorElementPtrName);
    if (rows < 2) throw std::invalid_argument(kSensorElementPtrName + ": needs E + 1 >= 2 entries");
    mSensorElementNnz   = checkCsr(kSensorElementPtrName, rows - 1, kSensorElementIndexName, kSensorElementWeightName,
                                   gridPoints, "weighted sensor");
    mSensorElementCount = rows - 1;
    checkDelays(kSensorElementDelayName, kSensorElementIndexName, mSensorElementNnz, mSensorElementDelayed,
                mSensorElementMaxDelay);
  }
  else if (!in.datasetExists(kSensorElementIndexName))
    refuseLoneDelays(kSensorElementDelayName, kSensorElementIndexName, "weighted sensor");
}

// ---------------------------------------------------------------------------------------------------------------------
void HipParameters::selectDevice(int deviceIdx)
{
  if (mCtx != nullptr) return; // one context per process, like the reference's single device
  kwCheck(kw_init(deviceIdx, &mCtx));
  kw_device_info info;
  kwCheck(kw_device_info_get(mCtx, &info));
  mDeviceIdx = info.device_id;
}

std::string HipParameters::getDeviceName() const
{
  if (!mCtx) return "";
  kw_device_info info;
  kwCheck(kw_device_info_get(mCtx, &info));
  return std::string(info.name) + " (" + info.arch + ")";
}

void HipParameters::release()
{
  if (mCtx) kw_destroy(mCtx);
  mCtx = nullptr;
}

void HipParameters::setUpDeviceConstants() const
{
  const Parameters& params = Parameters::getInstance();
  const DimensionSizes full = params.getFullDimensionSizes(), red = params.getReducedDimensionSizes();
  kw_constants k{};
  k.nx = static_cast<uint32_t>(full.nx);
  k.ny = static_cast<uint32_t>(full.ny);
  k.nz = static_cast<uint32_t>(full.nz);
  k.n_elements = static_cast<uint32_t>(full.nElements());
  k.nx_complex = static_cast<uint32_t>(red.nx);
  k.ny_complex = static_cast<uint32_t>(red.ny);
  k.nz_complex = static_cast<uint32_t>(red.nz);
  k.n_elements_complex = static_cast<uint32_t>(red.nElements());
  const DimensionSizes global = params.getGlobalDimensionSizes();
  k.fft_divider   = 1.0f / global.nElements(); // 1/N of the whole grid also on a slab
  k.fft_divider_x = 1.0f / global.nx;
  k.fft_divider_y = 1.0f / global.ny;
  k.fft_divider_z = 1.0f / global.nz;
  k.dt      = params.getDt();
  k.dt_by_2 = params.getDt() * 2.0f;
  k.c2      = params.getC2Scalar();
  k.rho0    = params.getRho0Scalar();
  k.dt_rho0 = params.getRho0Scalar() * params.getDt();
  if (params.getRho0ScalarFlag())
  {
    k.dt_rho0_sgx = params.getDtRho0SgxScalar();
    k.dt_rho0_sgy = params.getDtRho0SgyScalar();
    k.dt_rho0_sgz = params.getDtRho0SgzScalar();
  }
  k.b_on_a     = params.getBOnAScalar();
  k.absorb_tau = params.getAbsorbTauScalar();
  k.absorb_eta = params.getAbsorbEtaScalar();
  k.pressure_source_size = static_cast<uint32_t>(params.getPressureSourceIndexSize());
  k.pressure_source_mode = static_cast<uint32_t>(params.getPressureSourceMode());
  k.pressure_source_many = static_cast<uint32_t>(params.getPressureSourceMany());
  k.velocity_source_size = static_cast<uint32_t>(params.getVelocitySourceIndexSize());
  k.velocity_source_mode = static_cast<uint32_t>(params.getVelocitySourceMode());
  k.velocity_source_many = static_cast<uint32_t>(params.getVelocitySourceMany());
  kwCheck(kw_set_constants(mCtx, &k));
}
