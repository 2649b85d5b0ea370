// AngularSpectrumTime.cpp — the host side of the time-domain angular-spectrum projector around the device library's
// kw_angular_time_* and kw_fused_angular_time_* entry points.
#include "AngularSpectrumTime.h"

AngularSpectrumTime::AngularSpectrumTime(const AngularTimeParameters& parameters) : mPar(parameters), mGrid(mPar.options.deviceIdx)
{
  const size_t ne = mPar.nExpanded(), nr = mPar.nReduced();
  mGrid.setConstants(gridConstants(mPar.ex, mPar.ey, mPar.lt));
  const bool fused = mGrid.choosePipeline(mPar.fastPath);

  mVol = mGrid.array(ne);
  size_t kept = nr;
  if (fused) mGrid.check(kw_fused_angular_time_elems(context(), &kept));
  else mSpec = mGrid.array(2 * nr);
  mKept   = mGrid.array(2 * kept);
  mRecord = mGrid.array(mPar.nRecord());
  mMax    = mGrid.array(mPar.nPlane() * mPar.z.size());
  mMin    = mGrid.array(mPar.nPlane() * mPar.z.size());
  if (mPar.alphaCoeff > 0.0)
  {
    const std::vector<double> ak = mPar.akTable();
    mAk = static_cast<double*>(mGrid.bytes(ak.size() * sizeof(double)));
    mGrid.check(kw_memcpy_h2d(context(), mAk, ak.data(), ak.size() * sizeof(double)));
  }
  mGrid.check(kw_sync(context()));
}

void AngularSpectrumTime::setInput(const float* p0)
{
  const uint32_t ex = static_cast<uint32_t>(mPar.ex), ey = static_cast<uint32_t>(mPar.ey), lt = static_cast<uint32_t>(mPar.lt);
  mGrid.check(kw_memcpy_h2d(context(), mRecord, p0, mPar.nRecord() * sizeof(float)));
  mGrid.check(kw_angular_time_embed(context(), mVol, mRecord, ex, ey, lt, static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny),
                                    static_cast<uint32_t>(mPar.nt)));
  if (mGrid.fused()) mGrid.check(kw_fused_angular_time_forward(context(), mVol, mKept));
  else mGrid.check(kw_fft_r2c_3d(context(), mVol, mKept));
  mHaveInput = true;
}

void AngularSpectrumTime::plane(size_t j, float* pMax, float* pMin, float* series)
{
  kw_angular_time_op op{};
  op.dx = mPar.dx; op.dy = mPar.dy; op.dt = mPar.dt; op.c0 = mPar.c0;
  op.z  = mPar.z[j];
  op.ak = mAk;
  op.restriction = mPar.restriction ? 1 : 0;
  op.retarded    = mPar.retarded ? 1 : 0;
  if (mGrid.fused()) mGrid.check(kw_fused_angular_time_plane(context(), mKept, &op, mVol));
  else
  {
    mGrid.check(kw_angular_time_mix(context(), mSpec, mKept, &op, 1.0f / static_cast<float>(mPar.nExpanded())));
    mGrid.check(kw_fft_c2r_3d(context(), mSpec, mVol));
  }
  mGrid.check(kw_angular_time_reduce(context(), mVol, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey),
                                     static_cast<uint32_t>(mPar.lt), static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny),
                                     static_cast<uint32_t>(mPar.nt), pMax, pMin, series));
}

void AngularSpectrumTime::project()
{
  if (!mHaveInput) throw std::invalid_argument("project: no input yet");
  const size_t np = mPar.nPlane();
  for (size_t j = 0; j < mPar.z.size(); j++) plane(j, mMax + j * np, mMin + j * np, nullptr);
}

void AngularSpectrumTime::run(const float* p0)
{
  setInput(p0);
  project();
  mRuns++;
}

void AngularSpectrumTime::get(const std::string& name, float* dst, size_t n)
{
  if (name != "p_max" && name != "p_min") throw std::invalid_argument("no projector output named " + name + " (p_max, p_min)");
  if (n != mPar.nPlane() * mPar.z.size()) throw std::invalid_argument("size mismatch for " + name);
  if (mRuns == 0) throw std::invalid_argument(name + ": no run yet");
  mGrid.check(kw_memcpy_d2h(context(), dst, name == "p_max" ? mMax : mMin, n * sizeof(float)));
}

void AngularSpectrumTime::series(size_t j, float* dst, size_t n)
{
  if (j >= mPar.z.size()) throw std::invalid_argument("series: plane " + std::to_string(j) + " of " + std::to_string(mPar.z.size()));
  if (n != mPar.nRecord()) throw std::invalid_argument("size mismatch for series");
  if (!mHaveInput) throw std::invalid_argument("series: no input yet");
  plane(j, nullptr, nullptr, mRecord); // (the record's copy has been embedded: its array is free)
  mGrid.check(kw_memcpy_d2h(context(), dst, mRecord, n * sizeof(float)));
}
