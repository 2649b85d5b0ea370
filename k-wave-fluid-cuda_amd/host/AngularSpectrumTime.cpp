// AngularSpectrumTime.cpp — the host side of the time-domain angular-spectrum projector around the device library's
// kw_angular_time_* and kw_fused_angular_time_* entry points.
#include "AngularSpectrumTime.h"

#include <new>

void AngularSpectrumTime::check(kw_status s) const
{
  if (s == KW_OK) return;
  if (s == KW_ERR_ALLOC) throw std::bad_alloc();
  throw CwDeviceError(s, kw_last_error());
}

AngularSpectrumTime::AngularSpectrumTime(const AngularTimeParameters& parameters) : mPar(parameters)
{
  check(kw_init(mPar.options.deviceIdx, &mCtx));
  try
  {
    const size_t ne = mPar.nExpanded(), nr = mPar.nReduced();
    kw_constants k{};
    k.nx = static_cast<uint32_t>(mPar.ex);
    k.ny = static_cast<uint32_t>(mPar.ey);
    k.nz = static_cast<uint32_t>(mPar.lt);
    k.n_elements = static_cast<uint32_t>(ne);
    k.nx_complex = static_cast<uint32_t>(mPar.ex / 2 + 1);
    k.ny_complex = k.ny;
    k.nz_complex = k.nz;
    k.n_elements_complex = static_cast<uint32_t>(nr);
    k.fft_divider   = 1.0f / static_cast<float>(ne);
    k.fft_divider_x = 1.0f / static_cast<float>(mPar.ex);
    k.fft_divider_y = 1.0f / static_cast<float>(mPar.ey);
    k.fft_divider_z = 1.0f / static_cast<float>(mPar.lt);
    check(kw_set_constants(mCtx, &k));
    int fusedOk = 0;
    if (mPar.fastPath) check(kw_fused_supported(mCtx, &fusedOk));
    mFused = fusedOk != 0;
    if (mFused) check(kw_fused_create(mCtx));
    else check(kw_fft_create_plans_3d(mCtx));

    mVol = deviceArray(ne);
    size_t kept = nr;
    if (mFused) check(kw_fused_angular_time_elems(mCtx, &kept));
    else mSpec = deviceArray(2 * nr);
    mKept   = deviceArray(2 * kept);
    mRecord = deviceArray(mPar.nRecord());
    mMax    = deviceArray(mPar.nPlane() * mPar.z.size());
    mMin    = deviceArray(mPar.nPlane() * mPar.z.size());
    if (mPar.alphaCoeff > 0.0)
    {
      const std::vector<double> ak = mPar.akTable();
      mAk = static_cast<double*>(deviceBytes(ak.size() * sizeof(double)));
      check(kw_memcpy_h2d(mCtx, mAk, ak.data(), ak.size() * sizeof(double)));
    }
    check(kw_sync(mCtx));
  }
  catch (...)
  {
    for (void* p : mOwned) kw_free(mCtx, p);
    if (mFused) kw_fused_destroy(mCtx);
    kw_destroy(mCtx);
    throw;
  }
}

AngularSpectrumTime::~AngularSpectrumTime()
{
  if (mCtx == nullptr) return;
  kw_sync(mCtx);
  for (void* p : mOwned) kw_free(mCtx, p);
  if (mFused) kw_fused_destroy(mCtx);
  kw_destroy(mCtx);
}

void* AngularSpectrumTime::deviceBytes(size_t bytes)
{
  void* d = nullptr;
  check(kw_malloc(mCtx, bytes, &d));
  mOwned.push_back(d);
  return d;
}

void AngularSpectrumTime::setInput(const float* p0)
{
  const uint32_t ex = static_cast<uint32_t>(mPar.ex), ey = static_cast<uint32_t>(mPar.ey), lt = static_cast<uint32_t>(mPar.lt);
  check(kw_memcpy_h2d(mCtx, mRecord, p0, mPar.nRecord() * sizeof(float)));
  check(kw_angular_time_embed(mCtx, mVol, mRecord, ex, ey, lt, static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny),
                              static_cast<uint32_t>(mPar.nt)));
  if (mFused) check(kw_fused_angular_time_forward(mCtx, mVol, mKept));
  else check(kw_fft_r2c_3d(mCtx, mVol, mKept));
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
  if (mFused) check(kw_fused_angular_time_plane(mCtx, mKept, &op, mVol));
  else
  {
    check(kw_angular_time_mix(mCtx, mSpec, mKept, &op, 1.0f / static_cast<float>(mPar.nExpanded())));
    check(kw_fft_c2r_3d(mCtx, mSpec, mVol));
  }
  check(kw_angular_time_reduce(mCtx, mVol, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey),
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
  check(kw_memcpy_d2h(mCtx, dst, name == "p_max" ? mMax : mMin, n * sizeof(float)));
}

void AngularSpectrumTime::series(size_t j, float* dst, size_t n)
{
  if (j >= mPar.z.size()) throw std::invalid_argument("series: plane " + std::to_string(j) + " of " + std::to_string(mPar.z.size()));
  if (n != mPar.nRecord()) throw std::invalid_argument("size mismatch for series");
  if (!mHaveInput) throw std::invalid_argument("series: no input yet");
  plane(j, nullptr, nullptr, mRecord); // (the record's copy has been embedded: its array is free)
  check(kw_memcpy_d2h(mCtx, dst, mRecord, n * sizeof(float)));
}
