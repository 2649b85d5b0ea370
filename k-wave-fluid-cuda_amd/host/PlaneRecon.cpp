// PlaneRecon.cpp — the host side of the k-space plane reconstruction around the device library's kw_plane_recon_* and
// kw_fused_plane_recon entry points.
#include "PlaneRecon.h"

#include <new>

void PlaneRecon::check(kw_status s) const
{
  if (s == KW_OK) return;
  if (s == KW_ERR_ALLOC) throw std::bad_alloc();
  throw CwDeviceError(s, kw_last_error());
}

PlaneRecon::PlaneRecon(const PlaneReconParameters& parameters) : mPar(parameters)
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
    if (!mFused)
    {
      mSpecA = deviceArray(2 * nr);
      mSpecB = deviceArray(2 * nr);
    }
    mRecord = deviceArray(mPar.nRecord());
    mResult = deviceArray(mPar.nResult());
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

PlaneRecon::~PlaneRecon()
{
  if (mCtx == nullptr) return;
  kw_sync(mCtx);
  for (void* p : mOwned) kw_free(mCtx, p);
  if (mFused) kw_fused_destroy(mCtx);
  kw_destroy(mCtx);
}

void* PlaneRecon::deviceBytes(size_t bytes)
{
  void* d = nullptr;
  check(kw_malloc(mCtx, bytes, &d));
  mOwned.push_back(d);
  return d;
}

void PlaneRecon::reconstruct()
{
  kw_plane_recon_op op{};
  op.dx = mPar.dx; op.dy = mPar.dy; op.dt = mPar.dt; op.c0 = mPar.c0;
  op.interp = mPar.interp;
  if (mFused) check(kw_fused_plane_recon(mCtx, mVol, &op, mVol));
  else
  {
    check(kw_fft_r2c_3d(mCtx, mVol, mSpecA));
    check(kw_plane_recon_mix(mCtx, mSpecB, mSpecA, &op, static_cast<float>(2.0 / static_cast<double>(mPar.nExpanded()))));
    check(kw_fft_c2r_3d(mCtx, mSpecB, mVol));
  }
}

void PlaneRecon::run(const float* p)
{
  const uint32_t ex = static_cast<uint32_t>(mPar.ex), ey = static_cast<uint32_t>(mPar.ey), lt = static_cast<uint32_t>(mPar.lt);
  const uint32_t nx = static_cast<uint32_t>(mPar.nx), ny = static_cast<uint32_t>(mPar.ny);
  check(kw_memcpy_h2d(mCtx, mRecord, p, mPar.nRecord() * sizeof(float)));
  check(kw_plane_recon_embed(mCtx, mVol, mRecord, ex, ey, lt, nx, ny, static_cast<uint32_t>(mPar.nt)));
  reconstruct();
  check(kw_plane_recon_crop(mCtx, mResult, mVol, ex, ey, lt, nx, ny, static_cast<uint32_t>(mPar.planes), mPar.positivity ? 1 : 0));
  mRuns++;
}

void PlaneRecon::get(const std::string& name, float* dst, size_t n)
{
  if (name != "p0") throw std::invalid_argument("no reconstruction output named " + name + " (p0)");
  if (n != mPar.nResult()) throw std::invalid_argument("size mismatch for " + name);
  if (mRuns == 0) throw std::invalid_argument(name + ": no run yet");
  check(kw_memcpy_d2h(mCtx, dst, mResult, n * sizeof(float)));
}
