// PlaneRecon.cpp — the host side of the k-space plane reconstruction around the device library's kw_plane_recon_* and
// kw_fused_plane_recon entry points.
#include "PlaneRecon.h"

PlaneRecon::PlaneRecon(const PlaneReconParameters& parameters) : mPar(parameters), mGrid(mPar.options.deviceIdx)
{
  const size_t ne = mPar.nExpanded(), nr = mPar.nReduced();
  mGrid.setConstants(gridConstants(mPar.ex, mPar.ey, mPar.lt));
  const bool fused = mGrid.choosePipeline(mPar.fastPath);

  mVol = mGrid.array(ne);
  if (!fused)
  {
    mSpecA = mGrid.array(2 * nr);
    mSpecB = mGrid.array(2 * nr);
  }
  mRecord = mGrid.array(mPar.nRecord());
  mResult = mGrid.array(mPar.nResult());
  mGrid.check(kw_sync(context()));
}

void PlaneRecon::reconstruct()
{
  kw_plane_recon_op op{};
  op.dx = mPar.dx; op.dy = mPar.dy; op.dt = mPar.dt; op.c0 = mPar.c0;
  op.interp = mPar.interp;
  if (mGrid.fused()) mGrid.check(kw_fused_plane_recon(context(), mVol, &op, mVol));
  else
  {
    mGrid.check(kw_fft_r2c_3d(context(), mVol, mSpecA));
    mGrid.check(kw_plane_recon_mix(context(), mSpecB, mSpecA, &op, static_cast<float>(2.0 / static_cast<double>(mPar.nExpanded()))));
    mGrid.check(kw_fft_c2r_3d(context(), mSpecB, mVol));
  }
}

void PlaneRecon::run(const float* p)
{
  const uint32_t ex = static_cast<uint32_t>(mPar.ex), ey = static_cast<uint32_t>(mPar.ey), lt = static_cast<uint32_t>(mPar.lt);
  const uint32_t nx = static_cast<uint32_t>(mPar.nx), ny = static_cast<uint32_t>(mPar.ny);
  mGrid.check(kw_memcpy_h2d(context(), mRecord, p, mPar.nRecord() * sizeof(float)));
  mGrid.check(kw_plane_recon_embed(context(), mVol, mRecord, ex, ey, lt, nx, ny, static_cast<uint32_t>(mPar.nt)));
  reconstruct();
  mGrid.check(kw_plane_recon_crop(context(), mResult, mVol, ex, ey, lt, nx, ny, static_cast<uint32_t>(mPar.planes), mPar.positivity ? 1 : 0));
  mRuns++;
}

void PlaneRecon::get(const std::string& name, float* dst, size_t n)
{
  if (name != "p0") throw std::invalid_argument("no reconstruction output named " + name + " (p0)");
  if (n != mPar.nResult()) throw std::invalid_argument("size mismatch for " + name);
  if (mRuns == 0) throw std::invalid_argument(name + ": no run yet");
  mGrid.check(kw_memcpy_d2h(context(), dst, mResult, n * sizeof(float)));
}
