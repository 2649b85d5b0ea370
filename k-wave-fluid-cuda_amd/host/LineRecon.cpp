// LineRecon.cpp — the host side of the batched k-space line reconstruction around the device library's kw_line_recon_*
// and kw_fused_line_recon entry points.
#include "LineRecon.h"

#include <algorithm>

LineRecon::LineRecon(const LineReconParameters& parameters) : mPar(parameters), mGrid(mPar.options.deviceIdx)
{
  mGrid.setConstants(gridConstants(mPar.ey, mPar.lt, mPar.chunkFrames));
  // the pipeline in frames mode (the z axis of the constants is the batch) when wanted and supported for one chunk, the
  // batched 2-D rocFFT plans otherwise
  const bool fused = mGrid.choosePipeline(
    mPar.fastPath, [this](bool on) { mGrid.check(kw_fused_set_frames(context(), on ? 1 : 0)); },
    [this]() { mGrid.check(kw_fft_create_plans_frames(context())); });

  mVol = mGrid.array(mPar.nExpandedChunk());
  if (!fused)
  {
    mSpecA = mGrid.array(2 * mPar.nReducedChunk());
    mSpecB = mGrid.array(2 * mPar.nReducedChunk());
  }
  mRecord = mGrid.array(mPar.ny * mPar.nt * mPar.chunkFrames);
  mResult = mGrid.array(mPar.nResult());
  mGrid.check(kw_sync(context()));
}

void LineRecon::reconstruct()
{
  kw_plane_recon_op op{};
  op.dx = mPar.dy; // the sensor axis lies where the pipeline has x
  op.dy = mPar.dy; // (ignored)
  op.dt = mPar.dt; op.c0 = mPar.c0;
  op.interp = mPar.interp;
  if (mGrid.fused()) mGrid.check(kw_fused_line_recon(context(), mVol, &op, mVol));
  else
  {
    mGrid.check(kw_fft_r2c_frames(context(), mVol, mSpecA));
    const double points = static_cast<double>(mPar.ey) * static_cast<double>(mPar.lt); // of one frame
    mGrid.check(kw_line_recon_mix(context(), mSpecB, mSpecA, &op, static_cast<float>(2.0 / points)));
    mGrid.check(kw_fft_c2r_frames(context(), mSpecB, mVol));
  }
}

void LineRecon::run(const float* p)
{
  const uint32_t ey = static_cast<uint32_t>(mPar.ey), lt = static_cast<uint32_t>(mPar.lt), ny = static_cast<uint32_t>(mPar.ny);
  const uint32_t chunk = static_cast<uint32_t>(mPar.chunkFrames);
  const size_t   frame = mPar.ny * mPar.nt, image = mPar.ny * mPar.depth;
  for (size_t f0 = 0; f0 < mPar.frames; f0 += chunk)
  {
    const size_t n = std::min<size_t>(chunk, mPar.frames - f0); // the chunk's own frames; the others are zero records
    mGrid.check(kw_memcpy_h2d(context(), mRecord, p + f0 * frame, n * frame * sizeof(float)));
    if (n < chunk) mGrid.check(kw_memset(context(), mRecord + n * frame, 0, (chunk - n) * frame * sizeof(float)));
    mGrid.check(kw_line_recon_embed(context(), mVol, mRecord, ey, lt, chunk, ny, static_cast<uint32_t>(mPar.nt)));
    reconstruct();
    mGrid.check(kw_line_recon_crop(context(), mResult + f0 * image, mVol, ey, lt, static_cast<uint32_t>(n), ny,
                                   static_cast<uint32_t>(mPar.depth), mPar.positivity ? 1 : 0));
  }
  mRuns++;
}

void LineRecon::get(const std::string& name, float* dst, size_t n)
{
  if (name != "p0") throw std::invalid_argument("no reconstruction output named " + name + " (p0)");
  if (n != mPar.nResult()) throw std::invalid_argument("size mismatch for " + name);
  if (mRuns == 0) throw std::invalid_argument(name + ": no run yet");
  mGrid.check(kw_memcpy_d2h(context(), dst, mResult, n * sizeof(float)));
}
