// SecondOrderFrames.cpp — the frames form of the exact k-space propagator: the device library's kw_second_order_frames_mix
// and kw_fused_second_order_frames_* entry points under SecondOrderCore, and the line-sensor record around
// kw_second_order_line_*.
#include "SecondOrderFrames.h"

#include <algorithm>
#include <vector>

namespace
{
const SecondOrderEntries kEntries = { true,
                                      kw_fused_second_order_frames_elems,
                                      kw_fused_second_order_frames_forward,
                                      kw_fused_second_order_frames_time,
                                      kw_second_order_frames_mix,
                                      kw_fused_second_order_frames_time_pair,
                                      kw_second_order_frames_mix_pair,
                                      kw_fft_r2c_frames,
                                      kw_fft_c2r_frames };

SecondOrderForm form(const SecondOrderFramesParameters& p)
{
  kw_second_order_op op{};
  op.dx = p.dx; op.dy = p.dy; op.c0 = p.c0;
  op.dz = p.dy; // (not looked at)
  op.a  = p.a;
  op.alpha_power = p.alphaPower;
  op.absorbing   = p.a > 0.0 ? 1 : 0;
  const double points = static_cast<double>(p.ex) * static_cast<double>(p.ey); // of one frame
  return { p.ex, p.ey, p.frames, p.nx, p.ny, p.frames, static_cast<float>(1.0 / points), op, &kEntries };
}
} // namespace

SecondOrderFrames::SecondOrderFrames(const SecondOrderFramesParameters& parameters)
  : mPar(parameters), mCore(mPar, form(mPar), mPar.expandedSensorIndex())
{
}

void SecondOrderFrames::setP0(const float* p0)
{
  mCore.setP0(p0);
  if (mLineRow >= 0) prepareLine(); // (after the fused forward has read the batch)
}

// ---- the line-sensor record ---------------------------------------------------------------------------------------------
void SecondOrderFrames::freeLine()
{
  mLinePass.reset(); // its context, plans and arrays (after a sync of its own)
  for (void* p : { static_cast<void*>(mLine.q), static_cast<void*>(mLine.spec), static_cast<void*>(mLine.times) })
    if (p != nullptr) mCore.grid().release(p);
  mLine = Line();
}

void SecondOrderFrames::setLineRow(int64_t row)
{
  mPar.checkLineRow(row);
  mLineRow    = row;
  mLine.ready = false; // the next setP0 prepares the row
  if (row < 0)
  {
    mCore.grid().check(kw_sync(context()));
    freeLine();
  }
}

void SecondOrderFrames::setLineChunkTimes(uint64_t times)
{
  mPar.lineChunkTimes(times); // refuses what one pass cannot take
  mLineChunkGiven = times;
}

void SecondOrderFrames::prepareLine()
{
  DeviceGrid& grid = mCore.grid();
  mLine.ready = false;
  if (mLine.q == nullptr) mLine.q = grid.array(2 * mPar.lineElems());
  const float* spectra = mCore.kept(); // rocFFT path: the kept spectra are the natural (kx, ky) ones
  if (grid.fused())
  {
    // the pipeline keeps (kx, y, frame) in its own layout: one batched 2-D transform of the embedded batch, which the
    // fused forward has left as it was
    if (!mLinePlans) grid.check(kw_fft_create_plans_frames(context()));
    mLinePlans = true;
    if (mLine.spec == nullptr) mLine.spec = grid.array(2 * mPar.nReduced());
    grid.check(kw_fft_r2c_frames(context(), mCore.vol(), mLine.spec));
    spectra = mLine.spec;
  }
  grid.check(kw_second_order_line_prepare(context(), mLine.q, spectra, static_cast<uint32_t>(mLineRow)));
  mLine.ready = true;
}

SecondOrderFrames::LinePass::LinePass(const SecondOrderFramesParameters& par, size_t passTimes)
  : grid(par.options.deviceIdx), times(passTimes)
{
  const size_t n = par.frames * times; // rows
  grid.setConstants(gridConstants(par.ex, 1, n));
  grid.check(kw_fft_create_plans_frames(grid.ctx())); // ny == 1: batched 1-D plans of length Ex
  g    = grid.array(2 * par.lineSpectrumElems(times));
  rows = grid.array(par.ex * n);
  out  = grid.array(par.nx * n);
  // a last pass of fewer times transforms the whole batch: the rows past its own hold what an earlier pass left there
  grid.check(kw_memset(grid.ctx(), g, 0, 2 * par.lineSpectrumElems(times) * sizeof(float)));
  grid.check(kw_sync(grid.ctx()));
}

void SecondOrderFrames::makeLinePass(size_t times)
{
  if (mLinePass && mLinePass->times == times) return;
  mLinePass.reset(); // the old one goes first
  mLinePass.reset(new LinePass(mPar, times));
}

void SecondOrderFrames::lineRecord(const double* times, size_t nTimes, float* dst)
{
  if (mLineRow < 0) throw std::invalid_argument("line_record: no line row set");
  if (!mLine.ready) throw std::invalid_argument("line_record: no p0 since the line row was set");
  if (mCore.hasDp0dt())
    throw std::invalid_argument("line_record: a dp0dt is set and the line record takes p0 alone (not built: dp0dt in "
                                "line_record); clear it with set_dp0dt(NULL), or sample the row with run(times)");
  const size_t chunkTimes = std::min(lineChunkTimes(), std::max<size_t>(nTimes, 1));
  const std::vector<SecondOrderFramesParameters::LineChunk> chunks = SecondOrderFramesParameters::lineChunks(nTimes, chunkTimes);
  for (size_t i = 0; i < nTimes; i++) SecondOrderRules::checkTime(times[i]);

  DeviceGrid& grid = mCore.grid();
  if (nTimes > mLine.timesCapacity)
  {
    if (mLine.times != nullptr) grid.release(mLine.times);
    mLine.times = nullptr;
    mLine.timesCapacity = 0;
    mLine.times = static_cast<double*>(grid.bytes(nTimes * sizeof(double)));
    mLine.timesCapacity = nTimes;
  }
  grid.check(kw_memcpy_h2d(context(), mLine.times, times, nTimes * sizeof(double)));
  makeLinePass(chunkTimes);

  const kw_second_order_op op = mCore.op(0.0);
  LinePass& pass = *mLinePass;
  kw_ctx* second = pass.grid.ctx();
  const size_t F = mPar.frames;
  for (const auto& c : chunks)
  {
    const size_t rows = F * c.count;
    grid.check(kw_second_order_line_record(context(), pass.g, mLine.q, &op, mLine.times + c.first, static_cast<uint32_t>(c.count)));
    grid.check(kw_sync(context())); // the second context has a stream of its own
    pass.grid.check(kw_fft_c2r_frames(second, pass.g, pass.rows));
    pass.grid.check(kw_plane_recon_crop(second, pass.out, pass.rows, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(rows), 1,
                                        static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(rows), 1, 0));
    if (dst == nullptr) pass.grid.check(kw_sync(second));
    else if (c.count == nTimes) pass.grid.check(kw_memcpy_d2h(second, dst, pass.out, rows * mPar.nx * sizeof(float)));
    else
      for (size_t f = 0; f < F; f++) // the pass holds [F][count][Nx], the record [F][n_times][Nx]
        pass.grid.check(kw_memcpy_d2h(second, dst + mPar.lineOffset(f, c.first, nTimes), pass.out + f * c.count * mPar.nx,
                                      c.count * mPar.nx * sizeof(float)));
  }
}
