// SecondOrderFrames.cpp — the host side of the batched 2-D exact k-space propagator around the device library's
// kw_second_order_frames_mix, kw_fused_second_order_frames_* and kw_second_order_line_* entry points.
#include "SecondOrderFrames.h"

#include <algorithm>
#include <memory>
#include <vector>

#include "SecondOrderParameters.h"

SecondOrderFrames::SecondOrderFrames(const SecondOrderFramesParameters& parameters) : mPar(parameters), mGrid(mPar.options.deviceIdx)
{
  const size_t ne = mPar.nExpanded(), nr = mPar.nReduced(), nd = mPar.nDomain();
  mGrid.setConstants(gridConstants(mPar.ex, mPar.ey, mPar.frames));
  // the pipeline in frames mode (the z axis of the constants is the batch) when wanted and supported for the batch, the
  // batched 2-D rocFFT plans otherwise
  const bool fused = mGrid.choosePipeline(
    mPar.fastPath, [this](bool on) { mGrid.check(kw_fused_set_frames(context(), on ? 1 : 0)); },
    [this]() { mGrid.check(kw_fft_create_plans_frames(context())); });

  mVol = mGrid.array(ne);
  size_t kept = nr;
  if (fused) mGrid.check(kw_fused_second_order_frames_elems(context(), &kept));
  else mSpec = mGrid.array(2 * nr);
  mKept = mGrid.array(2 * kept);
  mP    = mGrid.array(nd);
  if (mPar.pMax) mMax = mGrid.array(nd);
  if (mPar.pMin) mMin = mGrid.array(nd);
  if (mPar.pRms) mRms = mGrid.array(nd);
  if (mPar.pFinal) mFinal = mGrid.array(nd);
  if (!mPar.sensorIndex.empty())
  {
    const std::vector<uint64_t> index = mPar.expandedSensorIndex();
    mIndex = static_cast<uint64_t*>(mGrid.bytes(index.size() * sizeof(uint64_t)));
    mGrid.check(kw_memcpy_h2d(context(), mIndex, index.data(), index.size() * sizeof(uint64_t)));
  }
  mGrid.check(kw_sync(context()));
}

void SecondOrderFrames::setP0(const float* p0)
{
  mGrid.check(kw_memcpy_h2d(context(), mP, p0, mPar.nDomain() * sizeof(float)));
  mGrid.check(kw_angular_time_embed(context(), mVol, mP, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey),
                                    static_cast<uint32_t>(mPar.frames), static_cast<uint32_t>(mPar.nx),
                                    static_cast<uint32_t>(mPar.ny), static_cast<uint32_t>(mPar.frames)));
  if (mGrid.fused()) mGrid.check(kw_fused_second_order_frames_forward(context(), mVol, mKept));
  else mGrid.check(kw_fft_r2c_frames(context(), mVol, mKept));
  mHaveInput = true;
  mHaveField = false;
  if (mLineRow >= 0) prepareLine(); // (after the fused forward has read mVol)
}

kw_second_order_op SecondOrderFrames::op(double t) const
{
  kw_second_order_op op{};
  op.dx = mPar.dx; op.dy = mPar.dy; op.c0 = mPar.c0;
  op.dz = mPar.dy; // (not looked at)
  op.t  = t;
  op.a  = mPar.a;
  op.alpha_power = mPar.alphaPower;
  op.absorbing   = mPar.a > 0.0 ? 1 : 0;
  return op;
}

void SecondOrderFrames::propagate(double t)
{
  const kw_second_order_op op = this->op(t);
  if (mGrid.fused()) mGrid.check(kw_fused_second_order_frames_time(context(), mKept, &op, mVol));
  else
  {
    const double points = static_cast<double>(mPar.ex) * static_cast<double>(mPar.ey); // of one frame
    mGrid.check(kw_second_order_frames_mix(context(), mSpec, mKept, &op, static_cast<float>(1.0 / points)));
    mGrid.check(kw_fft_c2r_frames(context(), mSpec, mVol));
  }
}

void SecondOrderFrames::crop()
{
  mGrid.check(kw_plane_recon_crop(context(), mP, mVol, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey),
                                  static_cast<uint32_t>(mPar.frames), static_cast<uint32_t>(mPar.nx),
                                  static_cast<uint32_t>(mPar.ny), static_cast<uint32_t>(mPar.frames), 0));
  mHaveField = true;
}

void SecondOrderFrames::field(double t, float* dst)
{
  SecondOrderParameters::checkTime(t);
  if (!mHaveInput) throw std::invalid_argument("field: no p0 yet");
  propagate(t);
  crop();
  if (dst != nullptr) mGrid.check(kw_memcpy_d2h(context(), dst, mP, mPar.nDomain() * sizeof(float)));
}

// SecondOrder::run with the frames' record: its sample row and its aggregates in its order
void SecondOrderFrames::run(const double* times, size_t nTimes)
{
  if (nTimes == 0) GridRule::refuse("n_times", "0 is not a number of output times");
  for (size_t i = 0; i < nTimes; i++) SecondOrderParameters::checkTime(times[i]);
  if (!mHaveInput) throw std::invalid_argument("run: no p0 yet");
  const size_t ns = mPar.sensorIndex.size() * mPar.frames, nd = mPar.nDomain();
  if (ns * nTimes > mRawCapacity)
  {
    if (mRaw != nullptr) mGrid.release(mRaw);
    mRaw = nullptr;
    mRawCapacity = 0;
    mRaw = mGrid.array(ns * nTimes);
    mRawCapacity = ns * nTimes;
  }
  const bool aggregates = mMax || mMin || mRms || mFinal;
  if (mRms != nullptr) mGrid.check(kw_memset(context(), mRms, 0, nd * sizeof(float)));
  for (size_t i = 0; i < nTimes; i++)
  {
    propagate(times[i]);
    if (ns != 0) mGrid.check(kw_sample_index(context(), KW_OP_NONE, mRaw + i * ns, mVol, mIndex, ns));
    if (!aggregates) continue;
    crop();
    // the first time initialises max and min by a copy: no fill with infinities is needed
    if (mMax != nullptr) mGrid.check(kw_sample_all(context(), i == 0 ? KW_OP_NONE : KW_OP_MAX, mMax, mP, nd));
    if (mMin != nullptr) mGrid.check(kw_sample_all(context(), i == 0 ? KW_OP_NONE : KW_OP_MIN, mMin, mP, nd));
    if (mRms != nullptr) mGrid.check(kw_sample_all(context(), KW_OP_RMS, mRms, mP, nd));
    if (mFinal != nullptr && i + 1 == nTimes) mGrid.check(kw_sample_all(context(), KW_OP_NONE, mFinal, mP, nd));
  }
  if (mRms != nullptr) mGrid.check(kw_post_processing_rms(context(), mRms, 1.0f / static_cast<float>(nTimes), nd));
  mTimes = nTimes;
  mRuns++;
}

// ---- the line-sensor record ---------------------------------------------------------------------------------------------
void SecondOrderFrames::freeLine()
{
  mLinePass.reset(); // its context, plans and arrays (after a sync of its own)
  mLinePassTimes = 0;
  mLineG = mLineRows = mLineOut = nullptr;
  for (void* p : { static_cast<void*>(mLineQ), static_cast<void*>(mLineSpec), static_cast<void*>(mLineTimes) })
    if (p != nullptr) mGrid.release(p);
  mLineQ = mLineSpec = nullptr;
  mLineTimes = nullptr;
  mLineTimesCapacity = 0;
  mLineReady = false;
}

void SecondOrderFrames::setLineRow(int64_t row)
{
  mPar.checkLineRow(row);
  mLineRow   = row;
  mLineReady = false; // the next setP0 prepares the row
  if (row < 0)
  {
    mGrid.check(kw_sync(context()));
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
  mLineReady = false;
  if (mLineQ == nullptr) mLineQ = mGrid.array(2 * mPar.lineElems());
  const float* spectra = mKept; // rocFFT path: the kept spectra are the natural (kx, ky) ones
  if (mGrid.fused())
  {
    // the pipeline keeps (kx, y, frame) in its own layout: one batched 2-D transform of the embedded batch, which the
    // fused forward has left as it was
    if (!mLinePlans) mGrid.check(kw_fft_create_plans_frames(context()));
    mLinePlans = true;
    if (mLineSpec == nullptr) mLineSpec = mGrid.array(2 * mPar.nReduced());
    mGrid.check(kw_fft_r2c_frames(context(), mVol, mLineSpec));
    spectra = mLineSpec;
  }
  mGrid.check(kw_second_order_line_prepare(context(), mLineQ, spectra, static_cast<uint32_t>(mLineRow)));
  mLineReady = true;
}

void SecondOrderFrames::makeLinePass(size_t times)
{
  if (mLinePass && mLinePassTimes == times) return;
  mLinePass.reset();
  mLinePassTimes = 0;
  mLineG = mLineRows = mLineOut = nullptr;
  const size_t rows = mPar.frames * times;
  std::unique_ptr<DeviceGrid> pass(new DeviceGrid(mPar.options.deviceIdx));
  pass->setConstants(gridConstants(mPar.ex, 1, rows));
  pass->check(kw_fft_create_plans_frames(pass->ctx())); // ny == 1: batched 1-D plans of length Ex
  float* g       = pass->array(2 * mPar.lineSpectrumElems(times));
  float* rowsOut = pass->array(mPar.ex * rows);
  float* cropped = pass->array(mPar.nx * rows);
  // a last pass of fewer times transforms the whole batch: the rows past its own hold what an earlier pass left there
  pass->check(kw_memset(pass->ctx(), g, 0, 2 * mPar.lineSpectrumElems(times) * sizeof(float)));
  pass->check(kw_sync(pass->ctx()));
  mLinePass = std::move(pass);
  mLineG = g; mLineRows = rowsOut; mLineOut = cropped;
  mLinePassTimes = times;
}

void SecondOrderFrames::lineRecord(const double* times, size_t nTimes, float* dst)
{
  if (mLineRow < 0) throw std::invalid_argument("line_record: no line row set");
  if (!mLineReady) throw std::invalid_argument("line_record: no p0 since the line row was set");
  const size_t chunkTimes = std::min(lineChunkTimes(), std::max<size_t>(nTimes, 1));
  const std::vector<SecondOrderFramesParameters::LineChunk> chunks = SecondOrderFramesParameters::lineChunks(nTimes, chunkTimes);
  for (size_t i = 0; i < nTimes; i++) SecondOrderParameters::checkTime(times[i]);

  if (nTimes > mLineTimesCapacity)
  {
    if (mLineTimes != nullptr) mGrid.release(mLineTimes);
    mLineTimes = nullptr;
    mLineTimesCapacity = 0;
    mLineTimes = static_cast<double*>(mGrid.bytes(nTimes * sizeof(double)));
    mLineTimesCapacity = nTimes;
  }
  mGrid.check(kw_memcpy_h2d(context(), mLineTimes, times, nTimes * sizeof(double)));
  makeLinePass(chunkTimes);

  const kw_second_order_op op = this->op(0.0);
  kw_ctx* pass = mLinePass->ctx();
  const size_t F = mPar.frames;
  for (const auto& c : chunks)
  {
    const size_t rows = F * c.count;
    mGrid.check(kw_second_order_line_record(context(), mLineG, mLineQ, &op, mLineTimes + c.first, static_cast<uint32_t>(c.count)));
    mGrid.check(kw_sync(context())); // the second context has a stream of its own
    mLinePass->check(kw_fft_c2r_frames(pass, mLineG, mLineRows));
    mLinePass->check(kw_plane_recon_crop(pass, mLineOut, mLineRows, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(rows), 1,
                                         static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(rows), 1, 0));
    if (dst == nullptr) mLinePass->check(kw_sync(pass));
    else if (c.count == nTimes) mLinePass->check(kw_memcpy_d2h(pass, dst, mLineOut, rows * mPar.nx * sizeof(float)));
    else
      for (size_t f = 0; f < F; f++) // the pass holds [F][count][Nx], the record [F][n_times][Nx]
        mLinePass->check(kw_memcpy_d2h(pass, dst + mPar.lineOffset(f, c.first, nTimes), mLineOut + f * c.count * mPar.nx,
                                       c.count * mPar.nx * sizeof(float)));
  }
}

void SecondOrderFrames::get(const std::string& name, float* dst, size_t n)
{
  const float* src = nullptr;
  size_t want = mPar.nDomain();
  if (name == "p")
  {
    if (!mHaveField) throw std::invalid_argument("p: no field yet");
    src = mP;
  }
  else
  {
    if (name == "p_raw") { src = mRaw; want = mTimes * mPar.frames * mPar.sensorIndex.size(); }
    else if (name == "p_max") src = mMax;
    else if (name == "p_min") src = mMin;
    else if (name == "p_rms") src = mRms;
    else if (name == "p_final") src = mFinal;
    else throw std::invalid_argument("no propagator output named " + name + " (p_raw, p_max, p_min, p_rms, p_final, p)");
    if (mRuns == 0) throw std::invalid_argument(name + ": no run yet");
    if (name == "p_raw" ? mPar.sensorIndex.empty() : src == nullptr) throw std::invalid_argument(name + ": not recorded");
  }
  if (n != want) throw std::invalid_argument("size mismatch for " + name);
  if (n != 0) mGrid.check(kw_memcpy_d2h(context(), dst, src, n * sizeof(float)));
}
