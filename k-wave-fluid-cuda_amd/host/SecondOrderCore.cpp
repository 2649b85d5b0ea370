// SecondOrderCore.cpp — see SecondOrderCore.h.
#include "SecondOrderCore.h"

SecondOrderCore::SecondOrderCore(const SecondOrderRules& rules, const SecondOrderForm& form, const std::vector<uint64_t>& index)
  : mForm(form), mRow(index.size()), mGrid(rules.options.deviceIdx)
{
  const size_t nr = mForm.nReduced(), nd = mForm.nDomain();
  mGrid.setConstants(gridConstants(mForm.ex, mForm.ey, mForm.ez));
  // a batch: the pipeline in frames mode (the z axis of the constants is the batch) when wanted and supported for it, the
  // batched 2-D rocFFT plans otherwise
  const bool fused = !mForm.entries->framesContext
                       ? mGrid.choosePipeline(rules.fastPath)
                       : mGrid.choosePipeline(
                           rules.fastPath, [this](bool on) { mGrid.check(kw_fused_set_frames(ctx(), on ? 1 : 0)); },
                           [this]() { mGrid.check(kw_fft_create_plans_frames(ctx())); });

  mVol = mGrid.array(mForm.nExpanded());
  size_t kept = nr;
  if (fused) mGrid.check(mForm.entries->elems(ctx(), &kept));
  else mSpec = mGrid.array(2 * nr);
  mKeptFloats = 2 * kept;
  mKept = mGrid.array(mKeptFloats);
  mP    = mGrid.array(nd);
  if (rules.pMax) mMax = mGrid.array(nd);
  if (rules.pMin) mMin = mGrid.array(nd);
  if (rules.pRms) mRms = mGrid.array(nd);
  if (rules.pFinal) mFinal = mGrid.array(nd);
  if (!index.empty())
  {
    mIndex = static_cast<uint64_t*>(mGrid.bytes(index.size() * sizeof(uint64_t)));
    mGrid.check(kw_memcpy_h2d(ctx(), mIndex, index.data(), index.size() * sizeof(uint64_t)));
  }
  mGrid.check(kw_sync(ctx()));
}

void SecondOrderCore::keep(const float* src, float* kept)
{
  const SecondOrderForm& f = mForm;
  mGrid.check(kw_memcpy_h2d(ctx(), mP, src, f.nDomain() * sizeof(float)));
  mGrid.check(kw_angular_time_embed(ctx(), mVol, mP, static_cast<uint32_t>(f.ex), static_cast<uint32_t>(f.ey),
                                    static_cast<uint32_t>(f.ez), static_cast<uint32_t>(f.nx), static_cast<uint32_t>(f.ny),
                                    static_cast<uint32_t>(f.nz)));
  if (mGrid.fused()) mGrid.check(f.entries->forward(ctx(), mVol, kept));
  else mGrid.check(f.entries->r2c(ctx(), mVol, kept));
  mHaveField = false; // (mP has been the staging array)
}

void SecondOrderCore::setP0(const float* p0)
{
  keep(p0, mKept);
  mHaveInput = true;
}

void SecondOrderCore::setDp0dt(const float* dp0dt)
{
  if (dp0dt == nullptr)
  {
    mHaveDp0dt = false; // (the array stays: the next setDp0dt finds it)
    return;
  }
  if (mKeptV == nullptr) mKeptV = mGrid.array(mKeptFloats);
  mHaveDp0dt = false;
  keep(dp0dt, mKeptV);
  mHaveDp0dt = true;
}

kw_second_order_op SecondOrderCore::op(double t) const
{
  kw_second_order_op op = mForm.op;
  op.t = t;
  return op;
}

void SecondOrderCore::propagate(double t)
{
  const kw_second_order_op op = this->op(t);
  if (mGrid.fused())
    mGrid.check(mHaveDp0dt ? mForm.entries->timePair(ctx(), mKept, mKeptV, &op, mVol) : mForm.entries->time(ctx(), mKept, &op, mVol));
  else
  {
    if (mHaveDp0dt) mGrid.check(mForm.entries->mixPair(ctx(), mSpec, mKept, mKeptV, &op, mForm.divider));
    else mGrid.check(mForm.entries->mix(ctx(), mSpec, mKept, &op, mForm.divider));
    mGrid.check(mForm.entries->c2r(ctx(), mSpec, mVol));
  }
}

void SecondOrderCore::crop()
{
  const SecondOrderForm& f = mForm;
  mGrid.check(kw_plane_recon_crop(ctx(), mP, mVol, static_cast<uint32_t>(f.ex), static_cast<uint32_t>(f.ey),
                                  static_cast<uint32_t>(f.ez), static_cast<uint32_t>(f.nx), static_cast<uint32_t>(f.ny),
                                  static_cast<uint32_t>(f.nz), 0));
  mHaveField = true;
}

void SecondOrderCore::field(double t, float* dst)
{
  SecondOrderRules::checkTime(t);
  if (!mHaveInput) throw std::invalid_argument("field: no p0 yet");
  propagate(t);
  crop();
  if (dst != nullptr) mGrid.check(kw_memcpy_d2h(ctx(), dst, mP, mForm.nDomain() * sizeof(float)));
}

void SecondOrderCore::run(const double* times, size_t nTimes)
{
  if (nTimes == 0) GridRule::refuse("n_times", "0 is not a number of output times");
  for (size_t i = 0; i < nTimes; i++) SecondOrderRules::checkTime(times[i]);
  if (!mHaveInput) throw std::invalid_argument("run: no p0 yet");
  const size_t ns = mRow, nd = mForm.nDomain();
  if (ns * nTimes > mRawCapacity)
  {
    if (mRaw != nullptr) mGrid.release(mRaw);
    mRaw = nullptr;
    mRawCapacity = 0;
    mRaw = mGrid.array(ns * nTimes);
    mRawCapacity = ns * nTimes;
  }
  const bool aggregates = mMax || mMin || mRms || mFinal;
  if (mRms != nullptr) mGrid.check(kw_memset(ctx(), mRms, 0, nd * sizeof(float)));
  for (size_t i = 0; i < nTimes; i++)
  {
    propagate(times[i]);
    if (ns != 0) mGrid.check(kw_sample_index(ctx(), KW_OP_NONE, mRaw + i * ns, mVol, mIndex, ns));
    if (!aggregates) continue;
    crop();
    // the first time initialises max and min by a copy: no fill with infinities is needed
    if (mMax != nullptr) mGrid.check(kw_sample_all(ctx(), i == 0 ? KW_OP_NONE : KW_OP_MAX, mMax, mP, nd));
    if (mMin != nullptr) mGrid.check(kw_sample_all(ctx(), i == 0 ? KW_OP_NONE : KW_OP_MIN, mMin, mP, nd));
    if (mRms != nullptr) mGrid.check(kw_sample_all(ctx(), KW_OP_RMS, mRms, mP, nd));
    if (mFinal != nullptr && i + 1 == nTimes) mGrid.check(kw_sample_all(ctx(), KW_OP_NONE, mFinal, mP, nd));
  }
  if (mRms != nullptr) mGrid.check(kw_post_processing_rms(ctx(), mRms, 1.0f / static_cast<float>(nTimes), nd));
  mTimes = nTimes;
  mRuns++;
}

void SecondOrderCore::get(const std::string& name, float* dst, size_t n)
{
  const float* src = nullptr;
  size_t want = mForm.nDomain();
  if (name == "p")
  {
    if (!mHaveField) throw std::invalid_argument("p: no field yet");
    src = mP;
  }
  else
  {
    if (name == "p_raw") { src = mRaw; want = mTimes * mRow; }
    else if (name == "p_max") src = mMax;
    else if (name == "p_min") src = mMin;
    else if (name == "p_rms") src = mRms;
    else if (name == "p_final") src = mFinal;
    else throw std::invalid_argument("no propagator output named " + name + " (p_raw, p_max, p_min, p_rms, p_final, p)");
    if (mRuns == 0) throw std::invalid_argument(name + ": no run yet");
    if (name == "p_raw" ? mRow == 0 : src == nullptr) throw std::invalid_argument(name + ": not recorded");
  }
  if (n != want) throw std::invalid_argument("size mismatch for " + name);
  if (n != 0) mGrid.check(kw_memcpy_d2h(ctx(), dst, src, n * sizeof(float)));
}
