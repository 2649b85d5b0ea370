// CwPropagator.cpp — the host side of the CW field propagator around the device library's kw_cw_* entry points.
#include "CwPropagator.h"

CwPropagator::CwPropagator(const CwParameters& parameters) : mPar(parameters), mGrid(mPar.options.deviceIdx)
{
  const size_t ne = mPar.nExpanded(), nr = mPar.nReduced(), nd = mPar.nElements();
  mGrid.setConstants(gridConstants(mPar.ex, mPar.ey, mPar.ez));
  const bool fused = mGrid.choosePipeline(mPar.options.fusedKernels);

  mRe = mGrid.array(ne);
  mIm = mGrid.array(ne);
  mA  = mGrid.array(nd);
  mB  = mGrid.array(nd);
  mOut = mGrid.array(nd);

  // the operator, once: float64 on the device, rounded once; the fast path reads it in the pipeline's own layout
  const double twoPi = 2.0 * 3.14159265358979323846;
  float* gRe = mGrid.array(nr);
  float* gIm = mGrid.array(nr);
  mGrid.check(kw_cw_operator(context(), gRe, gIm, mPar.c0, mPar.omega(), mPar.t,
                             twoPi / (static_cast<double>(mPar.ex) * mPar.dx), twoPi / (static_cast<double>(mPar.ey) * mPar.dy),
                             twoPi / (static_cast<double>(mPar.ez) * mPar.dz)));
  if (fused)
  {
    mGRe = mGrid.importReduced(gRe);
    mGIm = mGrid.importReduced(gIm);
    mGrid.check(kw_sync(context()));
    mGrid.release(gIm); // the reduced form is not needed again
    mGrid.release(gRe);
  }
  else
  {
    mGRe = gRe;
    mGIm = gIm;
    mSpecRe = mGrid.array(2 * nr);
    mSpecIm = mGrid.array(2 * nr);
  }
  mGrid.check(kw_memset(context(), mRe, 0, ne * sizeof(float)));
  mGrid.check(kw_memset(context(), mIm, 0, ne * sizeof(float)));
  mGrid.check(kw_sync(context()));
}

void CwPropagator::propagate()
{
  if (mGrid.fused())
  {
    mGrid.check(kw_fused_cw_pair(context(), mRe, mIm, mGRe, mGIm));
    return;
  }
  mGrid.check(kw_fft_r2c_3d(context(), mRe, mSpecRe));
  mGrid.check(kw_fft_r2c_3d(context(), mIm, mSpecIm));
  mGrid.check(kw_cw_mix(context(), mSpecRe, mSpecIm, mGRe, mGIm, mPar.nReduced()));
  mGrid.check(kw_fft_c2r_3d(context(), mSpecRe, mRe));
  mGrid.check(kw_fft_c2r_3d(context(), mSpecIm, mIm));
}

void CwPropagator::run(const float* a, const float* b, bool parts)
{
  const size_t nd = mPar.nElements();
  mGrid.check(kw_memcpy_h2d(context(), mA, a, nd * sizeof(float)));
  mGrid.check(kw_memcpy_h2d(context(), mB, b, nd * sizeof(float)));
  mGrid.check(kw_cw_embed(context(), mRe, mIm, mA, mB, parts ? 1 : 0, static_cast<float>(mPar.scaleRe), static_cast<float>(mPar.scaleIm),
                          static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey), static_cast<uint32_t>(mPar.ez),
                          static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny), static_cast<uint32_t>(mPar.nz)));
  propagate();
  mRuns++;
}

void CwPropagator::get(const std::string& name, float* dst, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for " + name);
  if (mRuns == 0) throw std::invalid_argument(name + ": no run yet");
  float *re = nullptr, *im = nullptr, *amp = nullptr, *phase = nullptr;
  if (name == "re") re = mOut;
  else if (name == "im") im = mOut;
  else if (name == "amplitude") amp = mOut;
  else if (name == "phase") phase = mOut;
  else throw std::invalid_argument("no CW output named " + name + " (re, im, amplitude, phase)");
  mGrid.check(kw_cw_extract(context(), mRe, mIm, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey),
                            static_cast<uint32_t>(mPar.ez), static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny),
                            static_cast<uint32_t>(mPar.nz), re, im, amp, phase, nullptr, nullptr, 0.0f));
  mGrid.check(kw_memcpy_d2h(context(), dst, mOut, n * sizeof(float)));
}

void CwPropagator::heat(const float* q, float qScalar, float* dst, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for Q");
  if (mRuns == 0) throw std::invalid_argument("Q: no run yet");
  if (q != nullptr)
  {
    if (mQ == nullptr) mQ = mGrid.array(n);
    mGrid.check(kw_memcpy_h2d(context(), mQ, q, n * sizeof(float)));
  }
  mGrid.check(kw_cw_extract(context(), mRe, mIm, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey),
                            static_cast<uint32_t>(mPar.ez), static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny),
                            static_cast<uint32_t>(mPar.nz), nullptr, nullptr, nullptr, nullptr, mOut, q != nullptr ? mQ : nullptr,
                            qScalar));
  mGrid.check(kw_memcpy_d2h(context(), dst, mOut, n * sizeof(float)));
}
