// AngularSpectrum.cpp — the host side of the angular-spectrum projector around the device library's kw_angular_* and
// kw_fused_angular_* entry points.
#include "AngularSpectrum.h"

#include <algorithm>

AngularSpectrum::AngularSpectrum(const AngularParameters& parameters) : mPar(parameters), mGrid(mPar.options.deviceIdx)
{
  const size_t zc = mPar.chunkPlanes, plane = mPar.ex * mPar.ey, nr = mPar.nReduced(), nd = mPar.nElements();
  auto constants = [&](size_t nz) {
    kw_constants k = gridConstants(mPar.ex, mPar.ey, nz);
    k.fft_divider   = 1.0f / static_cast<float>(plane); // no transform runs along z
    k.fft_divider_z = 1.0f;
    return k;
  };
  // fast path: a fused context of (Ex, Ey, Zc); otherwise the 2-D plans of (Ex, Ey, 1)
  const kw_constants planes2d = constants(1);
  if (mPar.fastPath) mGrid.setConstants(constants(zc));
  const bool fused = mGrid.choosePipeline(mPar.fastPath, &planes2d);

  mRe = mGrid.array(plane * zc);
  mIm = mGrid.array(plane * zc);
  mA  = mGrid.array(mPar.nPlane());
  mB  = mGrid.array(mPar.nPlane());
  mOutRe = mGrid.array(nd);
  mOutIm = mGrid.array(nd);
  mOut   = mGrid.array(nd);

  // the tables, once: float64 on the device, rounded once; the fast path reads them in the pipeline's plane layout
  mTab = static_cast<uint32_t*>(mGrid.bytes(5 * nr * sizeof(uint32_t)));
  size_t srcElems = nr;
  if (fused)
  {
    mGrid.check(kw_fused_angular_elems(context(), &srcElems));
    mTabImported = static_cast<uint32_t*>(mGrid.bytes(5 * srcElems * sizeof(uint32_t)));
  }
  else
  {
    mSpecRe = mGrid.array(2 * nr * zc);
    mSpecIm = mGrid.array(2 * nr * zc);
  }
  mSrcRe = mGrid.array(2 * srcElems);
  mSrcIm = mGrid.array(2 * srcElems);
  mGrid.check(kw_angular_operator(context(), mTab, mTabImported, mPar.dx, mPar.dy, mPar.k(), mPar.alphaNp, mPar.z0, mPar.dz,
                                  static_cast<uint32_t>(mPar.planes), mPar.restriction ? 1 : 0));
  mGrid.check(kw_sync(context()));
}

void AngularSpectrum::project()
{
  const uint32_t ex = static_cast<uint32_t>(mPar.ex), ey = static_cast<uint32_t>(mPar.ey);
  const uint32_t nx = static_cast<uint32_t>(mPar.nx), ny = static_cast<uint32_t>(mPar.ny);
  const size_t   zc = mPar.chunkPlanes, plane = mPar.ex * mPar.ey, nr = mPar.nReduced();
  for (size_t j0 = 0; j0 < mPar.planes; j0 += zc)
  {
    const size_t n = std::min(zc, mPar.planes - j0); // planes of this chunk that are kept
    if (mGrid.fused()) // the whole chunk is computed; planes past Nz are never extracted
      mGrid.check(kw_fused_angular_planes(context(), mSrcRe, mSrcIm, mTabImported, static_cast<uint32_t>(j0), mRe, mIm));
    else
    {
      mGrid.check(kw_angular_mix(context(), mSpecRe, mSpecIm, mSrcRe, mSrcIm, mTab, static_cast<uint32_t>(nr), static_cast<uint32_t>(n),
                                 static_cast<uint32_t>(j0), 1.0f / static_cast<float>(plane)));
      for (size_t z = 0; z < n; z++)
      {
        mGrid.check(kw_fft_c2r_3d(context(), mSpecRe + 2 * nr * z, mRe + plane * z));
        mGrid.check(kw_fft_c2r_3d(context(), mSpecIm + 2 * nr * z, mIm + plane * z));
      }
    }
    const size_t off = j0 * mPar.nPlane();
    mGrid.check(kw_cw_extract(context(), mRe, mIm, ex, ey, static_cast<uint32_t>(zc), nx, ny, static_cast<uint32_t>(n), mOutRe + off,
                              mOutIm + off, nullptr, nullptr, nullptr, nullptr, 0.0f));
  }
}

void AngularSpectrum::run(const float* a, const float* b, bool parts)
{
  const size_t np = mPar.nPlane();
  mGrid.check(kw_memcpy_h2d(context(), mA, a, np * sizeof(float)));
  mGrid.check(kw_memcpy_h2d(context(), mB, b, np * sizeof(float)));
  // the plane in the corner of plane 0; the fast path's x-forward reads whole tiles of rows, so the chunk is zero-filled
  const uint32_t ez = mGrid.fused() ? static_cast<uint32_t>(mPar.chunkPlanes) : 1u;
  mGrid.check(kw_cw_embed(context(), mRe, mIm, mA, mB, parts ? 1 : 0, 1.0f, 0.0f, static_cast<uint32_t>(mPar.ex),
                          static_cast<uint32_t>(mPar.ey), ez, static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny), 1u));
  if (mGrid.fused()) mGrid.check(kw_fused_angular_forward(context(), mRe, mIm, mSrcRe, mSrcIm));
  else
  {
    mGrid.check(kw_fft_r2c_3d(context(), mRe, mSrcRe));
    mGrid.check(kw_fft_r2c_3d(context(), mIm, mSrcIm));
  }
  project();
  mRuns++;
}

void AngularSpectrum::get(const std::string& name, float* dst, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for " + name);
  if (mRuns == 0) throw std::invalid_argument(name + ": no run yet");
  const uint32_t nx = static_cast<uint32_t>(mPar.nx), ny = static_cast<uint32_t>(mPar.ny), nz = static_cast<uint32_t>(mPar.planes);
  if (name == "re" || name == "im")
  {
    mGrid.check(kw_memcpy_d2h(context(), dst, name == "re" ? mOutRe : mOutIm, n * sizeof(float)));
    return;
  }
  float *amp = nullptr, *phase = nullptr;
  if (name == "amplitude") amp = mOut;
  else if (name == "phase") phase = mOut;
  else throw std::invalid_argument("no projector output named " + name + " (re, im, amplitude, phase)");
  mGrid.check(kw_cw_extract(context(), mOutRe, mOutIm, nx, ny, nz, nx, ny, nz, nullptr, nullptr, amp, phase, nullptr, nullptr, 0.0f));
  mGrid.check(kw_memcpy_d2h(context(), dst, mOut, n * sizeof(float)));
}

void AngularSpectrum::heat(const float* q, float qScalar, float* dst, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for Q");
  if (mRuns == 0) throw std::invalid_argument("Q: no run yet");
  const uint32_t nx = static_cast<uint32_t>(mPar.nx), ny = static_cast<uint32_t>(mPar.ny), nz = static_cast<uint32_t>(mPar.planes);
  if (q != nullptr)
  {
    if (mQ == nullptr) mQ = mGrid.array(n);
    mGrid.check(kw_memcpy_h2d(context(), mQ, q, n * sizeof(float)));
  }
  mGrid.check(kw_cw_extract(context(), mOutRe, mOutIm, nx, ny, nz, nx, ny, nz, nullptr, nullptr, nullptr, nullptr, mOut,
                            q != nullptr ? mQ : nullptr, qScalar));
  mGrid.check(kw_memcpy_d2h(context(), dst, mOut, n * sizeof(float)));
}
