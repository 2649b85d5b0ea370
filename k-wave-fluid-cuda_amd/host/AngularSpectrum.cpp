// AngularSpectrum.cpp — the host side of the angular-spectrum projector around the device library's kw_angular_* and
// kw_fused_angular_* entry points.
#include "AngularSpectrum.h"

#include <algorithm>
#include <new>

void AngularSpectrum::check(kw_status s) const
{
  if (s == KW_OK) return;
  if (s == KW_ERR_ALLOC) throw std::bad_alloc();
  throw CwDeviceError(s, kw_last_error());
}

AngularSpectrum::AngularSpectrum(const AngularParameters& parameters) : mPar(parameters)
{
  check(kw_init(mPar.options.deviceIdx, &mCtx));
  try
  {
    const size_t zc = mPar.chunkPlanes, plane = mPar.ex * mPar.ey, nr = mPar.nReduced(), nd = mPar.nElements();
    auto constants = [&](size_t nz) {
      kw_constants k{};
      k.nx = static_cast<uint32_t>(mPar.ex);
      k.ny = static_cast<uint32_t>(mPar.ey);
      k.nz = static_cast<uint32_t>(nz);
      k.n_elements = static_cast<uint32_t>(plane * nz);
      k.nx_complex = static_cast<uint32_t>(mPar.ex / 2 + 1);
      k.ny_complex = k.ny;
      k.nz_complex = k.nz;
      k.n_elements_complex = static_cast<uint32_t>(nr * nz);
      k.fft_divider   = 1.0f / static_cast<float>(plane); // no transform runs along z
      k.fft_divider_x = 1.0f / static_cast<float>(mPar.ex);
      k.fft_divider_y = 1.0f / static_cast<float>(mPar.ey);
      k.fft_divider_z = 1.0f;
      check(kw_set_constants(mCtx, &k));
    };
    // fast path: a fused context of (Ex, Ey, Zc); otherwise the 2-D plans of (Ex, Ey, 1)
    int fusedOk = 0;
    if (mPar.fastPath)
    {
      constants(zc);
      check(kw_fused_supported(mCtx, &fusedOk));
    }
    mFused = fusedOk != 0;
    if (mFused) check(kw_fused_create(mCtx));
    else
    {
      constants(1);
      check(kw_fft_create_plans_3d(mCtx));
    }

    mRe = deviceArray(plane * zc);
    mIm = deviceArray(plane * zc);
    mA  = deviceArray(mPar.nPlane());
    mB  = deviceArray(mPar.nPlane());
    mOutRe = deviceArray(nd);
    mOutIm = deviceArray(nd);
    mOut   = deviceArray(nd);

    // the tables, once: float64 on the device, rounded once; the fast path reads them in the pipeline's plane layout
    mTab = static_cast<uint32_t*>(deviceBytes(5 * nr * sizeof(uint32_t)));
    size_t srcElems = nr;
    if (mFused)
    {
      check(kw_fused_angular_elems(mCtx, &srcElems));
      mTabImported = static_cast<uint32_t*>(deviceBytes(5 * srcElems * sizeof(uint32_t)));
    }
    else
    {
      mSpecRe = deviceArray(2 * nr * zc);
      mSpecIm = deviceArray(2 * nr * zc);
    }
    mSrcRe = deviceArray(2 * srcElems);
    mSrcIm = deviceArray(2 * srcElems);
    check(kw_angular_operator(mCtx, mTab, mTabImported, mPar.dx, mPar.dy, mPar.k(), mPar.alphaNp, mPar.z0, mPar.dz,
                              static_cast<uint32_t>(mPar.planes), mPar.restriction ? 1 : 0));
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

AngularSpectrum::~AngularSpectrum()
{
  if (mCtx == nullptr) return;
  kw_sync(mCtx);
  for (void* p : mOwned) kw_free(mCtx, p);
  if (mFused) kw_fused_destroy(mCtx);
  kw_destroy(mCtx);
}

void* AngularSpectrum::deviceBytes(size_t bytes)
{
  void* d = nullptr;
  check(kw_malloc(mCtx, bytes, &d));
  mOwned.push_back(d);
  return d;
}

void AngularSpectrum::project()
{
  const uint32_t ex = static_cast<uint32_t>(mPar.ex), ey = static_cast<uint32_t>(mPar.ey);
  const uint32_t nx = static_cast<uint32_t>(mPar.nx), ny = static_cast<uint32_t>(mPar.ny);
  const size_t   zc = mPar.chunkPlanes, plane = mPar.ex * mPar.ey, nr = mPar.nReduced();
  for (size_t j0 = 0; j0 < mPar.planes; j0 += zc)
  {
    const size_t n = std::min(zc, mPar.planes - j0); // planes of this chunk that are kept
    if (mFused) // the whole chunk is computed; planes past Nz are never extracted
      check(kw_fused_angular_planes(mCtx, mSrcRe, mSrcIm, mTabImported, static_cast<uint32_t>(j0), mRe, mIm));
    else
    {
      check(kw_angular_mix(mCtx, mSpecRe, mSpecIm, mSrcRe, mSrcIm, mTab, static_cast<uint32_t>(nr), static_cast<uint32_t>(n),
                           static_cast<uint32_t>(j0), 1.0f / static_cast<float>(plane)));
      for (size_t z = 0; z < n; z++)
      {
        check(kw_fft_c2r_3d(mCtx, mSpecRe + 2 * nr * z, mRe + plane * z));
        check(kw_fft_c2r_3d(mCtx, mSpecIm + 2 * nr * z, mIm + plane * z));
      }
    }
    const size_t off = j0 * mPar.nPlane();
    check(kw_cw_extract(mCtx, mRe, mIm, ex, ey, static_cast<uint32_t>(zc), nx, ny, static_cast<uint32_t>(n), mOutRe + off,
                        mOutIm + off, nullptr, nullptr, nullptr, nullptr, 0.0f));
  }
}

void AngularSpectrum::run(const float* a, const float* b, bool parts)
{
  const size_t np = mPar.nPlane();
  check(kw_memcpy_h2d(mCtx, mA, a, np * sizeof(float)));
  check(kw_memcpy_h2d(mCtx, mB, b, np * sizeof(float)));
  // the plane in the corner of plane 0; the fast path's x-forward reads whole tiles of rows, so the chunk is zero-filled
  const uint32_t ez = mFused ? static_cast<uint32_t>(mPar.chunkPlanes) : 1u;
  check(kw_cw_embed(mCtx, mRe, mIm, mA, mB, parts ? 1 : 0, 1.0f, 0.0f, static_cast<uint32_t>(mPar.ex),
                    static_cast<uint32_t>(mPar.ey), ez, static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny), 1u));
  if (mFused) check(kw_fused_angular_forward(mCtx, mRe, mIm, mSrcRe, mSrcIm));
  else
  {
    check(kw_fft_r2c_3d(mCtx, mRe, mSrcRe));
    check(kw_fft_r2c_3d(mCtx, mIm, mSrcIm));
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
    check(kw_memcpy_d2h(mCtx, dst, name == "re" ? mOutRe : mOutIm, n * sizeof(float)));
    return;
  }
  float *amp = nullptr, *phase = nullptr;
  if (name == "amplitude") amp = mOut;
  else if (name == "phase") phase = mOut;
  else throw std::invalid_argument("no projector output named " + name + " (re, im, amplitude, phase)");
  check(kw_cw_extract(mCtx, mOutRe, mOutIm, nx, ny, nz, nx, ny, nz, nullptr, nullptr, amp, phase, nullptr, nullptr, 0.0f));
  check(kw_memcpy_d2h(mCtx, dst, mOut, n * sizeof(float)));
}

void AngularSpectrum::heat(const float* q, float qScalar, float* dst, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for Q");
  if (mRuns == 0) throw std::invalid_argument("Q: no run yet");
  const uint32_t nx = static_cast<uint32_t>(mPar.nx), ny = static_cast<uint32_t>(mPar.ny), nz = static_cast<uint32_t>(mPar.planes);
  if (q != nullptr)
  {
    if (mQ == nullptr) mQ = deviceArray(n);
    check(kw_memcpy_h2d(mCtx, mQ, q, n * sizeof(float)));
  }
  check(kw_cw_extract(mCtx, mOutRe, mOutIm, nx, ny, nz, nx, ny, nz, nullptr, nullptr, nullptr, nullptr, mOut,
                      q != nullptr ? mQ : nullptr, qScalar));
  check(kw_memcpy_d2h(mCtx, dst, mOut, n * sizeof(float)));
}
