// CwPropagator.cpp — the host side of the CW field propagator around the device library's kw_cw_* entry points.
#include "CwPropagator.h"

#include <new>

void CwPropagator::check(kw_status s) const
{
  if (s == KW_OK) return;
  if (s == KW_ERR_ALLOC) throw std::bad_alloc();
  throw CwDeviceError(s, kw_last_error());
}

CwPropagator::CwPropagator(const CwParameters& parameters) : mPar(parameters)
{
  check(kw_init(mPar.options.deviceIdx, &mCtx));
  try
  {
    const size_t ne = mPar.nExpanded(), nr = mPar.nReduced(), nd = mPar.nElements();
    kw_constants k{};
    k.nx = static_cast<uint32_t>(mPar.ex);
    k.ny = static_cast<uint32_t>(mPar.ey);
    k.nz = static_cast<uint32_t>(mPar.ez);
    k.n_elements = static_cast<uint32_t>(ne);
    k.nx_complex = static_cast<uint32_t>(mPar.ex / 2 + 1);
    k.ny_complex = k.ny;
    k.nz_complex = k.nz;
    k.n_elements_complex = static_cast<uint32_t>(nr);
    k.fft_divider   = 1.0f / static_cast<float>(ne);
    k.fft_divider_x = 1.0f / static_cast<float>(mPar.ex);
    k.fft_divider_y = 1.0f / static_cast<float>(mPar.ey);
    k.fft_divider_z = 1.0f / static_cast<float>(mPar.ez);
    check(kw_set_constants(mCtx, &k));

    int fusedOk = 0;
    if (mPar.options.fusedKernels) check(kw_fused_supported(mCtx, &fusedOk));
    mFused = fusedOk != 0;
    if (mFused) check(kw_fused_create(mCtx));
    else check(kw_fft_create_plans_3d(mCtx));

    mRe = deviceArray(ne);
    mIm = deviceArray(ne);
    mA  = deviceArray(nd);
    mB  = deviceArray(nd);
    mOut = deviceArray(nd);

    // the operator, once: float64 on the device, rounded once; the fast path reads it in the pipeline's own layout
    if (mFused)
    {
      size_t np = 0;
      check(kw_fused_reduced_elems(mCtx, &np));
      mGRe = deviceArray(np);
      mGIm = deviceArray(np);
    }
    const double twoPi = 2.0 * 3.14159265358979323846;
    float* gRe = deviceArray(nr);
    float* gIm = deviceArray(nr);
    check(kw_cw_operator(mCtx, gRe, gIm, mPar.c0, mPar.omega(), mPar.t, twoPi / (static_cast<double>(mPar.ex) * mPar.dx),
                         twoPi / (static_cast<double>(mPar.ey) * mPar.dy), twoPi / (static_cast<double>(mPar.ez) * mPar.dz)));
    if (mFused)
    {
      check(kw_fused_import_reduced(mCtx, mGRe, gRe));
      check(kw_fused_import_reduced(mCtx, mGIm, gIm));
      check(kw_sync(mCtx));
      for (float* g : { gIm, gRe })
      { // the reduced form is not needed again (the last two allocations)
        mOwned.pop_back();
        check(kw_free(mCtx, g));
      }
    }
    else
    {
      mGRe = gRe;
      mGIm = gIm;
      mSpecRe = deviceArray(2 * nr);
      mSpecIm = deviceArray(2 * nr);
    }
    check(kw_memset(mCtx, mRe, 0, ne * sizeof(float)));
    check(kw_memset(mCtx, mIm, 0, ne * sizeof(float)));
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

CwPropagator::~CwPropagator()
{
  if (mCtx == nullptr) return;
  kw_sync(mCtx);
  for (void* p : mOwned) kw_free(mCtx, p);
  if (mFused) kw_fused_destroy(mCtx);
  kw_destroy(mCtx);
}

float* CwPropagator::deviceArray(size_t nFloats)
{
  void* d = nullptr;
  check(kw_malloc(mCtx, nFloats * sizeof(float), &d));
  mOwned.push_back(d);
  return static_cast<float*>(d);
}

void CwPropagator::propagate()
{
  if (mFused)
  {
    check(kw_fused_cw_pair(mCtx, mRe, mIm, mGRe, mGIm));
    return;
  }
  check(kw_fft_r2c_3d(mCtx, mRe, mSpecRe));
  check(kw_fft_r2c_3d(mCtx, mIm, mSpecIm));
  check(kw_cw_mix(mCtx, mSpecRe, mSpecIm, mGRe, mGIm, mPar.nReduced()));
  check(kw_fft_c2r_3d(mCtx, mSpecRe, mRe));
  check(kw_fft_c2r_3d(mCtx, mSpecIm, mIm));
}

void CwPropagator::run(const float* a, const float* b, bool parts)
{
  const size_t nd = mPar.nElements();
  check(kw_memcpy_h2d(mCtx, mA, a, nd * sizeof(float)));
  check(kw_memcpy_h2d(mCtx, mB, b, nd * sizeof(float)));
  check(kw_cw_embed(mCtx, mRe, mIm, mA, mB, parts ? 1 : 0, static_cast<float>(mPar.scaleRe), static_cast<float>(mPar.scaleIm),
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
  check(kw_cw_extract(mCtx, mRe, mIm, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey),
                      static_cast<uint32_t>(mPar.ez), static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny),
                      static_cast<uint32_t>(mPar.nz), re, im, amp, phase, nullptr, nullptr, 0.0f));
  check(kw_memcpy_d2h(mCtx, dst, mOut, n * sizeof(float)));
}

void CwPropagator::heat(const float* q, float qScalar, float* dst, size_t n)
{
  if (n != mPar.nElements()) throw std::invalid_argument("size mismatch for Q");
  if (mRuns == 0) throw std::invalid_argument("Q: no run yet");
  if (q != nullptr)
  {
    if (mQ == nullptr) mQ = deviceArray(n);
    check(kw_memcpy_h2d(mCtx, mQ, q, n * sizeof(float)));
  }
  check(kw_cw_extract(mCtx, mRe, mIm, static_cast<uint32_t>(mPar.ex), static_cast<uint32_t>(mPar.ey),
                      static_cast<uint32_t>(mPar.ez), static_cast<uint32_t>(mPar.nx), static_cast<uint32_t>(mPar.ny),
                      static_cast<uint32_t>(mPar.nz), nullptr, nullptr, nullptr, nullptr, mOut, q != nullptr ? mQ : nullptr,
                      qScalar));
  check(kw_memcpy_d2h(mCtx, dst, mOut, n * sizeof(float)));
}
