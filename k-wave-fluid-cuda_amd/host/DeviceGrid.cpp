// DeviceGrid.cpp — see DeviceGrid.h.
#include "DeviceGrid.h"

#include <algorithm>
#include <new>

kw_constants gridConstants(size_t nx, size_t ny, size_t nz)
{
  const size_t n = nx * ny * nz;
  kw_constants k{};
  k.nx = static_cast<uint32_t>(nx);
  k.ny = static_cast<uint32_t>(ny);
  k.nz = static_cast<uint32_t>(nz);
  k.n_elements = static_cast<uint32_t>(n);
  k.nx_complex = static_cast<uint32_t>(nx / 2 + 1);
  k.ny_complex = k.ny;
  k.nz_complex = k.nz;
  k.n_elements_complex = static_cast<uint32_t>((nx / 2 + 1) * ny * nz);
  k.fft_divider   = 1.0f / static_cast<float>(n);
  k.fft_divider_x = 1.0f / static_cast<float>(nx);
  k.fft_divider_y = 1.0f / static_cast<float>(ny);
  k.fft_divider_z = 1.0f / static_cast<float>(nz);
  return k;
}

DeviceGrid::DeviceGrid(int deviceIdx) { check(kw_init(deviceIdx, &mCtx)); }

DeviceGrid::~DeviceGrid()
{
  kw_sync(mCtx);
  for (void* p : mOwned) kw_free(mCtx, p);
  if (mFused) kw_fused_destroy(mCtx); // the pipeline's scratch and twiddles
  kw_destroy(mCtx);                   // the FFT plans go with the context
}

void DeviceGrid::check(kw_status s) const
{
  if (s == KW_OK) return;
  if (s == KW_ERR_ALLOC) throw std::bad_alloc();
  throw DeviceError(s, kw_last_error());
}

bool DeviceGrid::choosePipeline(bool wantFused, const kw_constants* unfusedConstants)
{
  int fusedOk = 0;
  if (wantFused) check(kw_fused_supported(mCtx, &fusedOk));
  mFused = fusedOk != 0;
  if (mFused) check(kw_fused_create(mCtx));
  else
  {
    if (unfusedConstants != nullptr) setConstants(*unfusedConstants);
    check(kw_fft_create_plans_3d(mCtx));
  }
  return mFused;
}

bool DeviceGrid::choosePipeline(bool wantFused, const std::function<void(bool)>& setMode, const std::function<void()>& makePlans)
{
  int fusedOk = 0;
  if (wantFused)
  {
    setMode(true);
    check(kw_fused_supported(mCtx, &fusedOk));
  }
  mFused = fusedOk != 0;
  if (mFused) check(kw_fused_create(mCtx));
  else
  {
    setMode(false);
    makePlans();
  }
  return mFused;
}

void* DeviceGrid::bytes(size_t nBytes)
{
  void* d = nullptr;
  check(kw_malloc(mCtx, nBytes, &d));
  mOwned.push_back(d);
  return d;
}

float* DeviceGrid::upload(const std::vector<float>& host)
{
  float* d = array(host.size());
  check(kw_memcpy_h2d(mCtx, d, host.data(), host.size() * sizeof(float)));
  return d;
}

void DeviceGrid::release(void* p)
{
  const auto it = std::find(mOwned.begin(), mOwned.end(), p);
  if (it == mOwned.end()) throw std::invalid_argument("DeviceGrid::release: not an owned pointer");
  mOwned.erase(it);
  check(kw_free(mCtx, p));
}

float* DeviceGrid::importReduced(const float* reducedDevice)
{
  size_t n = 0;
  check(kw_fused_reduced_elems(mCtx, &n));
  float* d = array(n);
  check(kw_fused_import_reduced(mCtx, d, reducedDevice));
  return d;
}
