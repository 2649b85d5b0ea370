// device_grid_check.cpp — host/DeviceGrid.cpp as a stand-alone CPU program over a FAKE of the kw_* functions it calls (no
// device library, no GPU): what an operator's constructor and destructor do to the context, the pipeline and the device
// arrays on success and when the k-th call of one function fails.  Built with -fsanitize=address,undefined by
// tests/test_device_grid_host.py; the fake's "device memory" is malloc'ed, so a pointer freed twice or never is the
// sanitizer's finding as well as the log's.
// Every case prints "<name>: <outcome> | <the fake's call log>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "DeviceGrid.h"

struct kw_ctx
{
  void* fusedScratch = nullptr; // what kw_fused_create allocates, a failing one too
};

namespace fake {
std::vector<std::string> log;
std::map<std::string, int> calls;
std::map<void*, int> ids; // device pointers by the order of their allocation
int         nextId = 0;
std::string lastError;
std::string failFunction;
int         failAt = 0;
kw_status   failStatus = KW_OK;
int         fusedSupported = 1;
const size_t kReducedElems = 1234;

void reset(const std::string& function = "", int at = 0, kw_status status = KW_OK)
{
  log.clear();
  calls.clear();
  ids.clear();
  nextId = 0;
  failFunction = function;
  failAt = at;
  failStatus = status;
  fusedSupported = 1;
}

/// logs the call; the status the fake was told to give the k-th call of this function
kw_status call(const std::string& function, const std::string& what = "")
{
  log.push_back(function + what);
  if (function == failFunction && ++calls[function] == failAt)
  {
    lastError = "fake: " + function + " failed";
    log.back() += "!";
    return failStatus;
  }
  return KW_OK;
}

std::string id(const void* p)
{
  const auto it = ids.find(const_cast<void*>(p));
  return it == ids.end() ? "#?" : "#" + std::to_string(it->second);
}
} // namespace fake

extern "C" {
kw_status kw_init(int, kw_ctx** out)
{
  const kw_status s = fake::call("init");
  if (s == KW_OK) *out = new kw_ctx();
  return s;
}
kw_status kw_destroy(kw_ctx* ctx)
{
  fake::call("destroy", ctx == nullptr ? "(null)" : "");
  delete ctx;
  return KW_OK;
}
const char* kw_last_error(void) { return fake::lastError.c_str(); }
kw_status kw_sync(kw_ctx*) { return fake::call("sync"); }
kw_status kw_malloc(kw_ctx*, size_t bytes, void** out)
{
  const kw_status s = fake::call("malloc", "(" + std::to_string(bytes) + ")");
  if (s != KW_OK) return s;
  *out = std::malloc(bytes != 0 ? bytes : 1);
  fake::ids[*out] = fake::nextId++;
  fake::log.back() += fake::id(*out);
  return KW_OK;
}
kw_status kw_free(kw_ctx*, void* p)
{
  const kw_status s = fake::call("free", fake::id(p));
  fake::ids.erase(p); // (an address the allocator hands out again is a new pointer)
  std::free(p);
  return s;
}
kw_status kw_memcpy_h2d(kw_ctx*, void* dst, const void* src, size_t bytes)
{
  const kw_status s = fake::call("h2d", fake::id(dst));
  if (s == KW_OK) std::memcpy(dst, src, bytes);
  return s;
}
kw_status kw_set_constants(kw_ctx*, const kw_constants* k) { return fake::call("set_constants", "(" + std::to_string(k->nz) + ")"); }
kw_status kw_fused_supported(kw_ctx*, int* out)
{
  *out = fake::fusedSupported;
  return fake::call("fused_supported");
}
kw_status kw_fused_create(kw_ctx* ctx)
{
  ctx->fusedScratch = std::malloc(64); // left behind by a failing create as well: kw_fused_destroy frees it
  return fake::call("fused_create");
}
kw_status kw_fused_destroy(kw_ctx* ctx)
{
  std::free(ctx->fusedScratch);
  ctx->fusedScratch = nullptr;
  return fake::call("fused_destroy");
}
kw_status kw_fft_create_plans_3d(kw_ctx*) { return fake::call("plans_3d"); }
kw_status kw_fused_reduced_elems(kw_ctx*, size_t* out)
{
  *out = fake::kReducedElems;
  return fake::call("reduced_elems");
}
kw_status kw_fused_import_reduced(kw_ctx*, float* dst, const float* src)
{
  return fake::call("import", fake::id(dst) + "<-" + fake::id(src));
}
}

namespace {

/// an operator as the five host classes are built: the grid as a member, everything else in the constructor's body
struct Operator
{
  DeviceGrid grid;
  float*     arrays[5] = {};
  explicit Operator(bool wantFused, const kw_constants* unfused = nullptr) : grid(0)
  {
    grid.setConstants(gridConstants(16, 32, 48));
    grid.choosePipeline(wantFused, unfused);
    for (int i = 0; i < 5; i++) arrays[i] = grid.array(100 * (i + 1));
  }
};

template <class Body> void run(const char* name, Body body)
{
  std::string outcome;
  try
  {
    outcome = body();
  }
  catch (const std::bad_alloc&) { outcome = "bad_alloc"; }
  catch (const DeviceError& e) { outcome = "DeviceError " + std::to_string(static_cast<int>(e.status)) + " " + e.what(); }
  catch (const std::exception& e) { outcome = std::string("exception ") + e.what(); }
  std::string line;
  for (const std::string& entry : fake::log) line += " " + entry;
  std::printf("%s: %s |%s\n", name, outcome.c_str(), line.c_str());
}

std::string constantsCase()
{
  const kw_constants k = gridConstants(16, 32, 48);
  const float want[4] = { 1.0f / 24576.0f, 1.0f / 16.0f, 1.0f / 32.0f, 1.0f / 48.0f };
  const float got[4]  = { k.fft_divider, k.fft_divider_x, k.fft_divider_y, k.fft_divider_z };
  kw_constants rest = k, zero;
  std::memset(&zero, 0, sizeof zero);
  rest.nx = rest.ny = rest.nz = rest.n_elements = 0;
  rest.nx_complex = rest.ny_complex = rest.nz_complex = rest.n_elements_complex = 0;
  rest.fft_divider = rest.fft_divider_x = rest.fft_divider_y = rest.fft_divider_z = 0.0f;
  char text[256];
  std::snprintf(text, sizeof text, "n=%ux%ux%u=%u complex=%ux%ux%u=%u dividers_bit_equal=%d others_zero=%d", k.nx, k.ny, k.nz,
                k.n_elements, k.nx_complex, k.ny_complex, k.nz_complex, k.n_elements_complex,
                std::memcmp(got, want, sizeof want) == 0 ? 1 : 0, std::memcmp(&rest, &zero, sizeof zero) == 0 ? 1 : 0);
  return text;
}
} // namespace

int main()
{
  fake::reset();
  run("success_fused", [] { Operator op(true); return std::string(op.grid.fused() ? "fused" : "rocfft"); });
  fake::reset();
  run("success_rocfft", [] { Operator op(false); return std::string(op.grid.fused() ? "fused" : "rocfft"); });
  fake::reset();
  run("unsupported", [] {
    fake::fusedSupported = 0;
    const kw_constants plane = gridConstants(16, 32, 1);
    Operator op(true, &plane);
    return std::string(op.grid.fused() ? "fused" : "rocfft");
  });
  fake::reset("init", 1, KW_ERR_NO_DEVICE);
  run("init_fails", [] { Operator op(true); return std::string("built"); });
  for (int k = 1; k <= 5; k++)
  {
    fake::reset("malloc", k, KW_ERR_ALLOC);
    run(("malloc_" + std::to_string(k) + "_fails").c_str(), [] { Operator op(true); return std::string("built"); });
  }
  fake::reset("fused_create", 1, KW_ERR_HIP);
  run("fused_create_fails", [] { Operator op(true); return std::string("built"); });
  fake::reset("set_constants", 1, KW_ERR_INVALID);
  run("set_constants_fails", [] { Operator op(true); return std::string("built"); });
  fake::reset();
  run("release", [] {
    DeviceGrid grid(0);
    float* p = grid.array(10);
    grid.array(20);
    grid.release(p);
    fake::log.push_back("released");
    return std::string("ok");
  });
  fake::reset();
  run("import_reduced", [] {
    DeviceGrid grid(0);
    grid.setConstants(gridConstants(16, 32, 48));
    grid.choosePipeline(true);
    grid.importReduced(grid.upload(std::vector<float>{ 1.0f, 2.0f, 3.0f }));
    return std::string("ok");
  });
  fake::reset();
  run("grid_constants", constantsCase);
  return 0;
}
