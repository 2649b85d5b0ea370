// element_arrays_check.cpp — Parameters::init on in-memory inputs carrying weighted transducer arrays, as a stand-alone
// CPU program: built with -fsanitize=address,undefined by tests/test_velocity_elements_host.py together with
// host/Parameters.cpp and host/CompressHelper.cpp.  Every case prints "<name>: ok" (accepted) or "<name>: <message>"
// (refused); the test compares those lines.  No device: the few device-library symbols Parameters.cpp refers to are
// stubbed below and never reached (init() does not select a device).
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "InputProvider.h"
#include "MatrixNames.h"
#include "Parameters.h"

extern "C" {
kw_status   kw_init(int, kw_ctx**) { return KW_ERR_INVALID; }
kw_status   kw_destroy(kw_ctx*) { return KW_OK; }
kw_status   kw_device_info_get(kw_ctx*, kw_device_info*) { return KW_ERR_INVALID; }
kw_status   kw_set_constants(kw_ctx*, const kw_constants*) { return KW_ERR_INVALID; }
const char* kw_last_error(void) { return "no device in this program"; }
}

namespace {
using DT = InputProvider::DataType;

struct Problem
{
  std::vector<std::pair<std::string, size_t>> scalarsU = {
    {"Nt", 30}, {"Nx", 8}, {"Ny", 8}, {"Nz", 8}, {"p_source_flag", 0}, {"p0_source_flag", 0}, {"transducer_source_flag", 0},
    {"ux_source_flag", 20}, {"uy_source_flag", 0}, {"uz_source_flag", 12}, {"nonuniform_grid_flag", 0}, {"absorbing_flag", 0},
    {"nonlinear_flag", 0}, {"u_source_mode", 2}, {"u_source_many", 1}};
  std::vector<std::pair<std::string, float>> scalarsF = {
    {"dt", 1e-7f}, {"dx", 1e-3f}, {"dy", 1e-3f}, {"dz", 1e-3f}, {"c_ref", 1500.f}, {"c0", 1500.f}, {"rho0", 1000.f},
    {"rho0_sgx", 1000.f}, {"rho0_sgy", 1000.f}, {"rho0_sgz", 1000.f}};
  // four source points, three elements; a sensor of two elements
  std::vector<size_t> uIndex = {10, 11, 70, 200}, ptr = {0, 2, 3, 3, 5}, col = {1, 3, 2, 1, 2}, sPtr = {0, 2, 3}, sCol = {5, 512, 77};
  std::vector<float>  weight = {.5f, .25f, 1.f, .75f, .1f}, sWeight = {1.f, 2.f, 3.f}, sx = std::vector<float>(20 * 3, 1.f),
                      sz = std::vector<float>(12 * 3, 2.f), plain = std::vector<float>(20 * 4, 0.f);
  size_t elementsX = 3, elementsZ = 3;
  size_t reportedPoints = 0, reportedEntries = 0; // > 0: the dataset reports this size (it is refused before any read)
  bool   withUy = false, withPlainUx = false, plainUy = false, withPtr = true, withTransducer = false;

  void fill(MemoryInput& in) const
  {
    for (auto& s : scalarsU) in.add(s.first, &s.second, DT::kLong, DimensionSizes(1, 1, 1));
    for (auto& s : scalarsF) in.add(s.first, &s.second, DT::kFloat, DimensionSizes(1, 1, 1));
    in.add("u_source_index", uIndex.data(), DT::kLong, DimensionSizes(reportedPoints ? reportedPoints : uIndex.size(), 1, 1));
    if (withPtr) in.add("u_source_element_ptr", ptr.data(), DT::kLong, DimensionSizes(ptr.size(), 1, 1));
    in.add("u_source_element_index", col.data(), DT::kLong, DimensionSizes(reportedEntries ? reportedEntries : col.size(), 1, 1));
    in.add("u_source_element_weight", weight.data(), DT::kFloat, DimensionSizes(reportedEntries ? reportedEntries : weight.size(), 1, 1));
    in.add("ux_source_element_input", sx.data(), DT::kFloat, DimensionSizes(elementsX, sx.size() / elementsX, 1));
    in.add("uz_source_element_input", sz.data(), DT::kFloat, DimensionSizes(elementsZ, sz.size() / elementsZ, 1));
    if (withUy) in.add("uy_source_element_input", sx.data(), DT::kFloat, DimensionSizes(3, 20, 1));
    if (withPlainUx) in.add("ux_source_input", plain.data(), DT::kFloat, DimensionSizes(4, 20, 1));
    if (withTransducer) in.add("transducer_source_input", plain.data(), DT::kFloat, DimensionSizes(plain.size(), 1, 1));
    if (plainUy) in.add("uy_source_input", plain.data(), DT::kFloat, DimensionSizes(4, 20, 1));
    in.add("sensor_element_ptr", sPtr.data(), DT::kLong, DimensionSizes(sPtr.size(), 1, 1));
    in.add("sensor_element_index", sCol.data(), DT::kLong, DimensionSizes(sCol.size(), 1, 1));
    in.add("sensor_element_weight", sWeight.data(), DT::kFloat, DimensionSizes(sWeight.size(), 1, 1));
  }
  size_t& scalar(const std::string& name)
  {
    for (auto& s : scalarsU)
      if (s.first == name) return s.second;
    scalarsU.emplace_back(name, 0);
    return scalarsU.back().second;
  }
};

void run(const char* name, const std::function<void(Problem&)>& edit)
{
  Problem p;
  edit(p);
  MemoryInput in;
  p.fill(in);
  Parameters::Options o;
  o.storeVelocityElements = o.storeVelocityNonStaggeredElements = true;
  std::unique_ptr<Parameters> params = Parameters::createDetached();
  try
  {
    params->init(in, o);
    std::printf("%s: ok E=%zu nnz=%zu sensor=%zu shifted=%d\n", name, params->getVelocitySourceElementCount(),
                params->getVelocitySourceElementNnz(), params->getSensorElementCount(), int(params->needsShiftedVelocity()));
  }
  catch (const std::exception& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}
} // namespace

int main()
{
  run("good", [](Problem&) {});
  run("flag0", [](Problem& p) { p.withUy = true; });
  run("both", [](Problem& p) { p.withPlainUx = true; });
  run("mixed", [](Problem& p) { p.scalar("uy_source_flag") = 20; p.plainUy = true; });
  run("many", [](Problem& p) { p.scalar("u_source_many") = 0; });
  run("elements", [](Problem& p) { p.elementsZ = 2; p.sz.resize(12 * 2); });
  run("transducer", [](Problem& p) { p.scalar("transducer_source_flag") = 5; p.withTransducer = true; });
  run("points", [](Problem& p) { p.reportedPoints = (size_t(1) << 32); });
  run("entries", [](Problem& p) { p.reportedEntries = (size_t(1) << 32); });
  run("monotone", [](Problem& p) { p.ptr = {0, 3, 2, 3, 5}; });
  run("last", [](Problem& p) { p.ptr = {0, 2, 3, 3, 4}; });
  run("column", [](Problem& p) { p.col[4] = 4; });
  run("zero", [](Problem& p) { p.col[0] = 0; });
  run("missing", [](Problem& p) { p.withPtr = false; });
  run("grid", [](Problem& p) { p.sCol[1] = 513; });
  return 0;
}
