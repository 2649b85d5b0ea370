// element_delay_check.cpp — per-entry time delays of the weighted transducer arrays as a stand-alone CPU program: the
// regrouping of a delayed sensor (ElementCsr::regroup) and the create-time checks of the three delay datasets in
// Parameters::init.  Built with -fsanitize=address,undefined by tests/test_element_delays_host.py together with
// host/Parameters.cpp, host/CompressHelper.cpp and host/ElementGroups.cpp.  Every case prints "<name>: ok ..." or
// "<name>: <message>"; the test compares those lines.  No device: the few device-library symbols Parameters.cpp refers to
// are stubbed below and never reached.
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "ElementArrays.h"
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

std::string list(const std::vector<uint32_t>& v)
{
  std::string s;
  for (uint32_t x : v) s += (s.empty() ? "" : ",") + std::to_string(x);
  return s;
}

// ---- the regrouping ------------------------------------------------------------------------------------------------------
void regroup(const char* name, const std::vector<size_t>& ptr, const std::vector<size_t>& delays)
{
  const ElementGroups g = ElementCsr::regroup(ptr.data(), ptr.size() - 1, delays.data());
  std::printf("%s: ok order=%s gptr=%s gdelay=%s egp=%s chunks=%s\n", name, list(g.order).c_str(), list(g.groupPtr).c_str(),
              list(g.groupDelay).c_str(), list(g.elementGroupPtr).c_str(), list(g.chunkPtr).c_str());
}

void regroupLong()
{ // one row of 2500 entries: delay 1 for the even entries (1250: two chunks), 0 for the odd ones; then an empty row
  std::vector<size_t> ptr = {0, 2500, 2500}, delays(2500);
  for (size_t j = 0; j < delays.size(); j++) delays[j] = (j % 2 == 0) ? 1 : 0;
  const ElementGroups g = ElementCsr::regroup(ptr.data(), 2, delays.data());
  bool stable = g.order.size() == 2500;
  for (size_t j = 0; stable && j < 1250; j++) stable = g.order[j] == 2 * j + 1 && g.order[1250 + j] == 2 * j;
  std::printf("long: ok stable=%d gptr=%s gdelay=%s egp=%s chunks=%s\n", int(stable), list(g.groupPtr).c_str(),
              list(g.groupDelay).c_str(), list(g.elementGroupPtr).c_str(), list(g.chunkPtr).c_str());
}

// ---- Parameters::init ------------------------------------------------------------------------------------------------------
struct Problem
{
  std::vector<std::pair<std::string, size_t>> scalarsU = {
    {"Nt", 30}, {"Nx", 8}, {"Ny", 8}, {"Nz", 8}, {"p_source_flag", 10}, {"p0_source_flag", 0}, {"transducer_source_flag", 0},
    {"ux_source_flag", 20}, {"uy_source_flag", 0}, {"uz_source_flag", 12}, {"nonuniform_grid_flag", 0}, {"absorbing_flag", 0},
    {"nonlinear_flag", 0}, {"u_source_mode", 2}, {"u_source_many", 1}, {"p_source_mode", 0}, {"p_source_many", 1}};
  std::vector<std::pair<std::string, float>> scalarsF = {
    {"dt", 1e-7f}, {"dx", 1e-3f}, {"dy", 1e-3f}, {"dz", 1e-3f}, {"c_ref", 1500.f}, {"c0", 1500.f}, {"rho0", 1000.f},
    {"rho0_sgx", 1000.f}, {"rho0_sgy", 1000.f}, {"rho0_sgz", 1000.f}};
  // four source points and three elements for the pressure and the velocity alike; a sensor of two elements
  std::vector<size_t> index = {10, 11, 70, 200}, ptr = {0, 2, 3, 3, 5}, col = {1, 3, 2, 1, 2}, sPtr = {0, 2, 3}, sCol = {5, 512, 77};
  std::vector<size_t> pDelay = {0, 4, 2, 1, 3}, uDelay = {7, 0, 0, 2, 1}, sDelay = {6, 0, 3};
  std::vector<float>  weight = {.5f, .25f, 1.f, .75f, .1f}, sWeight = {1.f, 2.f, 3.f}, sp = std::vector<float>(10 * 3, 1.f),
                      sx = std::vector<float>(20 * 3, 1.f), sz = std::vector<float>(12 * 3, 2.f),
                      plain = std::vector<float>(20 * 4, 0.f);
  std::vector<std::pair<std::string, size_t>> horizons;
  bool pCsr = true, uCsr = true, sCsr = true, elements = true;

  void fill(MemoryInput& in) const
  {
    for (auto& s : scalarsU) in.add(s.first, &s.second, DT::kLong, DimensionSizes(1, 1, 1));
    for (auto& s : scalarsF) in.add(s.first, &s.second, DT::kFloat, DimensionSizes(1, 1, 1));
    for (auto& s : horizons) in.add(s.first, &s.second, DT::kLong, DimensionSizes(1, 1, 1));
    in.add("p_source_index", index.data(), DT::kLong, DimensionSizes(index.size(), 1, 1));
    in.add("u_source_index", index.data(), DT::kLong, DimensionSizes(index.size(), 1, 1));
    for (const char* q : {"p", "u"})
    {
      const std::string s = std::string(q) + "_source_element_";
      if (q[0] == 'p' ? pCsr : uCsr)
      {
        in.add(s + "ptr", ptr.data(), DT::kLong, DimensionSizes(ptr.size(), 1, 1));
        in.add(s + "index", col.data(), DT::kLong, DimensionSizes(col.size(), 1, 1));
        in.add(s + "weight", weight.data(), DT::kFloat, DimensionSizes(weight.size(), 1, 1));
      }
    }
    if (pCsr) in.add("p_source_element_input", sp.data(), DT::kFloat, DimensionSizes(3, 10, 1));
    else in.add("p_source_input", plain.data(), DT::kFloat, DimensionSizes(4, 10, 1));
    if (uCsr)
    {
      in.add("ux_source_element_input", sx.data(), DT::kFloat, DimensionSizes(3, 20, 1));
      in.add("uz_source_element_input", sz.data(), DT::kFloat, DimensionSizes(3, 12, 1));
    }
    else
    {
      in.add("ux_source_input", plain.data(), DT::kFloat, DimensionSizes(4, 20, 1));
      in.add("uz_source_input", plain.data(), DT::kFloat, DimensionSizes(4, 12, 1));
    }
    if (sCsr)
    {
      in.add("sensor_element_ptr", sPtr.data(), DT::kLong, DimensionSizes(sPtr.size(), 1, 1));
      in.add("sensor_element_index", sCol.data(), DT::kLong, DimensionSizes(sCol.size(), 1, 1));
      in.add("sensor_element_weight", sWeight.data(), DT::kFloat, DimensionSizes(sWeight.size(), 1, 1));
    }
    if (!pDelay.empty()) in.add("p_source_element_delay", pDelay.data(), DT::kLong, DimensionSizes(pDelay.size(), 1, 1));
    if (!uDelay.empty()) in.add("u_source_element_delay", uDelay.data(), DT::kLong, DimensionSizes(uDelay.size(), 1, 1));
    if (!sDelay.empty()) in.add("sensor_element_delay", sDelay.data(), DT::kLong, DimensionSizes(sDelay.size(), 1, 1));
  }
};

void run(const char* name, const std::function<void(Problem&)>& edit)
{
  Problem p;
  edit(p);
  MemoryInput in;
  p.fill(in);
  Parameters::Options o;
  o.storePressureElements = o.storeVelocityElements = p.elements;
  std::unique_ptr<Parameters> params = Parameters::createDetached();
  try
  {
    params->init(in, o);
    std::printf("%s: ok delayed=%d%d%d max=%zu,%zu,%zu length=%zu,%zu,%zu,%zu\n", name,
                int(params->getPressureSourceElementDelayFlag()), int(params->getVelocitySourceElementDelayFlag()),
                int(params->getSensorElementDelayFlag()), params->getPressureSourceElementMaxDelay(),
                params->getVelocitySourceElementMaxDelay(), params->getSensorElementMaxDelay(),
                params->getPressureSourceLength(), params->getVelocityXSourceLength(), params->getVelocityYSourceLength(),
                params->getVelocityZSourceLength());
  }
  catch (const std::exception& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}
} // namespace

int main()
{
  // rows: {d = 2, 0, 2, 0, 1}, empty, one group, every entry its own group
  regroup("mixed", {0, 5, 5, 8, 11}, {2, 0, 2, 0, 1, 4, 4, 4, 3, 2, 1});
  regroup("empty", {0, 0, 0}, {});
  regroupLong();

  run("good", [](Problem&) {});
  run("none", [](Problem& p) { p.pDelay.clear(); p.uDelay.clear(); p.sDelay.clear(); });
  run("capped", [](Problem& p) { p.uDelay[0] = 15; });                   // ux: 20 + 15 steps, capped by Nt = 30
  run("p_length", [](Problem& p) { p.pDelay.pop_back(); });
  run("u_length", [](Problem& p) { p.uDelay.push_back(0); });
  run("s_length", [](Problem& p) { p.sDelay.pop_back(); });
  run("p_high", [](Problem& p) { p.pDelay[1] = KW_ELEMENT_MAX_DELAY + 1; });
  run("u_high", [](Problem& p) { p.uDelay[4] = size_t(1) << 40; });
  run("s_high", [](Problem& p) { p.sDelay[2] = KW_ELEMENT_MAX_DELAY + 1; });
  run("s_top", [](Problem& p) { p.sDelay[2] = KW_ELEMENT_MAX_DELAY; });
  run("p_lone", [](Problem& p) { p.pCsr = false; });
  run("u_lone", [](Problem& p) { p.uCsr = false; });
  run("s_lone", [](Problem& p) { p.sCsr = false; p.elements = false; });
  run("s_unused", [](Problem& p) { p.elements = false; });              // the sensor CSR is there but no stream asks for it
  run("horizon", [](Problem& p) { p.horizons = {{"p_source_element_delay_max", 9}, {"u_source_element_delay_max", 8}}; });
  run("horizon_low", [](Problem& p) { p.horizons = {{"p_source_element_delay_max", 3}}; });
  run("horizon_lone", [](Problem& p) { p.uDelay.clear(); p.horizons = {{"u_source_element_delay_max", 8}}; });
  return 0;
}
