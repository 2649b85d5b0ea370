// thermal_host_check.cpp — the host side of the bioheat solver as a stand-alone CPU program: the operator generators of
// host/ThermalParameters.cpp against values the test computed in NumPy float64, the default staggered conductivities, and
// every refusal of ThermalParameters::init.  Built with -fsanitize=address,undefined by tests/test_thermal_host.py together
// with host/ThermalParameters.cpp.  argv[1]: a file of doubles written by the test — nx ny nz dx dy dz dt dRef, then
// kappa_d and -|k|^2 kappa_d on the reduced grid.  Every case prints "<name>: ok ..." or "<name>: <message>".
#include <cmath>
#include <cstdio>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "InputProvider.h"
#include "ThermalParameters.h"

namespace {
using DT = InputProvider::DataType;

// ---- operators ----------------------------------------------------------------------------------------------------------
/// worst |got - expected| in units of the float32 spacing at `expected` (one rounding of the exact value: at most 0.5)
double worstUlp(const std::vector<float>& got, const double* expected)
{
  double worst = 0.0;
  for (size_t i = 0; i < got.size(); i++)
  {
    const double e = expected[i];
    int exp2 = 0;
    std::frexp(e, &exp2);
    const double ulp = (e == 0.0) ? 1e-300 : std::ldexp(1.0, exp2 - 24);
    worst = std::max(worst, std::fabs(static_cast<double>(got[i]) - e) / ulp);
  }
  return worst;
}

int operators(const char* path)
{
  std::FILE* f = std::fopen(path, "rb");
  if (f == nullptr) { std::printf("operators: cannot open %s\n", path); return 1; }
  double head[8];
  if (std::fread(head, sizeof(double), 8, f) != 8) { std::fclose(f); std::printf("operators: short file\n"); return 1; }
  const size_t nx = static_cast<size_t>(head[0]), ny = static_cast<size_t>(head[1]), nz = static_cast<size_t>(head[2]);
  const size_t nr = (nx / 2 + 1) * ny * nz;
  std::vector<double> want(2 * nr);
  const size_t got = std::fread(want.data(), sizeof(double), 2 * nr, f);
  std::fclose(f);
  if (got != 2 * nr) { std::printf("operators: short file\n"); return 1; }
  std::vector<float> kappaD(nr), laplacian(nr);
  ThermalOperators::generate(nx, ny, nz, head[3], head[4], head[5], head[6], head[7], kappaD.data(), laplacian.data());
  const double w0 = worstUlp(kappaD, want.data()), w1 = worstUlp(laplacian, want.data() + nr);
  // one rounding of the exact value is half a float32 spacing; the two float64 evaluations differ by far less than the margin
  std::printf("operators: %s kappa_d=%.3f laplacian=%.3f dc=%g,%g\n", (w0 <= 0.5 + 1e-6 && w1 <= 0.5 + 1e-6) ? "ok" : "outside one float32 rounding",
              w0, w1, kappaD[0], laplacian[0]);
  // derivative vectors: i k exp(+- i k d / 2); their product is -k^2
  std::vector<float> pos(2 * nx), neg(2 * nx);
  ThermalOperators::derivative(nx, nx, head[3], true, pos.data());
  ThermalOperators::derivative(nx, nx, head[3], false, neg.data());
  double worst = 0.0;
  for (size_t j = 0; j < nx; j++)
  {
    const double k  = ThermalOperators::wavenumber(j, nx, head[3]);
    const double re = static_cast<double>(pos[2 * j]) * neg[2 * j] - static_cast<double>(pos[2 * j + 1]) * neg[2 * j + 1];
    const double im = static_cast<double>(pos[2 * j]) * neg[2 * j + 1] + static_cast<double>(pos[2 * j + 1]) * neg[2 * j];
    if (k != 0.0) worst = std::max(worst, std::hypot(re + k * k, im) / (k * k));
  }
  std::printf("derivative: %s nyquist=%g\n", worst < 4e-7 ? "ok" : "product is not -k^2",
              ThermalOperators::wavenumber(nx / 2, nx, head[3]) * head[3] / M_PI); // an even side: the Nyquist bin is -pi / d
  return 0;
}

void staggered()
{ // K = 1 + linear index on a 2 x 3 x 2 grid: the sums with the +1 neighbour, the last point of an axis twice its own value
  const size_t nx = 2, ny = 3, nz = 2;
  std::vector<float> K(nx * ny * nz), out(K.size());
  for (size_t i = 0; i < K.size(); i++) K[i] = 1.0f + static_cast<float>(i);
  for (int axis = 0; axis < 3; axis++)
  {
    ThermalOperators::staggeredTwice(K.data(), nx, ny, nz, axis, out.data());
    std::string s;
    for (float v : out) s += (s.empty() ? "" : ",") + std::to_string(static_cast<int>(v));
    std::printf("staggered_%c: ok %s\n", "xyz"[axis], s.c_str());
  }
}

// ---- ThermalParameters::init --------------------------------------------------------------------------------------------
struct Problem
{
  std::vector<std::pair<std::string, size_t>> sizes = { {"Nx", 4}, {"Ny", 3}, {"Nz", 2} };
  std::vector<std::pair<std::string, std::vector<float>>> fields = {
    {"dx", {1e-3f}}, {"dy", {1e-3f}}, {"dz", {1e-3f}}, {"dt", {0.5f}}, {"T0", {37.f}},
    {"thermal_conductivity", std::vector<float>(24, 0.5f)}, {"density", {1000.f}}, {"specific_heat", std::vector<float>(24, 3600.f)},
    {"blood_density", {1060.f}}, {"blood_specific_heat", {3600.f}}, {"blood_perfusion_rate", {0.01f}},
    {"blood_ambient_temperature", {37.f}}, {"Q", std::vector<float>(24, 1e6f)} };
  std::vector<size_t> sensor = { 1, 24, 7 };
  ThermalOptions options;

  std::vector<float>& field(const std::string& name)
  {
    for (auto& f : fields) if (f.first == name) return f.second;
    fields.push_back({name, {}});
    return fields.back().second;
  }
  void drop(const std::string& name)
  {
    for (size_t i = 0; i < fields.size(); i++) if (fields[i].first == name) { fields.erase(fields.begin() + i); return; }
    for (size_t i = 0; i < sizes.size(); i++) if (sizes[i].first == name) { sizes.erase(sizes.begin() + i); return; }
  }
  void fill(MemoryInput& in) const
  {
    for (auto& s : sizes) in.add(s.first, &s.second, DT::kLong, DimensionSizes(1, 1, 1));
    for (auto& f : fields)
      in.add(f.first, f.second.data(), DT::kFloat, f.second.size() == 24 ? DimensionSizes(4, 3, 2) : DimensionSizes(f.second.size(), 1, 1));
    if (!sensor.empty()) in.add("sensor_mask_index", sensor.data(), DT::kLong, DimensionSizes(sensor.size(), 1, 1));
  }
};

void attempt(const char* name, const std::function<void(Problem&)>& change)
{
  Problem p;
  change(p);
  MemoryInput in;
  p.fill(in);
  ThermalParameters par;
  try
  {
    par.init(in, p.options);
    std::printf("%s: ok flux=%d a=%d P=%d Ta=%d Q=%d sensor=%zu a0=%.6g P0=%.6g dref=%.6g\n", name, int(par.fluxForm), int(par.a.isArray),
                int(par.P.isArray), int(par.Ta.isArray), int(par.hasQ), par.sensorIndex.size(),
                par.a.isArray ? par.a.data[0] : par.a.scalar, par.P.isArray ? par.P.data[0] : par.P.scalar, par.dRef);
  }
  catch (const std::exception& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}
} // namespace

int main(int argc, char** argv)
{
  if (argc < 2) { std::printf("usage: thermal_host_check <operators file>\n"); return 2; }
  if (operators(argv[1]) != 0) return 1;
  staggered();
  attempt("good", [](Problem&) {});
  attempt("scalar_k", [](Problem& p) { p.field("thermal_conductivity") = {0.5f}; p.drop("Q"); p.sensor.clear(); });
  attempt("no_perfusion", [](Problem& p) { for (auto n : {"blood_density", "blood_specific_heat", "blood_perfusion_rate", "blood_ambient_temperature"}) p.drop(n); });
  attempt("coeff", [](Problem& p) { for (auto n : {"blood_density", "blood_specific_heat", "blood_perfusion_rate"}) p.drop(n); p.field("perfusion_coeff") = {0.02f}; });
  attempt("ref", [](Problem& p) { p.field("diffusion_coeff_ref") = {2e-7f}; });
  for (auto n : {"Nx", "dz", "dt", "T0", "thermal_conductivity", "density", "specific_heat"})
    attempt((std::string("missing_") + n).c_str(), [n](Problem& p) { p.drop(n); });
  attempt("size_k", [](Problem& p) { p.field("thermal_conductivity") = std::vector<float>(12, 0.5f); });
  attempt("size_q", [](Problem& p) { p.field("Q") = std::vector<float>(23, 0.f); });
  attempt("size_t0", [](Problem& p) { p.field("T0") = std::vector<float>(2, 0.f); });
  attempt("density_zero", [](Problem& p) { p.field("density") = {0.f}; });
  attempt("heat_negative", [](Problem& p) { p.field("specific_heat")[5] = -1.f; });
  attempt("dt_zero", [](Problem& p) { p.field("dt") = {0.f}; });
  attempt("k_negative", [](Problem& p) { p.field("thermal_conductivity")[7] = -0.5f; });
  attempt("perfusion_negative", [](Problem& p) { p.field("blood_perfusion_rate") = {-0.01f}; });
  attempt("coeff_negative", [](Problem& p) { for (auto n : {"blood_density", "blood_specific_heat", "blood_perfusion_rate"}) p.drop(n); p.field("perfusion_coeff") = {-1.f}; });
  attempt("half_blood", [](Problem& p) { p.drop("blood_specific_heat"); });
  attempt("half_ambient", [](Problem& p) { p.drop("blood_ambient_temperature"); });
  attempt("lone_ambient", [](Problem& p) { for (auto n : {"blood_density", "blood_specific_heat", "blood_perfusion_rate"}) p.drop(n); });
  attempt("half_coeff", [](Problem& p) { for (auto n : {"blood_density", "blood_specific_heat", "blood_perfusion_rate", "blood_ambient_temperature"}) p.drop(n); p.field("perfusion_coeff") = {0.02f}; });
  attempt("both_forms", [](Problem& p) { p.field("perfusion_coeff") = {0.02f}; });
  attempt("two_d", [](Problem& p) { p.sizes[2].second = 1; });
  attempt("slab", [](Problem& p) { p.options.slabRanks = 2; });
  attempt("half_sg", [](Problem& p) { p.field("thermal_conductivity_sgx") = std::vector<float>(24, 0.5f); });
  attempt("sg_scalar_k", [](Problem& p) { p.field("thermal_conductivity") = {0.5f}; for (auto n : {"thermal_conductivity_sgx", "thermal_conductivity_sgy", "thermal_conductivity_sgz"}) p.field(n) = std::vector<float>(24, 0.5f); });
  attempt("sg_size", [](Problem& p) { for (auto n : {"thermal_conductivity_sgx", "thermal_conductivity_sgy", "thermal_conductivity_sgz"}) p.field(n) = std::vector<float>(24, 0.5f); p.field("thermal_conductivity_sgy") = {0.5f}; });
  attempt("sg_good", [](Problem& p) { for (auto n : {"thermal_conductivity_sgx", "thermal_conductivity_sgy", "thermal_conductivity_sgz"}) p.field(n) = std::vector<float>(24, 0.25f); });
  attempt("ref_zero", [](Problem& p) { p.field("diffusion_coeff_ref") = {0.f}; });
  attempt("sensor_high", [](Problem& p) { p.sensor[1] = 25; });
  attempt("sensor_zero", [](Problem& p) { p.sensor[0] = 0; });
  return 0;
}
