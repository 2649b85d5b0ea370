// ThermalParameters.cpp — validation of a thermal problem and the host generators of its operators (no device call).
#include "ThermalParameters.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace
{
// (its own, not GridRule::refuse: this file is built alone by tests/test_thermal_host.py)
[[noreturn]] void refuse(const std::string& dataset, const std::string& what)
{
  throw std::invalid_argument(dataset + ": " + what);
}

void require(const InputProvider& in, const std::string& name)
{
  if (!in.datasetExists(name)) refuse(name, "required dataset is missing from the thermal input");
}

size_t readSize(const InputProvider& in, const std::string& name)
{
  require(in, name);
  if (in.getDatasetSize(name) != 1) refuse(name, "has " + std::to_string(in.getDatasetSize(name)) + " elements, expected 1");
  size_t v = 0;
  in.readScalarValue(name, v);
  if (v == 0) refuse(name, "0 is not a grid size");
  return v;
}

float readSpacing(const InputProvider& in, const std::string& name)
{
  require(in, name);
  if (in.getDatasetSize(name) != 1) refuse(name, "has " + std::to_string(in.getDatasetSize(name)) + " elements, expected 1");
  float v = 0.0f;
  in.readScalarValue(name, v);
  if (!(v > 0.0f)) refuse(name, std::to_string(v) + " is not positive");
  return v;
}

/// a dataset of 1 or n floats
std::vector<float> readField(const InputProvider& in, const std::string& name, size_t n)
{
  const size_t size = in.getDatasetSize(name);
  if (size != 1 && size != n)
    refuse(name, "has " + std::to_string(size) + " elements, expected 1 or Nx * Ny * Nz = " + std::to_string(n));
  std::vector<float> v(size);
  in.readFloat(name, v.data(), size);
  return v;
}

void checkPositive(const std::vector<float>& v, const std::string& name)
{
  for (size_t i = 0; i < v.size(); i++)
    if (!(v[i] > 0.0f)) refuse(name, "entry " + std::to_string(i) + " = " + std::to_string(v[i]) + " is not positive");
}

void checkNonNegative(const std::vector<float>& v, const std::string& name)
{
  for (size_t i = 0; i < v.size(); i++)
    if (!(v[i] >= 0.0f)) refuse(name, "entry " + std::to_string(i) + " = " + std::to_string(v[i]) + " is negative");
}

inline double at(const std::vector<float>& v, size_t i) { return static_cast<double>(v.size() == 1 ? v[0] : v[i]); }

ThermalCoefficient coefficient(size_t n, bool isArray, const std::vector<double>& values)
{
  ThermalCoefficient c;
  c.isArray = isArray;
  if (isArray)
  {
    c.data.resize(n);
    for (size_t i = 0; i < n; i++) c.data[i] = static_cast<float>(values[i]);
  }
  else c.scalar = static_cast<float>(values[0]);
  return c;
}
} // namespace

// ---------------------------------------------------------------------------------------------------------------------
// operators
// ---------------------------------------------------------------------------------------------------------------------
double ThermalOperators::wavenumber(size_t j, size_t n, double d)
{
  if (n == 1) return 0.0;
  const double idx = (j < (n + 1) / 2) ? static_cast<double>(j) : static_cast<double>(j) - static_cast<double>(n);
  return 2.0 * M_PI / (static_cast<double>(n) * d) * idx;
}

void ThermalOperators::generate(size_t nx, size_t ny, size_t nz, double dx, double dy, double dz, double dt, double dRef,
                                float* kappaD, float* laplacian)
{
  const size_t nxr = nx / 2 + 1;
  std::vector<double> kx2(nxr), ky2(ny), kz2(nz);
  for (size_t x = 0; x < nxr; x++) { const double k = wavenumber(x, nx, dx); kx2[x] = k * k; }
  for (size_t y = 0; y < ny; y++) { const double k = wavenumber(y, ny, dy); ky2[y] = k * k; }
  for (size_t z = 0; z < nz; z++) { const double k = wavenumber(z, nz, dz); kz2[z] = k * k; }
  for (size_t z = 0; z < nz; z++)
    for (size_t y = 0; y < ny; y++)
      for (size_t x = 0; x < nxr; x++)
      {
        const double k2 = kx2[x] + ky2[y] + kz2[z];
        const double e  = dRef * k2 * dt;
        const double kd = (e == 0.0) ? 1.0 : -std::expm1(-e) / e;
        const size_t i  = (z * ny + y) * nxr + x;
        if (kappaD != nullptr) kappaD[i] = static_cast<float>(kd);
        if (laplacian != nullptr) laplacian[i] = static_cast<float>(-k2 * kd);
      }
}

void ThermalOperators::derivative(size_t n, size_t count, double d, bool positive, float* out)
{
  for (size_t j = 0; j < count; j++)
  {
    const double k     = wavenumber(j, n, d);
    const double phase = (positive ? 0.5 : -0.5) * k * d;
    out[2 * j]     = static_cast<float>(-k * std::sin(phase)); // i k (cos + i sin)
    out[2 * j + 1] = static_cast<float>(k * std::cos(phase));
  }
}

void ThermalOperators::staggeredTwice(const float* K, size_t nx, size_t ny, size_t nz, int axis, float* out)
{
  const size_t dims[3]   = { nx, ny, nz };
  const size_t stride[3] = { 1, nx, nx * ny };
  for (size_t z = 0; z < nz; z++)
    for (size_t y = 0; y < ny; y++)
      for (size_t x = 0; x < nx; x++)
      {
        const size_t pos[3] = { x, y, z };
        const size_t i      = (z * ny + y) * nx + x;
        const bool   last   = pos[axis] + 1 == dims[axis];
        const double next   = last ? K[i] : K[i + stride[axis]];
        out[i] = static_cast<float>(static_cast<double>(K[i]) + next);
      }
}

// ---------------------------------------------------------------------------------------------------------------------
// input
// ---------------------------------------------------------------------------------------------------------------------
void ThermalParameters::init(const InputProvider& in, const ThermalOptions& opt)
{
  options = opt;
  if (opt.slabRanks > 1) refuse("slab_ranks", "Z-slab decomposition is not built for the thermal solver");
  nx = readSize(in, "Nx");
  ny = readSize(in, "Ny");
  nz = readSize(in, "Nz");
  if (nz == 1) refuse("Nz", "1 selects a 2-D simulation, which is not built for the thermal solver");
  dx = readSpacing(in, "dx");
  dy = readSpacing(in, "dy");
  dz = readSpacing(in, "dz");
  dt = readSpacing(in, "dt");
  const size_t n = nElements();

  for (const char* name : { "T0", "thermal_conductivity", "density", "specific_heat" }) require(in, name);
  const std::vector<float> t0 = readField(in, "T0", n);
  T0.assign(n, t0[0]);
  if (t0.size() == n) T0 = t0;
  const std::vector<float> K   = readField(in, "thermal_conductivity", n);
  const std::vector<float> rho = readField(in, "density", n);
  const std::vector<float> C   = readField(in, "specific_heat", n);
  checkNonNegative(K, "thermal_conductivity");
  checkPositive(rho, "density");
  checkPositive(C, "specific_heat");

  // a = 1 / (rho C)
  const bool aArray = rho.size() == n || C.size() == n;
  std::vector<double> aD(aArray ? n : 1);
  for (size_t i = 0; i < aD.size(); i++) aD[i] = 1.0 / (at(rho, i) * at(C, i));
  a = coefficient(n, aArray, aD);

  // perfusion: the four blood datasets, or perfusion_coeff with the ambient temperature, or nothing
  const char* blood[4] = { "blood_density", "blood_specific_heat", "blood_perfusion_rate", "blood_ambient_temperature" };
  const bool  coeff    = in.datasetExists("perfusion_coeff");
  int given = 0;
  for (int i = 0; i < 3; i++) given += in.datasetExists(blood[i]) ? 1 : 0;
  const bool ambient = in.datasetExists(blood[3]);
  if (coeff && given != 0)
  {
    for (int i = 0; i < 3; i++)
      if (in.datasetExists(blood[i])) refuse("perfusion_coeff", std::string("given together with ") + blood[i] + " (one form of the perfusion term only)");
  }
  if (coeff && !ambient) refuse(blood[3], "missing while perfusion_coeff is given");
  if (!coeff && (given != 0 || ambient) && !(given == 3 && ambient))
  {
    const char* present = ambient ? blood[3] : nullptr;
    for (int i = 0; i < 3; i++) if (in.datasetExists(blood[i])) present = blood[i];
    for (int i = 0; i < 4; i++)
      if (!in.datasetExists(blood[i]))
        refuse(blood[i], std::string("missing while ") + present + " is given (the perfusion term needs blood_density, blood_specific_heat, "
                         "blood_perfusion_rate and blood_ambient_temperature, or perfusion_coeff and blood_ambient_temperature)");
  }
  P  = ThermalCoefficient();
  Ta = ThermalCoefficient();
  if (coeff)
  {
    const std::vector<float> pc = readField(in, "perfusion_coeff", n);
    checkNonNegative(pc, "perfusion_coeff");
    std::vector<double> pD(pc.size());
    for (size_t i = 0; i < pc.size(); i++) pD[i] = pc[i];
    P = coefficient(n, pc.size() == n, pD);
  }
  else if (given == 3)
  {
    const std::vector<float> rb = readField(in, blood[0], n), cb = readField(in, blood[1], n), wb = readField(in, blood[2], n);
    checkNonNegative(rb, blood[0]);
    checkNonNegative(cb, blood[1]);
    checkNonNegative(wb, blood[2]);
    const bool pArray = aArray || rb.size() == n || cb.size() == n || wb.size() == n;
    std::vector<double> pD(pArray ? n : 1);
    for (size_t i = 0; i < pD.size(); i++) pD[i] = at(rb, i) * at(cb, i) * at(wb, i) * (aArray ? aD[i] : aD[0]);
    P = coefficient(n, pArray, pD);
  }
  if (ambient)
  {
    const std::vector<float> ta = readField(in, blood[3], n);
    std::vector<double> tD(ta.size());
    for (size_t i = 0; i < ta.size(); i++) tD[i] = ta[i];
    Ta = coefficient(n, ta.size() == n, tD);
  }

  // diffusion: Laplacian form for a scalar conductivity, flux form for an array
  fluxForm     = K.size() == n;
  conductivity = K[0];
  const char* sg[3] = { "thermal_conductivity_sgx", "thermal_conductivity_sgy", "thermal_conductivity_sgz" };
  int sgGiven = 0;
  for (int i = 0; i < 3; i++) sgGiven += in.datasetExists(sg[i]) ? 1 : 0;
  if (sgGiven != 0 && sgGiven != 3)
    for (int i = 0; i < 3; i++)
      if (!in.datasetExists(sg[i])) refuse(sg[i], "missing while another staggered conductivity is given (all three or none)");
  if (sgGiven == 3 && !fluxForm) refuse(sg[0], "given with a scalar thermal_conductivity (the Laplacian form has no staggered conductivity)");
  for (int i = 0; i < 3; i++) twoKsg[i].clear();
  if (fluxForm)
    for (int i = 0; i < 3; i++)
    {
      twoKsg[i].resize(n);
      if (sgGiven == 3)
      {
        if (in.getDatasetSize(sg[i]) != n)
          refuse(sg[i], "has " + std::to_string(in.getDatasetSize(sg[i])) + " elements, expected Nx * Ny * Nz = " + std::to_string(n));
        in.readFloat(sg[i], twoKsg[i].data(), n);
        checkNonNegative(twoKsg[i], sg[i]);
        for (float& v : twoKsg[i]) v *= 2.0f;
      }
      else ThermalOperators::staggeredTwice(K.data(), nx, ny, nz, i, twoKsg[i].data());
    }

  // D_ref = max K a
  dRef = 0.0;
  for (size_t i = 0; i < std::max(K.size(), aD.size()); i++) dRef = std::max(dRef, at(K, i) * (aArray ? aD[i] : aD[0]));
  if (in.datasetExists("diffusion_coeff_ref"))
  {
    const std::vector<float> ref = readField(in, "diffusion_coeff_ref", 1);
    if (!(ref[0] > 0.0f)) refuse("diffusion_coeff_ref", std::to_string(ref[0]) + " is not positive");
    dRef = ref[0];
  }

  hasQ = in.datasetExists("Q");
  Q.clear();
  if (hasQ)
  {
    const std::vector<float> q = readField(in, "Q", n);
    Q.assign(n, q[0]);
    if (q.size() == n) Q = q;
  }

  sensorIndex.clear();
  if (in.datasetExists("sensor_mask_index"))
  {
    const size_t ns = in.getDatasetSize("sensor_mask_index");
    std::vector<size_t> idx(ns);
    in.readIndex("sensor_mask_index", idx.data(), ns);
    sensorIndex.resize(ns);
    for (size_t i = 0; i < ns; i++)
    {
      if (idx[i] < 1 || idx[i] > n)
        refuse("sensor_mask_index", "entry " + std::to_string(i) + " = " + std::to_string(idx[i]) + " lies outside 1.." + std::to_string(n));
      sensorIndex[i] = idx[i] - 1;
    }
  }
}
