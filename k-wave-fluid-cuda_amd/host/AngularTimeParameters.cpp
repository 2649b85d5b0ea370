// AngularTimeParameters.cpp — validation of a time-domain angular-spectrum projection and its size rules (no device call).
#include "AngularTimeParameters.h"

#include <cmath>
#include <stdexcept>

#include "CwParameters.h"

namespace
{
[[noreturn]] void refuse(const std::string& parameter, const std::string& what)
{
  throw std::invalid_argument(parameter + ": " + what);
}

void checkSize(size_t n, const char* name)
{
  if (n == 0) refuse(name, "0 is not a grid size");
  if (n >= (1ull << 31)) refuse(name, std::to_string(n) + " is not a grid size");
}

void checkPositive(double v, const char* name, const char* unit)
{
  if (!(v > 0.0) || !std::isfinite(v)) refuse(name, std::to_string(v) + " is not a positive " + unit);
}
} // namespace

void AngularTimeParameters::init(const AngularOptions& opt)
{
  options = opt;
  checkSize(nx, "Nx");
  checkSize(ny, "Ny");
  checkSize(nt, "Nt");
  checkPositive(dx, "dx", "spacing");
  checkPositive(dy, "dy", "spacing");
  checkPositive(dt, "dt", "time step");
  checkPositive(c0, "c0", "sound speed");
  if (!(alphaCoeff >= 0.0) || !std::isfinite(alphaCoeff))
    refuse("alpha_coeff", std::to_string(alphaCoeff) + " is not an absorption >= 0 in dB/(MHz^y cm)");
  if (!(alphaPower >= 0.0) || !std::isfinite(alphaPower)) refuse("alpha_power", std::to_string(alphaPower) + " is not a power >= 0");
  if (z.empty()) refuse("n_planes", "0 is not a number of planes");
  if (z.size() > AngularRule::kMaxPlanes)
    refuse("n_planes", std::to_string(z.size()) + " is above " + std::to_string(AngularRule::kMaxPlanes));
  for (size_t j = 0; j < z.size(); j++)
    if (!(z[j] >= 0.0) || !std::isfinite(z[j]))
      refuse("z", "z[" + std::to_string(j) + "] = " + std::to_string(z[j]) + " is not a distance >= 0 (reverse projection is not built)");

  const size_t n[2]     = { nx, ny };
  size_t*      e[2]     = { &ex, &ey };
  const char*  names[2] = { "Ex", "Ey" };
  if (ex != 0 || ey != 0)
  {
    for (int a = 0; a < 2; a++)
    {
      if (*e[a] == 0) refuse(names[a], "missing while the other side of the expanded grid is given");
      if (*e[a] % 2 != 0) refuse(names[a], std::to_string(*e[a]) + " is odd (the real transforms need even sides)");
      if (*e[a] < n[a]) refuse(names[a], std::to_string(*e[a]) + " is below N = " + std::to_string(n[a]));
      if (*e[a] >= (1ull << 31)) refuse(names[a], std::to_string(*e[a]) + " is not a grid size");
    }
  }
  else
  {
    bool fast = options.fusedKernels;
    for (int a = 0; a < 2 && fast; a++) fast = CwRule::nextFastLength(2 * n[a]) != 0;
    for (int a = 0; a < 2; a++) *e[a] = fast ? CwRule::nextFastLength(2 * n[a]) : 2 * n[a];
  }
  if (lt != 0)
  {
    if (lt % 2 != 0) refuse("Lt", std::to_string(lt) + " is odd (the Nyquist bin of the record is dropped: Lt is even)");
    if (lt < nt) refuse("Lt", std::to_string(lt) + " is below Nt = " + std::to_string(nt));
    if (lt >= (1ull << 31)) refuse("Lt", std::to_string(lt) + " is not a grid size");
  }
  else
  {
    const size_t fast = options.fusedKernels ? CwRule::nextFastLength(nt) : 0;
    lt = fast != 0 ? fast : nt + nt % 2;
  }
  // 32-bit element indices in the pipeline and in the FFT wrapper
  const long double total = static_cast<long double>(ex) * static_cast<long double>(ey) * static_cast<long double>(lt);
  if (total >= 4294967296.0L)
    refuse("E", std::to_string(ex) + " x " + std::to_string(ey) + " x " + std::to_string(lt) + " points is not below 2^32");
  fastPath = options.fusedKernels && CwRule::isFastLength(ex) && CwRule::isFastLength(ey) && CwRule::isFastLength(lt);
}

std::vector<double> AngularTimeParameters::akTable() const
{
  const double kPi = 3.14159265358979323846, kLog2e = 1.4426950408889634073599246810019;
  const double neperPerDb = std::log(10.0) / 20.0;
  std::vector<double> ak(lt / 2 + 1);
  for (size_t m = 0; m < ak.size(); m++)
  {
    const double f     = static_cast<double>(m) / (static_cast<double>(lt) * dt);
    const double alpha = alphaCoeff * std::pow(f * 1e-6, alphaPower) * 100.0 * neperPerDb;
    const double k     = 2.0 * kPi * f / c0;
    ak[m] = alpha * k * kLog2e;
  }
  return ak;
}
