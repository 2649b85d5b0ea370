// AngularTimeParameters.cpp — validation of a time-domain angular-spectrum projection and its size rules (no device call).
#include "AngularTimeParameters.h"

#include <cmath>
#include <stdexcept>

using namespace GridRule;

void AngularTimeParameters::init(const DeviceOptions& opt)
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

  if (ex != 0 || ey != 0) checkGivenSides(nx, ny, ex, ey, true);
  else defaultDoubledSides(nx, ny, ex, ey, options.fusedKernels);
  if (lt != 0)
  {
    if (lt % 2 != 0) refuse("Lt", std::to_string(lt) + " is odd (the Nyquist bin of the record is dropped: Lt is even)");
    if (lt < nt) refuse("Lt", std::to_string(lt) + " is below Nt = " + std::to_string(nt));
    if (lt >= (1ull << 31)) refuse("Lt", std::to_string(lt) + " is not a grid size");
  }
  else
  {
    const size_t fast = options.fusedKernels ? nextFastLength(nt) : 0;
    lt = fast != 0 ? fast : nt + nt % 2;
  }
  checkTotal(ex, ey, lt);
  fastPath = options.fusedKernels && isFastLength(ex) && isFastLength(ey) && isFastLength(lt);
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
