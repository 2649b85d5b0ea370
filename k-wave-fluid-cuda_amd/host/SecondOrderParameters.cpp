// SecondOrderParameters.cpp — validation of an exact k-space propagation and its size rules (no device call).
#include "SecondOrderParameters.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

using namespace GridRule;

namespace
{
const double kPi = 3.14159265358979323846;

// N + ceil(c0 t_max / d), and the fast-path length at or above it where there is one and it is wanted
size_t defaultSide(size_t n, double d, double reach, bool fusedKernels)
{
  const double cells = std::ceil(reach / d);
  if (!(cells < 4294967296.0)) refuse("t_max", "c0 t_max reaches over " + std::to_string(cells) + " grid points");
  const size_t m    = n + static_cast<size_t>(cells);
  const size_t fast = fusedKernels ? nextFastLength(m) : 0;
  return fast != 0 ? fast : m;
}
} // namespace

void SecondOrderParameters::checkTime(double t)
{
  if (!(t >= 0.0) || !std::isfinite(t)) refuse("t", std::to_string(t) + " is not a time >= 0");
}

double SecondOrderParameters::damping(double k) const
{
  if (!(a > 0.0) || !(k > 0.0)) return 1.0;
  const double T = alphaPower == 2.0 ? 0.0 : std::tan(kPi * alphaPower / 2.0);
  const double g = a * std::pow(c0, alphaPower) * std::pow(k, alphaPower - 1.0);
  return 1.0 - 2.0 * g * T - g * g;
}

void SecondOrderParameters::init(const DeviceOptions& opt)
{
  options = opt;
  checkSize(nx, "Nx");
  checkSize(ny, "Ny");
  checkSize(nz, "Nz");
  checkPositive(dx, "dx", "spacing");
  checkPositive(dy, "dy", "spacing");
  checkPositive(dz, "dz", "spacing");
  checkPositive(c0, "c0", "sound speed");
  if (!(alphaCoeff >= 0.0) || !std::isfinite(alphaCoeff))
    refuse("alpha_coeff", std::to_string(alphaCoeff) + " is not an absorption >= 0 in dB/(MHz^y cm)");
  if (!(alphaPower >= 0.0) || !(alphaPower < 3.0) || alphaPower == 1.0)
    refuse("alpha_power", std::to_string(alphaPower) + " is outside the power law's range 0 <= y < 3, y != 1");

  if (ex == 0 && ey == 0 && ez == 0)
  {
    checkPositive(tMax, "t_max", "time (the default expanded sides are sized by it)");
    const double reach = c0 * tMax;
    ex = defaultSide(nx, dx, reach, options.fusedKernels);
    ey = defaultSide(ny, dy, reach, options.fusedKernels);
    ez = defaultSide(nz, dz, reach, options.fusedKernels);
  }
  else
  {
    checkGivenSides(nx, ny, ex, ey, false);
    if (ez == 0) refuse("Ez", "missing while the other sides of the expanded grid are given");
    if (ez < nz) refuse("Ez", std::to_string(ez) + " is below N = " + std::to_string(nz));
    if (ez >= (1ull << 31)) refuse("Ez", std::to_string(ez) + " is not a grid size");
  }
  checkTotal(ex, ey, ez);
  fastPath = options.fusedKernels && isFastLength(ex) && isFastLength(ey) && isFastLength(ez);
  tFree = std::min({ static_cast<double>(ex - nx) * dx, static_cast<double>(ey - ny) * dy, static_cast<double>(ez - nz) * dz }) / c0;

  const size_t n = nDomain();
  for (size_t i = 0; i < sensorIndex.size(); i++)
    if (sensorIndex[i] >= n)
      refuse("sensor_index", "sensor_index[" + std::to_string(i) + "] = " + std::to_string(sensorIndex[i]) +
                               " is outside the domain of " + std::to_string(n) + " points");

  a = alphaCoeff * 100.0 * std::pow(1.0e-6 / (2.0 * kPi), alphaPower) / (20.0 * std::log10(std::exp(1.0)));
  bSmallest = bLargest = 1.0;
  if (a > 0.0)
  {
    const size_t e[3] = { ex, ey, ez };
    const double d[3] = { dx, dy, dz };
    double kSmallest = 0.0, k2Largest = 0.0;
    for (int i = 0; i < 3; i++)
    {
      const double dk = 2.0 * kPi / (static_cast<double>(e[i]) * d[i]);
      if (e[i] > 1 && (kSmallest == 0.0 || dk < kSmallest)) kSmallest = dk;
      const double kn = dk * static_cast<double>(e[i] / 2);
      k2Largest += kn * kn;
    }
    bSmallest = damping(kSmallest);
    bLargest  = damping(std::sqrt(k2Largest));
    const bool low = !(bSmallest >= 0.25);
    if (low || !(bLargest >= 0.25))
      refuse("alpha_coeff", std::to_string(alphaCoeff) + ": a mode of this grid is damped beyond B = 1/4 (B = " +
                              std::to_string(low ? bSmallest : bLargest) + " at the " + (low ? "smallest non-zero" : "largest") +
                              " |k|)");
  }
}

std::vector<uint64_t> SecondOrderParameters::expandedSensorIndex() const
{
  std::vector<uint64_t> out(sensorIndex.size());
  for (size_t i = 0; i < out.size(); i++)
  {
    const uint64_t s = sensorIndex[i];
    const uint64_t x = s % nx, y = (s / nx) % ny, z = s / (nx * ny);
    out[i] = (z * ey + y) * ex + x;
  }
  return out;
}
