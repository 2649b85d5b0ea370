// CwParameters.cpp — validation of a CW propagation and the no-wrap-around rule for T and the expanded grid (no device call).
#include "CwParameters.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

using namespace GridRule;

namespace CwRule
{
size_t leastSide(size_t n, double d, double c0, double t) { return n + static_cast<size_t>(std::ceil(c0 * t / d)); }
} // namespace CwRule

void CwParameters::init(const DeviceOptions& opt)
{
  options = opt;
  checkSize(nx, "Nx");
  checkSize(ny, "Ny");
  checkSize(nz, "Nz");
  if (nz == 1) refuse("Nz", "1 selects a 2-D simulation, which is not built for the CW propagator");
  checkPositive(dx, "dx", "spacing");
  checkPositive(dy, "dy", "spacing");
  checkPositive(dz, "dz", "spacing");
  checkPositive(c0, "c0", "sound speed");
  checkPositive(f0, "f0", "frequency");
  const double nyquist = c0 / (2.0 * std::max(dx, std::max(dy, dz)));
  if (f0 > nyquist)
    refuse("f0", std::to_string(f0) + " Hz is above the grid's Nyquist frequency c0 / (2 max d) = " + std::to_string(nyquist) + " Hz");
  if (!std::isfinite(scaleRe) || !std::isfinite(scaleIm)) refuse("source_scale", "is not finite");

  if (t == 0.0)
  {
    const double lx = static_cast<double>(nx) * dx, ly = static_cast<double>(ny) * dy, lz = static_cast<double>(nz) * dz;
    t = std::sqrt(lx * lx + ly * ly + lz * lz) / c0;
  }
  else if (!(t > 0.0) || !std::isfinite(t)) refuse("T", std::to_string(t) + " is not a positive time");

  const size_t n[3]     = { nx, ny, nz };
  const double d[3]     = { dx, dy, dz };
  size_t*      e[3]     = { &ex, &ey, &ez };
  const char*  names[3] = { "Ex", "Ey", "Ez" };
  size_t       least[3];
  for (int a = 0; a < 3; a++)
  {
    const double cells = std::ceil(c0 * t / d[a]);
    if (!(cells < 2147483648.0)) refuse("T", std::to_string(t) + " s needs an expanded grid of more than 2^31 points along one axis");
    least[a] = CwRule::leastSide(n[a], d[a], c0, t);
  }
  const bool given = ex != 0 || ey != 0 || ez != 0;
  if (given)
  {
    for (int a = 0; a < 3; a++)
    {
      if (*e[a] == 0) refuse(names[a], "missing while another side of the expanded grid is given");
      if (*e[a] % 2 != 0) refuse(names[a], std::to_string(*e[a]) + " is odd (the real transforms need even sides)");
      if (*e[a] < least[a])
        refuse(names[a], std::to_string(*e[a]) + " is below N + ceil(c0 T / d) = " + std::to_string(least[a]) +
                             ": the periodic images would reach the domain by T");
    }
  }
  else
  {
    bool fast = options.fusedKernels;
    for (int a = 0; a < 3 && fast; a++) fast = nextFastLength(least[a]) != 0;
    for (int a = 0; a < 3; a++) *e[a] = fast ? nextFastLength(least[a]) : least[a] + least[a] % 2;
  }
  checkTotal(ex, ey, ez);
  fastPath = options.fusedKernels && isFastLength(ex) && isFastLength(ey) && isFastLength(ez);
}
