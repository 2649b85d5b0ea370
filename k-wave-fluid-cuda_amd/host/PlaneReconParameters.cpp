// PlaneReconParameters.cpp — validation of a k-space plane reconstruction and its size rules (no device call).
#include "PlaneReconParameters.h"

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
  if (n >= (1ull << 30)) refuse(name, std::to_string(n) + " is not a grid size");
}

void checkPositive(double v, const char* name, const char* unit)
{
  if (!(v > 0.0) || !std::isfinite(v)) refuse(name, std::to_string(v) + " is not a positive " + unit);
}
} // namespace

void PlaneReconParameters::init(const AngularOptions& opt)
{
  options = opt;
  checkSize(nx, "Nx");
  checkSize(ny, "Ny");
  checkSize(nt, "Nt");
  checkPositive(dx, "dx", "spacing");
  checkPositive(dy, "dy", "spacing");
  checkPositive(dt, "dt", "time step");
  checkPositive(c0, "c0", "sound speed");
  if (interp != kLinear && interp != kNearest) refuse("interp", std::to_string(interp) + " is neither linear (0) nor nearest (1)");
  if (planes == 0) planes = nt;
  if (planes > nt) refuse("planes", std::to_string(planes) + " is above Nt = " + std::to_string(nt));

  const size_t n[2]     = { nx, ny };
  size_t*      e[2]     = { &ex, &ey };
  const char*  names[2] = { "Ex", "Ey" };
  if (ex != 0 || ey != 0)
  {
    for (int a = 0; a < 2; a++)
    {
      if (*e[a] == 0) refuse(names[a], "missing while the other side of the expanded grid is given");
      if (*e[a] < n[a]) refuse(names[a], std::to_string(*e[a]) + " is below N = " + std::to_string(n[a]));
      if (*e[a] >= (1ull << 31)) refuse(names[a], std::to_string(*e[a]) + " is not a grid size");
    }
  }
  else { ex = nx; ey = ny; }
  const size_t least = 2 * nt - 1;
  if (lt != 0)
  {
    if (lt < least) refuse("Lt", std::to_string(lt) + " is below 2 Nt - 1 = " + std::to_string(least));
    if (lt >= (1ull << 31)) refuse("Lt", std::to_string(lt) + " is not a grid size");
  }
  else
  {
    const size_t fast = options.fusedKernels ? CwRule::nextFastLength(least) : 0;
    lt = fast != 0 ? fast : least;
  }
  // 32-bit element indices in the pipeline and in the FFT wrapper
  const long double total = static_cast<long double>(ex) * static_cast<long double>(ey) * static_cast<long double>(lt);
  if (total >= 4294967296.0L)
    refuse("E", std::to_string(ex) + " x " + std::to_string(ey) + " x " + std::to_string(lt) + " points is not below 2^32");
  fastPath = options.fusedKernels && CwRule::isFastLength(ex) && CwRule::isFastLength(ey) && CwRule::isFastLength(lt);
}
