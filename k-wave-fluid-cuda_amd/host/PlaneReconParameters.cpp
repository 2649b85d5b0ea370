// PlaneReconParameters.cpp — validation of a k-space plane reconstruction and its size rules (no device call).
#include "PlaneReconParameters.h"

#include <cmath>
#include <stdexcept>

using namespace GridRule;

void PlaneReconParameters::init(const DeviceOptions& opt)
{
  options = opt;
  checkSize(nx, "Nx", size_t(1) << 30);
  checkSize(ny, "Ny", size_t(1) << 30);
  checkSize(nt, "Nt", size_t(1) << 30);
  checkPositive(dx, "dx", "spacing");
  checkPositive(dy, "dy", "spacing");
  checkPositive(dt, "dt", "time step");
  checkPositive(c0, "c0", "sound speed");
  if (interp != kLinear && interp != kNearest) refuse("interp", std::to_string(interp) + " is neither linear (0) nor nearest (1)");
  if (planes == 0) planes = nt;
  if (planes > nt) refuse("planes", std::to_string(planes) + " is above Nt = " + std::to_string(nt));

  if (ex != 0 || ey != 0) checkGivenSides(nx, ny, ex, ey, false); // (odd sides too: the rocFFT twin takes any size)
  else { ex = nx; ey = ny; }
  const size_t least = 2 * nt - 1;
  if (lt != 0)
  {
    if (lt < least) refuse("Lt", std::to_string(lt) + " is below 2 Nt - 1 = " + std::to_string(least));
    if (lt >= (1ull << 31)) refuse("Lt", std::to_string(lt) + " is not a grid size");
  }
  else
  {
    const size_t fast = options.fusedKernels ? nextFastLength(least) : 0;
    lt = fast != 0 ? fast : least;
  }
  checkTotal(ex, ey, lt);
  fastPath = options.fusedKernels && isFastLength(ex) && isFastLength(ey) && isFastLength(lt);
}
