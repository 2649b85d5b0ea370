// SecondOrderParameters.cpp — validation of an exact k-space propagation and its size rules (no device call).
#include "SecondOrderParameters.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

using namespace GridRule;

void SecondOrderParameters::init(const DeviceOptions& opt)
{
  options = opt;
  checkSize(nx, "Nx");
  checkSize(ny, "Ny");
  checkSize(nz, "Nz");
  checkPositive(dx, "dx", "spacing");
  checkPositive(dy, "dy", "spacing");
  checkPositive(dz, "dz", "spacing");
  checkMedium();

  if (ex == 0 && ey == 0 && ez == 0)
  {
    checkPositive(tMax, "t_max", "time (the default expanded sides are sized by it)");
    const double reach = c0 * tMax;
    ex = reachSide(nx, dx, reach, options.fusedKernels);
    ey = reachSide(ny, dy, reach, options.fusedKernels);
    ez = reachSide(nz, dz, reach, options.fusedKernels);
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

  checkSensors(nDomain(), "domain");
  const size_t e[3] = { ex, ey, ez };
  const double d[3] = { dx, dy, dz };
  completeAbsorption(e, d, 3);
}

void SecondOrderParameters::checkPlane(int64_t plane) const
{
  if (plane < -1 || (plane >= 0 && static_cast<uint64_t>(plane) >= nz))
    refuse("plane", std::to_string(plane) + " is outside the domain's planes 0 ... " + std::to_string(nz - 1) + " (-1: no record)");
}

size_t SecondOrderParameters::planeChunkTimes(uint64_t given) const
{
  // G of one output time; the planes of one pass [given][Ey][Ex]
  return passTimes(given, planeSpectrumElems(1) * 2 * sizeof(float), ex * ey, "plane_chunk_times",
                   "planes of " + std::to_string(ex) + " x " + std::to_string(ey) + " points");
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
