// AngularParameters.cpp — validation of an angular-spectrum projection and its size rules (no device call).
#include "AngularParameters.h"

#include <cmath>
#include <stdexcept>

using namespace GridRule;

namespace AngularRule
{
size_t chunkPlanes(size_t ex, size_t ey, size_t planes)
{
  for (size_t zc : { size_t(64), size_t(48), size_t(32) })
    if (planes > zc - 16 && static_cast<long double>(16) * ex * ey * zc <= static_cast<long double>(kChunkBudget)) return zc;
  return 16;
}
} // namespace AngularRule

void AngularParameters::init(const DeviceOptions& opt)
{
  options = opt;
  checkSize(nx, "Nx");
  checkSize(ny, "Ny");
  checkPositive(dx, "dx", "spacing");
  checkPositive(dy, "dy", "spacing");
  checkPositive(c0, "c0", "sound speed");
  checkPositive(f0, "f0", "frequency");
  if (!(z0 >= 0.0) || !std::isfinite(z0))
    refuse("z0", std::to_string(z0) + " is not a distance >= 0 (reverse projection is not built)");
  checkPositive(dz, "dz", "plane spacing");
  if (planes == 0) refuse("planes", "0 is not a number of planes");
  if (planes > AngularRule::kMaxPlanes)
    refuse("planes", std::to_string(planes) + " is above " + std::to_string(AngularRule::kMaxPlanes) +
                         " (the phase accumulator is specified up to plane index 4095)");
  if (!(alphaNp >= 0.0) || !std::isfinite(alphaNp)) refuse("alpha_np", std::to_string(alphaNp) + " is not an absorption >= 0 in Np/m");

  if (ex != 0 || ey != 0) checkGivenSides(nx, ny, ex, ey, true);
  else defaultDoubledSides(nx, ny, ex, ey, options.fusedKernels);
  const bool fastSides = options.fusedKernels && isFastLength(ex) && isFastLength(ey);
  if (chunkPlanes == 0) chunkPlanes = AngularRule::chunkPlanes(ex, ey, planes);
  else
  {
    if (chunkPlanes > AngularRule::kMaxPlanes) refuse("chunk_planes", std::to_string(chunkPlanes) + " is above 4096");
    if (fastSides && !isFastLength(chunkPlanes))
      refuse("chunk_planes", std::to_string(chunkPlanes) + " is no fast-path length (16, 32, 48, 64 ...) on a fast-path grid");
  }
  checkTotal(ex, ey, chunkPlanes, "points per chunk");
  fastPath = fastSides && isFastLength(chunkPlanes);
}
