// AngularParameters.cpp — validation of an angular-spectrum projection and its size rules (no device call).
#include "AngularParameters.h"

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

namespace AngularRule
{
size_t chunkPlanes(size_t ex, size_t ey, size_t planes)
{
  for (size_t zc : { size_t(64), size_t(48), size_t(32) })
    if (planes > zc - 16 && static_cast<long double>(16) * ex * ey * zc <= static_cast<long double>(kChunkBudget)) return zc;
  return 16;
}
} // namespace AngularRule

void AngularParameters::init(const AngularOptions& opt)
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
  const bool fastSides = options.fusedKernels && CwRule::isFastLength(ex) && CwRule::isFastLength(ey);
  if (chunkPlanes == 0) chunkPlanes = AngularRule::chunkPlanes(ex, ey, planes);
  else
  {
    if (chunkPlanes > AngularRule::kMaxPlanes) refuse("chunk_planes", std::to_string(chunkPlanes) + " is above 4096");
    if (fastSides && !CwRule::isFastLength(chunkPlanes))
      refuse("chunk_planes", std::to_string(chunkPlanes) + " is no fast-path length (16, 32, 48, 64 ...) on a fast-path grid");
  }
  // 32-bit element indices in the pipeline and in the FFT wrapper
  const long double total = static_cast<long double>(ex) * static_cast<long double>(ey) * static_cast<long double>(chunkPlanes);
  if (total >= 4294967296.0L)
    refuse("E", std::to_string(ex) + " x " + std::to_string(ey) + " x " + std::to_string(chunkPlanes) + " points per chunk is not below 2^32");
  fastPath = fastSides && CwRule::isFastLength(chunkPlanes);
}
