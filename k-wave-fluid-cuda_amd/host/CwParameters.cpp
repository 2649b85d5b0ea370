// CwParameters.cpp — validation of a CW propagation and the no-wrap-around rule for T and the expanded grid (no device call).
#include "CwParameters.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace
{
[[noreturn]] void refuse(const std::string& parameter, const std::string& what)
{
  throw std::invalid_argument(parameter + ": " + what);
}

// KW_FUSED_LENGTHS of csrc/kw_fused.hip, ascending
const size_t kFastLengths[] = { 16,  32,  48,  64,  72,  80,  96,  100, 108, 112, 120, 128, 140, 144, 160, 168,
                                180, 192, 196, 200, 216, 224, 240, 252, 256, 280, 288, 300, 320, 324, 336, 360,
                                384, 392, 400, 420, 432, 448, 480, 500, 504, 512, 540, 560, 576, 600, 640, 648,
                                672, 700, 720, 756, 768, 784, 800, 840, 864, 896, 900, 960, 1024 };

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

namespace CwRule
{
bool isFastLength(size_t n) { return std::binary_search(std::begin(kFastLengths), std::end(kFastLengths), n); }

size_t nextFastLength(size_t n)
{
  const size_t* p = std::lower_bound(std::begin(kFastLengths), std::end(kFastLengths), n);
  return p == std::end(kFastLengths) ? 0 : *p;
}

size_t leastSide(size_t n, double d, double c0, double t) { return n + static_cast<size_t>(std::ceil(c0 * t / d)); }
} // namespace CwRule

void CwParameters::init(const CwOptions& opt)
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
    for (int a = 0; a < 3 && fast; a++) fast = CwRule::nextFastLength(least[a]) != 0;
    for (int a = 0; a < 3; a++) *e[a] = fast ? CwRule::nextFastLength(least[a]) : least[a] + least[a] % 2;
  }
  // 32-bit element indices in the pipeline and in the FFT wrapper
  const long double total = static_cast<long double>(ex) * static_cast<long double>(ey) * static_cast<long double>(ez);
  if (total >= 4294967296.0L)
    refuse("E", std::to_string(ex) + " x " + std::to_string(ey) + " x " + std::to_string(ez) + " points is not below 2^32");
  fastPath = options.fusedKernels && CwRule::isFastLength(ex) && CwRule::isFastLength(ey) && CwRule::isFastLength(ez);
}
