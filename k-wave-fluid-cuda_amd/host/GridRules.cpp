// GridRules.cpp — see GridRules.h.
#include "GridRules.h"

#include <algorithm>
#include <cmath>
#include <iterator>
#include <stdexcept>

namespace
{
const double kPi = 3.14159265358979323846;

// KW_FUSED_LENGTHS of csrc/kw_fused.hip, ascending
const size_t kFastLengths[] = { 16,  32,  48,  64,  72,  80,  96,  100, 108, 112, 120, 128, 140, 144, 160, 168,
                                180, 192, 196, 200, 216, 224, 240, 252, 256, 280, 288, 300, 320, 324, 336, 360,
                                384, 392, 400, 420, 432, 448, 480, 500, 504, 512, 540, 560, 576, 600, 640, 648,
                                672, 700, 720, 756, 768, 784, 800, 840, 864, 896, 900, 960, 1024 };
} // namespace

namespace GridRule
{
void refuse(const std::string& parameter, const std::string& what) { throw std::invalid_argument(parameter + ": " + what); }

void checkSize(size_t n, const char* name, size_t limit)
{
  if (n == 0) refuse(name, "0 is not a grid size");
  if (n >= limit) refuse(name, std::to_string(n) + " is not a grid size");
}

void checkPositive(double v, const char* name, const char* unit)
{
  if (!(v > 0.0) || !std::isfinite(v)) refuse(name, std::to_string(v) + " is not a positive " + unit);
}

bool isFastLength(size_t n) { return std::binary_search(std::begin(kFastLengths), std::end(kFastLengths), n); }

size_t nextFastLength(size_t n)
{
  const size_t* p = std::lower_bound(std::begin(kFastLengths), std::end(kFastLengths), n);
  return p == std::end(kFastLengths) ? 0 : *p;
}

void checkTotal(size_t ex, size_t ey, size_t ez, const char* points)
{
  const long double total = static_cast<long double>(ex) * static_cast<long double>(ey) * static_cast<long double>(ez);
  if (total >= 4294967296.0L)
    refuse("E", std::to_string(ex) + " x " + std::to_string(ey) + " x " + std::to_string(ez) + " " + points + " is not below 2^32");
}

void checkGivenSides(size_t nx, size_t ny, size_t ex, size_t ey, bool requireEven)
{
  const size_t n[2] = { nx, ny }, e[2] = { ex, ey };
  const char*  names[2] = { "Ex", "Ey" };
  for (int a = 0; a < 2; a++)
  {
    if (e[a] == 0) refuse(names[a], "missing while the other side of the expanded grid is given");
    if (requireEven && e[a] % 2 != 0) refuse(names[a], std::to_string(e[a]) + " is odd (the real transforms need even sides)");
    if (e[a] < n[a]) refuse(names[a], std::to_string(e[a]) + " is below N = " + std::to_string(n[a]));
    if (e[a] >= (1ull << 31)) refuse(names[a], std::to_string(e[a]) + " is not a grid size");
  }
}

void defaultDoubledSides(size_t nx, size_t ny, size_t& ex, size_t& ey, bool fusedKernels)
{
  const bool fast = fusedKernels && nextFastLength(2 * nx) != 0 && nextFastLength(2 * ny) != 0;
  ex = fast ? nextFastLength(2 * nx) : 2 * nx;
  ey = fast ? nextFastLength(2 * ny) : 2 * ny;
}

size_t reachSide(size_t n, double d, double reach, bool fusedKernels)
{
  const double cells = std::ceil(reach / d);
  if (!(cells < 4294967296.0)) refuse("t_max", "c0 t_max reaches over " + std::to_string(cells) + " grid points");
  const size_t m    = n + static_cast<size_t>(cells);
  const size_t fast = fusedKernels ? nextFastLength(m) : 0;
  return fast != 0 ? fast : m;
}

double powerLawNepers(double alphaCoeff, double y)
{
  return alphaCoeff * 100.0 * std::pow(1.0e-6 / (2.0 * kPi), y) / (20.0 * std::log10(std::exp(1.0)));
}

double powerLawDamping(double a, double c0, double y, double k)
{
  if (!(a > 0.0) || !(k > 0.0)) return 1.0;
  const double T = y == 2.0 ? 0.0 : std::tan(kPi * y / 2.0);
  const double g = a * std::pow(c0, y) * std::pow(k, y - 1.0);
  return 1.0 - 2.0 * g * T - g * g;
}
} // namespace GridRule

using namespace GridRule;

void SecondOrderRules::checkTime(double t)
{
  if (!(t >= 0.0) || !std::isfinite(t)) refuse("t", std::to_string(t) + " is not a time >= 0");
}

size_t SecondOrderRules::passTimes(uint64_t given, size_t bytesPerTime, size_t pointsPerTime, const char* name, const std::string& of)
{
  if (given == 0) return std::min(kRecordTimesMost, std::max<size_t>(1, kRecordBudgetBytes / bytesPerTime));
  const bool rows = given <= (uint64_t(1) << 32) / pointsPerTime && pointsPerTime * given < (uint64_t(1) << 32);
  if (!rows || given > kRecordTimesMost)
    refuse(name, std::to_string(given) + " times of " + of + " are too many for one pass (2^32 points, " +
                   std::to_string(kRecordTimesMost) + " times)");
  return static_cast<size_t>(given);
}

std::vector<SecondOrderRules::TimeChunk> SecondOrderRules::timeChunks(size_t nTimes, size_t chunkTimes, const char* name)
{
  if (nTimes == 0) refuse("n_times", "0 is not a number of output times");
  if (chunkTimes == 0) refuse(name, "0 is not a number of output times");
  std::vector<TimeChunk> out;
  for (size_t first = 0; first < nTimes; first += chunkTimes) out.push_back({ first, std::min(chunkTimes, nTimes - first) });
  return out;
}

void SecondOrderRules::checkMedium() const
{
  checkPositive(c0, "c0", "sound speed");
  if (!(alphaCoeff >= 0.0) || !std::isfinite(alphaCoeff))
    refuse("alpha_coeff", std::to_string(alphaCoeff) + " is not an absorption >= 0 in dB/(MHz^y cm)");
  if (!(alphaPower >= 0.0) || !(alphaPower < 3.0) || alphaPower == 1.0)
    refuse("alpha_power", std::to_string(alphaPower) + " is outside the power law's range 0 <= y < 3, y != 1");
}

void SecondOrderRules::checkSensors(size_t points, const char* where) const
{
  for (size_t i = 0; i < sensorIndex.size(); i++)
    if (sensorIndex[i] >= points)
      refuse("sensor_index", "sensor_index[" + std::to_string(i) + "] = " + std::to_string(sensorIndex[i]) + " is outside the " +
                               where + " of " + std::to_string(points) + " points");
}

void SecondOrderRules::completeAbsorption(const size_t* e, const double* d, int axes)
{
  a = powerLawNepers(alphaCoeff, alphaPower);
  bSmallest = bLargest = 1.0;
  if (!(a > 0.0)) return;
  double kSmallest = 0.0, k2Largest = 0.0;
  for (int i = 0; i < axes; i++)
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
