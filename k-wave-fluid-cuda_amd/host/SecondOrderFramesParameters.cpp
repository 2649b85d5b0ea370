// SecondOrderFramesParameters.cpp — validation of a batched 2-D exact k-space propagation and its size rules (no device call).
#include "SecondOrderFramesParameters.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

using namespace GridRule;

namespace
{
const double kPi = 3.14159265358979323846;
const size_t kFramesMax = 65535; // the frame is a block index of the fused pass (csrc/kw_fused_main.hip kw_fused_supported)
} // namespace

void SecondOrderFramesParameters::init(const DeviceOptions& opt)
{
  options = opt;
  checkSize(nx, "Nx");
  checkSize(ny, "Ny");
  if (frames == 0) refuse("frames", "0 is not a number of frames");
  if (frames > kFramesMax)
    refuse("frames", std::to_string(frames) + " is above " + std::to_string(kFramesMax) + ", the most one batch takes");
  checkPositive(dx, "dx", "spacing");
  checkPositive(dy, "dy", "spacing");
  checkPositive(c0, "c0", "sound speed");
  if (!(alphaCoeff >= 0.0) || !std::isfinite(alphaCoeff))
    refuse("alpha_coeff", std::to_string(alphaCoeff) + " is not an absorption >= 0 in dB/(MHz^y cm)");
  if (!(alphaPower >= 0.0) || !(alphaPower < 3.0) || alphaPower == 1.0)
    refuse("alpha_power", std::to_string(alphaPower) + " is outside the power law's range 0 <= y < 3, y != 1");

  if (ex == 0 && ey == 0)
  {
    checkPositive(tMax, "t_max", "time (the default expanded sides are sized by it)");
    const double reach = c0 * tMax;
    ex = reachSide(nx, dx, reach, options.fusedKernels);
    ey = reachSide(ny, dy, reach, options.fusedKernels);
  }
  else checkGivenSides(nx, ny, ex, ey, false);
  checkTotal(ex, ey, frames);
  fastPath = options.fusedKernels && isFastLength(ex) && isFastLength(ey);
  tFree = std::min(static_cast<double>(ex - nx) * dx, static_cast<double>(ey - ny) * dy) / c0;

  const size_t n = nPlane();
  for (size_t i = 0; i < sensorIndex.size(); i++)
    if (sensorIndex[i] >= n)
      refuse("sensor_index", "sensor_index[" + std::to_string(i) + "] = " + std::to_string(sensorIndex[i]) +
                               " is outside the plane of " + std::to_string(n) + " points");

  a = powerLawNepers(alphaCoeff, alphaPower);
  bSmallest = bLargest = 1.0;
  if (a > 0.0)
  {
    const size_t e[2] = { ex, ey };
    const double d[2] = { dx, dy };
    double kSmallest = 0.0, k2Largest = 0.0;
    for (int i = 0; i < 2; i++)
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

std::vector<uint64_t> SecondOrderFramesParameters::expandedSensorIndex() const
{
  const size_t ns = sensorIndex.size();
  std::vector<uint64_t> out(ns * frames);
  for (size_t f = 0; f < frames; f++)
    for (size_t i = 0; i < ns; i++)
    {
      const uint64_t s = sensorIndex[i];
      out[f * ns + i] = (f * ey + s / nx) * ex + s % nx;
    }
  return out;
}

void SecondOrderFramesParameters::checkLineRow(int64_t row) const
{
  if (row < -1 || (row >= 0 && static_cast<uint64_t>(row) >= ny))
    refuse("line_row", std::to_string(row) + " is outside the plane's rows 0 ... " + std::to_string(ny - 1) + " (-1: no record)");
}

size_t SecondOrderFramesParameters::lineChunkTimes(uint64_t given) const
{
  const size_t perTime = lineSpectrumElems(1) * 2 * sizeof(float); // G of one output time
  if (given == 0) return std::min(kLineTimesMost, std::max<size_t>(1, kLineBudgetBytes / perTime));
  // the rows of one pass [F given][Ex] are indexed in 32 bits, as every batch here
  const bool rows = given <= (uint64_t(1) << 32) / (ex * frames) && ex * frames * given < (uint64_t(1) << 32);
  if (!rows || given > kLineTimesMost)
    refuse("line_chunk_times", std::to_string(given) + " times of " + std::to_string(frames) + " rows of " + std::to_string(ex) +
                                 " points are too many for one pass (2^32 points, " + std::to_string(kLineTimesMost) + " times)");
  return static_cast<size_t>(given);
}

std::vector<SecondOrderFramesParameters::LineChunk> SecondOrderFramesParameters::lineChunks(size_t nTimes, size_t chunkTimes)
{
  if (nTimes == 0) refuse("n_times", "0 is not a number of output times");
  if (chunkTimes == 0) refuse("line_chunk_times", "0 is not a number of output times");
  std::vector<LineChunk> out;
  for (size_t first = 0; first < nTimes; first += chunkTimes) out.push_back({ first, std::min(chunkTimes, nTimes - first) });
  return out;
}
