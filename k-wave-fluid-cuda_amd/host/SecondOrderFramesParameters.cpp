// SecondOrderFramesParameters.cpp — validation of a batched 2-D exact k-space propagation and its size rules (no device call).
#include "SecondOrderFramesParameters.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

using namespace GridRule;

namespace
{
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
  checkMedium();

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

  checkSensors(nPlane(), "plane");
  const size_t e[2] = { ex, ey };
  const double d[2] = { dx, dy };
  completeAbsorption(e, d, 2);
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
  // G of one output time; the rows of one pass [F given][Ex]
  return passTimes(given, lineSpectrumElems(1) * 2 * sizeof(float), ex * frames, "line_chunk_times",
                   std::to_string(frames) + " rows of " + std::to_string(ex) + " points");
}

std::vector<SecondOrderFramesParameters::LineChunk> SecondOrderFramesParameters::lineChunks(size_t nTimes, size_t chunkTimes)
{
  return timeChunks(nTimes, chunkTimes, "line_chunk_times");
}
