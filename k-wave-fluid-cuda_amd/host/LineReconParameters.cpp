// LineReconParameters.cpp — validation of a batched k-space line reconstruction and its size rules (no device call).
#include "LineReconParameters.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

using namespace GridRule;

namespace
{
// the x lengths whose masked (partial last tile) x kernels are not built (csrc/kw_fused.hip has_partial_x_tiles): their
// tiles take 2 nl_x = 16 rows, and a row count that is no multiple of it goes to the rocFFT path
// (tests/test_line_recon_host.py compares this list with the source)
const size_t kNoPartialTiles[] = { 672, 700, 720, 756, 784, 800, 840, 864, 900, 960 };
const size_t kRowsPerTile = 16;
const long double kChunkBins = 536870912.0L; // 2^29 complex bins: 4 GiB of one scratch array
const size_t kChunkFramesMax = 65535;
} // namespace

void LineReconParameters::init(const DeviceOptions& opt)
{
  options = opt;
  checkSize(ny, "Ny", size_t(1) << 30);
  checkSize(nt, "Nt", size_t(1) << 30);
  checkSize(frames, "frames", size_t(1) << 31);
  checkPositive(dy, "dy", "spacing");
  checkPositive(dt, "dt", "time step");
  checkPositive(c0, "c0", "sound speed");
  if (interp != kLinear && interp != kNearest) refuse("interp", std::to_string(interp) + " is neither linear (0) nor nearest (1)");
  if (depth == 0) depth = nt;
  if (depth > nt) refuse("depth", std::to_string(depth) + " is above Nt = " + std::to_string(nt));

  if (ey == 0) ey = ny;
  if (ey < ny) refuse("Ey", std::to_string(ey) + " is below Ny = " + std::to_string(ny));
  if (ey >= (1ull << 31)) refuse("Ey", std::to_string(ey) + " is not a grid size");
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
  // One chunk: the pass along t addresses a frame's lines by 32-bit BYTE offsets, so the P Lt F bins of the pipeline's padded
  // rows (P = Ey/2 + 1 rounded up to 16, 8 bytes each) stay below 2^29 — which keeps the Ey Lt F points below 2^30 — and the
  // frame is a block index of that pass, at most 65535 (csrc/kw_fused_main.hip kw_fused_supported).  One rule for both paths.
  const size_t pitch = (ey / 2 + 1 + 15) / 16 * 16;
  const long double perFrame = static_cast<long double>(pitch) * static_cast<long double>(lt);
  if (perFrame >= kChunkBins)
    refuse("E", std::to_string(ey) + " x " + std::to_string(lt) + " points of one frame is not below 2^29 bins of " +
                  std::to_string(pitch) + " per row");
  const size_t cap = std::min(kChunkFramesMax, static_cast<size_t>((kChunkBins - 1.0L) / perFrame));
  if (chunkFrames == 0) chunkFrames = std::min(frames, cap);
  if (chunkFrames > frames) refuse("chunk_frames", std::to_string(chunkFrames) + " is above frames = " + std::to_string(frames));
  if (chunkFrames > kChunkFramesMax)
    refuse("chunk_frames", std::to_string(chunkFrames) + " is above " + std::to_string(kChunkFramesMax) + ", the most one chunk takes");
  if (chunkFrames > cap)
    refuse("chunk_frames", std::to_string(chunkFrames) + " frames of " + std::to_string(ey) + " x " + std::to_string(lt) +
                             " points is not below 2^29 bins of " + std::to_string(pitch) + " per row (at most " +
                             std::to_string(cap) + ")");
  const bool wholeTiles = std::find(std::begin(kNoPartialTiles), std::end(kNoPartialTiles), ey) == std::end(kNoPartialTiles) ||
                          (lt * chunkFrames) % kRowsPerTile == 0;
  fastPath = options.fusedKernels && isFastLength(ey) && isFastLength(lt) && wholeTiles;
}
