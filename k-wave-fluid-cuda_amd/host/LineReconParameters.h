// LineReconParameters.h — input of the batched k-space line reconstruction (LineRecon): F frames p[t][y] of a linear array,
// a homogeneous medium, the depth of the images, the interpolant, the expanded sensor axis, the length of the mirrored
// record and the frames per chunk, validated and completed without touching a device (DESIGN.md "k-space line
// reconstruction").  Public names follow k-Wave: y is the sensor axis, t is time, x is depth with x_j = j c0 dt.
//
//   default Ey: Ny.  A given Ey: not below Ny.
//   default Lt: as PlaneReconParameters — the smallest fast-path line length of the fused pipeline at or above 2 Nt - 1;
//   2 Nt - 1 itself (odd: k-Wave's grid) when there is none (above 1024) or with fusedKernels off.  A given Lt: not below it.
//   depth: 1 ... Nt image rows; 0: all Nt.
//   chunkFrames: the frames one context holds; 0: all frames, capped so that one chunk stays inside the index limits of
//   the pass along t: P Lt chunk < 2^29 bins (P = Ey/2 + 1 rounded up to 16: 4 GiB of spectrum) and at most 65535 frames.
//   The fused stage runs when Ey and Lt are fast-path lengths and the rows of one chunk make whole x tiles where Ey is one
//   of the lengths without masked x kernels; the rocFFT twin otherwise (any sizes, odd ones too).
// A refusal names the parameter.
#ifndef KW_HOST_LINE_RECON_PARAMETERS_H
#define KW_HOST_LINE_RECON_PARAMETERS_H
#include <cstddef>
#include <cstdint>
#include <string>

#include "GridRules.h"

class LineReconParameters
{
 public:
  enum Interp : int { kLinear = 0, kNearest = 1 };

  /// checks every parameter and fills in ey / lt / depth / chunkFrames where they are 0; throws std::invalid_argument naming the parameter
  void init(const DeviceOptions& options);

  DeviceOptions options;
  size_t ny = 0, nt = 0;          ///< one frame
  size_t frames = 0;              ///< F
  double dy = 0, dt = 0;          ///< [m], [s]
  double c0 = 0;                  ///< [m/s]
  size_t depth = 0;               ///< image rows; 0: Nt
  int    interp = kLinear;        ///< kLinear or kNearest
  bool   positivity = false;      ///< clamp the result at 0
  size_t ey = 0;                  ///< expanded sensor axis; 0: Ny
  size_t lt = 0;                  ///< length of the mirrored record; 0: by the rule
  size_t chunkFrames = 0;         ///< frames per chunk; 0: by the rule

  bool   fastPath = false;        ///< the frames context of one chunk is on the fused pipeline's fast path (and fusedKernels is on)
  double dx() const { return c0 * dt; }
  size_t nChunks() const { return (frames + chunkFrames - 1) / chunkFrames; }
  size_t nRecord() const { return ny * nt * frames; }
  size_t nResult() const { return ny * depth * frames; }
  size_t nExpandedChunk() const { return ey * lt * chunkFrames; }
  size_t nReducedChunk() const { return (ey / 2 + 1) * lt * chunkFrames; }
};
#endif
