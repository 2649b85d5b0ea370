// SecondOrderFramesParameters.h — input of the batched 2-D exact k-space propagator (SecondOrderFrames): F independent
// initial pressures p0[f][y][x] on a domain Nx x Ny that share the homogeneous medium, the expanded periodic plane, the
// sensor points and the aggregates wanted, validated and completed without touching a device (DESIGN.md "Exact k-space
// propagator on frames").  SecondOrderParameters' rules with the z axis removed, on the same base (SecondOrderRules):
//
//   default E_a (both given sides 0): needs t_max > 0 — the smallest fast-path line length of the fused pipeline at or above
//   M_a = N_a + ceil(c0 t_max / d_a); where an axis has none (above 1024) or with fusedKernels off, M_a itself.
//   Given sides: both, not below N_a, odd ones allowed; E = N is the periodic plane.  t_max is then not read.
//   tFree = min over x, y of (E_a - N_a) d_a / c0.  Later times are not refused.
//   absorption: SecondOrderParameters' a and B; alpha_coeff is refused when B is below 1/4 at the smallest non-zero or at
//   the largest |k| of the 2-D grid.
//   frames: 1 ... 65535 (the frame is a block index of the fused pass; no chunks of frames in this version), and
//   Ex Ey frames < 2^32.  sensor_index: flat indices into one plane [Ny][Nx], applied to every frame.
//   The line-sensor record (SecondOrderFrames::lineRecord): line_row: -1 (off) or a row 0 ... Ny - 1 of the plane;
//   line_chunk_times: how many output times one pass of the record takes — 0: as many as keep G [F][times][Ex/2 + 1] within
//   kLineBudgetBytes, one at the least; given: Ex F times < 2^32 (the rows' 32-bit indices) and at most kLineTimesMost.
// A refusal names the parameter.
#ifndef KW_HOST_SECOND_ORDER_FRAMES_PARAMETERS_H
#define KW_HOST_SECOND_ORDER_FRAMES_PARAMETERS_H
#include <cstddef>
#include <cstdint>
#include <vector>

#include "GridRules.h"

class SecondOrderFramesParameters : public SecondOrderRules
{
 public:
  /// checks every parameter and fills in ex / ey where they are 0; throws std::invalid_argument naming the parameter
  void init(const DeviceOptions& options);

  size_t nx = 0, ny = 0;          ///< the domain of one frame; sensorIndex: flat indices into one plane [Ny][Nx]
  size_t frames = 0;              ///< F
  double dx = 0, dy = 0;          ///< [m]
  size_t ex = 0, ey = 0;          ///< expanded sides; both 0: by the rule

  size_t nPlane() const { return nx * ny; }
  size_t nDomain() const { return nx * ny * frames; }
  size_t nExpanded() const { return ex * ey * frames; }
  size_t nReduced() const { return (ex / 2 + 1) * ey * frames; }
  /// the sensor points of every frame as indices into the expanded batch [F][Ey][Ex], frame by frame
  std::vector<uint64_t> expandedSensorIndex() const;

  // ---- the line-sensor record: its sizes and the order of its chunks, after init() ----
  static constexpr size_t kLineBudgetBytes = kRecordBudgetBytes;    ///< of G in the default chunk
  static constexpr size_t kLineTimesMost   = kRecordTimesMost;      ///< the record kernel's time tiles are a block index
  using LineChunk = TimeChunk;                                       ///< output times first ... first + count - 1
  /// -1 or 0 ... Ny - 1; refuses "line_row"
  void   checkLineRow(int64_t row) const;
  /// the times of one pass: the default for 0, the given number otherwise; refuses "line_chunk_times"
  size_t lineChunkTimes(uint64_t given) const;
  /// n_times in passes of at most chunkTimes, in order; refuses "n_times" for 0
  static std::vector<LineChunk> lineChunks(size_t nTimes, size_t chunkTimes);
  /// complex values of Q [Ex/2 + 1][Ey/2 + 1][F] and of G [F][times][Ex/2 + 1]
  size_t lineElems() const { return (ex / 2 + 1) * (ey / 2 + 1) * frames; }
  size_t lineSpectrumElems(size_t times) const { return (ex / 2 + 1) * frames * times; }
  /// where time t of frame f stands in the record [F][n_times][Nx], in floats
  size_t lineOffset(size_t f, size_t t, size_t nTimes) const { return (f * nTimes + t) * nx; }
};
#endif
