// SecondOrderParameters.h — input of the exact k-space propagator (SecondOrder): an initial pressure p0[z][y][x] on a
// domain Nx x Ny x Nz, a homogeneous medium with optional power-law absorption, the expanded periodic grid, the sensor
// points and the aggregates wanted, validated and completed without touching a device (DESIGN.md "Exact k-space
// propagator").
//
//   default E_a (all three given sides 0): needs t_max > 0 — the smallest fast-path line length of the fused pipeline at or
//   above M_a = N_a + ceil(c0 t_max / d_a); where an axis has none (above 1024) or with fusedKernels off, M_a itself.
//   Given sides: all three, not below N_a, odd ones allowed; E = N is the periodic box.  t_max is then not read.
//   tFree = min_a (E_a - N_a) d_a / c0: up to that time the result inside the domain is the free-space one.  Later times
//   are not refused.
//   absorption: a = alpha_coeff 100 (1e-6 / 2 pi)^y / (20 log10 e) [Np (rad/s)^-y m^-1], the time loop's conversion in
//   float64; 0 <= y < 3, y != 1.  B = 1 - 2 g T - g^2 with g = a c0^y |k|^(y-1), T = tan(pi y / 2) (0 for y = 2) is concave
//   in |k|^(y-1), so its minimum over the grid's bins is at the smallest non-zero or at the largest |k|: alpha_coeff is
//   refused when B is below 1/4 at either.
//   The plane-sensor record (SecondOrder::planeRecord): plane: -1 (off) or a plane 0 ... Nz - 1 of the domain;
//   plane_chunk_times: how many output times one pass of the record takes — 0: as many as keep G [times][Ey][Ex/2 + 1] within
//   kRecordBudgetBytes, one at the least; given: Ex Ey times < 2^32 (the planes' 32-bit indices) and at most kRecordTimesMost.
// A refusal names the parameter.  The medium, the sensor points, the aggregates and the completed a, tFree, B, with
// checkTime, are SecondOrderRules (GridRules.h), shared with SecondOrderFramesParameters.
#ifndef KW_HOST_SECOND_ORDER_PARAMETERS_H
#define KW_HOST_SECOND_ORDER_PARAMETERS_H
#include <cstddef>
#include <cstdint>
#include <vector>

#include "GridRules.h"

class SecondOrderParameters : public SecondOrderRules
{
 public:
  /// checks every parameter and fills in ex / ey / ez where they are 0; throws std::invalid_argument naming the parameter
  void init(const DeviceOptions& options);

  size_t nx = 0, ny = 0, nz = 0;  ///< the domain; sensorIndex: flat indices into [Nz][Ny][Nx]
  double dx = 0, dy = 0, dz = 0;  ///< [m]
  size_t ex = 0, ey = 0, ez = 0;  ///< expanded sides; all 0: by the rule

  size_t nDomain() const { return nx * ny * nz; }
  size_t nExpanded() const { return ex * ey * ez; }
  size_t nReduced() const { return (ex / 2 + 1) * ey * ez; }
  /// the sensor points as indices into the expanded volume [Ez][Ey][Ex]
  std::vector<uint64_t> expandedSensorIndex() const;

  // ---- the plane-sensor record: its sizes and the order of its passes, after init() ----
  /// -1 or 0 ... Nz - 1; refuses "plane"
  void   checkPlane(int64_t plane) const;
  /// the times of one pass: the default for 0, the given number otherwise; refuses "plane_chunk_times"
  size_t planeChunkTimes(uint64_t given) const;
  /// n_times in passes of at most chunkTimes, in order; refuses "n_times" for 0
  static std::vector<TimeChunk> planeChunks(size_t nTimes, size_t chunkTimes) { return timeChunks(nTimes, chunkTimes, "plane_chunk_times"); }
  /// complex values of Q [Ey][Ex/2 + 1][Ez/2 + 1] and of G [times][Ey][Ex/2 + 1]
  size_t planeElems() const { return ey * (ex / 2 + 1) * (ez / 2 + 1); }
  size_t planeSpectrumElems(size_t times) const { return (ex / 2 + 1) * ey * times; }
  /// where time t stands in the record [n_times][Ny][Nx], in floats
  size_t planeOffset(size_t t) const { return t * ny * nx; }
};
#endif
