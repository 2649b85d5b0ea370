// PlaneReconParameters.h — input of the k-space plane reconstruction (PlaneRecon): the record p[t][y][x] of a planar sensor,
// a homogeneous medium, the number of output planes, the interpolant, the expanded sides and the length of the mirrored
// record, validated and completed without touching a device (DESIGN.md "k-space plane reconstruction").
//
//   default E: (Nx, Ny), k-Wave's choice.  Given sides: not below N.
//   default Lt: the smallest fast-path line length of the fused pipeline at or above 2 Nt - 1; 2 Nt - 1 itself (odd: k-Wave's
//   grid) when there is none (above 1024) or with fusedKernels off.  A given Lt: not below 2 Nt - 1.
//   planes: 1 ... Nt output planes z_j = j c0 dt; 0: all Nt.
//   The fused stage runs when Ex, Ey and Lt are all fast-path lengths; the rocFFT twin otherwise (any sizes, odd ones too).
// A refusal names the parameter.
#ifndef KW_HOST_PLANE_RECON_PARAMETERS_H
#define KW_HOST_PLANE_RECON_PARAMETERS_H
#include <cstddef>
#include <cstdint>
#include <string>

#include "AngularParameters.h"

class PlaneReconParameters
{
 public:
  enum Interp : int { kLinear = 0, kNearest = 1 };

  /// checks every parameter and fills in ex / ey / lt / planes where they are 0; throws std::invalid_argument naming the parameter
  void init(const DeviceOptions& options);

  DeviceOptions options;
  size_t nx = 0, ny = 0, nt = 0;  ///< the record
  double dx = 0, dy = 0, dt = 0;  ///< [m], [m], [s]
  double c0 = 0;                  ///< [m/s]
  size_t planes = 0;              ///< output planes; 0: Nt
  int    interp = kLinear;        ///< kLinear or kNearest
  bool   positivity = false;      ///< clamp the result at 0
  size_t ex = 0, ey = 0;          ///< expanded sides; both 0: (Nx, Ny)
  size_t lt = 0;                  ///< length of the mirrored record; 0: by the rule

  bool   fastPath = false;        ///< both sides and Lt are fast-path lengths (and fusedKernels is on)
  double dz() const { return c0 * dt; }
  size_t nRecord() const { return nx * ny * nt; }
  size_t nResult() const { return nx * ny * planes; }
  size_t nExpanded() const { return ex * ey * lt; }
  size_t nReduced() const { return (ex / 2 + 1) * ey * lt; }
};
#endif
