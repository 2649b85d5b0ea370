// CwParameters.h — input of the CW field propagator (CwPropagator): a homogeneous lossless medium, a frequency, the
// evaluation time T and the expanded grid, validated and completed without touching a device (DESIGN.md "CW field
// propagator").
//
// No wrap-around: the periodic images of the source must not reach the domain by time T.
//   T   default: the domain diagonal over c0 — after that time every point has seen every source point
//   E_a at least N_a + ceil(c0 T / d_a) on every axis
//   default E_a: the smallest fast-path line length of the fused pipeline at or above that; when an axis has none (above
//   1024) or with fusedKernels off, the smallest even number on every axis (the run takes the rocFFT path)
// A refusal names the parameter.
#ifndef KW_HOST_CW_PARAMETERS_H
#define KW_HOST_CW_PARAMETERS_H
#include <cstddef>
#include <cstdint>
#include <string>

#include "GridRules.h"

namespace CwRule
{
/// N + ceil(c0 T / d): the least side that keeps the periodic images out of the domain until T
size_t leastSide(size_t n, double d, double c0, double t);
} // namespace CwRule

class CwParameters
{
 public:
  /// checks every parameter and fills in t and ex / ey / ez where they are 0; throws std::invalid_argument naming the parameter
  void init(const DeviceOptions& options);

  DeviceOptions options;
  size_t nx = 0, ny = 0, nz = 0;   ///< domain
  double dx = 0, dy = 0, dz = 0;   ///< [m]
  double c0 = 0, f0 = 0;           ///< [m/s], [Hz]
  double t  = 0;                   ///< evaluation time [s]; 0: the default
  size_t ex = 0, ey = 0, ez = 0;   ///< expanded grid; all 0: by the rule, otherwise all three given
  double scaleRe = 1.0, scaleIm = 0.0; ///< complex factor on the source (kwaveScale() for the time loop's additive source)

  bool   fastPath = false;         ///< every side of the expanded grid is a fast-path length (and fusedKernels is on)
  double omega() const { return 2.0 * 3.14159265358979323846 * f0; }
  size_t nElements() const { return nx * ny * nz; }
  size_t nExpanded() const { return ex * ey * ez; }
  size_t nReduced() const { return (ex / 2 + 1) * ey * ez; }
  /// sets the source scale to 2 i w c0 / dx: the source term of the wave equation that the time loop's additive pressure
  /// source of amplitude p_s makes (mass rate 2 p_s / (c0 dx) summed over the density components)
  void kwaveScale() { scaleRe = 0.0; scaleIm = 2.0 * omega() * c0 / dx; }
};
#endif
