// AngularTimeParameters.h — input of the time-domain angular-spectrum projector (AngularSpectrumTime): a pressure record
// p0[t][y][x] on a plane, a homogeneous medium with optional power-law absorption, the distances of the output planes,
// the expanded sides and the expanded record length, validated and completed without touching a device (DESIGN.md
// "Time-domain angular-spectrum projector").
//
//   default E_a: AngularParameters' rule — the smallest fast-path line length of the fused pipeline at or above 2 N_a; when
//   an axis has none (above 1024) or with fusedKernels off, 2 N_a on both axes.  Given sides: even, not below N_a.
//   default Lt: the smallest fast-path length at or above Nt; Nt rounded up to even when there is none (above 1024) or with
//   fusedKernels off.  A given Lt: even, not below Nt.
//   planes: 1 ... 4096 distances z_j >= 0 in any order (each plane is computed on its own).
// A refusal names the parameter.
#ifndef KW_HOST_ANGULAR_TIME_PARAMETERS_H
#define KW_HOST_ANGULAR_TIME_PARAMETERS_H
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "AngularParameters.h"

class AngularTimeParameters
{
 public:
  /// checks every parameter and fills in ex / ey / lt where they are 0; throws std::invalid_argument naming the parameter
  void init(const DeviceOptions& options);

  DeviceOptions options;
  size_t nx = 0, ny = 0, nt = 0;  ///< the record
  double dx = 0, dy = 0, dt = 0;  ///< [m], [m], [s]
  double c0 = 0;                  ///< [m/s]
  double alphaCoeff = 0;          ///< [dB / (MHz^y cm)]; 0: lossless
  double alphaPower = 1.5;        ///< y
  bool   restriction = true;      ///< angular restriction
  bool   retarded = false;        ///< plane z reported at the times t_n + z / c0
  size_t ex = 0, ey = 0;          ///< expanded sides; both 0: by the rule
  size_t lt = 0;                  ///< expanded record length; 0: by the rule
  std::vector<double> z;          ///< [m], the output planes

  bool   fastPath = false;        ///< both sides and Lt are fast-path lengths (and fusedKernels is on)
  size_t nPlane() const { return nx * ny; }
  size_t nRecord() const { return nx * ny * nt; }
  size_t nExpanded() const { return ex * ey * lt; }
  size_t nReduced() const { return (ex / 2 + 1) * ey * lt; }
  /// alpha(m') k(m') log2(e) for m' = 0 ... Lt/2: alpha = a0 f^y [Np/m] at f = m' / (Lt dt), k = 2 pi f / c0
  std::vector<double> akTable() const;
};
#endif
