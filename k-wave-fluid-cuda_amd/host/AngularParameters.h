// AngularParameters.h — input of the angular-spectrum CW projector (AngularSpectrum): a pressure plane, a homogeneous
// medium with optional absorption, the output planes z_j = z0 + j dz, the expanded sides and the plane-chunk size,
// validated and completed without touching a device (DESIGN.md "Angular-spectrum projector").
//
//   default E_a: the smallest fast-path line length of the fused pipeline at or above 2 N_a; when an axis has none (above
//   1024) or with fusedKernels off, 2 N_a on both axes (the run takes the rocFFT path).  Given sides: even, not below N_a.
//   default chunk: the smallest of 16, 32, 48, 64 planes that holds all the planes, 64 beyond that (measured: the largest
//   chunk is the fastest at every expanded side from 256 to 1024), reduced while its two real arrays and two
//   spectra (16 B per expanded point and plane) exceed 1 GiB; 16 at least.  On the fast path a given chunk must be a
//   fast-path length.
//   planes: at most 4096 (the 32-bit phase accumulator of kw_angular_operator is specified up to plane index 4095).
// A refusal names the parameter.
#ifndef KW_HOST_ANGULAR_PARAMETERS_H
#define KW_HOST_ANGULAR_PARAMETERS_H
#include <cstddef>
#include <cstdint>
#include <string>

#include "GridRules.h"

namespace AngularRule
{
constexpr size_t kMaxPlanes   = 4096;
constexpr size_t kChunkBudget = size_t(1) << 30; ///< bytes of one chunk: 16 per expanded point and plane
/// default plane-chunk size for expanded sides ex x ey and `planes` output planes
size_t chunkPlanes(size_t ex, size_t ey, size_t planes);
} // namespace AngularRule

class AngularParameters
{
 public:
  /// checks every parameter and fills in ex / ey and chunkPlanes where they are 0; throws std::invalid_argument naming the parameter
  void init(const DeviceOptions& options);

  DeviceOptions options;
  size_t nx = 0, ny = 0;          ///< the plane
  double dx = 0, dy = 0;          ///< [m]
  double c0 = 0, f0 = 0;          ///< [m/s], [Hz]
  double z0 = 0, dz = 0;          ///< [m]: first output plane (>= 0), plane spacing (> 0)
  size_t planes = 0;              ///< Nz
  double alphaNp = 0;             ///< [Np/m] at f0; 0: lossless
  bool   restriction = true;      ///< angular restriction
  size_t ex = 0, ey = 0;          ///< expanded sides; both 0: by the rule
  size_t chunkPlanes = 0;         ///< planes per chunk; 0: by the rule

  bool   fastPath = false;        ///< both sides and the chunk are fast-path lengths (and fusedKernels is on)
  double k() const { return 2.0 * 3.14159265358979323846 * f0 / c0; }
  size_t nPlane() const { return nx * ny; }
  size_t nElements() const { return nx * ny * planes; }
  size_t nReduced() const { return (ex / 2 + 1) * ey; }
};
#endif
