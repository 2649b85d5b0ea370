// GridRules.h — the parameter rules that the operators with their own context share (CwParameters, AngularParameters,
// AngularTimeParameters, PlaneReconParameters, LineReconParameters, SecondOrderParameters, SecondOrderFramesParameters): the refusal that names the parameter, the size and sign checks, the fused
// pipeline's line lengths and the checks of an expanded grid.  No device call.
#ifndef KW_HOST_GRID_RULES_H
#define KW_HOST_GRID_RULES_H
#include <cstddef>
#include <string>

/// what every such operator takes besides its own parameters
struct DeviceOptions
{
  int  deviceIdx    = -1;
  bool fusedKernels = true;
};

namespace GridRule
{
/// throws std::invalid_argument("<parameter>: <what>")
[[noreturn]] void refuse(const std::string& parameter, const std::string& what);
/// 0 < n < limit
void checkSize(size_t n, const char* name, size_t limit = size_t(1) << 31);
/// v > 0 and finite; unit completes "is not a positive ..."
void checkPositive(double v, const char* name, const char* unit);

/// the fused pipeline's line lengths (csrc/kw_fused.hip KW_FUSED_LENGTHS; tests/test_cw_host.py compares the two lists)
bool   isFastLength(size_t n);
/// smallest fast-path length >= n, 0 when there is none
size_t nextFastLength(size_t n);

/// 32-bit element indices in the pipeline and in the FFT wrapper: refuses "E" unless ex ey ez < 2^32 (`points`: the
/// message's word for them)
void checkTotal(size_t ex, size_t ey, size_t ez, const char* points = "points");
/// the expanded sides of a plane nx x ny, given (not both 0): both present, even where requireEven, not below N, a
/// grid size
void checkGivenSides(size_t nx, size_t ny, size_t ex, size_t ey, bool requireEven);
/// the projectors' default sides: the fast-path length at or above 2 N on both axes; 2 N where an axis has none or with
/// fusedKernels off
void defaultDoubledSides(size_t nx, size_t ny, size_t& ex, size_t& ey, bool fusedKernels);
/// the exact propagators' default side: N + ceil(reach / d) with reach = c0 t_max, and the fast-path length at or above it
/// where there is one and it is wanted; refuses "t_max" when the reach is over 2^32 grid points
size_t reachSide(size_t n, double d, double reach, bool fusedKernels);
/// the exact propagators' absorption: a = alpha_coeff 100 (1e-6 / 2 pi)^y / (20 log10 e) [Np (rad/s)^-y m^-1], and
/// B = 1 - 2 g T - g^2 with g = a c0^y k^(y-1), T = tan(pi y / 2) (0 for y = 2); B = 1 without absorption and at k = 0
double powerLawNepers(double alphaCoeff, double y);
double powerLawDamping(double a, double c0, double y, double k);
} // namespace GridRule
#endif
