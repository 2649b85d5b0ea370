// GridRules.h — the parameter rules that the operators with their own context share (CwParameters, AngularParameters,
// AngularTimeParameters, PlaneReconParameters, LineReconParameters, SecondOrderParameters, SecondOrderFramesParameters):
// the refusal that names the parameter, the size and sign checks, the fused pipeline's line lengths and the checks of an
// expanded grid; and SecondOrderRules, the base of the last two.  No device call.
#ifndef KW_HOST_GRID_RULES_H
#define KW_HOST_GRID_RULES_H
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

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

/// what the exact propagators' parameters have in common (the base of SecondOrderParameters and
/// SecondOrderFramesParameters): the medium, the sensor points, the aggregates wanted and what init() completes.  The
/// checks are protected: each init() calls them at its own place among the checks of its sizes.
struct SecondOrderRules
{
  /// throws unless t is finite and >= 0
  static void checkTime(double t);

  // ---- the records of many output times (SecondOrderFrames::lineRecord, SecondOrder::planeRecord) run in passes ----
  static constexpr size_t kRecordBudgetBytes = size_t(256) << 20;    ///< of G in the default pass
  static constexpr size_t kRecordTimesMost   = size_t(65535) * 256;  ///< the record kernels' time tiles are a block index
  struct TimeChunk { size_t first, count; };                         ///< output times first ... first + count - 1
  /// the times of one pass.  given == 0: as many as keep G (bytesPerTime each) within kRecordBudgetBytes, one at the least;
  /// otherwise `given`, refused as `name` ("<given> times of <of> are too many ...") when the pass's rows (pointsPerTime
  /// each, indexed in 32 bits as every batch here) reach 2^32 points or it is above kRecordTimesMost
  static size_t passTimes(uint64_t given, size_t bytesPerTime, size_t pointsPerTime, const char* name, const std::string& of);
  /// nTimes in passes of at most chunkTimes, in order; refuses "n_times" for 0 and `name` for a chunk of 0
  static std::vector<TimeChunk> timeChunks(size_t nTimes, size_t chunkTimes, const char* name);

  DeviceOptions options;
  double c0 = 0;                  ///< [m/s]
  double alphaCoeff = 0;          ///< [dB / (MHz^y cm)]; 0: lossless
  double alphaPower = 1.5;        ///< y
  double tMax = 0;                ///< [s]; read for the default sides only
  std::vector<uint64_t> sensorIndex; ///< 0-based flat indices into the domain (3-D) or into one plane (frames)
  bool   pMax = false, pMin = false, pRms = false, pFinal = false; ///< aggregates over the output times of a run

  bool   fastPath = false;        ///< every side is a fast-path length (and fusedKernels is on)
  double a = 0;                   ///< [Np (rad/s)^-y m^-1]
  double tFree = 0;               ///< [s]
  double bSmallest = 1, bLargest = 1; ///< B at the smallest non-zero and at the largest |k| of the grid
  /// B(|k|) of the completed parameters
  double damping(double k) const { return GridRule::powerLawDamping(a, c0, alphaPower, k); }

 protected:
  /// refuses "c0", "alpha_coeff", "alpha_power", in this order
  void checkMedium() const;
  /// refuses "sensor_index" at the first index not below `points`; `where`: "domain" or "plane"
  void checkSensors(size_t points, const char* where) const;
  /// a, bSmallest and bLargest over the `axes` sides e of spacings d; refuses "alpha_coeff" when B is below 1/4 at either
  void completeAbsorption(const size_t* e, const double* d, int axes);
};
#endif
