// ThermalParameters.h — input of the bioheat solver (ThermalSolver): the datasets of a thermal problem, validated and
// turned into the per-point coefficients of the scheme (DESIGN.md "Bioheat") without touching a device.
//
//   a = 1 / (rho C),  P = rho_b C_b W_b a,  D = K a   (computed in double from the float datasets, rounded once)
//   D_ref = max D, or the dataset diffusion_coeff_ref
//   kappa_d(k) = (1 - exp(-D_ref |k|^2 dt)) / (D_ref |k|^2 dt),  kappa_d(0) = 1
// Every medium dataset is a scalar or an Nx * Ny * Nz array; a refusal names the dataset.
#ifndef KW_HOST_THERMAL_PARAMETERS_H
#define KW_HOST_THERMAL_PARAMETERS_H
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "GridRules.h"
#include "InputProvider.h"

/// what the thermal solver takes from kwh_options
struct ThermalOptions : DeviceOptions
{
  size_t slabRanks = 1;
};

/// a per-point coefficient: an array of the grid's size, or one value
struct ThermalCoefficient
{
  bool               isArray = false;
  float              scalar  = 0.0f;
  std::vector<float> data;
};

/// generators of the thermal operators and vectors, in double, rounded to float once
namespace ThermalOperators
{
/// wavenumber of bin j of an n-point axis with spacing d (k-Wave's order: the Nyquist bin of an even axis is negative)
double wavenumber(size_t j, size_t n, double d);
/// kappa_d and -|k|^2 kappa_d on the reduced grid [nz][ny][nx / 2 + 1]; either output may be NULL
void generate(size_t nx, size_t ny, size_t nz, double dx, double dy, double dz, double dt, double dRef, float* kappaD,
              float* laplacian);
/// i k exp(+- i k d / 2) for the first `count` bins of an n-point axis, interleaved (re, im)
void derivative(size_t n, size_t count, double d, bool positive, float* out);
/// 2 K_sg along `axis` (0 x, 1 y, 2 z): K of each point plus K of its +1 neighbour; the last point: twice its own value
void staggeredTwice(const float* K, size_t nx, size_t ny, size_t nz, int axis, float* out);
} // namespace ThermalOperators

class ThermalParameters
{
 public:
  /// reads and checks every dataset; throws std::invalid_argument naming the dataset
  void init(const InputProvider& input, const ThermalOptions& options);

  ThermalOptions options;
  size_t nx = 0, ny = 0, nz = 0;
  float  dx = 0, dy = 0, dz = 0, dt = 0;
  size_t nElements() const { return nx * ny * nz; }
  size_t nReduced() const { return (nx / 2 + 1) * ny * nz; }

  ThermalCoefficient a, P, Ta; ///< 1 / (rho C), perfusion coefficient [1/s], ambient (blood) temperature
  bool   fluxForm      = false; ///< thermal_conductivity is an array
  float  conductivity  = 0.0f;  ///< the scalar K of the Laplacian form
  std::vector<float> twoKsg[3]; ///< flux form: 2 K_sg per axis (the fused epilogue multiplies by 0.5)
  double dRef = 0.0;            ///< reference diffusivity of the k-space correction
  std::vector<float> T0;        ///< initial temperature on the grid (a scalar T0 is expanded)
  bool               hasQ = false;
  std::vector<float> Q;         ///< volume rate of heat deposition [W/m^3] on the grid
  std::vector<uint64_t> sensorIndex; ///< 0-based linear indices of sensor_mask_index
};
#endif
