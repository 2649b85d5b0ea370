// SecondOrder.h — exact k-space propagator: an initial pressure p0[z][y][x] in a homogeneous medium, lossless or power-law
// absorbing, to the pressure at any time with no time loop (DESIGN.md "Exact k-space propagator"; what k-Wave's
// kspaceSecondOrder computes).  Its parameters and a SecondOrderCore in the 3-D form: the core owns the context through a
// DeviceGrid and holds the bodies of everything below, which SecondOrderFrames runs in its own form.
//
//   setP0: embed p0 into the zero-filled volume Ez x Ey x Ex (kw_angular_time_embed), transform it once and keep the
//         result — fast path: kw_fused_second_order_forward (the (kx, ky, z) half-spectrum); others: kw_fft_r2c_3d
//   field(t): fast path: kw_fused_second_order_time; others: kw_second_order_mix and kw_fft_c2r_3d — then the crop to the
//         domain (kw_plane_recon_crop), which stays on the device
//   run(times): for every time in the given order the three passes, the sample at the sensor points into row i of the
//         record (kw_sample_index on the expanded volume, indices translated once) and, where asked for, the crop and
//         kw_sample_all into the running max, min, sum of squares and the final field — all exact and in a fixed order.
//
// Device memory, E = Ex Ey Ez points, R = (Ex/2 + 1) Ey Ez bins, N the domain: the volume 4 E, the kept spectrum (8 R; a
// scratch array on the fast path) and the pipeline's three scratch arrays (fast path) or one more spectrum 8 R (rocFFT);
// the crop 4 N and 4 N per aggregate; the record 4 n_times n_sensor.  From the first setDp0dt on: a second kept spectrum.
#ifndef KW_HOST_SECOND_ORDER_H
#define KW_HOST_SECOND_ORDER_H
#include <string>

#include "SecondOrderCore.h"
#include "SecondOrderParameters.h"

class SecondOrder
{
 public:
  explicit SecondOrder(const SecondOrderParameters& parameters);
  SecondOrder(const SecondOrder&) = delete;
  SecondOrder& operator=(const SecondOrder&) = delete;

  /// p0: Nx Ny Nz floats on the host, [Nz][Ny][Nx]; may be called again
  void setP0(const float* p0) { mCore.setP0(p0); }
  /// dp/dt at t = 0 [Pa/s], Nx Ny Nz floats on the host, [Nz][Ny][Nx]; NULL clears it.  Independent of setP0.  field and
  /// run then take both conditions (kw_fused_second_order_time_pair / kw_second_order_mix_pair); the second kept spectrum
  /// (8 R more) exists from the first call on.
  void setDp0dt(const float* dp0dt) { mCore.setDp0dt(dp0dt); }
  bool hasDp0dt() const { return mCore.hasDp0dt(); }
  /// the pressure at time t on the domain; dst: Nx Ny Nz floats on the host or NULL (the crop stays on the device)
  void field(double t, float* dst) { mCore.field(t, dst); }
  /// every time in the given order: the record's row, the aggregates
  void run(const double* times, size_t nTimes) { mCore.run(times, nTimes); }
  /// "p_raw" [n_times][n_sensor], "p_max", "p_min", "p_rms", "p_final" of the last run, "p" (the last field computed)
  void get(const std::string& name, float* dst, size_t n) { mCore.get(name, dst, n); }
  bool    usesFusedPipeline() const { return mCore.grid().fused(); }
  size_t  runs() const { return mCore.runs(); }
  kw_ctx* context() const { return mCore.ctx(); }
  const SecondOrderParameters& parameters() const { return mPar; }

 private:
  SecondOrderParameters mPar;
  SecondOrderCore mCore;
};
#endif
