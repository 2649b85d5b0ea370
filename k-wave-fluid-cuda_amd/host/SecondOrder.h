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
//   planeRecord(times): the record of one plane z = r dz of the domain (csrc/kw_second_order_plane.hip): setPlane, then at
//         every setP0 the natural (kx, ky, kz) spectrum (rocFFT path: the kept one; fast path: one kw_fft_r2c_3d of the
//         embedded volume into an array of its own, after the fused forward has read it, freed again afterwards) goes
//         through kw_second_order_plane_prepare into Q; per pass of at most planeChunkTimes() output times
//         kw_second_order_plane_record into G, a batched 2-D C2R over its planes on a second context (Ex, Ey, times) and the
//         crop of (Ex, Ey) to (Nx, Ny).  Neither the field state nor the aggregates of run are touched.
//
// Device memory, E = Ex Ey Ez points, R = (Ex/2 + 1) Ey Ez bins, N the domain: the volume 4 E, the kept spectrum (8 R; a
// scratch array on the fast path) and the pipeline's three scratch arrays (fast path) or one more spectrum 8 R (rocFFT);
// the crop 4 N and 4 N per aggregate; the record 4 n_times n_sensor.  From the first setDp0dt on: a second kept spectrum.
// With a plane: Q 8 Ey (Ex/2 + 1) (Ez/2 + 1), on the fast path during setP0 the natural spectrum 8 R as well, the times
// 8 n_times, and per pass of T times G 8 (Ex/2 + 1) Ey T, its planes 4 Ex Ey T and their crop 4 Nx Ny T.
#ifndef KW_HOST_SECOND_ORDER_H
#define KW_HOST_SECOND_ORDER_H
#include <memory>
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
  void setP0(const float* p0);
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
  /// the plane of the domain that planeRecord records, 0 ... Nz - 1, from the next setP0 on; -1: none, its arrays are freed
  void setPlane(int64_t plane);
  /// how many output times one pass of planeRecord takes; 0: the default (SecondOrderParameters::planeChunkTimes)
  void setPlaneChunkTimes(uint64_t times);
  /// the plane's pressure at every time, in the given order; dst: [nTimes][Ny][Nx] floats on the host, or NULL
  void planeRecord(const double* times, size_t nTimes, float* dst);
  int64_t plane() const { return mPlaneWanted; }
  size_t  planeChunkTimes() const { return mPar.planeChunkTimes(mPlaneChunkGiven); }
  bool    usesFusedPipeline() const { return mCore.grid().fused(); }
  size_t  runs() const { return mCore.runs(); }
  kw_ctx* context() const { return mCore.ctx(); }
  const SecondOrderParameters& parameters() const { return mPar; }

 private:
  /// what the main context holds of the plane record
  struct Plane
  {
    bool    ready = false;     // q holds the current p0 at mPlaneWanted
    float*  q = nullptr;       // Q [Ey][Ex/2 + 1][Ez/2 + 1]
    double* times = nullptr;   // the output times of a call
    size_t  timesCapacity = 0;
  };
  /// a second context with constants (Ex, Ey, times): the batched 2-D plans and the arrays of a pass of `times` output times
  struct PlanePass
  {
    PlanePass(const SecondOrderParameters& par, size_t times);
    DeviceGrid grid;
    size_t     times;
    float     *g = nullptr, *planes = nullptr, *out = nullptr; // G, its planes of Ey x Ex, their crop to Ny x Nx
  };
  void preparePlane();              // mPlane.q <- the spectrum of the p0 just set
  void makePlanePass(size_t times); // mPlanePass <- a pass of `times` output times, unless it is one already
  void freePlane();

  SecondOrderParameters mPar;
  SecondOrderCore mCore;
  int64_t    mPlaneWanted = -1;      // the plane wanted
  uint64_t   mPlaneChunkGiven = 0;   // 0: the default
  bool       mPlanePlans = false;    // fast path: the 3-D rocFFT plans exist on the main context
  Plane      mPlane;
  std::unique_ptr<PlanePass> mPlanePass;
};
#endif
