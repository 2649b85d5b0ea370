// SecondOrderFrames.h — batched 2-D exact k-space propagator: F independent initial pressures p0[f][y][x] in a homogeneous
// medium, lossless or power-law absorbing, to the pressure of each at any time with no time loop (DESIGN.md "Exact k-space
// propagator on frames") — SecondOrder with the z axis removed and the frame count in its place.  Its parameters, a
// SecondOrderCore in the frames form and the line-sensor record.  The core owns the context through a DeviceGrid: the
// fused pipeline in frames mode (the z axis of the constants is the batch) where wanted and supported, the batched 2-D
// rocFFT plans otherwise.
//
//   setP0: embed every p0 into its zero-filled plane Ey x Ex (kw_angular_time_embed, the frame in the slowest position),
//         transform once and keep — fast path: kw_fused_second_order_frames_forward; others: kw_fft_r2c_frames
//   field(t): fast path: kw_fused_second_order_frames_time; others: kw_second_order_frames_mix and kw_fft_c2r_frames — then
//         the crop to the domain (kw_plane_recon_crop), which stays on the device
//   run(times): the core's loop, SecondOrder's too: per time the passes, the sample at the sensor points of every frame
//         into row i of the record [n_times][F][n_sensor] (kw_sample_index on the expanded batch, indices translated once) and, where asked
//         for, the crop and kw_sample_all into the running max, min, sum of squares and the final field.
//   lineRecord(times): the record of one row of every frame (csrc/kw_second_order_line.hip): setLineRow, then at every
//         setP0 the natural (kx, ky) spectra (rocFFT path: the kept ones; fast path: one kw_fft_r2c_frames of the embedded
//         batch into an array of its own, after the fused forward has read it) go through kw_second_order_line_prepare
//         into Q; per pass of at most lineChunkTimes() output times kw_second_order_line_record into G, a batched 1-D C2R
//         of length Ex over its F times rows on a second context (Ex, 1, F times) and the crop of Ex to Nx.  Neither the
//         field state nor the aggregates of run are touched.
//
// Device memory, E = Ex Ey F points, R = (Ex/2 + 1) Ey F bins, N = Nx Ny F: the batch 4 E, the kept spectrum (8 R; a scratch
// array on the fast path) and the pipeline's scratch arrays (fast path) or one more spectrum 8 R (rocFFT); the crop 4 N and
// 4 N per aggregate; the record 4 n_times F n_sensor.  From the first setDp0dt on: a second kept spectrum.  With a line row: Q 8 (Ex/2 + 1) (Ey/2 + 1) F, on the fast path the
// natural spectra 8 R as well, the times 8 n_times, and per pass of T times G 8 (Ex/2 + 1) F T, its rows 4 Ex F T and their
// crop 4 Nx F T.
#ifndef KW_HOST_SECOND_ORDER_FRAMES_H
#define KW_HOST_SECOND_ORDER_FRAMES_H
#include <memory>
#include <string>

#include "SecondOrderCore.h"
#include "SecondOrderFramesParameters.h"

class SecondOrderFrames
{
 public:
  explicit SecondOrderFrames(const SecondOrderFramesParameters& parameters);
  SecondOrderFrames(const SecondOrderFrames&) = delete;
  SecondOrderFrames& operator=(const SecondOrderFrames&) = delete;

  /// p0: Nx Ny F floats on the host, [F][Ny][Nx]; may be called again
  void setP0(const float* p0);
  /// dp/dt at t = 0 of every frame [Pa/s], Nx Ny F floats on the host, [F][Ny][Nx]; NULL clears it.  Independent of setP0.
  /// field and run then take both conditions (kw_fused_second_order_frames_time_pair / kw_second_order_frames_mix_pair);
  /// lineRecord refuses while one is set.
  void setDp0dt(const float* dp0dt) { mCore.setDp0dt(dp0dt); }
  bool hasDp0dt() const { return mCore.hasDp0dt(); }
  /// every frame's pressure at time t on the domain; dst: Nx Ny F floats on the host or NULL (the crop stays on the device)
  void field(double t, float* dst) { mCore.field(t, dst); }
  /// every time in the given order: the record's row, the aggregates
  void run(const double* times, size_t nTimes) { mCore.run(times, nTimes); }
  /// "p_raw" [n_times][F][n_sensor], "p_max", "p_min", "p_rms", "p_final" of the last run, "p" (the last field computed)
  void get(const std::string& name, float* dst, size_t n) { mCore.get(name, dst, n); }
  /// the row of every plane that lineRecord records, 0 ... Ny - 1, from the next setP0 on; -1: none, its arrays are freed
  void setLineRow(int64_t row);
  /// how many output times one pass of lineRecord takes; 0: the default (SecondOrderFramesParameters::lineChunkTimes)
  void setLineChunkTimes(uint64_t times);
  /// the row's pressure in every frame at every time, in the given order; dst: [F][nTimes][Nx] floats on the host, or NULL
  void lineRecord(const double* times, size_t nTimes, float* dst);
  int64_t lineRow() const { return mLineRow; }
  size_t  lineChunkTimes() const { return mPar.lineChunkTimes(mLineChunkGiven); }
  bool    usesFusedPipeline() const { return mCore.grid().fused(); }
  size_t  runs() const { return mCore.runs(); }
  kw_ctx* context() const { return mCore.ctx(); }
  const SecondOrderFramesParameters& parameters() const { return mPar; }

 private:
  /// what the main context holds of the line record
  struct Line
  {
    bool    ready = false;     // q holds the current p0 at mLineRow
    float*  q = nullptr;       // Q [Ex/2 + 1][Ey/2 + 1][F]
    float*  spec = nullptr;    // fast path: the natural spectra of p0
    double* times = nullptr;   // the output times of a call
    size_t  timesCapacity = 0;
  };
  /// a second context with constants (Ex, 1, F times): the batched 1-D plans and the arrays of a pass of `times` output times
  struct LinePass
  {
    LinePass(const SecondOrderFramesParameters& par, size_t times);
    DeviceGrid grid;
    size_t     times;
    float     *g = nullptr, *rows = nullptr, *out = nullptr; // G, its F times rows of Ex, their crop to Nx
  };
  void prepareLine();              // mLine.q <- the spectra of the p0 just set
  void makeLinePass(size_t times); // mLinePass <- a pass of `times` output times, unless it is one already
  void freeLine();

  SecondOrderFramesParameters mPar;
  SecondOrderCore mCore;
  int64_t    mLineRow = -1;          // the row wanted
  uint64_t   mLineChunkGiven = 0;    // 0: the default
  bool       mLinePlans = false;     // fast path: the batched 2-D rocFFT plans exist on the main context
  Line       mLine;
  std::unique_ptr<LinePass> mLinePass;
};
#endif
