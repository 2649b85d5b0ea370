// PlaneRecon.h — k-space plane reconstruction: the record p[t][y][x] of a planar sensor to the initial pressure
// p0[z][y][x] that produced it, homogeneous medium (DESIGN.md "k-space plane reconstruction"; what k-Wave's
// kspacePlaneRecon computes).  Owns its context through a DeviceGrid.
//
//   run:  the record to the device, kw_plane_recon_embed (mirrored in time into the zero volume Lt x Ey x Ex), then
//         fast path: kw_fused_plane_recon, in place — others: kw_fft_r2c_3d, kw_plane_recon_mix, kw_fft_c2r_3d —
//         then kw_plane_recon_crop into the result planes x Ny x Nx, which stays on the device until fetched with get.
//
// Device memory, E = Ex Ey Lt points, R = (Ex/2 + 1) Ey Lt bins: the volume 4 E and the pipeline's three scratch arrays
// (fast path) or two spectra 8 R each (rocFFT); the record 4 Nx Ny Nt; the result 4 Nx Ny planes.
#ifndef KW_HOST_PLANE_RECON_H
#define KW_HOST_PLANE_RECON_H
#include <string>

#include "DeviceGrid.h"
#include "PlaneReconParameters.h"

class PlaneRecon
{
 public:
  explicit PlaneRecon(const PlaneReconParameters& parameters);
  PlaneRecon(const PlaneRecon&) = delete;
  PlaneRecon& operator=(const PlaneRecon&) = delete;

  /// p: Nx Ny Nt floats on the host, [Nt][Ny][Nx]
  void run(const float* p);
  /// "p0" of the last run: n = Nx Ny planes
  void get(const std::string& name, float* dst, size_t n);
  bool    usesFusedPipeline() const { return mGrid.fused(); }
  size_t  runs() const { return mRuns; }
  kw_ctx* context() const { return mGrid.ctx(); }
  const PlaneReconParameters& parameters() const { return mPar; }

 private:
  void reconstruct(); // the transform stage, in place on the volume

  PlaneReconParameters mPar;
  DeviceGrid   mGrid; // the context, the pipeline and every device array below
  size_t       mRuns = 0;
  float* mVol = nullptr;     // Lt Ey Ex: the embedded record, then the reconstruction
  float* mSpecA = nullptr;   // rocFFT path: the spectrum of the volume
  float* mSpecB = nullptr;   // rocFFT path: the re-gridded spectrum
  float* mRecord = nullptr;  // the record as handed in
  float* mResult = nullptr;  // [planes][Ny][Nx]
};
#endif
