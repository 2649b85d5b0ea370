// LineRecon.h — batched k-space line reconstruction: F frames p[t][y] of a linear array to the F images p0[x][y] that
// produced them, homogeneous medium (DESIGN.md "k-space line reconstruction"; what k-Wave's kspaceLineRecon computes,
// frame by frame).  Owns its context through a DeviceGrid: ONE context of chunkFrames frames, which every chunk of a run
// goes through.
//
//   run:  per chunk — its frames to the device (a shorter last chunk is filled up with zero records),
//         kw_line_recon_embed (mirrored in time into the zero volume [chunk][Lt][Ey]), then
//         fast path: kw_fused_line_recon, in place — others: kw_fft_r2c_frames, kw_line_recon_mix, kw_fft_c2r_frames —
//         then kw_line_recon_crop of the chunk's own frames into the result [F][depth][Ny], which stays on the device until
//         fetched with get.
//
// Device memory, E = Ey Lt chunk points, R = (Ey/2 + 1) Lt chunk bins: the volume 4 E and ONE scratch array of the
// pipeline, 8 P Lt chunk bytes with P = Ey/2 + 1 rounded up to 16 (fast path: a frames context allocates the array its one
// stage uses), or two spectra 8 R each (rocFFT); one chunk of records 4 Ny Nt chunk; the result 4 Ny depth F.
#ifndef KW_HOST_LINE_RECON_H
#define KW_HOST_LINE_RECON_H
#include <string>

#include "DeviceGrid.h"
#include "LineReconParameters.h"

class LineRecon
{
 public:
  explicit LineRecon(const LineReconParameters& parameters);
  LineRecon(const LineRecon&) = delete;
  LineRecon& operator=(const LineRecon&) = delete;

  /// p: Ny Nt F floats on the host, [F][Nt][Ny]
  void run(const float* p);
  /// "p0" of the last run: n = Ny depth F
  void get(const std::string& name, float* dst, size_t n);
  bool    usesFusedPipeline() const { return mGrid.fused(); }
  size_t  runs() const { return mRuns; }
  kw_ctx* context() const { return mGrid.ctx(); }
  const LineReconParameters& parameters() const { return mPar; }

 private:
  void reconstruct(); // the transform stage of one chunk, in place on the volume

  LineReconParameters mPar;
  DeviceGrid   mGrid; // the context, the pipeline and every device array below
  size_t       mRuns = 0;
  float* mVol = nullptr;     // chunk Lt Ey: the embedded records, then the reconstructions
  float* mSpecA = nullptr;   // rocFFT path: the spectra of the volume
  float* mSpecB = nullptr;   // rocFFT path: the re-gridded spectra
  float* mRecord = nullptr;  // one chunk of records as handed in
  float* mResult = nullptr;  // [F][depth][Ny]
};
#endif
