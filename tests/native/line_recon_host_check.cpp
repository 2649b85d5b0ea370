// line_recon_host_check.cpp — the host side of the batched k-space line reconstruction as a stand-alone CPU program:
// LineReconParameters::init through valid inputs (the expanded axis, the length of the mirrored record and the frames per
// chunk by their rules) and refusals.  Built with -fsanitize=address,undefined by tests/test_line_recon_host.py together
// with host/LineReconParameters.cpp and host/GridRules.cpp (the shared rules and the fast-path length table).  Host code
// only.  Every case prints "<name>: ok ..." or "<name>: <message>".
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>

#include "LineReconParameters.h"

namespace {

LineReconParameters base()
{
  LineReconParameters p;
  p.ny = 24; p.nt = 40; p.frames = 6;
  p.dy = 1e-3;
  p.dt = 2e-7;
  p.c0 = 1500.0;
  return p;
}

void run(const char* name, const std::function<void(LineReconParameters&)>& change, bool fused = true)
{
  LineReconParameters p = base();
  change(p);
  DeviceOptions o;
  o.fusedKernels = fused;
  try
  {
    p.init(o);
    std::printf("%s: ok Ey=%zu Lt=%zu depth=%zu chunk=%zu chunks=%zu fast=%d dx=%.6e\n", name, p.ey, p.lt, p.depth,
                p.chunkFrames, p.nChunks(), p.fastPath ? 1 : 0, p.dx());
  }
  catch (const std::invalid_argument& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}

} // namespace

int main()
{
  run("default", [](LineReconParameters&) {});
  run("rocfft", [](LineReconParameters&) {}, false);
  run("fast_axis", [](LineReconParameters& p) { p.ny = 32; });
  run("beyond_1024", [](LineReconParameters& p) { p.nt = 513; });
  run("given", [](LineReconParameters& p) { p.ey = 32; p.lt = 96; p.depth = 17; p.chunkFrames = 4; });
  run("given_odd", [](LineReconParameters& p) { p.ey = 25; p.lt = 81; });
  run("nearest", [](LineReconParameters& p) { p.interp = LineReconParameters::kNearest; p.positivity = true; });
  run("no_masked_tiles_one", [](LineReconParameters& p) { p.ey = 672; p.lt = 100; p.chunkFrames = 1; });
  run("no_masked_tiles_four", [](LineReconParameters& p) { p.ey = 672; p.lt = 100; p.chunkFrames = 4; });
  run("chunk_capped", [](LineReconParameters& p) { p.ey = 1024; p.lt = 1024; p.frames = 5000; });
  run("depth_above", [](LineReconParameters& p) { p.depth = 41; });
  run("interp_other", [](LineReconParameters& p) { p.interp = 2; });
  run("ny_zero", [](LineReconParameters& p) { p.ny = 0; });
  run("nt_zero", [](LineReconParameters& p) { p.nt = 0; });
  run("frames_zero", [](LineReconParameters& p) { p.frames = 0; });
  run("dy_zero", [](LineReconParameters& p) { p.dy = 0.0; });
  run("dt_zero", [](LineReconParameters& p) { p.dt = 0.0; });
  run("c0_negative", [](LineReconParameters& p) { p.c0 = -1.0; });
  run("lt_small", [](LineReconParameters& p) { p.lt = 78; });
  run("ey_small", [](LineReconParameters& p) { p.ey = 23; });
  run("chunk_above", [](LineReconParameters& p) { p.chunkFrames = 7; });
  run("chunk_at_byte_limit", [](LineReconParameters& p) { p.ny = 128; p.nt = 512; p.frames = 10000; p.chunkFrames = 6553; });
  run("chunk_past_byte_limit", [](LineReconParameters& p) { p.ny = 128; p.nt = 512; p.frames = 10000; p.chunkFrames = 6554; });
  run("chunk_block_index", [](LineReconParameters& p) { p.ny = 16; p.nt = 8; p.frames = 100000; });
  run("chunk_past_block_index", [](LineReconParameters& p) { p.ny = 16; p.nt = 8; p.frames = 100000; p.chunkFrames = 65536; });
  run("chunk_too_large", [](LineReconParameters& p) { p.ey = 1024; p.lt = 1024; p.frames = 5000; p.chunkFrames = 993; });
  run("too_large", [](LineReconParameters& p) { p.ey = 1u << 22; p.lt = 1024; });
  return 0;
}
