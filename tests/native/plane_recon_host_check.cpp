// plane_recon_host_check.cpp — the host side of the k-space plane reconstruction as a stand-alone CPU program:
// PlaneReconParameters::init through valid inputs (the expanded sides and the length of the mirrored record by their rules)
// and refusals.  Built with -fsanitize=address,undefined by tests/test_plane_recon_host.py together with
// host/PlaneReconParameters.cpp and host/GridRules.cpp (the shared rules and the fast-path length table).  Host code only.
// Every case prints "<name>: ok ..." or "<name>: <message>".
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>

#include "PlaneReconParameters.h"

namespace {

PlaneReconParameters base()
{
  PlaneReconParameters p;
  p.nx = 24; p.ny = 20; p.nt = 40;
  p.dx = p.dy = 1e-3;
  p.dt = 2e-7;
  p.c0 = 1500.0;
  return p;
}

void run(const char* name, const std::function<void(PlaneReconParameters&)>& change, bool fused = true)
{
  PlaneReconParameters p = base();
  change(p);
  DeviceOptions o;
  o.fusedKernels = fused;
  try
  {
    p.init(o);
    std::printf("%s: ok E=%zux%zu Lt=%zu planes=%zu fast=%d dz=%.6e\n", name, p.ex, p.ey, p.lt, p.planes, p.fastPath ? 1 : 0,
                p.dz());
  }
  catch (const std::invalid_argument& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}

} // namespace

int main()
{
  run("default", [](PlaneReconParameters&) {});
  run("rocfft", [](PlaneReconParameters&) {}, false);
  run("fast_sides", [](PlaneReconParameters& p) { p.nx = 32; p.ny = 48; });
  run("beyond_1024", [](PlaneReconParameters& p) { p.nt = 513; });
  run("given", [](PlaneReconParameters& p) { p.ex = 32; p.ey = 32; p.lt = 96; p.planes = 17; });
  run("given_odd", [](PlaneReconParameters& p) { p.ex = 25; p.ey = 21; p.lt = 81; });
  run("nearest", [](PlaneReconParameters& p) { p.interp = PlaneReconParameters::kNearest; p.positivity = true; });
  run("planes_nt", [](PlaneReconParameters& p) { p.planes = 40; });
  run("planes_above", [](PlaneReconParameters& p) { p.planes = 41; });
  run("interp_other", [](PlaneReconParameters& p) { p.interp = 2; });
  run("nx_zero", [](PlaneReconParameters& p) { p.nx = 0; });
  run("nt_zero", [](PlaneReconParameters& p) { p.nt = 0; });
  run("dt_zero", [](PlaneReconParameters& p) { p.dt = 0.0; });
  run("c0_negative", [](PlaneReconParameters& p) { p.c0 = -1.0; });
  run("lt_small", [](PlaneReconParameters& p) { p.lt = 78; });
  run("e_missing", [](PlaneReconParameters& p) { p.ex = 24; });
  run("e_small", [](PlaneReconParameters& p) { p.ex = 24; p.ey = 18; });
  run("too_large", [](PlaneReconParameters& p) { p.ex = 2048; p.ey = 2048; p.lt = 1024; });
  return 0;
}
