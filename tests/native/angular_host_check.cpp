// angular_host_check.cpp — the host side of the angular-spectrum projector as a stand-alone CPU program:
// AngularParameters::init through valid inputs (the expanded sides and the plane-chunk size by their rules) and refusals.
// Built with -fsanitize=address,undefined by tests/test_angular_host.py together with host/AngularParameters.cpp and
// host/GridRules.cpp (the shared rules and the fast-path length table).  Host code only.
// Every case prints "<name>: ok ..." or "<name>: <message>".
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>

#include "AngularParameters.h"

namespace {

AngularParameters base()
{
  AngularParameters p;
  p.nx = 24; p.ny = 20;
  p.dx = p.dy = 1e-3;
  p.c0 = 1500.0;
  p.f0 = 500e3;
  p.z0 = 0.0;
  p.dz = 1e-3;
  p.planes = 20;
  return p;
}

void run(const char* name, const std::function<void(AngularParameters&)>& change, bool fused = true)
{
  AngularParameters p = base();
  change(p);
  DeviceOptions o;
  o.fusedKernels = fused;
  try
  {
    p.init(o);
    std::printf("%s: ok E=%zux%zu chunk=%zu fast=%d\n", name, p.ex, p.ey, p.chunkPlanes, p.fastPath ? 1 : 0);
  }
  catch (const std::invalid_argument& e)
  {
    std::printf("%s: %s\n", name, e.what());
  }
}

} // namespace

int main()
{
  run("default", [](AngularParameters&) {});
  run("rocfft", [](AngularParameters&) {}, false);
  run("chunk16", [](AngularParameters& p) { p.nx = p.ny = 1024; p.planes = 100; });
  run("chunk48", [](AngularParameters& p) { p.nx = 150; p.ny = 128; p.planes = 40; });
  run("beyond_1024", [](AngularParameters& p) { p.nx = 600; p.ny = 16; p.planes = 100; });
  run("given", [](AngularParameters& p) { p.ex = 32; p.ey = 48; p.chunkPlanes = 16; });
  run("planes_4096", [](AngularParameters& p) { p.planes = 4096; });
  run("z0_negative", [](AngularParameters& p) { p.z0 = -1e-3; });
  run("dz_zero", [](AngularParameters& p) { p.dz = 0.0; });
  run("planes_4097", [](AngularParameters& p) { p.planes = 4097; });
  run("e_odd", [](AngularParameters& p) { p.ex = 49; p.ey = 48; });
  run("e_small", [](AngularParameters& p) { p.ex = 48; p.ey = 18; });
  run("alpha_negative", [](AngularParameters& p) { p.alphaNp = -1.0; });
  run("f0_zero", [](AngularParameters& p) { p.f0 = 0.0; });
  run("chunk_20", [](AngularParameters& p) { p.chunkPlanes = 20; });
  return 0;
}
